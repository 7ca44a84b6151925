"""Ragged batches on the GPU: many independent streams, each with its own symbol count, every stream against the oracle.

BATCH_ROWS: one row per shape, naming the batch kernels the library must report for it (tests/test_batch_host.py holds the
rows to the names the launchers can report).  Every row runs in the regimes of tests/test_gpu_kernel_matrix.py --

  U  one stream per launch (each of the mandatory lengths in turn)
  H  about half as many streams as there are resident waves
  R  at least 4 x (CUs x 2 blocks x 16 waves) streams: several rounds of the persistent grid

-- with lengths drawn log-uniform from [0, 64 Ki] (fixed seed) that always include 0, 1, N-1, N, N+1, 4N+3 and 65536, once
with sym_align = 1 (odd output addresses: element stores) and once with sym_align = 4 (dword stores).  Input is
bench.gen_zipf with seed 1; the checker is the CPU oracle (Oracle.encode per stream, threaded over the host cores), never
the library itself.  Output buffers are filled with a poison value first: the padding between streams and a guard region
behind the last one must come back untouched."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from _around_coders import ref_order_keys
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

WAVES_PER_BLOCK = 16
GUARD = 4096  # symbols behind the last stream
POISON = 0xA5
MAX_LEN = 65536


def _row(rid, fmt, sb, K, ways, decode, encode):
    return {"id": rid, "fmt": fmt, "sb": sb, "K": K, "ways": ways, "decode": decode, "encode": encode}


BATCH_ROWS = [
    _row("word-64", FMT_WORD, 12, 256, 64, "k_decode_batch_word64", "k_encode_batch<word>"),
    _row("word-128", FMT_WORD, 12, 256, 128, "k_decode_batch<word>", "k_encode_batch<word>"),
    _row("word-8", FMT_WORD, 12, 256, 8, "k_decode_batch<word>", "k_encode_batch<word>"),
    _row("word-u16-64", FMT_WORD, 12, 1024, 64, "k_decode_batch<word, u16 symbols>", "k_encode_batch<word>"),
    _row("byte-64-14bit", FMT_BYTE, 14, 256, 64, "k_decode_batch<byte>", "k_encode_batch<byte>"),
    _row("byte-64-12bit", FMT_BYTE, 12, 256, 64, "k_decode_batch<byte, slot records>", "k_encode_batch<byte>"),
    _row("byte-2", FMT_BYTE, 14, 256, 2, "k_decode_batch<byte>", "k_encode_batch<byte>"),
    _row("r64-64", FMT_R64, 14, 256, 64, "k_decode_batch<r64>", "k_encode_batch<r64>"),
    _row("r64-2", FMT_R64, 14, 256, 2, "k_decode_batch<r64>", "k_encode_batch<r64>"),
    _row("r64-search-64", FMT_R64, 20, 256, 64, "k_decode_batch<r64 search>", "k_encode_batch<r64 full-width>"),
    _row("alias256-64", FMT_ALIAS, 16, 256, 64, "k_decode_batch<alias>", "k_encode_batch<alias, LDS remap>"),
]
ROW = {r["id"]: r for r in BATCH_ROWS}
UNIT = {FMT_BYTE: 1, FMT_ALIAS: 1, FMT_WORD: 2, FMT_R64: 4}


def mandatory_lengths(ways):
    return [0, 1, ways - 1, ways, ways + 1, 4 * ways + 3, MAX_LEN]


def draw_lengths(n_streams, ways, seed):
    """Log-uniform in [0, 64 Ki]; the mandatory lengths at fixed-seed positions (all of them from seven streams on)."""
    rng = np.random.default_rng(seed)
    c = (np.exp(rng.random(n_streams) * np.log(MAX_LEN + 1.0)) - 1.0).astype(np.int64).clip(0, MAX_LEN).astype(np.uint32)
    must = mandatory_lengths(ways)
    if n_streams >= len(must):
        c[rng.choice(n_streams, len(must), replace=False)] = must
    return c


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def resident_waves(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * WAVES_PER_BLOCK


class Batch:
    """The symbols of a batch (dense, bench.gen_zipf seed 1), its models and the oracle's stream of every stream.
    contents: {stream: its symbols} in place of the generator's (tests/test_gpu_rate_extremes.py); freqs: a normalised model
    in place of the one counted from the generator's sample."""

    def __init__(self, R, ctx, torch, oracle, row, counts, seed=1, contents=None, freqs=None):
        import bench
        self.R, self.ctx, self.torch, self.row = R, ctx, torch, row
        self.counts = np.ascontiguousarray(counts, dtype=np.uint32)
        self.n = self.counts.size
        self.dense_offs = np.concatenate(([0], np.cumsum(self.counts.astype(np.int64))))
        total = int(self.dense_offs[-1])
        self.d_dense = bench.gen_zipf(torch, max(total, 1), row["K"], 1.0, seed, "cuda")[:total]
        if contents:
            h = self.d_dense.cpu().numpy()
            for c, content in contents.items():
                assert content.size == self.counts[c]
                h[self.dense_offs[c]:self.dense_offs[c + 1]] = np.asarray(content).astype(np.uint16).astype(h.dtype)
            self.d_dense = torch.from_numpy(h).cuda()
        if freqs is not None:
            self.freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        else:
            # (the model comes from a fixed 1 Mi-symbol sample of the same generator: every symbol of the alphabet is in it)
            sample = bench.gen_zipf(torch, 1 << 20, row["K"], 1.0, seed, "cuda")
            self.freqs, _ = R.normalize_freqs(ctx.count_freqs_device(sample, row["K"]), 1 << row["sb"])
        self.gm = ctx.model(row["fmt"], self.freqs, row["sb"])
        self.om = oracle.model(self.freqs, row["sb"], with_alias=(row["fmt"] == FMT_ALIAS))
        h = self.d_dense.cpu().numpy()
        self.h_dense = h.view(np.uint16) if h.dtype == np.int16 else h
        fmt, ways, om, offs = row["fmt"], row["ways"], self.om, self.dense_offs

        def run(c):
            return oracle.encode(fmt, om, self.h_dense[offs[c]:offs[c + 1]], ways)
        with ThreadPoolExecutor(oracle.host_threads()) as ex:
            self.streams = list(ex.map(run, range(self.n), chunksize=64))
        self.lens = np.array([s.size for s in self.streams], dtype=np.uint32)
        self.d_counts = torch.from_numpy(self.counts.view(np.int32)).cuda()

    def poison(self):
        return POISON if self.d_dense.dtype == self.torch.uint8 else -23131  # 0xA5A5 as int16

    def laid_out(self, align):
        """-> (d_buf, sym_offs, slot_offs): the symbols at batch_layout's offsets in a poison-filled buffer with a guard."""
        torch = self.torch
        sym_offs, slot_offs = self.R.batch_layout(self.counts, self.row["fmt"], self.row["ways"], align)
        d_buf = torch.full((int(sym_offs[-1]) + GUARD,), self.poison(), dtype=self.d_dense.dtype, device="cuda")
        if self.d_dense.numel():
            shift = torch.from_numpy(sym_offs[:-1].astype(np.int64) - self.dense_offs[:-1]).cuda()
            idx = torch.arange(self.d_dense.numel(), device="cuda") + torch.repeat_interleave(shift, self.d_counts.to(torch.int64))
            d_buf[idx] = self.d_dense
        return d_buf, sym_offs, slot_offs

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()

    def oracle_container(self, seed=5):
        """The oracle's streams concatenated in a shuffled order at unit-aligned offsets with small gaps -> (cont, offs, lens)."""
        unit = UNIT[self.row["fmt"]]
        rng = np.random.default_rng(seed)
        order = rng.permutation(self.n)
        gaps = rng.integers(0, 4, self.n).astype(np.int64) * unit
        starts = np.zeros(self.n, dtype=np.int64)
        at = unit  # (not even the first stream starts on 16 bytes)
        for k, c in enumerate(order):
            at += int(gaps[k])
            starts[c] = at
            at += int(self.lens[c])
        cont = np.zeros(at + 16, dtype=np.uint8)
        for c in range(self.n):
            cont[starts[c]:starts[c] + self.lens[c]] = self.streams[c]
        return cont, starts, at

    def check_streams(self, cont, offs, lens, what):
        """Every stream of a GPU-made container (host arrays) == the oracle's, byte for byte."""
        assert np.array_equal(lens.astype(np.uint32), self.lens), (what, "lengths differ from the oracle's")
        for c in range(self.n):
            a = int(offs[c])
            assert np.array_equal(cont[a:a + int(lens[c])], self.streams[c]), (what, "stream", c, "count", int(self.counts[c]))


def run_row(b, align, with_oracle_container=True):
    R, ctx, torch, row = b.R, b.ctx, b.torch, b.row
    ways = row["ways"]
    d_buf, sym_offs, slot_offs = b.laid_out(align)
    d_sym = b.dev(sym_offs, np.int64)
    d_slot = b.dev(slot_offs, np.int64)
    # 1. encode_batch: every stream == Oracle.encode of its input, ending at its slot's end
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, ways, d_slot)
    assert ctx.last_encode_kernel()[0] == row["encode"] and ctx.last_encode_placement() == 2, ctx.last_encode_kernel()
    ctx.encode_status()
    h_offs, h_lens = offs.cpu().numpy().astype(np.uint64)[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n]
    assert np.array_equal(h_offs + h_lens, slot_offs[1:]), "a stream does not end at its slot's end"
    b.check_streams(cont.cpu().numpy(), h_offs, h_lens, "encode_batch align %d" % align)
    # 2. decode_batch of the GPU's own container: the input, padding and guard untouched
    out = torch.full_like(d_buf, b.poison())
    ctx.decode_batch(b.gm, cont, int(slot_offs[-1]), offs, lens, d_sym, b.d_counts, ways, out)
    assert ctx.last_decode_kernel() == row["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_buf), "decode of the GPU's container (align %d)" % align
    # 3. decode_batch of a batch the oracle made: unordered, unit-aligned offsets
    if with_oracle_container:
        o_cont, o_starts, o_bytes = b.oracle_container()
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, b.dev(o_cont, np.uint8), o_bytes, b.dev(o_starts, np.int64), b.dev(b.lens, np.int32), d_sym, b.d_counts,
                         ways, out)
        assert ctx.last_decode_kernel() == row["decode"], ctx.last_decode_kernel()
        assert torch.equal(out, d_buf), "decode of the oracle's container (align %d)" % align
    return cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs


def _cases():
    for r in BATCH_ROWS:
        for regime in ("U", "H", "R"):
            yield pytest.param(r, regime, id="%s-%s" % (r["id"], regime), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,regime", list(_cases()))
def test_batch_row_every_stream_equals_oracle(gpu, oracle, row, regime):
    R, ctx, torch = gpu
    resident = resident_waves(torch)
    if regime == "U":
        batches = [np.array([ln], dtype=np.uint32) for ln in mandatory_lengths(row["ways"])]
    else:
        n_streams = resident // 2 if regime == "H" else 4 * resident
        assert (0 < n_streams < resident) if regime == "H" else n_streams >= 4 * resident
        batches = [draw_lengths(n_streams, row["ways"], 7)]
        assert set(mandatory_lengths(row["ways"])) <= set(batches[0].tolist())
    for counts in batches:
        b = Batch(R, ctx, torch, oracle, row, counts)
        for align in (1, 4):
            run_row(b, align)
        assert ctx.decode_errors() == 0


LARGE = [("word-64", 20000), ("word-8", 20000), ("byte-2", 20000), ("r64-2", 20000)]


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", LARGE)
def test_batch_large_reference_layouts(gpu, oracle, rid, n_streams):
    """2 x 10^4 streams of a reference layout (word 64-way, word 8-way, byte 2-way, rans64 2-way), every stream against the
    oracle (threaded over the host cores).  Wall time on an MI355X with 16 host threads: 2.1 s (byte 2-way), 1.7 s (word
    8-way), less than that for word 64-way and rans64 2-way; this whole file takes 56 s."""
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW[rid], draw_lengths(n_streams, ROW[rid]["ways"], 13))
    run_row(b, 4)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_batch_damage_is_counted_and_contained(gpu, oracle):
    """One flipped byte in k streams, one length shortened by a unit, one sym_offset past out_syms: h_bad_streams is exactly
    the number damaged, every other stream decodes right, nothing outside the streams' ranges is written."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = Batch(R, ctx, torch, oracle, row, draw_lengths(600, 64, 21))
    for align in (1, 4):
        d_buf, sym_offs, slot_offs = b.laid_out(align)
        d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
        cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 64, d_slot)
        ctx.encode_status()
        h_offs, h_lens = offs.cpu().numpy()[:b.n], lens.cpu().numpy()[:b.n]
        rng = np.random.default_rng(3)
        # (a flipped byte is only certain to be noticed where symbols depend on it: streams of at least 4 N + 3 symbols)
        long_ones = np.nonzero(b.counts >= 4 * 64 + 3)[0]
        picked = rng.choice(long_ones, 7, replace=False)
        flipped, short, far = picked[:5], picked[5], picked[6]
        bad_cont = cont.clone()
        for c in flipped:  # inside the flushed states: a final state can no longer be L... or the cursor misses its end
            bad_cont[int(h_offs[c]) + 1] ^= 0x40
        bad_lens = lens.clone()
        bad_lens[int(short)] -= 2
        bad_sym = d_sym.clone()
        bad_sym[int(far)] = d_buf.numel() - int(b.counts[far]) + 1  # one symbol past the end
        out = torch.full_like(d_buf, b.poison())
        with pytest.raises(R.RansAmdError) as e:
            ctx.decode_batch(b.gm, bad_cont, int(slot_offs[-1]), offs, bad_lens, bad_sym, b.d_counts, 64, out)
        assert e.value.status == R.E_CORRUPT
        assert e.value.bad_streams == 7, "h_bad_streams as the call wrote it"
        assert ctx.decode_errors() == 0  # (reported and reset by that call)
        got, want = out.cpu().numpy(), d_buf.cpu().numpy()
        damaged = set(int(c) for c in picked)
        keep = np.ones(want.size, dtype=bool)
        for c in damaged:
            keep[int(sym_offs[c]):int(sym_offs[c]) + int(b.counts[c])] = False
        assert np.array_equal(got[keep], want[keep]), "an undamaged stream, the padding or the guard differs"
        assert np.all(got[int(sym_offs[far]):int(sym_offs[far]) + int(b.counts[far])] == POISON), "the stream with the bad sym_offset was written"
        assert np.all(got[int(sym_offs[-1]):] == POISON)


@pytest.mark.gpu
def test_batch_encode_rejects_bad_slots(gpu, oracle):
    """The slot index is data.  A slot that starts or ends off 16 bytes, is smaller than rans_amd_chunk_bound of its count,
    ends before it starts or ends beyond out_cap is not written: d_lengths[c] = 0, encode_status() reports E_SPACE, every
    other stream is the oracle's, and the poison in the rejected slots, between the slots and behind out_cap is intact."""
    R, ctx, torch = gpu
    for rid in ("word-64", "byte-2"):
        row = ROW[rid]
        ways = row["ways"]
        counts = draw_lengths(400, ways, 71)
        b = Batch(R, ctx, torch, oracle, row, counts)
        d_buf, sym_offs, _ = b.laid_out(4)
        bound = np.array([R.chunk_bound(row["fmt"], int(c), ways) for c in counts], dtype=np.int64)
        # every slot is 32 bytes larger than rans_amd_chunk_bound of its count: a stream ends at its slot's end, so the
        # head of every slot must stay poison
        sizes = bound + 32
        idx = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        cap = int(idx[-1])
        big = np.nonzero(counts >= 1000)[0]
        off16, past = int(big[0]), 399
        small = int(big[(big > off16 + 2) & (big < past - 1)][0])
        bad_idx = idx.copy()
        bad_idx[off16 + 1] += 8          # slot off16 ends off 16 bytes, and slot off16 + 1 starts there
        bad_idx[small] = bad_idx[small + 1] - (bound[small] - 16)  # slot `small` one granule too small (and slot small - 1 larger)
        rejected = {off16, off16 + 1, small}
        out_cap = cap - 16               # the last slot ends beyond out_cap
        rejected.add(past)
        assert len(rejected) == 4
        d_out = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
        cont, offs, lens = ctx.encode_batch(b.gm, d_buf, b.dev(sym_offs, np.int64), b.d_counts, ways, b.dev(bad_idx, np.int64), d_out=d_out,
                                            out_cap=out_cap)
        with pytest.raises(R.RansAmdError) as e:
            ctx.encode_status()
        assert e.value.status == R.E_SPACE
        h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy().view(np.uint32)
        for c in range(b.n):
            lo, hi = int(bad_idx[c]), int(bad_idx[c + 1])
            if c in rejected:
                assert h_lens[c] == 0, (rid, c)
                if hi > lo:
                    assert np.all(h[lo:hi] == POISON), (rid, "a rejected slot was written", c)
            else:
                ln = int(h_lens[c])
                assert ln == b.lens[c] and int(h_offs[c]) == hi - ln, (rid, c)
                assert np.array_equal(h[hi - ln:hi], b.streams[c]), (rid, "stream", c)
                # (below the stream only what a 16-byte flush may touch: the slack of the slot's first 16 bytes stays poison)
                assert np.all(h[lo:lo + 16] == POISON), (rid, "the head of a slot was written", c)
        assert np.all(h[cap:] == POISON), "written behind the container"


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [1, 33, 100000])
def test_batch_order(gpu, oracle, n_streams):
    R, ctx, torch = gpu
    counts = draw_lengths(n_streams, 64, 31)
    if n_streams == 33:
        counts = np.array([(1 << k) - 1 for k in range(33)], dtype=np.uint64).clip(0, 0xffffffff).astype(np.uint32)  # one per bucket
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    order = ctx.batch_order(d_counts).cpu().numpy().view(np.uint32)
    assert np.array_equal(np.sort(order), np.arange(n_streams, dtype=np.uint32)), "not a permutation"
    keys = ref_order_keys(counts[order])  # (in integers: no float log2 next to a power of two)
    assert np.all(np.diff(keys) <= 0), "bucket keys increase"
    if n_streams == 33:
        assert keys.tolist() == list(range(32, -1, -1))
        return
    # decode_batch with the order gives what it gives without
    small = counts.copy()
    if n_streams > 1000:
        small = np.minimum(counts, 2048)  # (10^5 streams: short ones, the order is what is under test)
    b = Batch(R, ctx, torch, oracle, ROW["word-64"], small)
    d_order = ctx.batch_order(b.d_counts)
    d_buf, sym_offs, slot_offs = b.laid_out(4)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 64, d_slot)
    ctx.encode_status()
    outs = []
    for o in (None, d_order):
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, cont, int(slot_offs[-1]), offs, lens, d_sym, b.d_counts, 64, out, d_order=o)
        outs.append(out)
    assert torch.equal(outs[0], d_buf) and torch.equal(outs[1], outs[0])


@pytest.mark.gpu
def test_batch_slice_ranges_decode_like_one_shot(gpu, oracle):
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW["byte-2"], draw_lengths(3000, 2, 41))
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 4, with_oracle_container=False)
    h_cont, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n]
    bounds = R.batch_slice(h_lens, 8)
    out = torch.full_like(d_buf, b.poison())
    for g in range(8):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        if lo == hi:
            continue
        bb, be, rebased = R.container_slice(h_offs, h_lens, lo, hi)
        piece = torch.zeros(be - bb + 16, dtype=torch.uint8, device="cuda")
        piece[:be - bb] = torch.from_numpy(h_cont[bb:be]).cuda()
        ctx.decode_batch(b.gm, piece, be - bb, b.dev(rebased[:hi - lo], np.int64), lens[lo:hi], d_sym[lo:hi], b.d_counts[lo:hi], 2, out,
                         n_streams=hi - lo)
    assert torch.equal(out, d_buf)
    sizes = [int(h_lens[int(bounds[g]):int(bounds[g + 1])].sum()) for g in range(8)]
    assert max(sizes) <= sum(sizes) / 8 + int(h_lens.max())


@pytest.mark.gpu
def test_batch_container_compact_then_decode(gpu, oracle):
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW["r64-2"], draw_lengths(2000, 2, 51))
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 1, with_oracle_container=False)
    c_cont, c_offs, c_total = ctx.compact(cont, int(slot_offs[-1]), offs, lens, b.n)
    assert c_total < int(slot_offs[-1])
    b.check_streams(c_cont.cpu().numpy(), c_offs.cpu().numpy()[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n], "compacted batch")
    out = torch.full_like(d_buf, b.poison())
    ctx.decode_batch(b.gm, c_cont, c_total, c_offs, lens, d_sym, b.d_counts, 2, out)
    assert torch.equal(out, d_buf)


_GRAPH_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import bench, ryg_rans_amd as R
from test_gpu_batch import draw_lengths, POISON
ctx = R.Context(0)
counts = draw_lengths(3000, 64, 61)
sym_offs, slot_offs = R.batch_layout(counts, R.FMT_WORD, 64, 4)
d_syms = bench.gen_zipf(torch, int(sym_offs[-1]), 256, 1.0, 1, "cuda")
freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, 256), 4096)
gm = ctx.model(R.FMT_WORD, freqs, 12)
d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda(); d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
cont, offs, lens = ctx.encode_batch(gm, d_syms, d_sym, d_counts, 64, d_slot)
ctx.encode_status()
want = torch.full_like(d_syms, POISON)
ctx.decode_batch(gm, cont, int(slot_offs[-1]), offs, lens, d_sym, d_counts, 64, want)   # (outside the capture first)
out = torch.full_like(d_syms, POISON)
s = torch.cuda.Stream()
g = torch.cuda.CUDAGraph()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        ctx.decode_batch(gm, cont, int(slot_offs[-1]), offs, lens, d_sym, d_counts, 64, out, sync=False)
for _ in range(3):
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "replay differs"
assert ctx.decode_errors() == 0 and ctx.last_decode_kernel() == "k_decode_batch_word64"
print("graph ok")
"""


@pytest.mark.gpu
def test_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch, replayed three times, in a child process under a time limit of its own.  Graph replay
    needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    import subprocess
    import sys
    q = os.environ.get("GPU_MAX_HW_QUEUES")
    if q is not None and int(q) < 4:
        pytest.skip("fewer than 4 hardware queues: captured graphs are not replayed here")
    script = tmp_path / "graph_batch.py"
    script.write_text(_GRAPH_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
