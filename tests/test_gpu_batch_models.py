"""Ragged batches with one model per stream on the GPU (rans_amd_encode_batch_adaptive / rans_amd_decode_batch_adaptive):
every stream's frequency row and bytes against the oracle, which builds the model of each stream from that stream alone
(Oracle.count_freqs + normalize + encode per stream, threaded over the host cores; the library never checks itself).

MODEL_ROWS: one row per shape, naming the kernels the library must report for it (tests/test_batch_models_host.py holds the
rows to the names the launchers can report).  Regimes U, H and R, the lengths and the poison rules are those of
tests/test_gpu_batch.py.  Input is bench.gen_zipf with seed 1, stream c's symbols rotated by (37 c) mod 256, so that the
rows differ from stream to stream; four more streams are always in: 4096 and 16384 symbols exactly (the sizes the uniform
encoder keeps register-resident: here they take the two-pass form), one value repeated 4 N + 3 times (word format: frequency
4096, a word leaves per symbol) and all 256 values once (at 8 bits every frequency is 1)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from _oracle import FMT_BYTE, FMT_WORD
from test_gpu_batch import GUARD, POISON, draw_lengths, mandatory_lengths, resident_waves


def _row(rid, fmt, sb, ways):
    f = "word" if fmt == FMT_WORD else "byte"
    return {"id": rid, "fmt": fmt, "sb": sb, "ways": ways, "decode": "k_decode_batch_models<%s>" % f,
            "encode": "k_encode_batch_models<%s>" % f}


MODEL_ROWS = [
    _row("word-64", FMT_WORD, 12, 64),
    _row("word-8", FMT_WORD, 12, 8),
    _row("word-128", FMT_WORD, 12, 128),
    _row("byte-64-12bit", FMT_BYTE, 12, 64),
    _row("byte-2-12bit", FMT_BYTE, 12, 2),
    _row("byte-64-8bit", FMT_BYTE, 8, 64),
]
ROW = {r["id"]: r for r in MODEL_ROWS}
UNIT = {FMT_BYTE: 1, FMT_WORD: 2}
ONE_VALUE = 201


def special_streams(ways):
    """(count, content) of the four streams every batch carries behind the drawn ones; content None = the rotated zipf symbols."""
    return [(4096, None), (16384, None), (4 * ways + 3, np.full(4 * ways + 3, ONE_VALUE, dtype=np.uint8)),
            (256, np.arange(256, dtype=np.uint8))]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


class ModelBatch:
    """The symbols of a batch, and the oracle's row and stream of every stream under the stream's own model."""

    def __init__(self, R, ctx, torch, oracle, row, counts, contents=None):
        import bench
        self.R, self.ctx, self.torch, self.row = R, ctx, torch, row
        self.counts = np.ascontiguousarray(counts, dtype=np.uint32)
        self.n = self.counts.size
        self.dense_offs = np.concatenate(([0], np.cumsum(self.counts.astype(np.int64))))
        total = int(self.dense_offs[-1])
        h = bench.gen_zipf(torch, max(total, 1), 256, 1.0, 1, "cuda")[:total].cpu().numpy()
        h = h + np.repeat(((37 * np.arange(self.n)) % 256).astype(np.uint8), self.counts)  # (u8: wraps modulo 256)
        for c, content in (contents or {}).items():
            assert content.size == self.counts[c]
            h[self.dense_offs[c]:self.dense_offs[c + 1]] = content
        self.h_dense = h
        self.d_dense = torch.from_numpy(h).cuda()
        self.d_counts = torch.from_numpy(self.counts.view(np.int32)).cuda()
        fmt, sb, ways, offs = row["fmt"], row["sb"], row["ways"], self.dense_offs
        any_model = oracle.model(np.full(256, (1 << sb) // 256, dtype=np.uint32), sb)  # (an empty stream looks nothing up)

        def run(c):
            syms = h[offs[c]:offs[c + 1]]
            if syms.size == 0:
                return np.zeros(256, dtype=np.uint16), oracle.encode(fmt, any_model, syms, ways)
            f, _ = oracle.normalize(oracle.count_freqs(syms, 256), 1 << sb)
            return f.astype(np.uint16), oracle.encode(fmt, oracle.model(f, sb), syms, ways)
        with ThreadPoolExecutor(oracle.host_threads()) as ex:
            done = list(ex.map(run, range(self.n), chunksize=64))
        self.rows = np.stack([d[0] for d in done]) if self.n else np.zeros((0, 256), np.uint16)
        self.streams = [d[1] for d in done]
        self.lens = np.array([s.size for s in self.streams], dtype=np.uint32)
        self.bound = R.encode_batch_adaptive_bound(fmt, self.counts, ways)

    def laid_out(self, align):
        """-> (d_buf, sym_offs): the symbols at batch_layout's offsets in a poison-filled buffer with a guard behind them."""
        torch = self.torch
        sym_offs, _ = self.R.batch_layout(self.counts, self.row["fmt"], self.row["ways"], align)
        d_buf = torch.full((int(sym_offs[-1]) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        if self.d_dense.numel():
            shift = torch.from_numpy(sym_offs[:-1].astype(np.int64) - self.dense_offs[:-1]).cuda()
            idx = torch.arange(self.d_dense.numel(), device="cuda") + torch.repeat_interleave(shift, self.d_counts.to(torch.int64))
            d_buf[idx] = self.d_dense
        return d_buf, sym_offs

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()

    def d_rows(self, rows=None):
        return self.torch.from_numpy(np.ascontiguousarray(self.rows if rows is None else rows).view(np.int16).reshape(-1)).cuda()

    def encode(self, d_buf, d_sym, cap=None):
        """One encode_batch_adaptive into a poison-filled buffer of bound + 4096 bytes -> host (cont, offs[n + 1], lens, rows, total)
        and the device tensors."""
        torch, row = self.torch, self.row
        d_out = torch.full((self.bound + 4096,), POISON, dtype=torch.uint8, device="cuda")
        t = self.ctx.encode_batch_adaptive(d_buf, d_sym, self.d_counts, row["ways"], row["sb"], fmt=row["fmt"], d_out=d_out,
                                           cap=self.bound if cap is None else cap)
        cont, offs, lens, rows, total = t
        return (cont.cpu().numpy(), offs.cpu().numpy().astype(np.uint64), lens.cpu().numpy().view(np.uint32)[:self.n],
                rows.cpu().numpy().view(np.uint16).reshape(-1, 256)[:self.n], total), t

    def decode(self, cont, cbytes, offs, lens, d_rows, d_sym, out, **kw):
        row = self.row
        return self.ctx.decode_batch_adaptive(cont, cbytes, offs, lens, d_rows, d_sym, self.d_counts, row["ways"], row["sb"], out,
                                              fmt=row["fmt"], **kw)

    def oracle_container(self, seed=5):
        """The oracle's streams in a shuffled order at unit-aligned offsets with small gaps -> (cont, starts, bytes)."""
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

    def check_encoded(self, h, what):
        """Rows, streams and the layout of one encode (host arrays of ModelBatch.encode) against the oracle."""
        cont, offs, lens, rows, total = h
        assert np.array_equal(rows, self.rows), (what, "rows differ from the oracle's", np.nonzero((rows != self.rows).any(axis=1))[0][:8])
        assert np.array_equal(lens, self.lens), (what, "lengths differ from the oracle's", np.nonzero(lens != self.lens)[0][:8])
        ends = offs[:self.n] + lens
        assert np.all(ends % 64 == 0), (what, "a stream does not end on a line")
        starts = np.concatenate(([0], ends[:-1])).astype(np.uint64)  # piece c lies behind piece c - 1
        assert np.all(offs[:self.n] >= starts) and np.all(np.diff(ends.astype(np.int64)) > 0), (what, "pieces out of order or overlapping")
        assert int(offs[self.n]) == int(ends[-1]) == total <= self.bound, (what, "bytes in use", int(offs[self.n]), total, self.bound)
        assert np.all(cont[total:] == POISON), (what, "written behind the bytes in use")
        for c in range(self.n):
            a = int(offs[c])
            assert np.array_equal(cont[a:a + int(lens[c])], self.streams[c]), (what, "stream", c, "count", int(self.counts[c]))


def run_row(b, align):
    ctx, torch, row = b.ctx, b.torch, b.row
    d_buf, sym_offs = b.laid_out(align)
    d_sym = b.dev(sym_offs, np.int64)
    what = "%s align %d" % (row["id"], align)
    # 1. rows, streams, layout
    h, (cont, offs, lens, rows, total) = b.encode(d_buf, d_sym)
    assert ctx.last_encode_kernel()[0] == row["encode"], ctx.last_encode_kernel()
    b.check_encoded(h, what)
    # 2. the same layout from run to run
    h2, _ = b.encode(d_buf, d_sym)
    assert np.array_equal(h2[1], h[1]) and np.array_equal(h2[2], h[2]) and h2[4] == h[4], (what, "layout differs between two runs")
    # 3. decode of the GPU's own container
    out = torch.full_like(d_buf, POISON)
    b.decode(cont, total, offs, lens, rows, d_sym, out)
    assert ctx.last_decode_kernel() == row["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_buf), (what, "decode of the GPU's container")
    # 4. decode of a batch the oracle made: shuffled, unit-aligned offsets with gaps, the oracle's rows
    o_cont, o_starts, o_bytes = b.oracle_container()
    out = torch.full_like(d_buf, POISON)
    b.decode(b.dev(o_cont, np.uint8), o_bytes, b.dev(o_starts, np.int64), b.dev(b.lens, np.int32), b.d_rows(), d_sym, out)
    assert ctx.last_decode_kernel() == row["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_buf), (what, "decode of the oracle's container")


def with_specials(counts, ways):
    sp = special_streams(ways)
    all_counts = np.concatenate((counts, np.array([s[0] for s in sp], dtype=np.uint32)))
    return all_counts, {counts.size + i: s[1] for i, s in enumerate(sp) if s[1] is not None}


def _cases():
    for r in MODEL_ROWS:
        for regime in ("U", "H", "R"):
            yield pytest.param(r, regime, id="%s-%s" % (r["id"], regime), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,regime", list(_cases()))
def test_models_row_every_stream_equals_oracle(gpu, oracle, row, regime):
    R, ctx, torch = gpu
    resident = resident_waves(torch)
    ways = row["ways"]
    if regime == "U":  # one stream per launch
        batches = [(np.array([ln], dtype=np.uint32), None) for ln in mandatory_lengths(ways)]
        batches += [(np.array([s[0]], dtype=np.uint32), None if s[1] is None else {0: s[1]}) for s in special_streams(ways)]
    else:
        n_streams = resident // 2 if regime == "H" else 4 * resident
        drawn = draw_lengths(n_streams - 4, ways, 7)
        assert set(mandatory_lengths(ways)) <= set(drawn.tolist())
        batches = [with_specials(drawn, ways)]
        assert (0 < batches[0][0].size < resident) if regime == "H" else batches[0][0].size >= 4 * resident
    for counts, contents in batches:
        b = ModelBatch(R, ctx, torch, oracle, row, counts, contents)
        if b.n > 1:  # (a shared-model shortcut cannot pass)
            nonempty = b.rows[b.counts > 0]
            assert np.unique(nonempty, axis=0).shape[0] >= 2, "the streams' rows do not differ"
        for align in (1, 4):
            run_row(b, align)
        assert ctx.decode_errors() == 0


def test_the_oracle_takes_the_required_shapes(oracle):
    """No GPU: the checker itself on the shapes the batches must hold -- a one-symbol stream (word 8-way: 32 bytes of states
    and one word), one value repeated, all 256 values once, N - 1 symbols, an empty stream -- encode and decode again."""
    for fmt, sb in ((FMT_WORD, 12), (FMT_BYTE, 12), (FMT_BYTE, 8)):
        for ways in (2, 8, 64, 128):
            shapes = [np.array([7], np.uint8), np.full(ways + 1, 9, np.uint8), np.full(4 * ways + 3, 9, np.uint8),
                      np.arange(256, dtype=np.uint8), (np.arange(ways - 1) * 37 % 256).astype(np.uint8)]
            for syms in shapes:
                om = oracle.model_for(syms, 256, sb)
                stream = oracle.encode(fmt, om, syms, ways)
                assert np.array_equal(oracle.decode(fmt, om, stream, syms.size, ways), syms)
                if fmt == FMT_WORD and syms.size == 1:
                    assert stream.size == 4 * ways + 2
            assert oracle.encode(fmt, om, np.zeros(0, np.uint8), ways).size == 4 * ways


@pytest.mark.gpu
def test_models_large_word8(gpu, oracle):
    """2 x 10^4 streams of the reference's 8-way word layout, sym_align = 4, every stream against the oracle."""
    R, ctx, torch = gpu
    row = ROW["word-8"]
    counts, contents = with_specials(draw_lengths(20000, 8, 13), 8)
    b = ModelBatch(R, ctx, torch, oracle, row, counts, contents)
    run_row(b, 4)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_models_damage_is_counted_and_contained(gpu, oracle):
    """A flipped byte in the flushed states of five streams, one row whose sum is off by one, one sym_offset past out_syms:
    E_CORRUPT with bad_streams exactly seven; every other stream, the padding and the guard are intact; a stream of 0
    symbols whose row is garbage still decodes (its row is neither read nor validated)."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(600, 64, 21))
    for align in (1, 4):
        d_buf, sym_offs = b.laid_out(align)
        d_sym = b.dev(sym_offs, np.int64)
        h, (cont, offs, lens, rows, total) = b.encode(d_buf, d_sym)
        rng = np.random.default_rng(3)
        # (a flipped byte is only certain to be noticed where symbols depend on it: streams of at least 4 N + 3 symbols)
        long_ones = np.nonzero(b.counts >= 4 * 64 + 3)[0]
        picked = rng.choice(long_ones, 7, replace=False)
        flipped, bad_row, far = picked[:5], int(picked[5]), int(picked[6])
        empty = np.nonzero(b.counts == 0)[0]
        assert empty.size >= 1
        bad_cont = cont.clone()
        for c in flipped:
            bad_cont[int(h[1][c]) + 1] ^= 0x40
        bad_rows = h[3].copy()
        bad_rows[bad_row, int(np.argmax(bad_rows[bad_row]))] += 1  # the sum is 4097
        bad_rows[int(empty[0])] = 0xA5A5                           # garbage where nothing is read
        bad_sym = d_sym.clone()
        bad_sym[far] = d_buf.numel() - int(b.counts[far]) + 1      # one symbol past the end
        out = torch.full_like(d_buf, POISON)
        with pytest.raises(R.RansAmdError) as e:
            b.decode(bad_cont, total, offs, lens, b.d_rows(bad_rows), bad_sym, out)
        assert e.value.status == R.E_CORRUPT
        assert e.value.bad_streams == 7, "h_bad_streams as the call wrote it"
        assert ctx.decode_errors() == 0  # (reported and reset by that call)
        got, want = out.cpu().numpy(), d_buf.cpu().numpy()
        keep = np.ones(want.size, dtype=bool)
        for c in picked:
            keep[int(sym_offs[c]):int(sym_offs[c]) + int(b.counts[c])] = False
        assert np.array_equal(got[keep], want[keep]), "an undamaged stream, the padding or the guard differs"
        assert np.all(got[int(sym_offs[far]):int(sym_offs[far]) + int(b.counts[far])] == POISON), "the stream with the bad sym_offset was written"
        assert np.all(got[int(sym_offs[bad_row]):int(sym_offs[bad_row]) + int(b.counts[bad_row])] == POISON), "the stream with the bad row was written"
        assert np.all(got[int(sym_offs[-1]):] == POISON)
        # the garbage row alone is no damage
        ok_rows = h[3].copy()
        ok_rows[int(empty[0])] = 0xA5A5
        out = torch.full_like(d_buf, POISON)
        b.decode(cont, total, offs, lens, b.d_rows(ok_rows), d_sym, out)
        assert torch.equal(out, d_buf)


@pytest.mark.gpu
def test_models_encode_without_room(gpu, oracle):
    """out_cap one line short of what the batch uses: E_SPACE, the streams that fit are the oracle's, the lengths of the
    others are 0, nothing at or behind out_cap is written.  And a symbol range outside [0, in_syms) is not read: E_ARG."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(300, 64, 71))
    d_buf, sym_offs = b.laid_out(4)
    d_sym = b.dev(sym_offs, np.int64)
    h, _ = b.encode(d_buf, d_sym)
    used = h[4]
    cap = used - 64
    d_out = torch.full((b.bound + 4096,), POISON, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda")
    d_lens = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    d_freqs = torch.zeros(b.n * 256, dtype=torch.int16, device="cuda")
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_batch_adaptive(d_buf, d_sym, b.d_counts, 64, 12, fmt=FMT_WORD, d_out=d_out, cap=cap, d_offsets=d_offs,
                                  d_lengths=d_lens, d_freqs=d_freqs)
    assert e.value.status == R.E_SPACE
    cont, offs, lens = d_out.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32)
    ends = h[1][:b.n] + h[2]  # (the layout does not depend on the capacity)
    fits = ends <= cap
    assert 0 < np.count_nonzero(~fits) < b.n
    for c in range(b.n):
        if fits[c]:
            assert lens[c] == b.lens[c] and offs[c] == h[1][c], c
            assert np.array_equal(cont[int(offs[c]):int(offs[c]) + int(lens[c])], b.streams[c]), c
        else:
            assert lens[c] == 0, c
    assert np.all(cont[cap:] == POISON), "written at or behind out_cap"
    # the symbol index is data: the last stream pushed one symbol past in_syms
    bad_sym = d_sym.clone()
    last = int(np.nonzero(b.counts > 0)[0][-1])
    bad_sym[last] = d_buf.numel() - int(b.counts[last]) + 1
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_batch_adaptive(d_buf, bad_sym, b.d_counts, 64, 12, fmt=FMT_WORD)
    assert e.value.status == R.E_ARG


@pytest.mark.gpu
def test_models_decode_order(gpu, oracle):
    """decode_batch_adaptive with rans_amd_batch_order's permutation gives what it gives without: the row index is the stream
    index after the order."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(3000, 64, 31))
    d_buf, sym_offs = b.laid_out(4)
    d_sym = b.dev(sym_offs, np.int64)
    _, (cont, offs, lens, rows, total) = b.encode(d_buf, d_sym)
    d_order = ctx.batch_order(b.d_counts)
    assert not np.array_equal(d_order.cpu().numpy(), np.arange(b.n))
    outs = []
    for o in (None, d_order):
        out = torch.full_like(d_buf, POISON)
        b.decode(cont, total, offs, lens, rows, d_sym, out, d_order=o)
        outs.append(out)
    assert torch.equal(outs[0], d_buf) and torch.equal(outs[1], outs[0])


_GRAPH_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import bench, ryg_rans_amd as R
from test_gpu_batch import draw_lengths, POISON
ctx = R.Context(0)
counts = draw_lengths(3000, 64, 61)
sym_offs, _ = R.batch_layout(counts, R.FMT_WORD, 64, 4)
d_syms = bench.gen_zipf(torch, int(sym_offs[-1]), 256, 1.0, 1, "cuda")
d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
cont, offs, lens, rows, total = ctx.encode_batch_adaptive(d_syms, d_sym, d_counts, 64, 12, fmt=R.FMT_WORD)
want = torch.full_like(d_syms, POISON)
ctx.decode_batch_adaptive(cont, total, offs, lens, rows, d_sym, d_counts, 64, 12, want, fmt=R.FMT_WORD)   # (outside the capture first)
ref = torch.full_like(d_syms, POISON)
for c in range(counts.size):
    a = int(sym_offs[c]); ref[a:a + int(counts[c])] = d_syms[a:a + int(counts[c])]
assert torch.equal(want, ref), "eager decode differs from the input"
out = torch.full_like(d_syms, POISON)
s = torch.cuda.Stream()
g = torch.cuda.CUDAGraph()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        ctx.decode_batch_adaptive(cont, total, offs, lens, rows, d_sym, d_counts, 64, 12, out, fmt=R.FMT_WORD, sync=False)
for _ in range(3):
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "replay differs"
assert ctx.decode_errors() == 0 and ctx.last_decode_kernel() == "k_decode_batch_models<word>"
print("graph ok")
"""


@pytest.mark.gpu
def test_models_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch_adaptive, replayed three times, in a child process under a time limit of its own.  Graph
    replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    import subprocess
    import sys
    q = os.environ.get("GPU_MAX_HW_QUEUES")
    if q is not None and int(q) < 4:
        pytest.skip("fewer than 4 hardware queues: captured graphs are not replayed here")
    script = tmp_path / "graph_batch_models.py"
    script.write_text(_GRAPH_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
