"""The ragged-batch harness the GPU files and their host files share: lengths, the batches with the oracle's stream of every
stream (Batch, ModelBatch, PoolBatch), the row runners, the rate inputs whose bounds the host files prove, and the child
programs of the captured-graph tests.

Lengths are drawn log-uniform from [0, 64 Ki] (fixed seed) and always include 0, 1, N-1, N, N+1, 4N+3 and 65536.  Input is
bench.gen_zipf; the checker is the CPU oracle (Oracle.encode per stream, threaded over the host cores), never the library
itself.  Output buffers are filled with a poison value first: the padding between streams and a guard region behind the last
one must come back untouched."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _stream_rate as S
from _kernel_rows import ROW
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

WAVES_PER_BLOCK = 16  # kDecBlockThreads / 64: no launcher uses a larger block
GUARD = 4096  # symbols behind the last stream
POISON = 0xA5
MAX_LEN = 65536
UNIT = {FMT_BYTE: 1, FMT_ALIAS: 1, FMT_WORD: 2, FMT_R64: 4}
POOL = 4096  # prototypes of the half and several batches of the pair kernels, each coded once by the oracle


def mandatory_lengths(ways):
    return [0, 1, ways - 1, ways, ways + 1, 4 * ways + 3, MAX_LEN]


def _log_uniform(rng, n_streams, max_len):
    return (np.exp(rng.random(n_streams) * np.log(max_len + 1.0)) - 1.0).astype(np.int64).clip(0, max_len).astype(np.uint32)


def draw_log_uniform(n_streams, max_len, seed):
    """Log-uniform in [0, max_len]."""
    return _log_uniform(np.random.default_rng(seed), n_streams, max_len)


def draw_lengths(n_streams, ways, seed):
    """Log-uniform in [0, 64 Ki]; the mandatory lengths at fixed-seed positions (all of them from seven streams on)."""
    rng = np.random.default_rng(seed)
    c = _log_uniform(rng, n_streams, MAX_LEN)
    must = mandatory_lengths(ways)
    if n_streams >= len(must):
        c[rng.choice(n_streams, len(must), replace=False)] = must
    return c


def edge_counts(seed, n=300):
    """n log-uniform counts up to 64 Ki, the first seven at the edges: what the host tests of the layout and bound functions take."""
    rng = np.random.default_rng(seed)
    c = (np.exp(rng.random(n) * np.log(65537.0)) - 1).astype(np.uint32)
    c[:7] = (0, 1, 63, 64, 65, 259, 65536)
    return c


def resident_waves(torch):
    """CUs x 2 blocks x 16 waves: an upper bound of the resident waves of every kernel."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * WAVES_PER_BLOCK


class _Laid:
    """What Batch and ModelBatch share: R, torch, row, counts, n, dense_offs, d_dense, d_counts, lens and streams are theirs."""

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()

    def _lay(self, sym_offs, poison):
        """The symbols at sym_offs in a poison-filled buffer with a guard behind them."""
        torch = self.torch
        d_buf = torch.full((int(sym_offs[-1]) + GUARD,), poison, dtype=self.d_dense.dtype, device="cuda")
        if self.d_dense.numel():
            shift = torch.from_numpy(sym_offs[:-1].astype(np.int64) - self.dense_offs[:-1]).cuda()
            idx = torch.arange(self.d_dense.numel(), device="cuda") + torch.repeat_interleave(shift, self.d_counts.to(torch.int64))
            d_buf[idx] = self.d_dense
        return d_buf

    def oracle_container(self, seed=5):
        """The oracle's streams concatenated in a shuffled order at unit-aligned offsets with small gaps -> (cont, starts, bytes)."""
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


class Batch(_Laid):
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
        sym_offs, slot_offs = self.R.batch_layout(self.counts, self.row["fmt"], self.row["ways"], align)
        return self._lay(sym_offs, self.poison()), sym_offs, slot_offs

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


class Coded:
    """A batch laid out, coded by the GPU and concatenated by the oracle: what the order and damage tests decode."""

    def __init__(self, b, align):
        self.b = b
        self.d_buf, self.sym_offs, self.slot_offs = b.laid_out(align)
        self.d_sym, d_slot = b.dev(self.sym_offs, np.int64), b.dev(self.slot_offs, np.int64)
        self.cont, self.offs, self.lens = b.ctx.encode_batch(b.gm, self.d_buf, self.d_sym, b.d_counts, b.row["ways"], d_slot)
        b.ctx.encode_status()
        o_cont, o_starts, self.o_bytes = b.oracle_container()
        self.o_cont, self.o_offs, self.o_lens = b.dev(o_cont, np.uint8), b.dev(o_starts, np.int64), b.dev(b.lens, np.int32)

    def containers(self):
        yield "gpu", self.cont, int(self.slot_offs[-1]), self.offs, self.lens
        yield "oracle", self.o_cont, self.o_bytes, self.o_offs, self.o_lens

    def decode_all(self, d_order, what):
        """Both containers into poison-filled buffers; each must equal the laid-out input, padding and guard included."""
        b = self.b
        for name, cont, nbytes, offs, lens in self.containers():
            out = b.torch.full_like(self.d_buf, b.poison())
            b.ctx.decode_batch(b.gm, cont, nbytes, offs, lens, self.d_sym, b.d_counts, b.row["ways"], out, d_order=d_order)
            assert b.ctx.last_decode_kernel() == b.row["decode"], b.ctx.last_decode_kernel()
            assert b.torch.equal(out, self.d_buf), (what, name)


class PoolBatch:
    """n streams, each one of at most POOL prototypes: the oracle codes every prototype once, the batch (index, container,
    expected output) is put together from them on the device.  The container is the oracle's -- the prototypes' streams in a
    shuffled order at 1-byte-aligned offsets with gaps, every stream of the batch pointing at its prototype's.  The symbols are
    laid out at sym_align = `align`."""

    def __init__(self, R, ctx, torch, oracle, row, proto_counts, n, seed, align=4):
        import bench
        self.R, self.torch = R, torch
        pc = np.ascontiguousarray(proto_counts, dtype=np.uint32)
        p_offs = np.concatenate(([0], np.cumsum(pc.astype(np.int64))))
        d_proto = bench.gen_zipf(torch, int(p_offs[-1]), row["K"], 1.0, 3, "cuda")
        sample = bench.gen_zipf(torch, 1 << 20, row["K"], 1.0, 3, "cuda")
        freqs, _ = R.normalize_freqs(ctx.count_freqs_device(sample, row["K"]), 1 << row["sb"])
        self.gm = ctx.model(row["fmt"], freqs, row["sb"])
        om = oracle.model(freqs, row["sb"])
        h = d_proto.cpu().numpy()
        with ThreadPoolExecutor(oracle.host_threads()) as ex:
            streams = list(ex.map(lambda c: oracle.encode(row["fmt"], om, h[p_offs[c]:p_offs[c + 1]], 2), range(pc.size), chunksize=64))
        p_lens = np.array([s.size for s in streams], dtype=np.int64)
        rng = np.random.default_rng(seed)
        gaps = rng.integers(0, 4, pc.size).astype(np.int64)
        p_starts = np.zeros(pc.size, dtype=np.int64)
        at = 1
        for k, c in enumerate(rng.permutation(pc.size)):
            at += int(gaps[k])
            p_starts[c] = at
            at += int(p_lens[c])
        cont = np.zeros(at + 16, dtype=np.uint8)
        for c, s in enumerate(streams):
            cont[p_starts[c]:p_starts[c] + s.size] = s
        self.cont, self.cont_bytes = torch.from_numpy(cont).cuda(), at
        # the batch: the first prototypes once each (every prototype length occurs), the rest drawn
        pick = np.concatenate((np.arange(min(pc.size, n)), rng.integers(0, pc.size, max(0, n - pc.size))))
        pick = pick[rng.permutation(pick.size)]
        self.counts = pc[pick]
        self.sym_offs, self.slot_offs = R.batch_layout(self.counts, row["fmt"], 2, align)

        def dev(a, t):
            return torch.from_numpy(np.ascontiguousarray(a).astype(t)).cuda()
        self.d_counts, self.d_sym = dev(self.counts.view(np.int32), np.int32), dev(self.sym_offs, np.int64)
        self.d_offs, self.d_lens = dev(p_starts[pick], np.int64), dev(p_lens[pick], np.int32)
        self.d_slot = dev(self.slot_offs, np.int64)
        self.d_buf = torch.full((int(self.sym_offs[-1]) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        reps = self.d_counts.to(torch.int64)
        total = int(reps.sum())
        within = torch.arange(total, device="cuda") - torch.repeat_interleave(torch.cumsum(reps, 0) - reps, reps)
        self.d_buf[torch.repeat_interleave(self.d_sym[:-1], reps) + within] = d_proto[torch.repeat_interleave(dev(p_offs[pick], np.int64), reps) + within]


# ---- one model per stream ---------------------------------------------------------------------------------------------
class ModelBatch(_Laid):
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
        sym_offs, _ = self.R.batch_layout(self.counts, self.row["fmt"], self.row["ways"], align)
        return self._lay(sym_offs, POISON), sym_offs

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


def run_model_row(b, align):
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


# ---- two results of the batch encoders ----------------------------------------------------------------------------------
def stream_mask(torch, n_bytes, offs, lens, n):
    """True for the bytes of [offs[c], offs[c] + lens[c]), c < n."""
    d = torch.zeros(n_bytes + 1, dtype=torch.int32, device="cuda")
    o, ln = offs[:n].to(torch.int64), lens[:n].to(torch.int64)
    d.index_add_(0, o, torch.ones(n, dtype=torch.int32, device="cuda"))
    d.index_add_(0, o + ln, torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    return torch.cumsum(d[:n_bytes], 0) > 0


def same_result(torch, a, b, n, what):
    """Two (container, offsets, lengths) results: equal index entries, equal stream bytes."""
    assert torch.equal(a[1][:n], b[1][:n]) and torch.equal(a[2][:n], b[2][:n]), (what, "index entries differ")
    m = stream_mask(torch, a[0].numel(), a[1], a[2], n)
    assert torch.equal(a[0][m], b[0][m]), (what, "stream bytes differ")


def encode_poisoned(b, cx, gm, d_buf, d_sym, d_slot, cap, d_order=None, sentinel=None):
    """encode_batch into a poison-filled container with 4096 guard bytes behind `cap`; sentinel: pre-filled index entries."""
    torch = b.torch
    d_out = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
    d_offs = torch.full((b.n,), 0 if sentinel is None else sentinel, dtype=torch.int64, device="cuda")
    d_lens = torch.full((b.n,), 0 if sentinel is None else sentinel, dtype=torch.int32, device="cuda")
    return cx.encode_batch(gm, d_buf, d_sym, b.d_counts, b.row["ways"], d_slot, d_out=d_out, d_offsets=d_offs, d_lengths=d_lens,
                           out_cap=cap, d_order=d_order)


# ---- rate inputs of the word-group batch encoder (tests/test_batch_encode_groups_host.py proves their bounds) ------------------
def finish_octet():
    """Counts 128 k, k = 1..8, bursts under 3841 + 255 x 1: every stream BEGINS with a run of 64 rare symbols -- the last the
    coder sees --, so a finished group's state is large, and the common symbol (byte value 0, what a dead group is fed)
    pushes it over its threshold: the dead group's lanes write into its ring while the others run on."""
    freqs = S.rate_model()
    counts = np.array([128 * k for k in range(1, 9)], dtype=np.uint32)
    return freqs, counts, {g: S.bursts(freqs, int(counts[g]), 40 + g) for g in range(8)}


RATE_OCTET_KINDS = ("quiet", "rare+0", "bursts", "rare+1", "quiet", "bursts", "rare+2", "rare+0")
RATE_OCTET_COUNTS = (12288, 128 * 9 + 77, 1500, 128 * 20, 9001, 333, 641, 12288)


def rate_octet():
    """One wave under 4065 + 16 + 15 x 1: rare-only streams (96 bytes in every eight rounds: a block per check), quiet
    streams (common-only: no block for a thousand rounds and more, then only the states) and bursts, at different lengths
    -> (freqs, counts, {group: symbols})."""
    freqs = S.quiet_model()
    contents = {}
    for g, (kind, n) in enumerate(zip(RATE_OCTET_KINDS, RATE_OCTET_COUNTS)):
        if kind == "quiet":
            contents[g] = S.common_only(freqs, n)
        elif kind == "bursts":
            contents[g] = S.bursts(freqs, n, 60 + g, lead=8 * g)
        else:
            contents[g] = S.rare_only(freqs, n, 60 + g, shift=int(kind[5:]))
    return freqs, np.array(RATE_OCTET_COUNTS, dtype=np.uint32), contents


def no_zero_model(sb):
    """Byte value 0 has no record (frequency 0), every other value has: 2^sb - 254 and 254 x 1.  dense256 is false: TRACK."""
    f = np.ones(256, dtype=np.uint32)
    f[0] = 0
    f[1] = (1 << sb) - 254
    return f


def no_zero_batch(sb, n_streams, empty=()):
    """n_streams streams of uneven counts -- the first and those of `empty` are 0 --, drawn from no_zero_model(sb): the wave's
    groups or pairs die at different times, some from the start (NO_ZERO_OCTETS: three octets at 12 bits;
    NO_ZERO_WAVE_LOADS: three wave-loads at 14 bits)."""
    freqs = no_zero_model(sb)
    counts = np.array([(37 * k * k + 11 * k) % 1500 for k in range(n_streams)], dtype=np.uint32)
    counts[list(empty)] = 0
    return freqs, counts, {k: S.drawn(freqs, int(counts[k]), 80 + k) for k in range(n_streams)}


NO_ZERO_OCTETS, NO_ZERO_WAVE_LOADS = (12, 24, (5,)), (14, 96)  # the word-group encoder's no_zero_batch and the byte-pair encoder's


# ---- rate x phase x parking of the byte-pair batch kernels (tests/test_batch_pairs_host.py, test_batch_encode_pairs_host.py) ---
RATE_BITS = (16, 14)
RATE_STREAMS = 64
RATE_COUNTS = tuple(128 * b + t for b in (0, 1, 5) for t in (0, 1, 77, 127))


def rate_model(sb):
    """255 symbols of frequency 1 and one common symbol (tests/test_gpu_rate_extremes.py b_case's byte model)."""
    freqs = np.ones(256, dtype=np.uint32)
    freqs[S.COMMON] = (1 << sb) - 255
    return freqs


def rate_kind(k):
    return "common" if k % 3 == 2 else "rare"


def rate_count(k):
    """Every count meets both kinds, lines in different quad positions: 12 counts against the period 3 of the kinds."""
    return RATE_COUNTS[(5 * k + k // 12) % len(RATE_COUNTS)]


def rate_content(freqs, kind, n, seed):
    return S.common_only(freqs, n) if kind == "common" else S.rare_only(freqs, n, seed)


def rate_batch(sb):
    """-> (freqs, counts, {stream: symbols}, phases): stream k at offset == k (mod 64), every start phase of the 32-byte blocks
    and of the 64-byte ring."""
    freqs = rate_model(sb)
    counts = np.array([rate_count(k) for k in range(RATE_STREAMS)], dtype=np.uint32)
    contents = {k: rate_content(freqs, rate_kind(k), int(counts[k]), 800 + k) for k in range(RATE_STREAMS)}
    return freqs, counts, contents, list(range(RATE_STREAMS))


# one wave-load each: a pair at the ring's bound for 512 lines beside parked ones, and a cursor that stands still for a
# thousand rounds and more beside pairs that drain and park one after the other
RATE_WAVES = {
    "fast-beside-parked": ([65536] + [255] * 31, ["rare"] + ["common"] * 31),
    "stalled-beside-draining": ([65536] + [128 * (g % 8 + 1) for g in range(31)], ["common"] + ["rare"] * 31),
}


def rate_wave(sb, name):
    freqs = rate_model(sb)
    counts, kinds = RATE_WAVES[name]
    contents = {k: rate_content(freqs, kinds[k], counts[k], 900 + k) for k in range(32)}
    return freqs, np.array(counts, dtype=np.uint32), contents, [(21 * k + 5) % 64 for k in range(32)]


def mirrored_model():
    """255 x 1 and one common symbol at 2^16, the common one LAST: byte value 0 -- what a dead pair is fed -- has frequency 1."""
    f = np.ones(256, dtype=np.uint32)
    f[255] = (1 << 16) - 255
    return f


def finish_batch():
    """One wave-load under the mirrored model, counts 128 (g % 8 + 1): whole pieces only, every pair finishes at a piece
    boundary while others run on.  Every stream BEGINS with 64 frequency-1 symbols other than 0 -- the last the coder sees --
    and holds no 0; runs of 64 frequency-1 and 64 common symbols in turn.  A dead pair is fed zeros: two bytes per lane and
    round, 32 bytes per eight rounds, the ring's bound -> (freqs, counts, {stream: symbols})."""
    freqs = mirrored_model()
    counts = np.array([128 * (g % 8 + 1) for g in range(32)], dtype=np.uint32)
    contents = {}
    for g in range(32):
        n = int(counts[g])
        c = np.random.default_rng(40 + g).integers(1, 255, n).astype(np.uint8)
        c[(np.arange(n) // 64) % 2 == 1] = 255
        contents[g] = c
    return freqs, counts, contents


# ---- what the five streams-per-wave families' GPU files share: d is the family's descriptor (tests/_kernel_rows.py), gpu the
# ---- (R, ctx, torch, off) of option_contexts ------------------------------------------------------------------------------
def option_contexts(option):
    """The `gpu` fixture's body: a context with `option` on (only that option) and one with everything at its default, the
    wave-per-stream kernels."""
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    ctx.set_option(option, 1)
    off = R.Context(0)
    yield R, ctx, torch, off
    off.close()
    ctx.close()


def padded(n, lengths, pad=200):
    return list(lengths) + [pad] * (n - len(lengths))


def wave_load_cases(loads, rows, few):
    """Every row at the first wave-load, the rows `few` at the others."""
    import pytest
    for k, name in enumerate(loads):
        for row in (few if k else rows):
            yield pytest.param(name, row, id="%s-%s" % (name, row["id"]), marks=pytest.mark.gpu)


def _wave_row(d):
    """The main row's shape with the option off."""
    return dict(d.main, **{d.side: d.wave_kernel})


def check_option_takes_zero_or_one(gpu, oracle, d, align=4):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the family's -> the batch."""
    import pytest
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, d.main, np.array([300] * (d.streams + 1), dtype=np.uint32))
    for bad in (2, -1):
        with pytest.raises(R.RansAmdError) as e:
            ctx.set_option(d.option, bad)
        assert e.value.status == R.E_ARG
    run_row(b, align)
    ctx.set_option(d.option, 0)
    try:
        run_row(Batch(R, ctx, torch, oracle, _wave_row(d), b.counts), align)
    finally:
        ctx.set_option(d.option, 1)
    run_row(b, align)
    return b


def check_other_shape_keeps_its_kernels(gpu, oracle, d, rid, n_streams):
    R, ctx, torch, _ = gpu
    row = ROW[rid]
    assert row[d.side] != d.main[d.side]
    b = Batch(R, ctx, torch, oracle, row, draw_lengths(n_streams, row["ways"], 29))
    run_row(b, 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


def run_family_graph(tmp_path, d, name):
    fmt, sb, option = d.graph
    script = graph_decode_script(d.main["decode"], fmt=fmt, ways=d.ways, sb=sb, option=option) if d.side == "decode" else \
        graph_encode_script(d.main["encode"], fmt, d.ways, sb, option)
    run_graph_script(tmp_path, name, script)


def check_decode_order(gpu, oracle, d, n, aligns):
    import pytest
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, d.main, draw_lengths(n, d.ways, 23))
    for align in aligns:
        c = Coded(b, align)
        c.decode_all(None, "no order")
        c.decode_all(b.dev(np.arange(n)[::-1], np.int32), "reversed identity")
        d_order = ctx.batch_order(b.d_counts)
        assert sorted(d_order.cpu().tolist()) == list(range(n))
        c.decode_all(d_order, "batch_order")
        lost = int(np.argmax(b.counts))  # (a stream with symbols: its range would show a write)
        order = np.arange(n)
        order[lost] = n
        want = c.d_buf.cpu().numpy().copy()
        lo = int(c.sym_offs[lost])
        want[lo:lo + int(b.counts[lost])] = POISON
        for name, cont, nbytes, offs, lens in c.containers():
            out = torch.full_like(c.d_buf, b.poison())
            with pytest.raises(R.RansAmdError) as e:
                ctx.decode_batch(b.gm, cont, nbytes, offs, lens, c.d_sym, b.d_counts, d.ways, out, d_order=b.dev(order, np.int32))
            assert e.value.status == R.E_CORRUPT and e.value.bad_streams == 1, (name, e.value.bad_streams)
            assert ctx.last_decode_kernel() == d.main["decode"]
            assert np.array_equal(out.cpu().numpy(), want), (name, "a named stream differs, or the stream without a position was written")
    assert ctx.decode_errors() == 0


def check_rate_phase_parking(gpu, oracle, d, row, rate, aligns, start_phases=None):
    """rate: (freqs, counts, contents, phases) of a rate generator.  Each from three containers -- the GPU's, the oracle's and one
    packed by hand at the phases (start_phases: the offsets mod 64 it must show) --, with and without batch_order, with the
    option and without; all must equal the input."""
    R, ctx, torch, off = gpu
    freqs, counts, contents, phases = rate
    b = Batch(R, ctx, torch, oracle, row, counts, contents=contents, freqs=freqs)
    gm_off = off.model(d.fmt, b.freqs, row["sb"])
    p_cont, p_starts, p_bytes = S.pack_at_phases(b.streams, phases, 64, order=np.random.default_rng(11).permutation(b.n))
    assert start_phases is None or sorted(set(int(s) % 64 for s in p_starts)) == start_phases
    d_lens = b.dev(b.lens, np.int32)
    d_order = ctx.batch_order(b.d_counts)
    for align in aligns:
        cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, align)  # (the GPU's and the oracle's container)
        containers = (("gpu", cont, int(slot_offs[-1]), offs, lens),
                      ("phases", b.dev(p_cont, np.uint8), p_bytes, b.dev(p_starts, np.int64), d_lens))
        for cx, gm, kernel in ((ctx, b.gm, row["decode"]), (off, gm_off, d.wave_kernel)):
            for name, c, nbytes, o, ln in containers:
                for order in (None, d_order):
                    out = torch.full_like(d_buf, b.poison())
                    cx.decode_batch(gm, c, nbytes, o, ln, d_sym, b.d_counts, d.ways, out, d_order=order)
                    assert cx.last_decode_kernel() == kernel, (cx.last_decode_kernel(), name)
                    assert torch.equal(out, d_buf), (kernel, name, "align", align, "order" if order is not None else "no order")
                    assert cx.decode_errors() == 0, (kernel, name)


def check_damage_inside_one_wave_load(gpu, oracle, d, n, damaged, shorter_by, moved_to, accepted):
    """n streams of 300..5000 symbols; four streams of the FIRST wave-load `damaged` = (flipped, short, moved, far): a byte
    flipped in the flushed states, a length shortened by `shorter_by`, an offset replaced by moved_to(offset, length,
    container_bytes), a sym_offset one symbol past out_syms.  bad_streams is what the wave-per-stream kernel reports for the same
    damaged batch, one of `accepted`; the other streams, the padding and the guard are exact; the streams rejected on their
    index entry (moved, far) are not written."""
    import pytest
    R, ctx, torch, off = gpu
    counts = np.random.default_rng(17).integers(300, 5001, n).astype(np.uint32)
    b = Batch(R, ctx, torch, oracle, d.main, counts)
    gm_off = off.model(d.fmt, b.freqs, d.main["sb"])
    flipped, short, moved, far = damaged
    for align in (1, 4):
        c = Coded(b, align)
        for name, cont, nbytes, offs, lens in c.containers():
            h_offs, h_lens = offs.cpu().numpy(), lens.cpu().numpy()
            bad_cont = cont.clone()
            bad_cont[int(h_offs[flipped]) + 1] ^= 0x40  # inside the flushed states
            bad_lens = lens.clone()
            bad_lens[short] -= shorter_by
            bad_offs = offs.clone()
            bad_offs[moved] = moved_to(int(h_offs[moved]), int(h_lens[moved]), nbytes)
            bad_sym = c.d_sym.clone()
            bad_sym[far] = c.d_buf.numel() - int(counts[far]) + 1  # one symbol past the end
            reported = []
            for cx, gm, kernel in ((ctx, b.gm, d.main["decode"]), (off, gm_off, d.wave_kernel)):
                out = torch.full_like(c.d_buf, b.poison())
                with pytest.raises(R.RansAmdError) as e:
                    cx.decode_batch(gm, bad_cont, nbytes, bad_offs, bad_lens, bad_sym, b.d_counts, d.ways, out)
                assert e.value.status == R.E_CORRUPT and cx.last_decode_kernel() == kernel, (name, cx.last_decode_kernel())
                assert cx.decode_errors() == 0  # (reported and reset by that call)
                reported.append(e.value.bad_streams)
                got, want = out.cpu().numpy(), c.d_buf.cpu().numpy()
                keep = np.ones(want.size, dtype=bool)
                for s in damaged:
                    keep[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] = False
                assert np.array_equal(got[keep], want[keep]), (name, kernel, "an undamaged stream, the padding or the guard differs")
                for s in (far, moved):
                    assert np.all(got[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] == POISON), (name, kernel, "stream", s, "was written")
                assert np.all(got[int(c.sym_offs[-1]):] == POISON) and got.size == int(c.sym_offs[-1]) + GUARD
            print("bad_streams (the family's kernel, wave kernel):", name, "align", align, reported)
            assert reported[0] == reported[1] and reported[0] in accepted, (name, align, reported)


# ---- ... and the two encoder files
def check_encode_order(gpu, oracle, cx, row, counts):
    """No order, the reversed identity and batch_order's result give the same streams, offsets and lengths; an order with one
    entry replaced by n_streams reports E_ARG, every stream still named is exact, and the stream that lost its position keeps
    its slot's poison and its pre-filled index entries.  On context cx, which must report the row's encoder."""
    import pytest
    R, _, torch, _ = gpu
    n = counts.size
    b = Batch(R, cx, torch, oracle, row, counts)
    d_buf, sym_offs, slot_offs = b.laid_out(4)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    cap = int(slot_offs[-1])
    d_order = cx.batch_order(b.d_counts)
    assert sorted(d_order.cpu().tolist()) == list(range(n))
    results = []
    for name, order in (("no order", None), ("reversed identity", b.dev(np.arange(n)[::-1], np.int32)), ("batch_order", d_order)):
        res = encode_poisoned(b, cx, b.gm, d_buf, d_sym, d_slot, cap, d_order=order)
        assert cx.last_encode_kernel()[0] == row["encode"] and cx.last_encode_placement() == 2, (name, cx.last_encode_kernel())
        cx.encode_status()
        b.check_streams(res[0].cpu().numpy(), res[1].cpu().numpy().astype(np.uint64), res[2].cpu().numpy().view(np.uint32),
                        "%s, %s" % (row["id"], name))
        assert np.all(res[0].cpu().numpy()[cap:] == POISON)
        results.append(res)
    same_result(torch, results[0], results[1], n, "reversed identity")
    same_result(torch, results[0], results[2], n, "batch_order")
    lost = int(np.argmax(counts))
    order = np.arange(n)
    order[lost] = n
    cont, offs, lens = encode_poisoned(b, cx, b.gm, d_buf, d_sym, d_slot, cap, d_order=b.dev(order, np.int32), sentinel=-77)
    assert cx.last_encode_kernel()[0] == row["encode"], cx.last_encode_kernel()
    with pytest.raises(R.RansAmdError) as e:
        cx.encode_status()
    assert e.value.status == R.E_ARG, row["id"]
    h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
    for c in range(n):
        lo, hi = int(slot_offs[c]), int(slot_offs[c + 1])
        if c == lost:
            assert h_offs[c] == -77 and h_lens[c] == -77, "the index entry of the stream without a position was written"
            assert np.all(h[lo:hi] == POISON), "the slot of the stream without a position was written"
        else:
            ln = int(h_lens[c])
            assert ln == b.lens[c] and int(h_offs[c]) == hi - ln, (row["id"], c)
            assert np.array_equal(h[hi - ln:hi], b.streams[c]), (row["id"], "stream", c)
    assert np.all(h[cap:] == POISON)


def check_bad_slots(gpu, oracle, d):
    """test_batch_encode_rejects_bad_slots' construction on 400 streams of the family's shape with the option on: every slot 32
    bytes larger than its bound; a slot off 16 bytes on both sides (two streams), one a granule too small, one beyond out_cap --
    each in a wave-load with valid streams.  E_SPACE, the rejected slots keep their poison and get lengths 0, every other stream
    is exact, the first 16 bytes of every accepted slot are still poison, nothing is written behind the container."""
    import pytest
    R, ctx, torch, _ = gpu
    counts = draw_lengths(400, d.ways, 71)
    b = Batch(R, ctx, torch, oracle, d.main, counts)
    d_buf, sym_offs, _ = b.laid_out(4)
    bound = np.array([R.chunk_bound(d.fmt, int(c), d.ways) for c in counts], dtype=np.int64)
    sizes = bound + 32
    idx = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    cap = int(idx[-1])
    big = np.nonzero(counts >= 1000)[0]
    off16, past = int(big[0]), 399
    small = int(big[(big > off16 + 2) & (big < past - 1)][0])
    bad_idx = idx.copy()
    bad_idx[off16 + 1] += 8
    bad_idx[small] = bad_idx[small + 1] - (bound[small] - 16)
    rejected = {off16, off16 + 1, small, past}
    assert len(rejected) == 4
    for c in rejected:  # (its wave-load holds valid streams as well)
        assert any(k not in rejected for k in range(d.streams * (c // d.streams), min(d.streams * (c // d.streams) + d.streams, 400)))
    d_out = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, b.dev(sym_offs, np.int64), b.d_counts, d.ways, b.dev(bad_idx, np.int64), d_out=d_out,
                                        out_cap=cap - 16)
    assert ctx.last_encode_kernel()[0] == d.main["encode"], ctx.last_encode_kernel()
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_status()
    assert e.value.status == R.E_SPACE
    h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy().view(np.uint32)
    for c in range(b.n):
        lo, hi = int(bad_idx[c]), int(bad_idx[c + 1])
        if c in rejected:
            assert h_lens[c] == 0 and int(h_offs[c]) == hi, c
            if hi > lo:
                assert np.all(h[lo:hi] == POISON), ("a rejected slot was written", c)
        else:
            ln = int(h_lens[c])
            assert ln == b.lens[c] and int(h_offs[c]) == hi - ln, c
            assert np.array_equal(h[hi - ln:hi], b.streams[c]), ("stream", c)
            assert np.all(h[lo:lo + 16] == POISON), ("the head of a slot was written", c)
    assert np.all(h[cap:] == POISON), "written behind the container"


def check_no_false_e_model(gpu, oracle, d, no_zero):
    """no_zero: no_zero_batch's arguments.  encode_status() is OK (run_row asks) and every stream is the oracle's, at both
    alignments."""
    R, ctx, torch, _ = gpu
    freqs, counts, contents = no_zero_batch(*no_zero)
    assert freqs[0] == 0 and all(not np.any(c == 0) for c in contents.values())
    b = Batch(R, ctx, torch, oracle, d.main, counts, contents=contents, freqs=freqs)
    for align in (4, 1):
        run_row(b, align)


def check_true_e_model(gpu, oracle, d, no_zero):
    """The same batch with one symbol of the longest stream of the second wave-load overwritten by 0 on the device: E_MODEL, as
    the default context reports for the same batch; every stream of the other wave-loads is the oracle's; the poison behind
    out_cap is intact; the next call succeeds, on the family's kernel."""
    import pytest
    R, ctx, torch, off = gpu
    freqs, counts, contents = no_zero_batch(*no_zero)
    b = Batch(R, ctx, torch, oracle, d.main, counts, contents=contents, freqs=freqs)
    gm_off = off.model(d.fmt, freqs, d.main["sb"])
    d_buf, sym_offs, slot_offs = b.laid_out(4)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    victim = d.streams + int(np.argmax(counts[d.streams:2 * d.streams]))
    assert counts[victim] >= 256
    bad = d_buf.clone()
    bad[int(sym_offs[victim]) + int(counts[victim]) // 2] = 0
    cap = int(slot_offs[-1])
    for cx, gm, kernel in ((ctx, b.gm, d.main["encode"]), (off, gm_off, d.wave_kernel)):
        cont, offs, lens = encode_poisoned(b, cx, gm, bad, d_sym, d_slot, cap)
        assert cx.last_encode_kernel()[0] == kernel, cx.last_encode_kernel()
        with pytest.raises(R.RansAmdError) as e:
            cx.encode_status()
        assert e.value.status == R.E_MODEL, kernel
        h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy().view(np.uint32)
        for c in range(b.n):
            if c // d.streams != victim // d.streams:
                a = int(h_offs[c])
                assert h_lens[c] == b.lens[c] and a + int(h_lens[c]) == int(slot_offs[c + 1]), (kernel, c)
                assert np.array_equal(h[a:a + int(h_lens[c])], b.streams[c]), (kernel, "stream", c)
        assert np.all(h[cap:] == POISON), (kernel, "written behind the container")
    ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, d.ways, d_slot)  # the next call succeeds
    assert ctx.last_encode_kernel()[0] == d.main["encode"]
    ctx.encode_status()


# ---- the captured-graph tests' child programs ---------------------------------------------------------------------------
_GRAPH_HEAD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import bench, ryg_rans_amd as R
from _batch import draw_lengths, stream_mask, POISON
ctx = R.Context(0)
%(set_option)s
counts = draw_lengths(3000, %(ways)d, 61)
n = counts.size
sym_offs, slot_offs = R.batch_layout(counts, R.%(fmt)s, %(ways)d, 4)
d_syms = bench.gen_zipf(torch, int(sym_offs[-1]), 256, 1.0, 1, "cuda")
d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda(); d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
"""

_GRAPH_SHARED_MODEL = r"""
freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, 256), 1 << %(sb)d)
gm = ctx.model(R.%(fmt)s, freqs, %(sb)d)
"""

_GRAPH_DECODE = r"""
want = torch.full_like(d_syms, POISON)
decode(want)   # (outside the capture first)
assert ctx.last_decode_kernel() == "%(kernel)s", ctx.last_decode_kernel()
covered = torch.zeros(d_syms.numel(), dtype=torch.bool, device="cuda")
idx = torch.repeat_interleave(d_sym[:-1], d_counts.to(torch.int64)) + (torch.arange(int(counts.sum()), device="cuda") -
      torch.repeat_interleave(torch.cumsum(d_counts.to(torch.int64), 0) - d_counts.to(torch.int64), d_counts.to(torch.int64)))
covered[idx] = True
assert torch.equal(want[covered], d_syms[covered]) and bool((want[~covered] == POISON).all()), "eager decode differs from the input"
out = torch.full_like(d_syms, POISON)
s = torch.cuda.Stream()
g = torch.cuda.CUDAGraph()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        decode(out, sync=False)
for _ in range(3):
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "replay differs"
assert ctx.decode_errors() == 0 and ctx.last_decode_kernel() == "%(kernel)s"
print("graph ok")
"""


def graph_decode_script(kernel, fmt="FMT_WORD", ways=64, sb=12, option=None, per_stream_models=False):
    """One captured decode_batch (per_stream_models: decode_batch_adaptive) of 3000 streams: one eager call first -- it must
    report `kernel` and give back the input, padding untouched --, then three replays, each equal to the eager result."""
    v = {"kernel": kernel, "fmt": fmt, "ways": ways, "sb": sb,
         "set_option": "ctx.set_option(R.%s, 1)" % option if option else ""}
    if per_stream_models:
        coded = r"""
cont, offs, lens, rows, total = ctx.encode_batch_adaptive(d_syms, d_sym, d_counts, %(ways)d, %(sb)d, fmt=R.%(fmt)s)
def decode(to, **kw):
    ctx.decode_batch_adaptive(cont, total, offs, lens, rows, d_sym, d_counts, %(ways)d, %(sb)d, to, fmt=R.%(fmt)s, **kw)
"""
    else:
        coded = _GRAPH_SHARED_MODEL + r"""
cont, offs, lens = ctx.encode_batch(gm, d_syms, d_sym, d_counts, %(ways)d, d_slot)
ctx.encode_status()
def decode(to, **kw):
    ctx.decode_batch(gm, cont, int(slot_offs[-1]), offs, lens, d_sym, d_counts, %(ways)d, to, **kw)
"""
    return (_GRAPH_HEAD + coded + _GRAPH_DECODE) % v


def graph_encode_script(kernel, fmt, ways, sb, option):
    """One captured encode_batch of 3000 streams with `option` on: one eager call first -- it must report `kernel` --, then
    three replays into a poison-refilled container, each equal to the eager result (stream bytes, offsets, lengths)."""
    v = {"kernel": kernel, "fmt": fmt, "ways": ways, "sb": sb, "set_option": "ctx.set_option(R.%s, 1)" % option}
    return (_GRAPH_HEAD + _GRAPH_SHARED_MODEL + r"""
cap = int(slot_offs[-1])
want, w_offs, w_lens = ctx.encode_batch(gm, d_syms, d_sym, d_counts, %(ways)d, d_slot)   # (outside the capture first)
ctx.encode_status()
assert ctx.last_encode_kernel()[0] == "%(kernel)s", ctx.last_encode_kernel()
back = torch.full_like(d_syms, POISON)
ctx.decode_batch(gm, want, cap, w_offs, w_lens, d_sym, d_counts, %(ways)d, back)
m = stream_mask(torch, cap, w_offs, w_lens, n)
out = torch.full((cap,), POISON, dtype=torch.uint8, device="cuda")
offs = torch.zeros(n, dtype=torch.int64, device="cuda"); lens = torch.zeros(n, dtype=torch.int32, device="cuda")
s = torch.cuda.Stream()
g = torch.cuda.CUDAGraph()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        ctx.encode_batch(gm, d_syms, d_sym, d_counts, %(ways)d, d_slot, d_out=out, d_offsets=offs, d_lengths=lens, out_cap=cap)
for _ in range(3):
    out.fill_(POISON); offs.zero_(); lens.zero_()
    g.replay()
    torch.cuda.synchronize()
    ctx.encode_status()
    assert torch.equal(offs, w_offs[:n]) and torch.equal(lens, w_lens[:n]), "replay: index entries differ"
    assert torch.equal(out[m], want[:cap][m]), "replay: stream bytes differ"
assert ctx.last_encode_kernel()[0] == "%(kernel)s"
print("graph ok")
""") % v


def run_graph_script(tmp_path, name, script):
    """The child program as a fresh process under a time limit of its own.  Graph replay needs the process's default of four
    hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    import subprocess
    import sys

    import pytest
    q = os.environ.get("GPU_MAX_HW_QUEUES")
    if q is not None and int(q) < 4:
        pytest.skip("fewer than 4 hardware queues: captured graphs are not replayed here")
    path = tmp_path / name
    path.write_text(script)
    r = subprocess.run([sys.executable, str(path), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "graph ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
