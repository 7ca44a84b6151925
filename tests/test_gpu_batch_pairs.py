"""Ragged batches of the reference's 2-way byte layout with THIRTY-TWO streams per wave: k_decode_batch_byte_pairs, the kernel
rans_amd_decode_batch launches on a context with RANS_AMD_OPT_BATCH_PAIRS = 1.

PAIR_ROWS names the kernel the library must report (tests/test_batch_pairs_host.py holds the rows to the names the
launchers can report).  The helpers are tests/test_gpu_batch.py's: every decode is checked against the symbols the
oracle's streams were made from, from the GPU's own container and from one the oracle made (shuffled, 1-byte-aligned
offsets, gaps), into a poison-filled buffer whose padding and guard must come back untouched.

A wave's 32 pairs hold 32 streams with 32 different symbol counts: the wave runs the 64-round line body max(count >> 7)
times, a pair that has run out of 128-byte lines is parked (its refill check gated off, its state and cursor put back
behind every line, its line not stored) and free-runs on whatever its state becomes, and what count - 128 (count >> 7)
leaves goes one round at a time.  The shapes below are the smallest at which that can go wrong; the rate inputs (a
frequency-1-only stream takes the ring's bound of 32 bytes per eight rounds, a common-only stream takes nothing) are
proved to reach their bounds without a GPU by tests/test_batch_pairs_host.py, which imports the generators below."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _stream_rate as S
from _oracle import FMT_BYTE
from test_gpu_batch import GUARD, POISON, ROW, Batch, draw_lengths, mandatory_lengths, resident_waves, run_row

OPT_BATCH_GROUPS = 5
OPT_BATCH_PAIRS = 7


def _pair_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_BYTE, "sb": sb, "K": K, "ways": 2, "decode": "k_decode_batch_byte_pairs", "encode": "k_encode_batch<byte>"}


PAIR_ROWS = [
    _pair_row("byte-2-pairs", 14, 256),           # the reference's scale_bits (main.cpp:139)
    _pair_row("byte-2-pairs-16bit", 16, 256),     # 64 KiB of cum2sym: one block per CU
    _pair_row("byte-2-pairs-12bit", 12, 256),     # (the wave kernel would take the fused slot records here)
    _pair_row("byte-2-pairs-8bit", 8, 256),
    _pair_row("byte-2-pairs-64sym-10bit", 10, 64),
]
PROW = {r["id"]: r for r in PAIR_ROWS}
PMAIN = PROW["byte-2-pairs"]
WAVE_KERNEL = "k_decode_batch<byte>"  # what the 14-bit and 16-bit rows report with the option off


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    ctx.set_option(OPT_BATCH_PAIRS, 1)
    off = R.Context(0)  # the option at its default: the wave-per-stream kernels
    yield R, ctx, torch, off
    off.close()
    ctx.close()


def draw_log_uniform(n_streams, max_len, seed):
    """Log-uniform in [0, max_len]."""
    rng = np.random.default_rng(seed)
    return (np.exp(rng.random(n_streams) * np.log(max_len + 1.0)) - 1.0).astype(np.int64).clip(0, max_len).astype(np.uint32)


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


def _padded(lengths, n=32, pad=200):
    return list(lengths) + [pad] * (n - len(lengths))


WAVE_LOADS = {
    "one-line-each": [128] * 32,
    "boundaries": _padded([0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256]),
    "31-parked-511-lines": [65536] + [255] * 31,
    "every-pair-parks-elsewhere": [128 * (g + 1) + 3 * g for g in range(32)],
    "quad-mates-differ": [640, 0, 128, 385] * 8,
    "all-empty": [0] * 32,
    "second-load-of-one": [300] * 33,
    "mandatory-and-200s": _padded(mandatory_lengths(2)),
}


def _wave_load_cases():
    for name in WAVE_LOADS:
        for row in (PAIR_ROWS if name == "one-line-each" else (PROW["byte-2-pairs"], PROW["byte-2-pairs-16bit"])):
            yield pytest.param(name, row, id="%s-%s" % (name, row["id"]), marks=pytest.mark.gpu)


@pytest.mark.parametrize("name,row", list(_wave_load_cases()))
def test_single_wave_loads(gpu, oracle, name, row):
    """One or two wave-loads: one line each and no tail; every line and tail boundary in one wave; 31 pairs parked for 511
    lines while one refills its ring throughout, each owing a 127-symbol tail afterwards; every pair parking at another
    line with another tail; quad-mates of which A runs while B is parked and the reverse (the predicated quad stores);
    32 empty streams; a second wave-load of one stream and 31 empty pairs; the mandatory lengths.  Each at sym_align 1 (all
    symbols a round at a time, byte stores) and 4.  Wall time on an MI355X: 1.6 s of setup and 0.6 s for the first case (it
    loads the kernels), 0.01 to 0.05 s for each of the others; this whole file takes 7 s."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, row, np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in (1, 4):
        run_row(b, align)
    assert ctx.decode_errors() == 0
    assert ctx.launch_spans(1)[0] > 0.0, "the launch recorded no span"


# ---- rate x phase x parking: the generators tests/test_batch_pairs_host.py proves things about ---------------------------
RATE_BITS = (16, 14)
RATE_STREAMS = 64
RATE_COUNTS = tuple(128 * b + t for b in (0, 1, 5) for t in (0, 1, 77, 127))
RATE_ROW = {16: PROW["byte-2-pairs-16bit"], 14: PROW["byte-2-pairs"]}


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


def _rate_cases():
    for sb in RATE_BITS:
        yield pytest.param(sb, None, id="%dbit-batch" % sb, marks=pytest.mark.gpu)
        for name in RATE_WAVES:
            yield pytest.param(sb, name, id="%dbit-%s" % (sb, name), marks=pytest.mark.gpu)


@pytest.mark.parametrize("sb,which", list(_rate_cases()))
def test_rate_phase_parking(gpu, oracle, sb, which):
    """64 streams under 255 x 1 + one common symbol: stream k frequency-1-only (k % 3 != 2: at 16 bits every state takes two
    bytes in every round, 32 bytes per eight rounds, the refill's bound) or common-only (nothing at all at 16 bits), its count
    one of 128 b + t, b in {0, 1, 5}, t in {0, 1, 77, 127}, the oracle's stream at offset == k (mod 64) of a container packed
    by hand.  Pairs with b = 0 and b = 1 are parked while their quad- and wave-mates run on: a parked pair free-runs, and an
    ungated checkpoint() would move its ring, pend and thr under it -- its tail would then read the wrong bytes.  The two
    single wave-loads: 65536 frequency-1 symbols beside 31 parked common-only streams of 255, and 65536 common-only symbols
    beside 31 rare-only streams that park one after the other.  Each from three containers at sym_align 4 and 1, with and
    without batch_order, with the option and without; all must equal the input.  Wall time on an MI355X: 0.02 s for each of
    the two batches, 0.15 s for each single wave-load."""
    R, ctx, torch, off = gpu
    row = RATE_ROW[sb]
    freqs, counts, contents, phases = rate_batch(sb) if which is None else rate_wave(sb, which)
    b = Batch(R, ctx, torch, oracle, row, counts, contents=contents, freqs=freqs)
    gm_off = off.model(FMT_BYTE, b.freqs, sb)
    p_cont, p_starts, p_bytes = S.pack_at_phases(b.streams, phases, 64, order=np.random.default_rng(11).permutation(b.n))
    d_lens = b.dev(b.lens, np.int32)
    d_order = ctx.batch_order(b.d_counts)
    for align in (4, 1):
        cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, align)  # (the GPU's and the oracle's container)
        containers = (("gpu", cont, int(slot_offs[-1]), offs, lens),
                      ("phases", b.dev(p_cont, np.uint8), p_bytes, b.dev(p_starts, np.int64), d_lens))
        for cx, gm, kernel in ((ctx, b.gm, row["decode"]), (off, gm_off, WAVE_KERNEL)):
            for name, c, nbytes, o, ln in containers:
                for order in (None, d_order):
                    out = torch.full_like(d_buf, b.poison())
                    cx.decode_batch(gm, c, nbytes, o, ln, d_sym, b.d_counts, 2, out, d_order=order)
                    assert cx.last_decode_kernel() == kernel, (cx.last_decode_kernel(), name)
                    assert torch.equal(out, d_buf), (kernel, name, "align", align, "order" if order is not None else "no order")
                    assert cx.decode_errors() == 0, (kernel, name)


@pytest.mark.gpu
def test_order(gpu, oracle):
    """70 streams (two wave-loads and a partial third): the reversed identity, the result of batch_order, and an order with
    one entry replaced by n_streams -- that position is one failed stream, every stream still named decodes right, the
    stream that lost its position is not written.  Wall time on an MI355X: 0.15 s."""
    R, ctx, torch, _ = gpu
    n = 70
    b = Batch(R, ctx, torch, oracle, PMAIN, draw_lengths(n, 2, 23))
    for align in (1, 4):
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
                ctx.decode_batch(b.gm, cont, nbytes, offs, lens, c.d_sym, b.d_counts, 2, out, d_order=b.dev(order, np.int32))
            assert e.value.status == R.E_CORRUPT and e.value.bad_streams == 1, (name, e.value.bad_streams)
            assert ctx.last_decode_kernel() == PMAIN["decode"]
            assert np.array_equal(out.cpu().numpy(), want), (name, "a named stream differs, or the stream without a position was written")
    assert ctx.decode_errors() == 0


POOL = 4096  # prototypes of the half and several batches, each coded once by the oracle


class PoolBatch:
    """n streams, each one of at most POOL prototypes: the oracle codes every prototype once, the batch (index, container,
    expected output) is put together from them on the device.  The container is the oracle's -- the prototypes' streams in a
    shuffled order at 1-byte-aligned offsets with gaps, every stream of the batch pointing at its prototype's."""

    def __init__(self, R, ctx, torch, oracle, row, proto_counts, n, seed):
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
        self.sym_offs, self.slot_offs = R.batch_layout(self.counts, row["fmt"], 2, 4)

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


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer wave-loads than the launch has resident waves, prototype lengths log-uniform up to 64 Ki with the
    mandatory ones.  several: at least 1.25 x as many wave-loads as resident waves (several hundred thousand streams), so
    that waves come back for further claims; prototype lengths log-uniform up to 1024.  Every stream is one of at most 4096
    prototypes the oracle coded once; index, container and expected output are put together on the device.  The last
    wave-load of each is partial; each with and without d_order at sym_align = 4, from the oracle's container and from the
    GPU's own coding of the same symbols.  Wall time on an MI355X: 0.26 s (half), 0.21 s (several)."""
    R, ctx, torch, _ = gpu
    resident = resident_waves(torch)
    if regime == "half":
        loads = resident // 32
        protos = draw_lengths(1024, 2, 7)
        assert 0 < loads < resident and set(mandatory_lengths(2)) <= set(protos.tolist())
    else:
        loads = resident + resident // 4 + 1
        protos = draw_log_uniform(POOL, 1024, 9)
        assert 4 * loads >= 5 * resident
    n = loads * 32 - 5
    pb = PoolBatch(R, ctx, torch, oracle, PMAIN, protos, n, 31)
    assert pb.counts.size == n and n % 32 != 0 and protos.size <= POOL
    g_cont, g_offs, g_lens = ctx.encode_batch(pb.gm, pb.d_buf, pb.d_sym, pb.d_counts, 2, pb.d_slot)
    ctx.encode_status()
    d_order = ctx.batch_order(pb.d_counts)
    for name, cont, nbytes, offs, lens in (("oracle", pb.cont, pb.cont_bytes, pb.d_offs, pb.d_lens),
                                          ("gpu", g_cont, int(pb.slot_offs[-1]), g_offs, g_lens)):
        for order in (None, d_order):
            out = torch.full_like(pb.d_buf, POISON)
            ctx.decode_batch(pb.gm, cont, nbytes, offs, lens, pb.d_sym, pb.d_counts, 2, out, d_order=order)
            assert ctx.last_decode_kernel() == PMAIN["decode"], ctx.last_decode_kernel()
            assert torch.equal(out, pb.d_buf), (name, "order" if order is not None else "no order")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_damage_is_counted_and_contained_inside_one_wave_load(gpu, oracle):
    """64 streams of 300..5000 symbols; four streams of the FIRST wave-load are damaged: a byte flipped in the flushed states,
    a length shortened by 1, an offset that puts the stream's end one byte past container_bytes, a sym_offset one symbol
    past out_syms -- pairs 2, 5, 8 and 13, each with an undamaged quad-mate (3, 4, 9, 12).  bad_streams equals what the
    wave-per-stream kernel reports for the same damaged batch (the three that are certain, and the flipped byte where the
    final states show it: 4 on an MI355X); the other sixty streams, the padding and the guard are exact; the two streams
    rejected on their index are not written.  Wall time on an MI355X: 0.02 s."""
    R, ctx, torch, off = gpu
    counts = np.random.default_rng(17).integers(300, 5001, 64).astype(np.uint32)
    b = Batch(R, ctx, torch, oracle, PMAIN, counts)
    gm_off = off.model(FMT_BYTE, b.freqs, PMAIN["sb"])
    flipped, short, past, far = 2, 5, 8, 13
    damaged = (flipped, short, past, far)
    for align in (1, 4):
        c = Coded(b, align)
        for name, cont, nbytes, offs, lens in c.containers():
            h_offs, h_lens = offs.cpu().numpy(), lens.cpu().numpy()
            bad_cont = cont.clone()
            bad_cont[int(h_offs[flipped]) + 1] ^= 0x40  # inside the flushed states
            bad_lens = lens.clone()
            bad_lens[short] -= 1
            bad_offs = offs.clone()
            bad_offs[past] = nbytes - int(h_lens[past]) + 1  # off + len one byte past container_bytes
            bad_sym = c.d_sym.clone()
            bad_sym[far] = c.d_buf.numel() - int(counts[far]) + 1  # one symbol past the end
            reported = []
            for cx, gm, kernel in ((ctx, b.gm, PMAIN["decode"]), (off, gm_off, WAVE_KERNEL)):
                out = torch.full_like(c.d_buf, b.poison())
                with pytest.raises(R.RansAmdError) as e:
                    cx.decode_batch(gm, bad_cont, nbytes, bad_offs, bad_lens, bad_sym, b.d_counts, 2, out)
                assert e.value.status == R.E_CORRUPT and cx.last_decode_kernel() == kernel, (name, cx.last_decode_kernel())
                assert cx.decode_errors() == 0  # (reported and reset by that call)
                reported.append(e.value.bad_streams)
                got, want = out.cpu().numpy(), c.d_buf.cpu().numpy()
                keep = np.ones(want.size, dtype=bool)
                for s in damaged:
                    keep[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] = False
                assert np.array_equal(got[keep], want[keep]), (name, kernel, "an undamaged stream, the padding or the guard differs")
                for s in (far, past):
                    assert np.all(got[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] == POISON), (name, kernel, "stream", s, "was written")
                assert np.all(got[int(c.sym_offs[-1]):] == POISON) and got.size == int(c.sym_offs[-1]) + GUARD
            print("bad_streams (pair kernel, wave kernel):", name, "align", align, reported)
            assert reported[0] == reported[1] and reported[0] in (3, 4), (name, align, reported)


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("byte-2", 31), ("byte-64-14bit", 40), ("byte-64-12bit", 40), ("word-8", 40), ("alias256-64", 40), ("r64-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """Fewer than 32 2-way byte streams, the 64-way byte rows, the 8-way word layout, the alias and the rans64 2-way rows take
    the wave-per-stream kernels on the context with the option on, and decode right.  Wall time on an MI355X: 0.01 to 0.03 s
    per case."""
    R, ctx, torch, _ = gpu
    row = ROW[rid]
    assert row["decode"] != PMAIN["decode"]
    b = Batch(R, ctx, torch, oracle, row, draw_lengths(n_streams, row["ways"], 29))
    run_row(b, 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_per_stream_models_keep_their_kernel_with_the_option_on(gpu, oracle):
    """decode_batch_adaptive of 40 2-way byte streams, each with its own model, on the context with the option on: the wave
    kernel with one model per stream, every stream against the oracle.  Wall time on an MI355X: 0.03 s."""
    from test_gpu_batch_models import ROW as MODEL_ROW
    from test_gpu_batch_models import ModelBatch
    from test_gpu_batch_models import run_row as run_model_row
    R, ctx, torch, _ = gpu
    row = MODEL_ROW["byte-2-12bit"]
    assert row["decode"] != PMAIN["decode"]
    run_model_row(ModelBatch(R, ctx, torch, oracle, row, draw_lengths(40, 2, 37).clip(0, 4096)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_options_five_and_seven_are_independent(gpu, oracle):
    """With RANS_AMD_OPT_BATCH_GROUPS and RANS_AMD_OPT_BATCH_PAIRS both on, nine 8-way word streams report
    k_decode_batch_word_groups and forty 2-way byte streams the pair kernel.  Wall time on an MI355X: 0.03 s."""
    R, ctx, torch, _ = gpu
    ctx.set_option(OPT_BATCH_GROUPS, 1)
    try:
        word = dict(ROW["word-8"], decode="k_decode_batch_word_groups")
        run_row(Batch(R, ctx, torch, oracle, word, draw_lengths(9, 8, 43)), 4)
        run_row(Batch(R, ctx, torch, oracle, PMAIN, draw_lengths(40, 2, 47)), 4)
    finally:
        ctx.set_option(OPT_BATCH_GROUPS, 0)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the pair kernel.  Wall time on an
    MI355X: 0.01 s."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, PMAIN, np.array([300] * 33, dtype=np.uint32))
    for bad in (2, -1):
        with pytest.raises(R.RansAmdError) as e:
            ctx.set_option(OPT_BATCH_PAIRS, bad)
        assert e.value.status == R.E_ARG
    run_row(b, 4)
    ctx.set_option(OPT_BATCH_PAIRS, 0)
    try:
        run_row(Batch(R, ctx, torch, oracle, ROW["byte-2"], b.counts), 4)
    finally:
        ctx.set_option(OPT_BATCH_PAIRS, 1)
    run_row(b, 4)


_GRAPH_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import bench, ryg_rans_amd as R
from test_gpu_batch import draw_lengths, POISON
ctx = R.Context(0)
ctx.set_option(R.OPT_BATCH_PAIRS, 1)
counts = draw_lengths(3000, 2, 61)
sym_offs, slot_offs = R.batch_layout(counts, R.FMT_BYTE, 2, 4)
d_syms = bench.gen_zipf(torch, int(sym_offs[-1]), 256, 1.0, 1, "cuda")
freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, 256), 1 << 14)
gm = ctx.model(R.FMT_BYTE, freqs, 14)
d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda(); d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
cont, offs, lens = ctx.encode_batch(gm, d_syms, d_sym, d_counts, 2, d_slot)
ctx.encode_status()
want = torch.full_like(d_syms, POISON)
ctx.decode_batch(gm, cont, int(slot_offs[-1]), offs, lens, d_sym, d_counts, 2, want)   # (outside the capture first)
assert ctx.last_decode_kernel() == "k_decode_batch_byte_pairs", ctx.last_decode_kernel()
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
        ctx.decode_batch(gm, cont, int(slot_offs[-1]), offs, lens, d_sym, d_counts, 2, out, sync=False)
for _ in range(3):
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "replay differs"
assert ctx.decode_errors() == 0 and ctx.last_decode_kernel() == "k_decode_batch_byte_pairs"
print("graph ok")
"""


@pytest.mark.gpu
def test_pair_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 2-way byte streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply.  Wall time on an MI355X:
    2.4 s."""
    import subprocess
    import sys
    q = os.environ.get("GPU_MAX_HW_QUEUES")
    if q is not None and int(q) < 4:
        pytest.skip("fewer than 4 hardware queues: captured graphs are not replayed here")
    script = tmp_path / "graph_batch_pairs.py"
    script.write_text(_GRAPH_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
