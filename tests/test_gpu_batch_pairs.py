"""Ragged batches of the reference's 2-way byte layout with THIRTY-TWO streams per wave: k_decode_batch_byte_pairs, the kernel
rans_amd_decode_batch launches on a context with RANS_AMD_OPT_BATCH_PAIRS = 1.

PAIR_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_pairs_host.py holds the rows to
the names the launchers can report).  The helpers are tests/_batch.py's: every decode is checked against the symbols the
oracle's streams were made from, from the GPU's own container and from one the oracle made (shuffled, 1-byte-aligned
offsets, gaps), into a poison-filled buffer whose padding and guard must come back untouched.

A wave's 32 pairs hold 32 streams with 32 different symbol counts: the wave runs the 64-round line body max(count >> 7)
times, a pair that has run out of 128-byte lines is parked (its refill check gated off, its state and cursor put back
behind every line, its line not stored) and free-runs on whatever its state becomes, and what count - 128 (count >> 7)
leaves goes one round at a time.  The shapes below are the smallest at which that can go wrong; the rate inputs (a
frequency-1-only stream takes the ring's bound of 32 bytes per eight rounds, a common-only stream takes nothing) are
tests/_batch.py's generators, proved to reach their bounds without a GPU by tests/test_batch_pairs_host.py."""
import numpy as np
import pytest

import _stream_rate as S
from _batch import (GUARD, POISON, POOL, RATE_BITS, RATE_WAVES, Batch, Coded, ModelBatch, PoolBatch, draw_lengths, draw_log_uniform,
                    graph_decode_script, mandatory_lengths, rate_batch, rate_wave, resident_waves, run_graph_script, run_model_row, run_row)
from _kernel_rows import MODEL_ROW, OPT_BATCH_GROUPS, OPT_BATCH_PAIRS, PAIR_ROWS, PMAIN, PROW, RATE_ROW, ROW
from _oracle import FMT_BYTE

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


@pytest.mark.gpu
def test_pair_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 2-way byte streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply.  Wall time on an MI355X:
    2.4 s."""
    run_graph_script(tmp_path, "graph_batch_pairs.py",
                     graph_decode_script(PMAIN["decode"], fmt="FMT_BYTE", ways=2, sb=14, option="OPT_BATCH_PAIRS"))
