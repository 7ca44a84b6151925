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

from _batch import (POISON, POOL, RATE_BITS, RATE_WAVES, Batch, ModelBatch, PoolBatch, check_damage_inside_one_wave_load, check_decode_order,
                    check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels, check_rate_phase_parking, draw_lengths,
                    draw_log_uniform, mandatory_lengths, option_contexts, padded, rate_batch, rate_wave, resident_waves, run_family_graph,
                    run_model_row, run_row, wave_load_cases)
from _kernel_rows import MODEL_ROW, OPT_BATCH_GROUPS, OPT_BATCH_PAIRS, PAIR_RATE_ROW, PAIR_ROWS, PAIRS, PMAIN, PROW, ROW


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_PAIRS)


WAVE_LOADS = {
    "one-line-each": [128] * 32,
    "boundaries": padded(32, [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256]),
    "31-parked-511-lines": [65536] + [255] * 31,
    "every-pair-parks-elsewhere": [128 * (g + 1) + 3 * g for g in range(32)],
    "quad-mates-differ": [640, 0, 128, 385] * 8,
    "all-empty": [0] * 32,
    "second-load-of-one": [300] * 33,
    "mandatory-and-200s": padded(32, mandatory_lengths(2)),
}


@pytest.mark.parametrize("name,row", list(wave_load_cases(WAVE_LOADS, PAIR_ROWS, (PMAIN, PROW["byte-2-pairs-16bit"]))))
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
    rate = rate_batch(sb) if which is None else rate_wave(sb, which)
    check_rate_phase_parking(gpu, oracle, PAIRS, PAIR_RATE_ROW[sb], rate, (4, 1))


@pytest.mark.gpu
def test_order(gpu, oracle):
    """70 streams (two wave-loads and a partial third): the reversed identity, the result of batch_order, and an order with
    one entry replaced by n_streams -- that position is one failed stream, every stream still named decodes right, the
    stream that lost its position is not written.  Wall time on an MI355X: 0.15 s."""
    check_decode_order(gpu, oracle, PAIRS, 70, (1, 4))


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
    check_damage_inside_one_wave_load(gpu, oracle, PAIRS, 64, (2, 5, 8, 13), 1, lambda off, ln, nbytes: nbytes - ln + 1, (3, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("byte-2", 31), ("byte-64-14bit", 40), ("byte-64-12bit", 40), ("word-8", 40), ("alias256-64", 40), ("r64-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """Fewer than 32 2-way byte streams, the 64-way byte rows, the 8-way word layout, the alias and the rans64 2-way rows take
    the wave-per-stream kernels on the context with the option on, and decode right.  Wall time on an MI355X: 0.01 to 0.03 s
    per case."""
    check_other_shape_keeps_its_kernels(gpu, oracle, PAIRS, rid, n_streams)


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
    check_option_takes_zero_or_one(gpu, oracle, PAIRS)


@pytest.mark.gpu
def test_pair_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 2-way byte streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply.  Wall time on an MI355X:
    2.4 s."""
    run_family_graph(tmp_path, PAIRS, "graph_batch_pairs.py")
