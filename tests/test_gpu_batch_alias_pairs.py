"""Ragged batches of the reference's 2-way ALIAS layout (main_alias.cpp) with THIRTY-TWO streams per wave:
k_decode_batch_alias_pairs, the kernel rans_amd_decode_batch launches on a context with RANS_AMD_OPT_BATCH_ALIAS_PAIRS = 1.  The
counterpart of tests/test_gpu_batch_pairs.py, test for test, on the descriptor and rows of tests/_batch_alias_pairs.py.

ALIAS_PAIR_ROWS names the kernel the library must report (tests/test_batch_alias_pairs_host.py holds the rows to the registry's
second list).  The helpers are tests/_batch.py's: every decode is checked against the symbols the oracle's streams were made
from, from the GPU's own container and from one the oracle made (shuffled, 1-byte-aligned offsets, gaps), into a poison-filled
buffer whose padding and guard must come back untouched.

The plan is the byte pairs': a pair that has run out of 128-byte lines is parked and free-runs on whatever its state becomes.
What is new is the symbol step -- divider, half-bucket record, symbol out of the record --, so the rows cover its table shapes:
256 slots per bucket at 16 bits down to one slot per bucket, bucket shift 0, at 8 bits, and a 64-symbol alphabet.  The rate
inputs (a frequency-1-only stream takes the ring's bound of 32 bytes per eight rounds at 16 bits, a common-only stream takes
nothing) are tests/_batch.py's generators, proved to reach their bounds for ALIAS streams without a GPU by
tests/test_batch_alias_pairs_host.py."""
import numpy as np
import pytest

from _batch import (POISON, POOL, RATE_BITS, RATE_WAVES, Batch, ModelBatch, PoolBatch, check_damage_inside_one_wave_load, check_decode_order,
                    check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels, check_rate_phase_parking, draw_lengths,
                    draw_log_uniform, mandatory_lengths, option_contexts, rate_batch, rate_wave, resident_waves, run_family_graph,
                    run_model_row, run_row, wave_load_cases)
from _batch_alias_pairs import (A8, ALIAS_2_WAVE, ALIAS_PAIR_RATE_ROW, ALIAS_PAIR_ROWS, ALIAS_PAIRS, ALIAS_U16_2_WAVE, AMAIN,
                                OPT_BATCH_ALIAS_PAIRS, AliasOracle)
from _kernel_rows import MODEL_ROW, OPT_BATCH_PAIRS, PMAIN, ROW
from test_gpu_batch_pairs import WAVE_LOADS


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_ALIAS_PAIRS)


@pytest.mark.parametrize("name,row", list(wave_load_cases(WAVE_LOADS, ALIAS_PAIR_ROWS, (AMAIN, A8))))
def test_single_wave_loads(gpu, oracle, name, row):
    """The byte file's wave-loads: one line each and no tail (every row); every line and tail boundary in one wave; 31 pairs
    parked for 511 lines while one refills its ring throughout; every pair parking at another line with another tail;
    quad-mates of which A runs while B is parked and the reverse; 32 empty streams; a second wave-load of one stream; the
    mandatory lengths -- on the 16-bit main row and the 8-bit row.  Each at sym_align 1 (all symbols a round at a time, byte
    stores) and 4."""
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
    """tests/test_gpu_batch_pairs.py's rate x phase x parking inputs as ALIAS streams: 64 streams under 255 x 1 + one common
    symbol, frequency-1-only (at 16 bits two bytes per state and round, the refill's bound) or common-only, counts 128 b + t,
    the oracle's stream at offset == k (mod 64) of a container packed by hand; and the two single wave-loads.  Each from three
    containers at sym_align 4 and 1, with and without batch_order, with the option and without; all must equal the input."""
    rate = rate_batch(sb) if which is None else rate_wave(sb, which)
    check_rate_phase_parking(gpu, oracle, ALIAS_PAIRS, ALIAS_PAIR_RATE_ROW[sb], rate, (4, 1))


@pytest.mark.gpu
def test_order(gpu, oracle):
    """70 streams (two wave-loads and a partial third): the reversed identity, the result of batch_order, and an order with
    one entry replaced by n_streams -- that position is one failed stream, every stream still named decodes right, the
    stream that lost its position is not written."""
    check_decode_order(gpu, oracle, ALIAS_PAIRS, 70, (1, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer wave-loads than the launch has resident waves, prototype lengths log-uniform up to 64 Ki with the
    mandatory ones.  several: at least 1.25 x as many wave-loads as resident waves, so that waves come back for further
    claims; prototype lengths log-uniform up to 1024.  Every stream is one of at most 4096 prototypes the oracle coded once
    (PoolBatch).  The last wave-load of each is partial; each with and without d_order at sym_align = 4, from the oracle's
    container and from the GPU's own coding of the same symbols."""
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
    pb = PoolBatch(R, ctx, torch, AliasOracle(oracle), AMAIN, protos, n, 31)
    assert pb.counts.size == n and n % 32 != 0 and protos.size <= POOL
    g_cont, g_offs, g_lens = ctx.encode_batch(pb.gm, pb.d_buf, pb.d_sym, pb.d_counts, 2, pb.d_slot)
    ctx.encode_status()
    d_order = ctx.batch_order(pb.d_counts)
    for name, cont, nbytes, offs, lens in (("oracle", pb.cont, pb.cont_bytes, pb.d_offs, pb.d_lens),
                                          ("gpu", g_cont, int(pb.slot_offs[-1]), g_offs, g_lens)):
        for order in (None, d_order):
            out = torch.full_like(pb.d_buf, POISON)
            ctx.decode_batch(pb.gm, cont, nbytes, offs, lens, pb.d_sym, pb.d_counts, 2, out, d_order=order)
            assert ctx.last_decode_kernel() == AMAIN["decode"], ctx.last_decode_kernel()
            assert torch.equal(out, pb.d_buf), (name, "order" if order is not None else "no order")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_damage_is_counted_and_contained_inside_one_wave_load(gpu, oracle):
    """64 streams of 300..5000 symbols; four streams of the FIRST wave-load are damaged: a byte flipped in the flushed states,
    a length shortened by 1, an offset that puts the stream's end one byte past container_bytes, a sym_offset one symbol
    past out_syms -- pairs 2, 5, 8 and 13, each with an undamaged quad-mate (3, 4, 9, 12).  bad_streams equals what the
    wave-per-stream kernel reports for the same damaged batch (the three that are certain, and the flipped byte where the
    final states show it); the other sixty streams, the padding and the guard are exact; the two streams rejected on their
    index are not written."""
    check_damage_inside_one_wave_load(gpu, oracle, ALIAS_PAIRS, 64, (2, 5, 8, 13), 1, lambda off, ln, nbytes: nbytes - ln + 1, (3, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("alias256-64", 40), ("byte-2", 40), ("word-8", 40), ("r64-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """The 64-way alias row, and one byte, word and rans64 shape each, take the wave-per-stream kernels on the context with
    the option on, and decode right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, ALIAS_PAIRS, rid, n_streams)


@pytest.mark.gpu
@pytest.mark.parametrize("row,n_streams", [(ALIAS_2_WAVE, 31), (ALIAS_U16_2_WAVE, 40)], ids=["alias-2-31-streams", "alias-u16-2"])
def test_alias_shapes_the_kernel_does_not_take(gpu, oracle, row, n_streams):
    """Fewer than 32 2-way alias streams of the main row's shape, and forty 2-way alias streams over u16 symbols (1024 of them),
    keep k_decode_batch<alias> with the option on, and decode right."""
    R, ctx, torch, _ = gpu
    assert row["decode"] != AMAIN["decode"]
    run_row(Batch(R, ctx, torch, oracle, row, draw_lengths(n_streams, 2, 29).clip(0, 8192)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_per_stream_models_keep_their_kernel_with_the_option_on(gpu, oracle):
    """decode_batch_adaptive of 40 2-way byte streams, each with its own model, on the context with the option on: the wave
    kernel with one model per stream, every stream against the oracle."""
    R, ctx, torch, _ = gpu
    row = MODEL_ROW["byte-2-12bit"]
    assert row["decode"] != AMAIN["decode"]
    run_model_row(ModelBatch(R, ctx, torch, oracle, row, draw_lengths(40, 2, 37).clip(0, 4096)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_options_seven_and_eleven_are_independent(gpu, oracle):
    """Each with only its own option on: on the alias context forty 2-way byte streams keep k_decode_batch<byte> and forty 2-way
    alias streams take the alias pairs; with RANS_AMD_OPT_BATCH_PAIRS on as well the byte streams take the byte pairs and the
    alias streams still the alias pairs; with option 11 off and 7 on the alias streams are back on k_decode_batch<alias>."""
    R, ctx, torch, _ = gpu
    counts = draw_lengths(40, 2, 47)
    run_row(Batch(R, ctx, torch, oracle, ROW["byte-2"], counts), 4)
    run_row(Batch(R, ctx, torch, oracle, AMAIN, counts), 4)
    ctx.set_option(OPT_BATCH_PAIRS, 1)
    try:
        run_row(Batch(R, ctx, torch, oracle, PMAIN, counts), 4)
        run_row(Batch(R, ctx, torch, oracle, AMAIN, counts), 4)
        ctx.set_option(OPT_BATCH_ALIAS_PAIRS, 0)
        try:
            run_row(Batch(R, ctx, torch, oracle, PMAIN, counts), 4)
            run_row(Batch(R, ctx, torch, oracle, ALIAS_2_WAVE, counts), 4)
        finally:
            ctx.set_option(OPT_BATCH_ALIAS_PAIRS, 1)
    finally:
        ctx.set_option(OPT_BATCH_PAIRS, 0)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG, in the other families' words, and changes nothing; 0 restores the wave-per-stream kernel, 1 the
    alias pairs."""
    R, ctx, _, _ = gpu
    check_option_takes_zero_or_one(gpu, oracle, ALIAS_PAIRS)
    with pytest.raises(R.RansAmdError) as e:
        ctx.set_option(OPT_BATCH_ALIAS_PAIRS, 2)
    assert "takes 0 (one stream per wave) or 1 (thirty-two 2-way alias streams per wave)" in str(e.value)


@pytest.mark.gpu
def test_alias_pair_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 2-way alias streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    run_family_graph(tmp_path, ALIAS_PAIRS, "graph_batch_alias_pairs.py")
