"""Ragged batches of the reference's 2-way rans64 layout CODED with sixty-four streams per wave: k_encode_batch_r64_lanes, the
kernel rans_amd_encode_batch[_ordered] launches on a context with RANS_AMD_OPT_BATCH_ENCODE_LANES = 1.

ENC_LANE_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_encode_lanes_host.py holds the
rows to the registry's family).  The helpers are tests/_batch.py's: run_row checks the reported kernel, every
stream byte for byte against the oracle's, each ending at its slot's end, and decodes the result (k_decode_batch<r64>: the
context has the encoder's option alone).

The coder works from a stream's last symbol to its first, so a wave's 64 lanes start together and finish at different
times: a lane is finalised (states, last lines, index entry) right behind its last group and is dead from then on, while the
wave's sixteen-symbol sequence -- full exec -- runs on for the others: a dead lane keeps writing into its column of the ring
and keeps taking part in its quad-mates' flushes.  The shapes below are the smallest at which that can go wrong; the rate
inputs are proved to reach their bounds without a GPU by tests/test_batch_encode_lanes_host.py, from the same generators.
Symbols are fetched by the quad (sym_align 64), by the lane in 16-byte pieces (16 and 4) or a byte at a time (1): every
wave-load runs at all four.

Containers of two encodes are compared over the bytes of their streams: the 16-byte piece that holds a stream's first byte
is stored whole, and what it holds below the stream is whatever the lane's ring held (as with the wave kernels' flushes).
Wall time on an MI355X: 6.8 s for the 45 cases of this file -- 2.3 s of it the captured graph's child process, 0.8 s the first
case's setup and call (they load the kernels), 0.3 s each the `half` and `several` regimes, 0.2 s the 65536-symbol rare stream
beside dead lanes, 0.1 s and less for each of the others."""
import numpy as np
import pytest

import _batch_lanes as L
from _batch import (POISON, POOL, Batch, ModelBatch, PoolBatch, check_bad_slots, check_encode_order, check_no_false_e_model,
                    check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels, check_true_e_model, draw_lengths, draw_log_uniform,
                    mandatory_lengths, option_contexts, resident_waves, run_family_graph, run_model_row, run_row, same_result)
from _batch_encode_lanes import ALIGNS, NO_ZERO_LANE_LOADS, WAVE_LOADS, rate_wave
from _kernel_rows import (EL16, ELMAIN, EMAIN, ENC_LANE_RATE_ROW, ENC_LANE_ROWS, ENC_LANES, EROW, LMAIN, MODEL_ROW, OPT_BATCH_ENCODE_GROUPS,
                          OPT_BATCH_ENCODE_LANES, OPT_BATCH_ENCODE_PAIRS, OPT_BATCH_LANES)
from _oracle import FMT_R64

KERNEL, WAVE = ELMAIN["encode"], ENC_LANES.wave_kernel


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_ENCODE_LANES)


def _wave_load_cases():
    """Every row at the first two wave-loads, the 14-bit and the 16-bit row at the others."""
    for k, name in enumerate(WAVE_LOADS):
        for row in (ENC_LANE_ROWS if k < 2 else (ELMAIN, EL16)):
            yield pytest.param(name, row, id="%s-%s" % (name, row["id"]), marks=pytest.mark.gpu)


@pytest.mark.parametrize("name,row", list(_wave_load_cases()))
def test_single_wave_loads(gpu, oracle, name, row):
    """One or two wave-loads: one whole block each and no tail; every group and block boundary in one wave; 63 lanes dead for
    1023 blocks while one keeps flushing; every lane finishing at another block, some with an odd count; quad-mates that
    differ; 64 empty streams (16 bytes each: the flushed initial states); a second wave-load of one stream; the mandatory
    lengths.  Each at sym_align 1 (a symbol and a byte load at a time), 4 and 16 (the lane's own 16-byte pieces) and 64 (the
    quad's lines)."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, row, np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in ALIGNS:
        run_row(b, align)
    assert ctx.decode_errors() == 0


def _rate_cases():
    for which in ("fast-beside-dead", "stalled-beside-draining", 16, 14):
        yield pytest.param(which, id=str(which), marks=pytest.mark.gpu)


@pytest.mark.parametrize("which", list(_rate_cases()))
def test_rate_extremes_in_one_wave(gpu, oracle, which):
    """A frequency-1-only stream of 65536 symbols (32 bytes in every group: a line every second flush) beside 63 common-only
    ones that are dead for most of it; a common-only stream of 65536 (no line for thousands of groups) beside rare-only ones
    that drain one after the other; and the lane decoder's 64-stream batches at 16 and 14 bits (rare-only, common-only and
    bursts at every count).  At sym_align 64 and 1, without an order (run_row) and under batch_order's (the same result)."""
    R, ctx, torch, _ = gpu
    if isinstance(which, str):
        freqs, counts, contents = rate_wave(16, which)
        row = EL16
    else:
        freqs, counts, contents, _ = L.rate_batch(which)
        row = ENC_LANE_RATE_ROW[which]
    b = Batch(R, ctx, torch, oracle, row, counts, contents=contents, freqs=freqs)
    d_order = ctx.batch_order(b.d_counts)
    for align in (64, 1):
        cont, offs, lens, d_buf, d_sym, d_slot, _, _ = run_row(b, align)
        ordered = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 2, d_slot, d_order=d_order)
        assert ctx.last_encode_kernel()[0] == KERNEL, ctx.last_encode_kernel()
        ctx.encode_status()
        same_result(torch, (cont, offs, lens), ordered, b.n, "under batch_order, align %d" % align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,kernel", [(63, WAVE), (64, KERNEL), (64 * 3 - 5, KERNEL)])
def test_thresholds(gpu, oracle, n, kernel):
    """63 streams report the wave kernel, 64 the lane kernel; 64 k - 5 streams have a partial last wave-load."""
    R, ctx, torch, _ = gpu
    run_row(Batch(R, ctx, torch, oracle, dict(ELMAIN, encode=kernel), draw_lengths(n, 2, 19).clip(0, 3000)), 64)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_no_false_e_model_from_dead_lanes(gpu, oracle):
    """A model without byte value 0, contents that never use it, uneven counts over three wave-loads: dead lanes are fed
    zeros and read the record of byte value 0, which must not reach the flags.  encode_status() is OK (run_row asks) and
    every stream is the oracle's, at sym_align 4 and 1."""
    check_no_false_e_model(gpu, oracle, ENC_LANES, NO_ZERO_LANE_LOADS)
    R, ctx, torch, _ = gpu  # ... and on the quad's load path
    from _batch import no_zero_batch
    freqs, counts, contents = no_zero_batch(*NO_ZERO_LANE_LOADS)
    run_row(Batch(R, ctx, torch, oracle, ELMAIN, counts, contents=contents, freqs=freqs), 64)


@pytest.mark.gpu
def test_true_e_model_is_reported_and_contained(gpu, oracle):
    """The same batch with one symbol of the longest stream of the second wave-load overwritten by 0 on the device: E_MODEL, as
    the default context reports for the same batch; every stream of the other wave-loads is the oracle's; the poison behind
    out_cap is intact; the next call succeeds."""
    check_true_e_model(gpu, oracle, ENC_LANES, NO_ZERO_LANE_LOADS)


@pytest.mark.gpu
def test_order(gpu, oracle):
    """150 streams (two wave-loads and a partial third).  No order, the reversed identity and batch_order's result give the same
    streams, offsets and lengths; an order with one entry replaced by n_streams reports E_ARG, every stream still named is
    exact, and the stream that lost its position keeps its slot's poison and its pre-filled index entries."""
    check_encode_order(gpu, oracle, gpu[1], ELMAIN, draw_lengths(150, 2, 23))


@pytest.mark.gpu
def test_bad_slots(gpu, oracle):
    """test_batch_encode_rejects_bad_slots' construction on 400 2-way rans64 streams with the option on: every slot 32 bytes
    larger than its bound; a slot off 16 bytes on both sides (two streams), one a granule too small, one beyond out_cap -- each
    in a wave-load with valid streams.  E_SPACE, the rejected slots keep their poison and get lengths 0, every other stream is
    exact, the first 16 bytes of every accepted slot are still poison, nothing is written behind the container."""
    check_bad_slots(gpu, oracle, ENC_LANES)


def _streams_equal_prototypes(torch, pb, cont, offs, lens, what):
    """Every stream of a coded PoolBatch, on the device: ends at its slot's end, has its prototype's length and bytes."""
    n = pb.counts.size
    assert torch.equal(lens[:n], pb.d_lens), (what, "lengths differ from the prototypes'")
    ln = pb.d_lens.to(torch.int64)
    assert torch.equal(offs[:n] + ln, pb.d_slot[1:]), (what, "a stream does not end at its slot's end")
    within = torch.arange(int(ln.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln)
    got = cont[torch.repeat_interleave(offs[:n], ln) + within]
    want = pb.cont[torch.repeat_interleave(pb.d_offs, ln) + within]
    assert torch.equal(got, want), (what, "stream bytes differ from the prototypes'")


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer wave-loads than the launch has resident waves (one block of sixteen per CU), prototype lengths log-uniform
    up to 64 Ki with the mandatory ones.  several: at least 1.25 x as many wave-loads as resident waves, so that waves come
    back for further claims and must reset states, ring position and flush count; prototype lengths log-uniform up to 1024.
    Every stream is one of at most 4096 prototypes the oracle coded once (tests/_batch.py's PoolBatch at
    sym_align = 64); every stream of the batch is compared on the device with its prototype's.  The last wave-load is
    partial; with and without d_order; the result decodes back on the wave kernel and, on a third context with
    RANS_AMD_OPT_BATCH_LANES, on k_decode_batch_r64_lanes."""
    import bench
    R, ctx, torch, _ = gpu
    waves = resident_waves(torch) // 2  # CUs x 16
    if regime == "half":
        loads = waves // 16
        protos = draw_lengths(1024, 2, 7)
        assert 0 < loads < waves and set(mandatory_lengths(2)) <= set(protos.tolist())
    else:
        loads = waves + waves // 4 + 1
        protos = draw_log_uniform(POOL, 1024, 9)
        assert 4 * loads >= 5 * waves
    n = loads * 64 - 5
    pb = PoolBatch(R, ctx, torch, oracle, ELMAIN, protos, n, 31, align=64)
    assert pb.counts.size == n and n % 64 != 0 and protos.size <= POOL
    cap = int(pb.slot_offs[-1])
    dec = R.Context(0)
    dec.set_option(OPT_BATCH_LANES, 1)
    try:
        sample = bench.gen_zipf(torch, 1 << 20, ELMAIN["K"], 1.0, 3, "cuda")  # (PoolBatch's model)
        freqs, _ = R.normalize_freqs(dec.count_freqs_device(sample, ELMAIN["K"]), 1 << ELMAIN["sb"])
        gm_dec = dec.model(FMT_R64, freqs, ELMAIN["sb"])
        for order in (None, ctx.batch_order(pb.d_counts)):
            what = "order" if order is not None else "no order"
            cont, offs, lens = ctx.encode_batch(pb.gm, pb.d_buf, pb.d_sym, pb.d_counts, 2, pb.d_slot, d_order=order)
            assert ctx.last_encode_kernel()[0] == KERNEL, ctx.last_encode_kernel()
            ctx.encode_status()
            _streams_equal_prototypes(torch, pb, cont, offs, lens, what)
            for cx, gm, kernel in ((ctx, pb.gm, ELMAIN["decode"]), (dec, gm_dec, LMAIN["decode"])):
                out = torch.full_like(pb.d_buf, POISON)
                cx.decode_batch(gm, cont, cap, offs, lens, pb.d_sym, pb.d_counts, 2, out)
                assert cx.last_decode_kernel() == kernel, cx.last_decode_kernel()
                assert torch.equal(out, pb.d_buf), (what, kernel)
                assert cx.decode_errors() == 0
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("r64-2", 63), ("r64-64", 70), ("r64-search-64", 70), ("byte-2", 70), ("word-8", 70), ("alias256-64", 70)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """Fewer than 64 2-way rans64 streams, the 64-way rans64 rows (cum2sym and, at 20 bits, full-width), the 2-way byte, the
    8-way word and the alias rows take the wave-per-stream kernels on the context with the option on, and code right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, ENC_LANES, rid, n_streams)


@pytest.mark.gpu
def test_per_stream_models_keep_their_kernel_with_the_option_on(gpu, oracle):
    """encode_batch_adaptive of 70 2-way byte streams, each with its own model, on the context with the option on: the wave
    kernel with one model per stream, every stream against the oracle."""
    R, ctx, torch, _ = gpu
    row = MODEL_ROW["byte-2-12bit"]
    assert row["encode"] != KERNEL
    run_model_row(ModelBatch(R, ctx, torch, oracle, row, draw_lengths(70, 2, 37).clip(0, 4096)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_options_are_independent(gpu, oracle):
    """With options 6, 8 and 10 all on, nine 8-way word streams report k_encode_batch_word_groups, forty 2-way byte streams
    k_encode_batch_byte_pairs and seventy 2-way rans64 streams the lane kernel; the decoder's option 9 alone leaves the
    encoder on k_encode_batch<r64>."""
    R, ctx, torch, off = gpu
    ctx.set_option(OPT_BATCH_ENCODE_GROUPS, 1)
    ctx.set_option(OPT_BATCH_ENCODE_PAIRS, 1)
    try:
        assert EROW["encode"] == "k_encode_batch_word_groups" and EMAIN["encode"] == "k_encode_batch_byte_pairs"
        run_row(Batch(R, ctx, torch, oracle, EROW, draw_lengths(9, 8, 43)), 4)
        run_row(Batch(R, ctx, torch, oracle, EMAIN, draw_lengths(40, 2, 47)), 4)
        run_row(Batch(R, ctx, torch, oracle, ELMAIN, draw_lengths(70, 2, 47)), 64)
    finally:
        ctx.set_option(OPT_BATCH_ENCODE_GROUPS, 0)
        ctx.set_option(OPT_BATCH_ENCODE_PAIRS, 0)
    off.set_option(OPT_BATCH_LANES, 1)
    try:
        assert LMAIN["encode"] == WAVE
        run_row(Batch(R, off, torch, oracle, LMAIN, draw_lengths(70, 2, 47)), 64)
    finally:
        off.set_option(OPT_BATCH_LANES, 0)
    assert ctx.decode_errors() == 0 and off.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the lane kernel."""
    check_option_takes_zero_or_one(gpu, oracle, ENC_LANES, align=64)


@pytest.mark.gpu
def test_lane_batch_encode_in_a_captured_graph(tmp_path):
    """One captured encode_batch of 3000 2-way rans64 streams with the option on: one eager call first, then three replays into
    a poison-refilled container, each equal to the eager result (stream bytes, offsets, lengths), in a child process under a
    time limit of its own.  Graph replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set
    below that the test does not apply."""
    run_family_graph(tmp_path, ENC_LANES, "graph_batch_encode_lanes.py")
