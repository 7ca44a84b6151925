"""Ragged batches of the reference's 2-way byte layout CODED with thirty-two streams per wave: k_encode_batch_byte_pairs, the
kernel rans_amd_encode_batch[_ordered] launches on a context with RANS_AMD_OPT_BATCH_ENCODE_PAIRS = 1.

ENC_PAIR_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_encode_pairs_host.py holds
the rows to the names the launchers can report).  The helpers are tests/_batch.py's: run_row checks the reported kernel,
every stream byte for byte against the oracle's, each ending at its slot's end, and decodes the result.  The decoder a row
names is the one the context reports for that shape with the option at its default: "k_decode_batch<byte>" for the 14-bit and
16-bit rows, and for the other three whatever the default context reports (asked at run time, decoder_of; run_row then
asserts it).

The coder works from a stream's last symbol to its first, so a wave's 32 pairs start together and finish at different
times: a pair is finalised (states, last blocks, index entry) right behind its last round and is dead from then on, while
the wave's eight-round sequence -- full exec, every lane's byte count its own two compares -- runs on for the others: a dead
pair's cursor moves, and its lanes keep writing into its ring.  The shapes below are the smallest at which that can go wrong;
the rate inputs are proved to reach their bounds without a GPU by tests/test_batch_encode_pairs_host.py, from the same
generators (tests/_batch.py).

Containers of two encodes are compared over the bytes of their streams: the 16-byte piece that holds a stream's first byte
is stored whole, and what it holds below the stream is whatever the pair's ring held (as with the wave kernels' flushes).
Wall time on an MI355X: 7.3 s for the 40 cases of this file -- 2.7 s of it the captured graph's child process, 1.7 s the first
case's setup and 0.6 s its call (they load the kernels), 0.4 s the `half` regime, 0.26 s the 65536-symbol rare stream beside
dead pairs, 0.13 s the `several` regime and the per-stream-models case, 0.06 s and less for each of the others."""
import numpy as np
import pytest

from _batch import (NO_ZERO_WAVE_LOADS, POISON, POOL, Batch, ModelBatch, PoolBatch, check_bad_slots, check_encode_order, check_no_false_e_model,
                    check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels, check_true_e_model, draw_lengths, draw_log_uniform,
                    finish_batch, mandatory_lengths, option_contexts, padded, rate_batch, rate_wave, resident_waves, run_family_graph,
                    run_model_row, run_row, same_result, wave_load_cases)
from _kernel_rows import (E16, EMAIN, ENC_PAIR_ROWS, ENC_PAIRS, MODEL_ROW, OPT_BATCH_ENCODE_GROUPS, OPT_BATCH_ENCODE_PAIRS, OPT_BATCH_PAIRS,
                          ROW)
from _kernel_rows import PMAIN as DEC_PAIR_ROW
from _oracle import FMT_BYTE

KERNEL, WAVE = EMAIN["encode"], ENC_PAIRS.wave_kernel


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_ENCODE_PAIRS)


_DECODERS = {}


def decoder_of(gpu, oracle, row):
    """The row with the decoder's name filled in: what the default context reports when it decodes the shape."""
    if row["decode"] is not None:
        return row
    if row["id"] not in _DECODERS:
        R, _, torch, off = gpu
        b = Batch(R, off, torch, oracle, dict(row, encode=WAVE), np.array([300] * 33, dtype=np.uint32))
        d_buf, sym_offs, slot_offs = b.laid_out(4)
        d_sym = b.dev(sym_offs, np.int64)
        cont, offs, lens = off.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 2, b.dev(slot_offs, np.int64))
        off.encode_status()
        assert off.last_encode_kernel()[0] == WAVE, off.last_encode_kernel()
        out = torch.full_like(d_buf, b.poison())
        off.decode_batch(b.gm, cont, int(slot_offs[-1]), offs, lens, d_sym, b.d_counts, 2, out)
        assert torch.equal(out, d_buf)
        _DECODERS[row["id"]] = off.last_decode_kernel()
    return dict(row, decode=_DECODERS[row["id"]])


WAVE_LOADS = {
    "one-piece-x4-each": [128] * 32,
    "boundaries": padded(32, [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]),
    "31-dead-one-flushing": [65536] + [255] * 31,
    "every-pair-finishes-elsewhere": [128 * (g + 1) + 3 * g for g in range(32)],
    "quad-mates-differ": [640, 0, 128, 385] * 8,
    "all-empty": [0] * 32,
    "second-load-of-one": [300] * 33,
    "mandatory-and-200s": padded(32, mandatory_lengths(2)),
}


@pytest.mark.parametrize("name,row", list(wave_load_cases(WAVE_LOADS, ENC_PAIR_ROWS, (EMAIN, E16))))
def test_single_wave_loads(gpu, oracle, name, row):
    """One or two wave-loads: four whole pieces each and no tail; every piece and tail boundary in one wave; 31 pairs dead for
    2040 pieces while one keeps flushing; every pair finishing at another piece, some with an odd count; quad-mates that
    differ; 32 empty streams (8 bytes each: the flushed initial states); a second wave-load of one stream; the mandatory
    lengths.  Each at sym_align 1 (every symbol a round at a time, byte loads) and 4."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, decoder_of(gpu, oracle, row), np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in (1, 4):
        run_row(b, align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_dead_pair_at_the_rings_bound(gpu, oracle):
    """finish_batch: every pair finishes at a piece boundary while others run on, and is then fed the frequency-1 symbol 0:
    its lanes write two bytes each in every round, wherever its cursor is.  Every stream equals the oracle's (run_row) -- in
    particular its first 10 bytes, the last written: the two flushed states and the two bytes below them."""
    R, ctx, torch, _ = gpu
    freqs, counts, contents = finish_batch()
    b = Batch(R, ctx, torch, oracle, E16, counts, contents=contents, freqs=freqs)
    cont, offs, lens = run_row(b, 4)[:3]  # (asks encode_status())
    h, h_offs = cont.cpu().numpy(), offs.cpu().numpy()
    for g in range(32):
        a = int(h_offs[g])
        assert b.lens[g] >= 10 and np.array_equal(h[a:a + 10], b.streams[g][:10]), ("states and last bytes of pair", g)
    ctx.encode_status()


def _rate_cases():
    for which in ("fast-beside-parked", "stalled-beside-draining", 16, 14):
        yield pytest.param(which, id=str(which), marks=pytest.mark.gpu)


@pytest.mark.parametrize("which", list(_rate_cases()))
def test_rate_extremes_in_one_wave(gpu, oracle, which):
    """The byte-pair rate inputs (tests/_batch.py) on the encoder: a frequency-1-only stream of 65536 symbols (32 bytes per
    eight rounds: a block per check) beside 31 common-only ones that are dead for most of it; a common-only stream of 65536
    (no block for a thousand rounds and more) beside rare-only ones that drain one after the other; and the 64-stream batches
    at 16 and 14 bits.  At sym_align 4 and 1, without an order (run_row) and under batch_order's (the same result)."""
    R, ctx, torch, _ = gpu
    if isinstance(which, str):
        freqs, counts, contents, _ = rate_wave(16, which)
        row = E16
    else:
        freqs, counts, contents, _ = rate_batch(which)
        row = E16 if which == 16 else EMAIN
    b = Batch(R, ctx, torch, oracle, row, counts, contents=contents, freqs=freqs)
    d_order = ctx.batch_order(b.d_counts)
    for align in (4, 1):
        cont, offs, lens, d_buf, d_sym, d_slot, _, _ = run_row(b, align)
        ordered = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 2, d_slot, d_order=d_order)
        assert ctx.last_encode_kernel()[0] == KERNEL, ctx.last_encode_kernel()
        ctx.encode_status()
        same_result(torch, (cont, offs, lens), ordered, b.n, "under batch_order, align %d" % align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_no_false_e_model_from_dead_pairs(gpu, oracle):
    """A model without byte value 0, contents that never use it, uneven counts: dead pairs are fed zeros and read the record
    of byte value 0, which must not reach the flags.  encode_status() is OK (run_row asks) and every stream is the oracle's,
    at both alignments."""
    check_no_false_e_model(gpu, oracle, ENC_PAIRS, NO_ZERO_WAVE_LOADS)


@pytest.mark.gpu
def test_true_e_model_is_reported_and_contained(gpu, oracle):
    """The same batch with one symbol of the longest stream of the second wave-load overwritten by 0 on the device: E_MODEL, as
    the default context reports for the same batch; every stream of the other wave-loads is the oracle's; the poison behind
    out_cap is intact; the next call succeeds."""
    check_true_e_model(gpu, oracle, ENC_PAIRS, NO_ZERO_WAVE_LOADS)


@pytest.mark.gpu
def test_order(gpu, oracle):
    """70 streams (two wave-loads and a partial third).  No order, the reversed identity and batch_order's result give the same
    streams, offsets and lengths; an order with one entry replaced by n_streams reports E_ARG, every stream still named is
    exact, and the stream that lost its position keeps its slot's poison and its pre-filled index entries."""
    check_encode_order(gpu, oracle, gpu[1], EMAIN, draw_lengths(70, 2, 23))


@pytest.mark.gpu
def test_bad_slots(gpu, oracle):
    """test_batch_encode_rejects_bad_slots' construction on 400 2-way streams with the option on: every slot 32 bytes larger
    than its bound; a slot off 16 bytes on both sides (two streams), one a granule too small, one beyond out_cap -- each in a
    wave-load with valid streams.  E_SPACE, the rejected slots keep their poison and get lengths 0, every other stream is
    exact, the first 16 bytes of every accepted slot are still poison, nothing is written behind the container."""
    check_bad_slots(gpu, oracle, ENC_PAIRS)


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
    """half: fewer wave-loads than the launch has resident waves, prototype lengths log-uniform up to 64 Ki with the
    mandatory ones.  several: at least 1.25 x as many wave-loads as resident waves, so that waves come back for further
    claims and must reset state, cursor, block count and ring; prototype lengths log-uniform up to 1024.  Every stream is one
    of at most 4096 prototypes the oracle coded once (tests/_batch.py PoolBatch); every stream of the batch is
    compared on the device with its prototype's.  The last wave-load is partial; with and without d_order at sym_align = 4;
    the result decodes back on the wave kernel and, on a third context with RANS_AMD_OPT_BATCH_PAIRS, on
    k_decode_batch_byte_pairs."""
    import bench
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
    pb = PoolBatch(R, ctx, torch, oracle, EMAIN, protos, n, 31)
    assert pb.counts.size == n and n % 32 != 0 and protos.size <= POOL
    cap = int(pb.slot_offs[-1])
    dec = R.Context(0)
    dec.set_option(OPT_BATCH_PAIRS, 1)
    try:
        sample = bench.gen_zipf(torch, 1 << 20, EMAIN["K"], 1.0, 3, "cuda")  # (PoolBatch's model)
        freqs, _ = R.normalize_freqs(dec.count_freqs_device(sample, EMAIN["K"]), 1 << EMAIN["sb"])
        gm_dec = dec.model(FMT_BYTE, freqs, EMAIN["sb"])
        for order in (None, ctx.batch_order(pb.d_counts)):
            what = "order" if order is not None else "no order"
            cont, offs, lens = ctx.encode_batch(pb.gm, pb.d_buf, pb.d_sym, pb.d_counts, 2, pb.d_slot, d_order=order)
            assert ctx.last_encode_kernel()[0] == KERNEL, ctx.last_encode_kernel()
            ctx.encode_status()
            _streams_equal_prototypes(torch, pb, cont, offs, lens, what)
            for cx, gm, kernel in ((ctx, pb.gm, EMAIN["decode"]), (dec, gm_dec, DEC_PAIR_ROW["decode"])):
                out = torch.full_like(pb.d_buf, POISON)
                cx.decode_batch(gm, cont, cap, offs, lens, pb.d_sym, pb.d_counts, 2, out)
                assert cx.last_decode_kernel() == kernel, cx.last_decode_kernel()
                assert torch.equal(out, pb.d_buf), (what, kernel)
                assert cx.decode_errors() == 0
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("byte-2", 31), ("byte-64-14bit", 40), ("byte-64-12bit", 40), ("word-8", 40), ("alias256-64", 40), ("r64-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """Fewer than 32 2-way byte streams, the 64-way byte rows, the 8-way word layout, the alias and the rans64 2-way rows take
    the wave-per-stream kernels on the context with the option on, and code right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, ENC_PAIRS, rid, n_streams)


@pytest.mark.gpu
def test_per_stream_models_keep_their_kernel_with_the_option_on(gpu, oracle):
    """encode_batch_adaptive of 40 2-way byte streams, each with its own model, on the context with the option on: the wave
    kernel with one model per stream, every stream against the oracle."""
    R, ctx, torch, _ = gpu
    row = MODEL_ROW["byte-2-12bit"]
    assert row["encode"] != KERNEL
    run_model_row(ModelBatch(R, ctx, torch, oracle, row, draw_lengths(40, 2, 37).clip(0, 4096)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_options_are_independent(gpu, oracle):
    """With RANS_AMD_OPT_BATCH_ENCODE_GROUPS and RANS_AMD_OPT_BATCH_ENCODE_PAIRS both on, nine 8-way word streams report
    k_encode_batch_word_groups and forty 2-way byte streams the pair kernel; the decoder's option 7 alone leaves the encoder
    on k_encode_batch<byte>."""
    R, ctx, torch, off = gpu
    ctx.set_option(OPT_BATCH_ENCODE_GROUPS, 1)
    try:
        word = dict(ROW["word-8"], encode="k_encode_batch_word_groups")
        run_row(Batch(R, ctx, torch, oracle, word, draw_lengths(9, 8, 43)), 4)
        run_row(Batch(R, ctx, torch, oracle, EMAIN, draw_lengths(40, 2, 47)), 4)
    finally:
        ctx.set_option(OPT_BATCH_ENCODE_GROUPS, 0)
    off.set_option(OPT_BATCH_PAIRS, 1)
    try:
        assert DEC_PAIR_ROW["encode"] == WAVE
        run_row(Batch(R, off, torch, oracle, DEC_PAIR_ROW, draw_lengths(40, 2, 47)), 4)
    finally:
        off.set_option(OPT_BATCH_PAIRS, 0)
    assert ctx.decode_errors() == 0 and off.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the pair kernel."""
    check_option_takes_zero_or_one(gpu, oracle, ENC_PAIRS)


@pytest.mark.gpu
def test_pair_batch_encode_in_a_captured_graph(tmp_path):
    """One captured encode_batch of 3000 2-way byte streams with the option on: one eager call first, then three replays into a
    poison-refilled container, each equal to the eager result (stream bytes, offsets, lengths), in a child process under a
    time limit of its own.  Graph replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set
    below that the test does not apply."""
    run_family_graph(tmp_path, ENC_PAIRS, "graph_batch_encode_pairs.py")
