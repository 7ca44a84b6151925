"""Ragged batches of the reference's 2-way ALIAS layout (main_alias.cpp) CODED with thirty-two streams per wave:
k_encode_batch_alias_pairs, the kernel rans_amd_encode_batch[_ordered] launches on a context with
RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS = 1.  The counterpart of tests/test_gpu_batch_encode_pairs.py, case for case, on the
descriptor and rows of tests/_batch_encode_alias_pairs.py.

ENC_ALIAS_PAIR_ROWS names the kernel the library must report (tests/test_batch_encode_alias_pairs_host.py holds the rows to the
registry's third list).  The helpers are tests/_batch.py's: run_row checks the reported kernel, every stream byte for byte
against the oracle's, each ending at its slot's end, and decodes the result on k_decode_batch<alias>.

The plan is the byte pairs' -- a pair is finalised right behind its last round and is dead from then on, while the wave's
eight-round sequence runs on under full exec -- and what is new is the put: one more gather, from remap16 in LDS, whose index a
dead pair, a pair without a stream and a byte value without a record fill with garbage.  The rows cover the block shapes (two
blocks of 16 waves per CU up to 14 bits, one at 15, one of 13 waves at 16 bits: test_every_scale_bits walks all nine) and the
records (frequency 1 throughout at 8 bits; byte values 64..255 without a record under the 64-symbol model).  The rate inputs are
proved to reach their bounds AS ALIAS STREAMS without a GPU by tests/test_batch_encode_alias_pairs_host.py, from the same
generators (tests/_batch.py).

Containers of two encodes are compared over the bytes of their streams: the 16-byte piece that holds a stream's first byte is
stored whole, and what it holds below the stream is whatever the pair's ring held.
Wall time on an MI355X: 7.0 s for the 51 cases of this file -- 2.4 s of it the captured graph's child process, 0.8 s the first
case's setup and call (they load the kernels), 0.3 s the `half` regime, 0.24 s `several`, 0.23 s the 65536-symbol rare stream
beside dead pairs, 0.06 s and less for each of the others."""
import numpy as np
import pytest

from _batch import (NO_ZERO_WAVE_LOADS, POISON, POOL, Batch, ModelBatch, PoolBatch, check_bad_slots, check_encode_order, check_no_false_e_model,
                    check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels, check_true_e_model, draw_lengths, draw_log_uniform,
                    encode_poisoned, finish_batch, mandatory_lengths, option_contexts, rate_batch, rate_wave, resident_waves, run_family_graph,
                    run_model_row, run_row, same_result, wave_load_cases)
from _batch_alias_pairs import AMAIN as DEC_ALIAS_PAIR_ROW
from _batch_alias_pairs import OPT_BATCH_ALIAS_PAIRS, AliasOracle
from _batch_encode_alias_pairs import (ALIAS_2_WAVE, ALIAS_U16_2_WAVE, EA14, EA64, EAMAIN, ENC_ALIAS_PAIR_RATE_ROW, ENC_ALIAS_PAIR_ROWS,
                                       ENC_ALIAS_PAIRS, OPT_BATCH_ENCODE_ALIAS_PAIRS, ad_hoc_row, lds_plan)
from _kernel_rows import EMAIN as ENC_BYTE_PAIR_ROW
from _kernel_rows import MODEL_ROW, OPT_BATCH_ENCODE_PAIRS, ROW
from _oracle import FMT_ALIAS
from test_gpu_batch_encode_pairs import WAVE_LOADS, _streams_equal_prototypes

KERNEL, WAVE = EAMAIN["encode"], ENC_ALIAS_PAIRS.wave_kernel
ENC_ALIAS_PAIRS_14 = ENC_ALIAS_PAIRS._replace(main=EA14)  # (the no-zero inputs are 14-bit models)


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_ENCODE_ALIAS_PAIRS)


@pytest.mark.parametrize("name,row", list(wave_load_cases(WAVE_LOADS, ENC_ALIAS_PAIR_ROWS, (EAMAIN, EA14))))
def test_single_wave_loads(gpu, oracle, name, row):
    """The byte file's wave-loads: four whole pieces each and no tail (every row); every piece and tail boundary in one wave; 31
    pairs dead for 2040 pieces while one keeps flushing; every pair finishing at another piece, some with an odd count;
    quad-mates that differ; 32 empty streams (8 bytes each: the flushed initial states); a second wave-load of one stream; the
    mandatory lengths -- on the 16-bit main row (a block of 13 waves) and the 14-bit row (two blocks of 16 per CU).  Each at
    sym_align 1 (every symbol a round at a time, byte loads) and 4."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, row, np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in (1, 4):
        run_row(b, align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_dead_pair_at_the_rings_bound(gpu, oracle):
    """finish_batch: every pair finishes at a piece boundary while others run on, and is then fed the frequency-1 symbol 0: its
    lanes write two bytes each in every round, wherever its cursor is, and gather with whatever its state has become.  Every
    stream equals the oracle's (run_row) -- in particular its first 10 bytes, the last written: the two flushed states and the
    two bytes below them."""
    R, ctx, torch, _ = gpu
    freqs, counts, contents = finish_batch()
    b = Batch(R, ctx, torch, oracle, EAMAIN, counts, contents=contents, freqs=freqs)
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
    """The pair rate inputs (tests/_batch.py) as alias streams: a frequency-1-only stream of 65536 symbols (32 bytes per eight
    rounds: a block per check) beside 31 common-only ones that are dead for most of it; a common-only stream of 65536 (no block
    for a thousand rounds and more) beside rare-only ones that drain one after the other; and the 64-stream batches at 16 and
    14 bits.  At sym_align 4 and 1, without an order (run_row) and under batch_order's (the same result)."""
    R, ctx, torch, _ = gpu
    if isinstance(which, str):
        freqs, counts, contents, _ = rate_wave(16, which)
        row = ENC_ALIAS_PAIR_RATE_ROW[16]
    else:
        freqs, counts, contents, _ = rate_batch(which)
        row = ENC_ALIAS_PAIR_RATE_ROW[which]
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
    """A model without byte value 0, contents that never use it, uneven counts: dead pairs are fed zeros and read the record of
    byte value 0, which must not reach the flags.  encode_status() is OK (run_row asks) and every stream is the oracle's, at
    both alignments."""
    check_no_false_e_model(gpu, oracle, ENC_ALIAS_PAIRS_14, NO_ZERO_WAVE_LOADS)


@pytest.mark.gpu
def test_true_e_model_is_reported_and_contained(gpu, oracle):
    """The same batch with one symbol of the longest stream of the second wave-load overwritten by 0 on the device: E_MODEL, as
    the default context reports for the same batch; every stream of the other wave-loads is the oracle's; the poison behind
    out_cap is intact; the next call succeeds."""
    check_true_e_model(gpu, oracle, ENC_ALIAS_PAIRS_14, NO_ZERO_WAVE_LOADS)


@pytest.mark.gpu
@pytest.mark.parametrize("align", [4, 1])
def test_no_record_symbols_in_every_pair(gpu, oracle, align):
    """One wave-load under the 64-symbol model at 10 bits, every stream with byte values 64..255 -- values without a record -- at
    drawn places, overwritten on the device: the gather's index is garbage on all 64 lanes.  E_MODEL, as the default context
    reports for the same batch; every slot is 32 bytes larger than its bound and those 32 bytes keep their poison (whatever a
    state becomes, a lane emits at most two bytes per round: a stream stays inside rans_amd_chunk_bound()); every index entry
    says a stream inside its slot that ends at the slot's end; nothing is written behind out_cap; and the next call, on the
    clean symbols, is clean and exact."""
    R, ctx, torch, off = gpu
    counts = np.array([(37 * k * k + 11 * k) % 1500 + 40 for k in range(32)], dtype=np.uint32)
    b = Batch(R, ctx, torch, oracle, EA64, counts)
    gm_off = off.model(FMT_ALIAS, b.freqs, EA64["sb"])
    d_buf, sym_offs, slot_offs = b.laid_out(align)
    bound = np.array([R.chunk_bound(FMT_ALIAS, int(c), 2) for c in counts], dtype=np.int64)
    idx = np.concatenate(([0], np.cumsum(bound + 32))).astype(np.int64)
    cap = int(idx[-1])
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(idx, np.int64)
    bad = d_buf.clone()
    rng = np.random.default_rng(97)
    for c in range(32):
        n = int(counts[c])
        at = rng.choice(n, size=n // 8 + 1, replace=False) + int(sym_offs[c])
        bad[torch.from_numpy(at.astype(np.int64)).cuda()] = torch.from_numpy(rng.integers(64, 256, at.size).astype(np.uint8)).cuda()
    for cx, gm, kernel in ((ctx, b.gm, KERNEL), (off, gm_off, WAVE)):
        cont, offs, lens = encode_poisoned(b, cx, gm, bad, d_sym, d_slot, cap)
        assert cx.last_encode_kernel()[0] == kernel, cx.last_encode_kernel()
        with pytest.raises(R.RansAmdError) as e:
            cx.encode_status()
        assert e.value.status == R.E_MODEL, kernel
        h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy().view(np.uint32)
        for c in range(32):
            lo, hi = int(idx[c]), int(idx[c + 1])
            assert np.all(h[lo:lo + 32] == POISON), (kernel, "written below the slot's bound", c)
            assert 8 <= int(h_lens[c]) <= bound[c] and int(h_offs[c]) == hi - int(h_lens[c]), (kernel, c, int(h_lens[c]))
        assert np.all(h[cap:] == POISON), (kernel, "written behind the container")
    cont, offs, lens = encode_poisoned(b, ctx, b.gm, d_buf, d_sym, d_slot, cap)  # the next call, on the clean symbols
    assert ctx.last_encode_kernel()[0] == KERNEL
    ctx.encode_status()
    h_offs, h_lens = offs.cpu().numpy().astype(np.uint64), lens.cpu().numpy().view(np.uint32)
    assert np.array_equal(h_offs + h_lens, idx[1:].astype(np.uint64))
    b.check_streams(cont.cpu().numpy(), h_offs, h_lens, "the call behind the failed one")


@pytest.mark.gpu
@pytest.mark.parametrize("sb", list(range(8, 17)))
def test_every_scale_bits(gpu, oracle, sb):
    """70 streams of drawn lengths (two wave-loads and a partial third) at every scale_bits the kernel takes, not only the five
    rows': the block is two of 16 waves per CU up to 14 bits, one at 15 and one of 13 waves at 16 (the plan a g++ driver prints),
    and remap16 doubles with every bit.  Every stream is the oracle's, byte for byte, and decodes back."""
    R, ctx, torch, _ = gpu
    waves, per_cu = lds_plan()[sb][1], lds_plan()[sb][3]
    assert (waves, per_cu) == ((16, 2) if sb <= 14 else (16, 1) if sb == 15 else (13, 1))
    run_row(Batch(R, ctx, torch, oracle, ad_hoc_row(sb), draw_lengths(70, 2, 23)), 4)  # (asserts the kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_order(gpu, oracle):
    """70 streams (two wave-loads and a partial third).  No order, the reversed identity and batch_order's result give the same
    streams, offsets and lengths; an order with one entry replaced by n_streams reports E_ARG, every stream still named is
    exact, and the stream that lost its position keeps its slot's poison and its pre-filled index entries."""
    check_encode_order(gpu, oracle, gpu[1], EAMAIN, draw_lengths(70, 2, 23))


@pytest.mark.gpu
def test_bad_slots(gpu, oracle):
    """test_batch_encode_rejects_bad_slots' construction on 400 2-way alias streams with the option on: every slot 32 bytes
    larger than its bound; a slot off 16 bytes on both sides (two streams), one a granule too small, one beyond out_cap -- each
    in a wave-load with valid streams.  E_SPACE, the rejected slots keep their poison and get lengths 0, every other stream is
    exact, the first 16 bytes of every accepted slot are still poison, nothing is written behind the container."""
    check_bad_slots(gpu, oracle, ENC_ALIAS_PAIRS)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer wave-loads than the launch has resident waves, prototype lengths log-uniform up to 64 Ki with the mandatory
    ones.  several: at least 1.25 x as many wave-loads as resident waves -- on the 16-BIT row, whose block is 13 waves, one per
    CU: every wave comes back for further claims and must reset state, cursor, block count and ring; prototype lengths
    log-uniform up to 1024.  Every stream is one of at most 4096 prototypes the oracle coded once (tests/_batch.py PoolBatch,
    with alias tables in its model); every stream of the batch is compared on the device with its prototype's.  The last
    wave-load is partial; with and without d_order at sym_align = 4; the result decodes back on the wave kernel and, on a third
    context with RANS_AMD_OPT_BATCH_ALIAS_PAIRS, on k_decode_batch_alias_pairs."""
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
    assert EAMAIN["sb"] == 16
    pb = PoolBatch(R, ctx, torch, AliasOracle(oracle), EAMAIN, protos, n, 31)
    assert pb.counts.size == n and n % 32 != 0 and protos.size <= POOL
    cap = int(pb.slot_offs[-1])
    dec = R.Context(0)
    dec.set_option(OPT_BATCH_ALIAS_PAIRS, 1)
    try:
        sample = bench.gen_zipf(torch, 1 << 20, EAMAIN["K"], 1.0, 3, "cuda")  # (PoolBatch's model)
        freqs, _ = R.normalize_freqs(dec.count_freqs_device(sample, EAMAIN["K"]), 1 << EAMAIN["sb"])
        gm_dec = dec.model(FMT_ALIAS, freqs, EAMAIN["sb"])
        for order in (None, ctx.batch_order(pb.d_counts)):
            what = "order" if order is not None else "no order"
            cont, offs, lens = ctx.encode_batch(pb.gm, pb.d_buf, pb.d_sym, pb.d_counts, 2, pb.d_slot, d_order=order)
            assert ctx.last_encode_kernel()[0] == KERNEL, ctx.last_encode_kernel()
            ctx.encode_status()
            _streams_equal_prototypes(torch, pb, cont, offs, lens, what)
            for cx, gm, kernel in ((ctx, pb.gm, EAMAIN["decode"]), (dec, gm_dec, DEC_ALIAS_PAIR_ROW["decode"])):
                out = torch.full_like(pb.d_buf, POISON)
                cx.decode_batch(gm, cont, cap, offs, lens, pb.d_sym, pb.d_counts, 2, out)
                assert cx.last_decode_kernel() == kernel, cx.last_decode_kernel()
                assert torch.equal(out, pb.d_buf), (what, kernel)
                assert cx.decode_errors() == 0
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("alias256-64", 40), ("byte-2", 40), ("word-8", 40), ("r64-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """The 64-way alias row, and one byte, word and rans64 shape each, take the wave-per-stream kernels on the context with the
    option on, and code right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, ENC_ALIAS_PAIRS, rid, n_streams)


@pytest.mark.gpu
@pytest.mark.parametrize("row,n_streams", [(ALIAS_2_WAVE, 31), (ALIAS_U16_2_WAVE, 40)], ids=["alias-2-31-streams", "alias-u16-2"])
def test_alias_shapes_the_kernel_does_not_take(gpu, oracle, row, n_streams):
    """Fewer than 32 2-way alias streams of the main row's shape, and forty 2-way alias streams over u16 symbols (1024 of them),
    keep k_encode_batch<alias, LDS remap> with the option on, and code right."""
    R, ctx, torch, _ = gpu
    assert row["encode"] != KERNEL
    run_row(Batch(R, ctx, torch, oracle, row, draw_lengths(n_streams, 2, 29).clip(0, 8192)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


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
    """With only option 12 on, forty 2-way byte streams keep k_encode_batch<byte> and forty 2-way alias streams take the alias
    pairs; with RANS_AMD_OPT_BATCH_ENCODE_PAIRS on as well the byte streams take the byte pairs and the alias streams still the
    alias pairs; the decoder's option 11 alone leaves the encoder on k_encode_batch<alias, LDS remap>."""
    R, ctx, torch, off = gpu
    counts = draw_lengths(40, 2, 47)
    run_row(Batch(R, ctx, torch, oracle, ROW["byte-2"], counts), 4)
    run_row(Batch(R, ctx, torch, oracle, EAMAIN, counts), 4)
    ctx.set_option(OPT_BATCH_ENCODE_PAIRS, 1)
    try:
        run_row(Batch(R, ctx, torch, oracle, ENC_BYTE_PAIR_ROW, counts), 4)
        run_row(Batch(R, ctx, torch, oracle, EAMAIN, counts), 4)
    finally:
        ctx.set_option(OPT_BATCH_ENCODE_PAIRS, 0)
    off.set_option(OPT_BATCH_ALIAS_PAIRS, 1)
    try:
        assert DEC_ALIAS_PAIR_ROW["encode"] == WAVE
        run_row(Batch(R, off, torch, oracle, DEC_ALIAS_PAIR_ROW, counts), 4)
    finally:
        off.set_option(OPT_BATCH_ALIAS_PAIRS, 0)
    assert ctx.decode_errors() == 0 and off.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG, in the other families' words, and changes nothing; 0 restores the wave-per-stream kernel, 1 the
    alias pairs."""
    R, ctx, _, _ = gpu
    check_option_takes_zero_or_one(gpu, oracle, ENC_ALIAS_PAIRS)
    with pytest.raises(R.RansAmdError) as e:
        ctx.set_option(OPT_BATCH_ENCODE_ALIAS_PAIRS, 2)
    assert "RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS takes 0 (one stream per wave) or 1 (thirty-two 2-way alias streams per wave)" in str(e.value)


@pytest.mark.gpu
def test_alias_pair_batch_encode_in_a_captured_graph(tmp_path):
    """One captured encode_batch of 3000 2-way alias streams with the option on: one eager call first, then three replays into a
    poison-refilled container, each equal to the eager result (stream bytes, offsets, lengths), in a child process under a
    time limit of its own.  Graph replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set
    below that the test does not apply."""
    run_family_graph(tmp_path, ENC_ALIAS_PAIRS, "graph_batch_encode_alias_pairs.py")
