"""Ragged batches of the reference's 2-way rans64 layout with SIXTY-FOUR streams per wave, one per lane:
k_decode_batch_r64_lanes, the kernel rans_amd_decode_batch launches on a context with RANS_AMD_OPT_BATCH_LANES = 1.

LANE_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_lanes_host.py holds the rows to
the registry's family).  The harness is tests/_batch.py's: every decode is checked against the symbols the oracle's
streams were made from, from the GPU's own container and from one the oracle made (shuffled, 4-byte-aligned offsets, gaps),
into a poison-filled buffer whose padding and guard must come back untouched.

A wave's 64 lanes hold 64 streams with 64 different symbol counts: the wave runs the 64-symbol trip max(count >> 6) times, a
lane that has run out of whole trips is parked (it asks for no line, its states, window, cursor and next line are put back
behind every trip, its 64 bytes are not stored) and free-runs on whatever its state becomes; count & 63 symbols follow
sixteen at a time.  A stream whose symbols start on a 64-byte line is stored by its quad, one on the 4-byte grid in 16-byte
pieces by its own lane, any other byte by byte: every shape runs at sym_align 1, 4 and 64.  The rate inputs and the damage
catalogue are tests/_batch_lanes.py's, their bounds and verdicts proved without a GPU by tests/test_batch_lanes_host.py.

Wall time on an MI355X: 7 s for the whole file -- 2.6 s the captured-graph child, 0.6 s the first case (it loads the kernels),
0.3 s the several-rounds batch, 0.2 s the mid-size one, 0.01 to 0.1 s each of the others."""
import functools

import numpy as np
import pytest

import _batch_lanes as L
from _batch import (GUARD, POISON, Batch, Coded, check_decode_order, check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels,
                    check_rate_phase_parking, draw_lengths, draw_log_uniform, option_contexts, resident_waves, run_family_graph, run_row,
                    wave_load_cases)
from _batch_lanes import ALIGNS, WAVE_LOADS
from _kernel_rows import LANE16, LANE_RATE_ROW, LANE_ROWS, LANES, LMAIN, OPT_BATCH_GROUPS, OPT_BATCH_LANES, OPT_BATCH_PAIRS, ROW
from _oracle import FMT_R64

LANE_KERNEL, WAVE_KERNEL = LMAIN["decode"], LANES.wave_kernel  # (the wave kernel: what every row reports with the option off)


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_LANES)


@pytest.mark.parametrize("name,row", list(wave_load_cases(WAVE_LOADS, LANE_ROWS, (LMAIN, LANE16))))
def test_single_wave_loads(gpu, oracle, name, row):
    """One or two wave-loads: one trip each and no tail (every row: 14, 16, 12 and 7 bits, 64 symbols at 10 bits); every trip
    and tail boundary in one wave; 63 lanes parked for 1023 trips while one refills its ring throughout, each owing a
    127-symbol tail afterwards; every lane parking at another trip with another tail; quad-mates parked at different trips
    (the per-member fetches and stores); 64 empty streams; a second wave-load of one stream; the mandatory lengths.  Each at
    sym_align 1 (byte stores), 4 (the lane's own 16-byte pieces) and 64 (the quad's line stores), from the GPU's container and
    from the oracle's."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, row, np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in ALIGNS:
        run_row(b, align)
    assert ctx.decode_errors() == 0
    assert ctx.launch_spans(1)[0] > 0.0, "the launch recorded no span"


@pytest.mark.gpu
def test_63_streams_take_the_wave_kernel(gpu, oracle):
    """One stream short of a wave-load: the wave-per-stream kernel is reported with the option on, and decodes right."""
    R, ctx, torch, _ = gpu
    run_row(Batch(R, ctx, torch, oracle, dict(LMAIN, decode=WAVE_KERNEL), draw_lengths(63, 2, 29)), 64)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sb", L.RATE_BITS)
def test_rate_phase_parking(gpu, oracle, sb):
    """64 streams under 255 x 1 + one common symbol: stream k rare-only (at 16 bits both states take a dword in every round, 32
    bytes per group: what the ring's invariant covers), common-only (nothing at all) or bursts of 16, its count one of
    64 b + t, b in {0, 1, 5}, t in {0, 1, 31, 63}, the oracle's stream at offset == 4 k (mod 64) of a container packed by hand.
    Lanes with b = 0 and b = 1 are parked while their quad- and wave-mates run on at the bound.  Each from three containers at
    sym_align 64, 4 and 1, with and without batch_order, with the option and without; all must equal the input."""
    check_rate_phase_parking(gpu, oracle, LANES, LANE_RATE_ROW[sb], L.rate_batch(sb), (64, 4, 1), start_phases=list(range(0, 64, 4)))


@pytest.mark.gpu
def test_order(gpu, oracle):
    """130 streams (two wave-loads and two streams of a third): the reversed identity, the result of batch_order, and an order
    with one entry replaced by n_streams -- that position is one failed stream, every stream still named decodes right, the
    stream that lost its position is not written."""
    check_decode_order(gpu, oracle, LANES, 130, (4, 64))


@functools.lru_cache(maxsize=None)
def _host_batch(oracle, n):
    return L.HostBatch(oracle, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", L.DAMAGE_KINDS)
@pytest.mark.parametrize("n", L.DAMAGE_LOADS)
def test_damage_is_counted_exactly_and_contained(gpu, oracle, n, kind):
    """One kind of damage on one wave-load (n = 64) or three (192), applied to one stream, to one lane of each quad position,
    to every second stream and to every stream.  The expectation is the CPU's (tests/test_batch_lanes_host.py proves every
    verdict): bad_streams equals the number of damaged streams, through h_bad_streams and, on a second launch without it,
    through decode_errors() once and 0 after; the undamaged streams equal the input; a stream rejected on its index entry or
    its symbol range is not written; a damaged stream that is decoded holds exactly the reference decoder's symbols; padding and
    guard are intact; a healthy call behind the failed ones succeeds.  Nothing here can fault: every read goes through the
    wave-load's bounds-checked window."""
    R, ctx, torch, _ = gpu
    hb = _host_batch(oracle, n)
    gm = ctx.model(FMT_R64, hb.freqs, hb.sb)

    def dev(a, t):
        return torch.from_numpy(np.ascontiguousarray(a).astype(t)).cuda()

    def decode(d, out, **kw):
        ctx.decode_batch(gm, dev(d.cont, np.uint8), hb.container_bytes, dev(d.offs, np.int64), dev(d.lens, np.int32),
                         dev(d.sym_offs, np.int64), dev(d.counts, np.int32), 2, out, out_syms=hb.out_syms, **kw)
        assert ctx.last_decode_kernel() == LANE_KERNEL

    guard = np.full(GUARD, POISON, dtype=np.uint8)
    for pname, which in L.damage_patterns(n).items():
        d = L.Damaged(hb, kind, which)
        want = np.concatenate((d.expected(hb, POISON), guard))
        out = torch.full((hb.out_syms + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        with pytest.raises(R.RansAmdError) as e:
            decode(d, out)
        assert e.value.status == R.E_CORRUPT and e.value.bad_streams == len(which), (pname, e.value.bad_streams, len(which))
        assert ctx.decode_errors() == 0  # (reported and reset by that call)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (pname, "first difference at symbol", int(np.nonzero(got != want)[0][0]))
        out.fill_(POISON)
        decode(d, out, sync=False)
        assert ctx.decode_errors() == len(which) and ctx.decode_errors() == 0, pname
        assert np.array_equal(out.cpu().numpy(), want), pname
    # a healthy call behind the failed ones
    healthy = L.Damaged(hb, kind, [])
    out = torch.full((hb.out_syms + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    decode(healthy, out)
    assert np.array_equal(out.cpu().numpy(), np.concatenate((healthy.expected(hb, POISON), guard))) and ctx.decode_errors() == 0


@pytest.mark.gpu
def test_streams_more_than_a_gibibyte_apart_in_one_wave_load(gpu, oracle):
    """One wave-load whose streams lie in a 1.25 GiB container, the first at its start, the last at its end, 62 spread evenly
    between them: the lanes 2^30 bytes and more above the lowest stream wait for a second pass of the wave over the same claim,
    whose window starts at the lowest of them."""
    R, ctx, torch, _ = gpu
    counts = np.array([64 * (k % 5) + k for k in range(64)], dtype=np.uint32)
    b = Batch(R, ctx, torch, oracle, LMAIN, counts)
    size = 5 << 28
    try:
        cont = torch.zeros(size, dtype=torch.uint8, device="cuda")
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for a 1.25 GiB container on this device: %s" % (e,))
    last = size - 64 - int(b.lens[63])
    starts = (np.arange(64, dtype=np.int64) * (last // 63)) & ~np.int64(3)
    starts[0], starts[63] = 16, last & ~3
    assert int(starts.max() - starts.min()) > (1 << 30) and np.count_nonzero(starts - starts.min() >= (1 << 30)) >= 8
    for c in range(64):
        cont[int(starts[c]):int(starts[c]) + int(b.lens[c])] = torch.from_numpy(b.streams[c]).cuda()
    d_buf, sym_offs, _ = b.laid_out(64)
    d_order = b.dev(np.random.default_rng(3).permutation(64), np.int32)
    for order in (None, d_order):
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, cont, size, b.dev(starts, np.int64), b.dev(b.lens, np.int32), b.dev(sym_offs, np.int64), b.d_counts, 2,
                         out, d_order=order)
        assert ctx.last_decode_kernel() == LANE_KERNEL
        assert torch.equal(out, d_buf)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_mid_size_batch(gpu, oracle):
    """4096 streams, log-uniform up to 64 Ki symbols with the mandatory lengths: 64 wave-loads, with and without d_order, at
    sym_align 64, from the GPU's container and from the oracle's."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, LMAIN, draw_lengths(4096, 2, 7))
    c = Coded(b, 64)
    c.decode_all(None, "no order")
    c.decode_all(ctx.batch_order(b.d_counts), "batch_order")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_several_rounds_of_the_grid(gpu, oracle):
    """More wave-loads than the launch has waves (at least 1.25 x 16 waves per CU), so that waves come back for further claims:
    every stream is one of 512 prototypes of up to 1024 symbols the oracle coded once; index and expected output are put
    together on the device.  The last wave-load is partial; with and without d_order, at sym_align 4."""
    R, ctx, torch, _ = gpu
    waves = resident_waves(torch) // 2  # CUs x 16
    loads = waves + waves // 4 + 1
    n = loads * 64 - 5
    protos = draw_log_uniform(512, 1024, 9)
    b = Batch(R, ctx, torch, oracle, LMAIN, protos)
    o_cont, o_starts, o_bytes = b.oracle_container()
    rng = np.random.default_rng(31)
    pick = np.concatenate((np.arange(512), rng.integers(0, 512, n - 512)))[rng.permutation(n)]
    counts = protos[pick]
    sym_offs, _ = R.batch_layout(counts, FMT_R64, 2, 4)
    d_counts, d_sym = b.dev(counts.view(np.int32), np.int32), b.dev(sym_offs, np.int64)
    reps = d_counts.to(torch.int64)
    within = torch.arange(int(reps.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(reps, 0) - reps, reps)
    want = torch.full((int(sym_offs[-1]) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    want[torch.repeat_interleave(d_sym[:-1], reps) + within] = b.d_dense[torch.repeat_interleave(b.dev(b.dense_offs[pick], np.int64), reps) + within]
    d_cont, d_offs, d_lens = b.dev(o_cont, np.uint8), b.dev(o_starts[pick], np.int64), b.dev(b.lens[pick], np.int32)
    for order in (None, ctx.batch_order(d_counts)):
        out = torch.full_like(want, POISON)
        ctx.decode_batch(b.gm, d_cont, o_bytes, d_offs, d_lens, d_sym, d_counts, 2, out, d_order=order)
        assert ctx.last_decode_kernel() == LANE_KERNEL
        assert torch.equal(out, want), "order" if order is not None else "no order"
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("r64-64", 70), ("r64-search-64", 70), ("byte-2", 70), ("word-8", 70)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """The 64-way rans64 rows (cum2sym and search), the 2-way byte and the 8-way word layout take the wave-per-stream kernels on
    the context with the option on, and decode right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, LANES, rid, n_streams)


@pytest.mark.gpu
def test_option_nine_is_independent_of_five_and_seven(gpu, oracle):
    """With RANS_AMD_OPT_BATCH_GROUPS, RANS_AMD_OPT_BATCH_PAIRS and RANS_AMD_OPT_BATCH_LANES all on, nine 8-way word streams
    report the group kernel, forty 2-way byte streams the pair kernel and seventy 2-way rans64 streams the lane kernel."""
    R, ctx, torch, _ = gpu
    ctx.set_option(OPT_BATCH_GROUPS, 1)
    ctx.set_option(OPT_BATCH_PAIRS, 1)
    try:
        run_row(Batch(R, ctx, torch, oracle, dict(ROW["word-8"], decode="k_decode_batch_word_groups"), draw_lengths(9, 8, 43)), 4)
        run_row(Batch(R, ctx, torch, oracle, dict(ROW["byte-2"], decode="k_decode_batch_byte_pairs"), draw_lengths(40, 2, 47)), 4)
        run_row(Batch(R, ctx, torch, oracle, LMAIN, draw_lengths(70, 2, 53)), 4)
    finally:
        ctx.set_option(OPT_BATCH_GROUPS, 0)
        ctx.set_option(OPT_BATCH_PAIRS, 0)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the lane kernel."""
    check_option_takes_zero_or_one(gpu, oracle, LANES, align=64)


@pytest.mark.gpu
def test_lane_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 2-way rans64 streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    run_family_graph(tmp_path, LANES, "graph_batch_lanes.py")
