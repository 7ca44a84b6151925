"""Ragged batches of the NON-INTERLEAVED layout every reference program writes first (one rANS state per stream) with SIXTY-FOUR
streams per wave, one per lane: k_decode_batch_singles<byte|word|r64|alias>, the kernels rans_amd_decode_batch launches on a
context with RANS_AMD_OPT_BATCH_SINGLES = 1.  One descriptor per format (tests/_batch_singles.py), every test over the four.

SINGLE_ROWS names the kernel the library must report (tests/test_batch_singles_host.py holds the rows to the registry's fourth
list).  The harness is tests/_batch.py's: every decode is checked against the symbols the oracle's streams were made from,
from the GPU's own container (the wave encoder's) and from one the oracle made (shuffled, unit-aligned offsets, gaps), into a
poison-filled buffer whose padding and guard must come back untouched.

A wave's 64 lanes hold 64 streams with 64 different symbol counts: the wave runs the 64-symbol trip max(count >> 6) times, a
lane takes part while it has whole trips left and requests no line afterwards; count & 63 symbols follow sixteen at a time.  A
stream whose symbols start on a 64-byte line is stored by its quad, one on the 4-byte grid in 16-byte pieces by its own lane,
any other byte by byte: every shape runs at sym_align 1, 4 and 64.  The rate inputs and the damage catalogue are
tests/_batch_singles.py's, their bounds and verdicts proved without a GPU by tests/test_batch_singles_host.py.  By construction
nothing here can fault: every read goes through the wave-load's bounds-checked window, every write lies inside a validated
stream's own symbol range.

Wall time on an MI355X: 12 s for the whole file, all four formats (169 cases; about 3 s per format) -- 2.3 s the captured-graph
child, 0.6 s the first case (it loads the kernels), 0.3 to 0.4 s each 4096-stream batch, 0.2 s each order test and the
several-rounds batches, 0.01 to 0.14 s each of the others."""
import functools

import numpy as np
import pytest

import _batch_singles as N
from _batch import (GUARD, POISON, Batch, Coded, check_decode_order, check_option_takes_zero_or_one, check_other_shape_keeps_its_kernels,
                    check_rate_phase_parking, draw_lengths, draw_log_uniform, option_contexts, resident_waves, run_family_graph, run_row,
                    wave_load_cases)
from _batch_alias_pairs import AMAIN, OPT_BATCH_ALIAS_PAIRS
from _batch_singles import ALIGNS, FORMATS, MAIN, OPT_BATCH_SINGLES, SINGLES, WAVE_LOADS
from _kernel_rows import LMAIN, OPT_BATCH_GROUPS, OPT_BATCH_LANES, OPT_BATCH_PAIRS, PMAIN, ROW


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_SINGLES)


def _wave_load_cases():
    for f in FORMATS:
        rows = N.SINGLE_ROWS[f]
        yield from wave_load_cases(WAVE_LOADS, rows, (rows[0], N.RATE_ROW[f]) if N.RATE_ROW[f] is not rows[0] else (rows[0],))


@pytest.mark.parametrize("name,row", list(_wave_load_cases()))
def test_single_wave_loads(gpu, oracle, name, row):
    """One or two wave-loads: one trip each and no tail (every row of every format); every trip and tail boundary in one wave;
    63 lanes idle for 1023 trips while one refills its ring throughout, each owing a 127-symbol tail afterwards; every lane
    finishing at another trip with another tail; quad-mates that finish at different trips (the per-member stores); 64 empty
    streams; a second wave-load of one stream; the mandatory lengths -- on each format's main row and its 16-bit row.  Each at
    sym_align 1 (byte stores), 4 (the lane's own 16-byte pieces) and 64 (the quad's line stores), from the GPU's container and
    from the oracle's."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, row, np.array(WAVE_LOADS[name], dtype=np.uint32))
    for align in ALIGNS:
        run_row(b, align)
    assert ctx.decode_errors() == 0
    assert ctx.launch_spans(1)[0] > 0.0, "the launch recorded no span"


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_63_streams_take_the_wave_kernel(gpu, oracle, f):
    """One stream short of a wave-load: the wave-per-stream kernel is reported with the option on, and decodes right."""
    R, ctx, torch, _ = gpu
    run_row(Batch(R, ctx, torch, oracle, dict(MAIN[f], decode=SINGLES[f].wave_kernel), draw_lengths(63, 1, 29).clip(0, 8192)), 64)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_rate_phase(gpu, oracle, f):
    """64 streams under 255 x 1 + one common symbol (16 bits; the word format's 12): stream k rare-only (32 bytes per group of
    sixteen symbols, the word format 24: the most a valid stream takes), common-only (nothing, or next to nothing) or bursts
    of 16, its count one of 64 b + t, b in {0, 1, 5}, t in {0, 1, 31, 63}, the oracle's stream at offset == k * unit (mod 64)
    of a container packed by hand: every unit phase of a 64-byte line.  Lanes with b = 0 and b = 1 request nothing while their
    quad- and wave-mates run on at the bound.  Each from three containers at sym_align 64, 4 and 1, with and without
    batch_order, with the option and without; all must equal the input."""
    unit = N.UNIT[N.FMT[f]]
    check_rate_phase_parking(gpu, oracle, SINGLES[f], N.RATE_ROW[f], N.rate_batch(f), (64, 4, 1), start_phases=list(range(0, 64, unit)))


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_order(gpu, oracle, f):
    """130 streams (two wave-loads and two streams of a third): the reversed identity, the result of batch_order, and an order
    with one entry replaced by n_streams -- that position is one failed stream, every stream still named decodes right, the
    stream that lost its position is not written."""
    check_decode_order(gpu, oracle, SINGLES[f], 130, (4, 64))


@functools.lru_cache(maxsize=None)
def _host_batch(oracle, f, n):
    return N.HostBatch(oracle, f, n)


def _damage_cases():
    for f in FORMATS:
        for n in N.DAMAGE_LOADS:
            for kind in N.damage_kinds(f):
                yield pytest.param(f, n, kind, id="%s-%d-%s" % (f, n, kind), marks=pytest.mark.gpu)


@pytest.mark.parametrize("f,n,kind", list(_damage_cases()))
def test_damage_is_counted_exactly_and_contained(gpu, oracle, f, n, kind):
    """One kind of damage on one wave-load (n = 64) or three (192), applied to one stream, to one lane of each quad position,
    to every second stream and to every stream.  The expectation is the CPU's (tests/test_batch_singles_host.py proves every
    verdict): bad_streams equals the number of damaged streams, through h_bad_streams and, on a second launch without it,
    through decode_errors() once and 0 after; the undamaged streams equal the input; a stream rejected on its index entry or
    its symbol range is not written; a damaged stream that is decoded holds exactly the reference decoder's symbols; padding and
    guard are intact; a healthy call behind the failed ones succeeds."""
    R, ctx, torch, _ = gpu
    hb = _host_batch(oracle, f, n)
    gm = ctx.model(hb.fmt, hb.freqs, hb.sb)

    def dev(a, t):
        return torch.from_numpy(np.ascontiguousarray(a).astype(t)).cuda()

    def decode(d, out, **kw):
        ctx.decode_batch(gm, dev(d.cont, np.uint8), hb.container_bytes, dev(d.offs, np.int64), dev(d.lens, np.int32),
                         dev(d.sym_offs, np.int64), dev(d.counts, np.int32), 1, out, out_syms=hb.out_syms, **kw)
        assert ctx.last_decode_kernel() == N.KERNEL[f]

    guard = np.full(GUARD, POISON, dtype=np.uint8)
    for pname, which in N.damage_patterns(n).items():
        d = N.Damaged(hb, kind, which)
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
    healthy = N.Damaged(hb, kind, [])
    out = torch.full((hb.out_syms + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    decode(healthy, out)
    assert np.array_equal(out.cpu().numpy(), np.concatenate((healthy.expected(hb, POISON), guard))) and ctx.decode_errors() == 0


@pytest.mark.gpu
def test_streams_more_than_a_gibibyte_apart_in_one_wave_load(gpu, oracle):
    """The byte format: one wave-load whose streams lie in a 1.25 GiB container at ODD offsets, the first at its start, the last
    at its end, 62 spread evenly between them: the lanes 2^30 bytes and more above the lowest stream wait for a second pass of
    the wave over the same claim, whose window starts at the lowest of them.  With and without an order."""
    R, ctx, torch, _ = gpu
    counts = np.array([64 * (k % 5) + k for k in range(64)], dtype=np.uint32)
    b = Batch(R, ctx, torch, oracle, MAIN["byte"], counts)
    size = 5 << 28
    cont = torch.zeros(size, dtype=torch.uint8, device="cuda")
    last = size - 64 - int(b.lens[63])
    starts = (np.arange(64, dtype=np.int64) * (last // 63)) | 1
    starts[0], starts[63] = 17, last | 1
    assert np.all(starts % 2 == 1) and int(starts[63]) + int(b.lens[63]) <= size
    assert int(starts.max() - starts.min()) > (1 << 30) and np.count_nonzero(starts - starts.min() >= (1 << 30)) >= 8
    for c in range(64):
        cont[int(starts[c]):int(starts[c]) + int(b.lens[c])] = torch.from_numpy(b.streams[c]).cuda()
    d_buf, sym_offs, _ = b.laid_out(64)
    d_order = b.dev(np.random.default_rng(3).permutation(64), np.int32)
    for order in (None, d_order):
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, cont, size, b.dev(starts, np.int64), b.dev(b.lens, np.int32), b.dev(sym_offs, np.int64), b.d_counts, 1,
                         out, d_order=order)
        assert ctx.last_decode_kernel() == N.KERNEL["byte"]
        assert torch.equal(out, d_buf)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_mid_size_batch(gpu, oracle, f):
    """4096 streams, log-uniform up to 64 Ki symbols with the mandatory lengths: 64 wave-loads, with and without d_order, at
    sym_align 64, from the GPU's container and from the oracle's."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, MAIN[f], draw_lengths(4096, 1, 7))
    c = Coded(b, 64)
    c.decode_all(None, "no order")
    c.decode_all(ctx.batch_order(b.d_counts), "batch_order")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_several_rounds_of_the_grid(gpu, oracle, f):
    """More wave-loads than the launch has waves (at least 1.25 x 16 waves per CU), so that waves come back for further claims:
    every stream is one of 512 prototypes of up to 1024 symbols the oracle coded once; index and expected output are put
    together on the device.  The last wave-load is partial; with and without d_order, at sym_align 4."""
    R, ctx, torch, _ = gpu
    waves = resident_waves(torch) // 2  # CUs x 16
    loads = waves + waves // 4 + 1
    n = loads * 64 - 5
    protos = draw_log_uniform(512, 1024, 9)
    b = Batch(R, ctx, torch, oracle, MAIN[f], protos)
    o_cont, o_starts, o_bytes = b.oracle_container()
    rng = np.random.default_rng(31)
    pick = np.concatenate((np.arange(512), rng.integers(0, 512, n - 512)))[rng.permutation(n)]
    counts = protos[pick]
    sym_offs, _ = R.batch_layout(counts, N.FMT[f], 1, 4)
    d_counts, d_sym = b.dev(counts.view(np.int32), np.int32), b.dev(sym_offs, np.int64)
    reps = d_counts.to(torch.int64)
    within = torch.arange(int(reps.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(reps, 0) - reps, reps)
    want = torch.full((int(sym_offs[-1]) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    want[torch.repeat_interleave(d_sym[:-1], reps) + within] = b.d_dense[torch.repeat_interleave(b.dev(b.dense_offs[pick], np.int64), reps) + within]
    d_cont, d_offs, d_lens = b.dev(o_cont, np.uint8), b.dev(o_starts[pick], np.int64), b.dev(b.lens[pick], np.int32)
    for order in (None, ctx.batch_order(d_counts)):
        out = torch.full_like(want, POISON)
        ctx.decode_batch(b.gm, d_cont, o_bytes, d_offs, d_lens, d_sym, d_counts, 1, out, d_order=order)
        assert ctx.last_decode_kernel() == N.KERNEL[f]
        assert torch.equal(out, want), "order" if order is not None else "no order"
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("byte-2", 70), ("r64-2", 70), ("word-8", 70), ("word-64", 70), ("byte-64-14bit", 70),
                                           ("r64-64", 70), ("alias256-64", 70)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """The 2-way byte and rans64 layouts, the 8-way word layout and the 64-way rows take the wave-per-stream kernels on the
    context with the option on, and decode right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, SINGLES["byte"], rid, n_streams)


@pytest.mark.gpu
def test_u16_alias_keeps_its_kernel_with_the_option_on(gpu, oracle):
    """Seventy 1-way alias streams over u16 symbols (1024 of them) keep k_decode_batch<alias> with the option on."""
    R, ctx, torch, _ = gpu
    row = N.ALIAS_U16_1_WAVE
    assert row["decode"] != MAIN["alias"]["decode"]
    run_row(Batch(R, ctx, torch, oracle, row, draw_lengths(70, 1, 29).clip(0, 8192)), 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_every_family_keeps_its_own_kernel_with_all_options_on(gpu, oracle):
    """With options 5, 7, 9, 11 and 13 all on, nine 8-way word streams report the group kernel, seventy 2-way byte streams the
    byte pairs, seventy 2-way rans64 streams the lane kernel, seventy 2-way alias streams the alias pairs, and seventy 1-way
    streams of each format the singles."""
    R, ctx, torch, _ = gpu
    others = (OPT_BATCH_GROUPS, OPT_BATCH_PAIRS, OPT_BATCH_LANES, OPT_BATCH_ALIAS_PAIRS)
    for o in others:
        ctx.set_option(o, 1)
    try:
        run_row(Batch(R, ctx, torch, oracle, dict(ROW["word-8"], decode="k_decode_batch_word_groups"), draw_lengths(9, 8, 43)), 4)
        run_row(Batch(R, ctx, torch, oracle, PMAIN, draw_lengths(70, 2, 47).clip(0, 8192)), 4)
        run_row(Batch(R, ctx, torch, oracle, LMAIN, draw_lengths(70, 2, 53).clip(0, 8192)), 4)
        run_row(Batch(R, ctx, torch, oracle, AMAIN, draw_lengths(70, 2, 59).clip(0, 8192)), 4)
        for f in FORMATS:
            run_row(Batch(R, ctx, torch, oracle, MAIN[f], draw_lengths(70, 1, 61).clip(0, 8192)), 4)
    finally:
        for o in others:
            ctx.set_option(o, 0)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMATS)
def test_option_takes_zero_or_one(gpu, oracle, f):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the singles."""
    R, ctx, _, _ = gpu
    check_option_takes_zero_or_one(gpu, oracle, SINGLES[f], align=64)
    with pytest.raises(R.RansAmdError) as e:
        ctx.set_option(OPT_BATCH_SINGLES, 2)
    assert "takes 0 (one stream per wave) or 1 (sixty-four 1-way streams per wave)" in str(e.value)


@pytest.mark.gpu
def test_singles_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 1-way byte streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    run_family_graph(tmp_path, SINGLES["byte"], "graph_batch_singles.py")
