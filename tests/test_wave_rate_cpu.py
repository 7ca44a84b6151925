"""No GPU: the proof that the inputs of tests/test_gpu_wave_extremes.py sit where that file says.  Every figure here comes from
tests/_stream_rate.py's models of the formats (simulate) and of the decoders' stream window (window_walk, written from the
comment at the top of decode_common.hpp) applied to the GPU file's own inputs; none is derived from the kernels.

  * the byte-count identity (tests/test_stream_rate_cpu.py identity) for every row and kind, the steered chunks and the model
    classes included: the model cannot drift from the oracle;
  * per row, some rare-only or steered chunk has a checkpoint interval whose bytes are interval_bound, and no interval of any
    chunk takes more; for byte-64-16bit every interval of the group part of every rare-only chunk does; for the per-chunk word
    row the proof is the oracle's stream size of 2 n + 256 bytes;
  * per section-b row both cursor events occur in front of a maximal interval -- one unit below the mark without a refill, on
    the mark with one --, the overshoot at refills takes every multiple of the unit modulo 16, and the largest ring offset
    reached is 2048 + interval_bound - unit, inside the 768-byte mirror;
  * the quiet word row has a common-only chunk that is silent for more than 1024 rounds;
  * the phase packings meet every residue the unit allows, modulo 16 and modulo 128;
  * WAVE_CASES names every kernel a unit-1 row of KERNEL_ROWS expects, under a rare-only and under a common-only input;
  * the ladder holds every g and t, and the batch form every ordered pair of g values as neighbours.

Two conditions of the issue that no input can meet, with the computation that shows it:
  * rans64 at 64-way never takes 512 bytes between two checkpoints of the kernels the library runs: the table decoder exists up
    to 16 bits, where two rounds of 64 states take at most 64 dwords (interval_bound(r64, 16, 64, 2) == 256), and the search
    decoder of 17 bits and more has element stores alone, a checkpoint in front of every sub-step: 256 again.  The row that
    reaches kMaxAdvance is r64-128-16bit (one round of 128 states).
  * r64-128-16bit: "on the mark with a refill, in front of a maximal interval" cannot happen.  At 16 bits a state that took a
    dword holds at least 2^47 and takes none in the next round, so every maximal round follows a silent one -- and the
    checkpoint in front of the silent round sees the same cursor and refills there.  test_steered_cursor_events asserts
    exactly that shape instead: on the mark with a refill, a silent interval, then the maximal one 1024 below the new mark."""
import numpy as np
import pytest

import _stream_rate as S
import test_gpu_wave_extremes as G
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD
from test_stream_rate_cpu import identity

IDS = [r["id"] for r in G.WAVE_ROWS]


def models_of(oracle, row, freqs=None):
    freqs = row["model"]() if freqs is None else freqs
    om = oracle.model(freqs, row["sb"], with_alias=(row["fmt"] == FMT_ALIAS))
    remap = om.table("alias_remap", 1 << row["sb"]) if row["fmt"] == FMT_ALIAS else None
    return freqs, om, remap


def walk(row, freqs, remap, syms, chunk, first):
    """-> window_walk of one chunk on the path a chunk of this size takes."""
    _, _, taken = S.simulate(row["fmt"], freqs, row["sb"], syms, row["ways"], remap, per_state=True)
    cadence, tail = G.fast_layout(row, chunk)
    return S.window_walk(S.substep_bytes(taken, row["fmt"], row["ways"]), first, cadence, every_from=tail)


def chunk_of(h_syms, chunk, c):
    return h_syms[c * chunk:(c + 1) * chunk]


# ---- the helpers ----------------------------------------------------------------------------------------------------------
def test_interval_bound_figures():
    """The issue's figures, from the formats alone."""
    ib = S.interval_bound
    assert ib(FMT_WORD, 12, 64, 4) == 384
    assert ib(FMT_BYTE, 16, 64, 4) == ib(FMT_WORD, 12, 128, 2) == ib(FMT_WORD, 12, 256, 1) == ib(FMT_R64, 31, 64, 2) == 512
    assert ib(FMT_R64, 16, 64, 2) == 256 and ib(FMT_BYTE, 14, 64, 4) == 448
    assert ib(FMT_ALIAS, 16, 64, 4) == 512 and ib(FMT_R64, 16, 128, 1) == 512 and ib(FMT_R64, 31, 64, 1) == 256
    # the rows: kMaxAdvance is reached, never exceeded
    assert max(r["bound"] for r in G.WAVE_ROWS) == 512
    want = {"word-64-rate": 384, "word-64-quiet": 384, "word-128": 512, "word-256": 512, "word-512": 512, "word-100": 128, "word-u16-64": 256,
            "word-u16-128": 512, "byte-64-16bit": 512, "byte-64-14bit": 448, "byte-128-16bit": 512, "byte-64-12bit": 384, "r64-64-16bit": 256,
            "r64-64-14bit": 256, "r64-128-16bit": 512, "r64-search-64-17bit": 256, "r64-search-64-31bit": 256, "alias256-64": 512,
            "alias256-64-dual": 512, "alias4096-64": 512}
    assert {r["id"]: r["bound"] for r in G.WAVE_ROWS} == want


def test_window_walk_is_the_ring_of_the_comment():
    """A hand-made walk: 512 bytes per interval from cursor 6 -- the mark is met at the second checkpoint behind every refill."""
    w, top = S.window_walk([128] * 40, 6, 4)
    assert [t for _, _, t in w] == [512] * 10
    assert [(rel, ref) for rel, ref, _ in w[:6]] == [(6 - 1024, False), (518 - 1024, False), (6, True), (1542 - 2048, False), (6, True), (518 - 1024, False)]
    assert top == 2048 + 6  # (the cursor wraps at the checkpoint that finds it past the end)
    # a cursor exactly on the mark refills, one unit below does not and runs 512 - unit past it
    w, top = S.window_walk([256] * 8 + [127, 1] + [256] * 6, 0, 2)
    assert w[2] == (0, True, 512) and w[4][:2] == (0, True)
    w, top = S.window_walk([256, 255] + [256] * 6, 0, 2)
    assert w[2] == (-1, False, 512) and w[3] == (511, True, 512)
    # the element-store tail checks in front of every sub-step
    w, _ = S.window_walk([10] * 10, 0, 4, every_from=8)
    assert [t for _, _, t in w] == [40, 40, 10, 10]
    assert S.substep_bytes(np.ones((3, 100), dtype=np.uint8), FMT_WORD, 100).tolist() == [128, 72] * 3


def test_steered_is_what_it_says():
    f = S.lane_model(16)
    rare, common = S.rare_and_common(f)
    s = S.steered(f, 21, 5, 7, 3, 64).reshape(12, 64)
    assert np.all(f[s[5:]] == 1) and np.all(f[s[:5, :21]] == 1) and np.all(s[:5, 21:] == common)
    # the rare-only part stays in lock-step whatever leads it
    a = S.round_bytes(FMT_BYTE, f, 16, S.steered(f, 21, 5, 7, 3, 64), 64)
    b = S.round_bytes(FMT_BYTE, f, 16, S.steered(f, 0, 5, 7, 3, 64), 64)
    assert np.array_equal(a[5:], b[5:]) and np.all(a[5:] == 128) and np.all(a[:5] == 42) and np.all(b[:5] == 0)
    m = S.model_rare(12, 1024)
    assert m.size == 1024 and int(m.sum()) == 4096 and int(m[S.COMMON]) == 3073 and np.count_nonzero(m == 1) == 1023
    m = S.model_rare(16, 4096)
    assert int(m.sum()) == 65536 and int(m[S.COMMON]) == 61441 and np.count_nonzero(m == 1) == 4095
    assert S.rare_only(m, 10, 1).dtype == np.uint16


# ---- the model against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.WAVE_ROWS, ids=IDS)
def test_identity_on_the_wave_rows(oracle, row):
    """Two chunks of every kind and the ragged last chunk of section a's input in turn, at the odd size and at 4 N; the first
    four all-rare chunks (the word rows' four shifts); eight steered chunks of the section-b rows."""
    freqs, om, remap = models_of(oracle, row)
    N = row["ways"]
    for chunk in (G.odd_size(N), 4 * N):
        h, kinds = G.wave_input(row, freqs, chunk, "turn")
        assert kinds[:5].tolist() == list(G.KINDS5)
        for c in list(range(10)) + [G.NCHUNKS]:
            identity(oracle, row["fmt"], freqs, row["sb"], chunk_of(h, chunk, c), N, om, remap)
        h, _ = G.wave_input(row, freqs, chunk, "all-rare")
        for c in range(4):
            identity(oracle, row["fmt"], freqs, row["sb"], chunk_of(h, chunk, c), N, om, remap)
    if row["id"] in G.B_ROWS:
        for d in G.b_chunks(row, freqs)[::8]:
            identity(oracle, row["fmt"], freqs, row["sb"], d, N, om, remap)


@pytest.mark.parametrize("row", G.class_rows(), ids=[r["id"] for r in G.class_rows()])
def test_identity_under_the_model_classes(oracle, row):
    """Section e's input: every class, the five kinds in turn by chunk, and the ragged last chunk."""
    row = dict(row, shift=False)
    chunk = G.tail_size(row["ways"])
    for name, f in G.classes_of(row):
        freqs, om, remap = models_of(oracle, row, f)
        h, kinds = G.wave_input(row, freqs, chunk, "turn", seed=900)
        for c in (0, 1, 2, 3, 4, G.NCHUNKS):
            per_round = identity(oracle, row["fmt"], freqs, row["sb"], chunk_of(h, chunk, c), row["ways"], om, remap)
            if name == "one-symbol":  # nothing but the flushed states leaves
                assert per_round.sum() == 0


# ---- the bounds reached -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.WAVE_ROWS, ids=IDS)
def test_some_chunk_reaches_the_interval_bound(oracle, row):
    """The first four rare-only chunks of section a's all-rare set at every size of the row, and the steered chunks of the
    section-b rows, walked on the path a chunk of that size takes: no checkpoint interval takes more than interval_bound of
    that path, and on the path the row names some interval takes exactly that.  byte-64-16bit: every interval of the group
    part of every rare-only chunk does."""
    freqs, om, remap = models_of(oracle, row)
    N, fmt = row["ways"], row["fmt"]
    reached = False
    for chunk in G.sizes(row):
        if chunk > 100 * N:
            continue
        cadence, tail = G.fast_layout(row, chunk)
        bound = row["bound"] if cadence == row["cadence"] else S.interval_bound(fmt, row["sb"], min(N, 64), 1)
        h, _ = G.wave_input(row, freqs, chunk, "all-rare")
        data = [chunk_of(h, chunk, c) for c in range(4)]
        if row["id"] in G.B_ROWS and chunk == G.b_size(row):
            data += G.b_chunks(row, freqs)
        for i, d in enumerate(data):
            w, top = walk(row, freqs, remap, d, chunk, 0)
            took = [t for _, _, t in w]
            assert max(took) <= bound, (row["id"], chunk, i, max(took))
            assert top <= S.RING_BYTES + S.RING_MIRROR
            if cadence == row["cadence"]:
                reached = reached or max(took) == bound
                if row["id"] == "byte-64-16bit" and i < 4:
                    groups = tail // cadence
                    assert groups in (1, 12) and took[:groups] == [512] * groups
    assert reached, (row["id"], "no interval of", row["bound"], "bytes")


def test_per_chunk_models_constant_chunks_are_the_extremes(oracle):
    """S.simulate does not model the wrap of the word format's threshold, so the proof is the oracle's stream size: a constant
    chunk of n symbols under its own model is 2 n + 256 bytes in the word format -- a word per symbol, 128 bytes in every round,
    512 per group of four: kMaxAdvance, which no static 64-way word model reaches (384) -- and the 256 bytes of the flushed
    states in the byte format.  The input mixes them with uniform and Zipf chunks, constant beside constant and beside both."""
    for row in G.ADAPTIVE_ROWS:
        for chunk in (G.odd_size(64), G.tail_size(64), 256):
            h, kinds = G.adaptive_input(chunk)
            _, _, lens, rows = oracle.encode_chunked_adaptive(row["fmt"], h, 64, chunk, row["sb"])
            n = np.array([chunk] * G.NCHUNKS + [G.ragged(chunk)])
            const = np.array([k == "constant" for k in kinds])
            assert const.sum() >= 33 and (~const).sum() >= 24 and {"uniform", "zipf"} <= set(kinds)
            assert np.all(rows[const].max(axis=1) == 4096)
            want = 2 * n + 256 if row["fmt"] == FMT_WORD else np.full(n.size, 256)
            assert np.array_equal(lens[const], want[const]), row["id"]
            assert np.all(lens[~const] < (2 * n + 256)[~const]) and np.all(lens[~const] > 256)
            pairs = {(kinds[c], kinds[c + 1]) for c in range(G.NCHUNKS)}
            assert {("constant", "constant"), ("constant", "uniform"), ("uniform", "constant"), ("zipf", "constant"), ("uniform", "uniform")} <= pairs
    assert S.interval_bound(FMT_WORD, 12, 64, 4) == 384 and 4 * 128 == 512


# ---- section b ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", G.B_ROWS)
def test_steered_cursor_events(oracle, rid):
    """Every steered chunk at every start residue (the GPU test's rotations put every chunk at every one): the cursor one unit
    below the mark without a refill and exactly on the mark with one, each in front of a maximal interval; at refills the
    overshoot takes every multiple of the unit modulo 16; the largest ring offset reached is 2048 + interval_bound - unit.
    (r64-128-16bit: see the module docstring for the shape the second event has there.)"""
    row = G.ROW[rid]
    freqs, om, remap = models_of(oracle, row)
    unit, bound, chunk = S.UNIT[row["fmt"]], row["bound"], G.b_size(row)
    assert G.fast_layout(row, chunk)[0] == row["cadence"] and G.aligned(row, chunk)
    below = on = on_then_silent = 0
    overshoot, top = set(), 0
    for d in G.b_chunks(row, freqs):
        assert d.size == chunk
        _, _, taken = S.simulate(row["fmt"], freqs, row["sb"], d, row["ways"], remap, per_state=True)
        sub = S.substep_bytes(taken, row["fmt"], row["ways"])
        cadence, tail = G.fast_layout(row, chunk)
        for first in range(0, 16, unit):
            w, t = S.window_walk(sub, first, cadence, every_from=tail)
            top = max(top, t)
            for j, (rel, refilled, took) in enumerate(w):
                assert took <= bound and refilled == (rel >= 0)
                below += rel == -unit and took == bound
                on += rel == 0 and took == bound
                if refilled:
                    overshoot.add(rel % 16)
                if rel == 0 and took == 0 and j + 1 < len(w) and w[j + 1] == (-S.RING_BLOCK, False, bound):
                    on_then_silent += 1
                if rid == "r64-128-16bit" and took == bound and j:  # every maximal interval follows a silent one
                    assert w[j - 1][2] == 0
    assert below > 0, "never one unit below the mark in front of a maximal interval"
    if rid == "r64-128-16bit":
        assert on == 0 and on_then_silent > 0
    else:
        assert on > 0, "never on the mark in front of a maximal interval"
    assert sorted(overshoot) == list(range(0, 16, unit)), sorted(overshoot)
    assert top == S.RING_BYTES + bound - unit <= S.RING_BYTES + S.RING_MIRROR, top


def test_section_b_rows_are_those_at_kmaxadvance():
    assert G.B_ROWS == ["word-128", "word-256", "word-512", "word-u16-128", "byte-64-16bit", "byte-128-16bit", "r64-128-16bit", "alias256-64",
                        "alias256-64-dual", "alias4096-64", "word-64-rate"]
    combos = {(G.B_LEADS[c % 4], G.B_LANES[(c // 4) % 7]) for c in range(G.NCHUNKS)}
    assert len(combos) == 28 and G.B_LANES == (0, 1, 3, 7, 21, 40, 63) and G.B_LEADS == (4, 5, 8, 12)


# ---- silence ------------------------------------------------------------------------------------------------------------------
def test_quiet_row_is_silent_for_1024_rounds(oracle):
    """The common-only chunks of the quiet row's long size take nothing after their states for 1030 rounds (a state loses
    0.011 bits per symbol); every row's common-only chunks of 51 rounds take at most a unit per state."""
    row = G.ROW["word-64-quiet"]
    freqs = row["model"]()
    chunk = G.LONG_ROUNDS * 64 + 4
    assert chunk in G.sizes(row) and chunk % 4 == 0
    h, kinds = G.wave_input(row, freqs, chunk, "turn")
    assert kinds[1] == S.COMMON_K
    rb = S.round_bytes(FMT_WORD, freqs, 12, chunk_of(h, chunk, 1), 64)
    assert S.longest_silence(rb) >= 1024 and rb.sum() == 0
    for row in G.WAVE_ROWS:
        freqs, om, remap = models_of(oracle, row)
        N = row["ways"]
        rb = S.round_bytes(row["fmt"], freqs, row["sb"], S.common_only(freqs, G.tail_size(N)), N, remap)
        assert rb.sum() <= N * S.UNIT[row["fmt"]], (row["id"], rb.sum())


# ---- what the GPU file covers -----------------------------------------------------------------------------------------------
def test_phase_packings_meet_every_residue():
    for unit in (1, 2, 4):
        n = G.NCHUNKS + 1
        assert sorted(set(G.phases16(n, unit).tolist())) == list(range(0, 16, unit))
        assert sorted(set(G.phases16(G.LADDER_CHUNKS + 1, unit).tolist())) == list(range(0, 16, unit))
        met = set()
        for ph in G.phases128(n, unit):
            assert np.all(ph % unit == 0) and np.all(ph < 128)
            met |= set(ph.tolist())
        assert sorted(met) == list(range(0, 128, unit)), (unit, len(met))
        # section b: over the rotations every chunk stands at every residue
        at = {(c, int(unit * ((c + rot) % (16 // unit)))) for rot in range(16 // unit) for c in range(G.NCHUNKS)}
        assert len(at) == G.NCHUNKS * (16 // unit)
    # neighbouring chunks differ in kind, and the pairs of the dual decoder hold every adjacent combination of two kinds
    kinds = G.set_kinds("turn", G.NCHUNKS + 1)
    assert np.all(kinds[1:] != kinds[:-1])
    pairs = {(int(kinds[2 * j]), int(kinds[2 * j + 1])) for j in range(G.NCHUNKS // 2)}
    assert pairs == {(G.KINDS5[i], G.KINDS5[(i + 1) % 5]) for i in range(5)}
    streams = [np.full(300 + c, c, dtype=np.uint8) for c in range(9)]
    cont, starts, used = S.pack_at_phases(streams, G.phases16(9, 2), 16)
    assert used == starts[-1] + streams[-1].size and all(starts[c] % 16 == (2 * c) % 16 for c in range(9))


def test_no_wave_kernel_without_an_extreme_case():
    """Every kernel a unit-1 row of KERNEL_ROWS expects -- the wave-per-chunk decoders and encoders, the dual decoder, the
    per-chunk-model kernels -- is asserted by a case of WAVE_CASES under a rare-only, a common-only and a mixed input: a new
    wave kernel needs a row in the matrix (tests/test_gpu_kernel_matrix.py test_no_kernel_without_a_row) and then fails here
    until it has an extreme case."""
    from _kernel_rows import KERNEL_ROWS, row_kernel_names
    need = row_kernel_names([r for r in KERNEL_ROWS if r["unit"] == 1])
    assert {G.D_W64, G.D_W, G.D_W16, G.D_B, G.D_BF, G.D_R, G.D_RS, G.D_A, G.D_DUAL, G.D_WA, G.D_BA, G.E_W, G.E_B, G.E_R, G.E_RF, G.E_A, G.E_WA,
            G.E_BA, G.E_WAD, G.E_BAD} == need, sorted(need)
    for inp in ("rare", "common", "mixed"):
        have = G.kernels_under(inp)
        assert not need - have, ("no wave case under a %s input" % inp, sorted(need - have))
    # the check has teeth: without its cases a kernel is reported missing
    less = [c for c in G.WAVE_CASES if G.D_DUAL not in c["kernels"]]
    assert G.D_DUAL in need - G.kernels_under("rare", less)
    less = [c for c in G.WAVE_CASES if not c["id"].startswith("r64-search")]
    assert {G.D_RS, G.E_RF} <= need - G.kernels_under("common", less)
    # and the table is what the tests run
    assert [c["id"] for c in G.WAVE_CASES if c["section"] == "a"] == [p.id for p in G._a_cases()] + [r["id"] for r in G.ADAPTIVE_ROWS]
    # the kernel of every size: the named one where the chunk is a multiple of 4 bytes
    for row in G.WAVE_ROWS:
        N = row["ways"]
        assert G.decoder_of(row, G.tail_size(N)) == G.decoder_of(row, 4 * N) == row["decode"]
        assert G.decoder_of(row, G.odd_size(N)) == row["unaligned"]
        assert G.fast_layout(row, G.odd_size(N)) == (1, 0)
        f = row["model"]()
        assert f.size == row["K"] and int(f.astype(np.uint64).sum()) == 1 << row["sb"]
    assert G.fast_layout(G.ROW["word-64-rate"], G.tail_size(64)) == (4, 48) and G.fast_layout(G.ROW["word-512"], G.tail_size(512)) == (4, 48 * 8)
    assert G.fast_layout(G.ROW["word-u16-64"], G.tail_size(64)) == (2, 50) and G.fast_layout(G.ROW["r64-128-16bit"], 51 * 128) == (2, 96)
    assert G.fast_layout(G.ROW["alias4096-64"], G.tail_size(64)) == (1, 0) and G.fast_layout(G.ROW["alias4096-64"], 3072) == (4, 48)


def test_ladder_holds_every_path_length():
    """k_decode_word64's hand-over (kClaimAhead = 10, kDataAhead = 5 groups) distinguishes chunks of 0 or 1 groups, of 2 to 6, of 7
    to 10 and of 11 and more: the ladder holds every g and every t listed and 7 besides -- both sides of each of those borders
    --, and in the batch form every ordered pair of g values as neighbours."""
    assert set(G.LADDER_G) == {0, 1, 2, 4, 5, 6, 9, 10, 11, 12} | {7} and G.LADDER_T == (0, 1, 63, 69)
    for lo, hi in ((1, 2), (6, 7), (10, 11)):
        assert lo in G.LADDER_G and hi in G.LADDER_G
    for g in G.LADDER_G:
        sizes = G.ladder_sizes(g)
        assert {256 * g + t for t in G.LADDER_T if 256 * g + t} <= set(sizes)
        assert all(s // 256 == g for s in sizes)
        assert sum(s % 4 == 0 for s in sizes) >= 3  # (those reach k_decode_word64 in a uniform call)
    counts, gs = G.ladder_batch_counts()
    assert {(gs[i], gs[i + 1]) for i in range(len(gs) - 1)} == {(a, b) for a in G.LADDER_G for b in G.LADDER_G}
    assert np.array_equal(counts // 256, gs)
    assert {int(c) % 256 for c in counts} == set(G.LADDER_T + G.LADDER_T4)
    for g in G.LADDER_G:
        assert len({int(c) % 256 for c in counts[np.array(gs) == g]}) >= 4
