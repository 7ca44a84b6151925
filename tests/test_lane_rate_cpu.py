"""No GPU: the proof that the inputs of tests/test_gpu_lane_extremes.py sit where that file says.

  * the byte-count identity: for every LANE_ROW, model class and content kind the GPU file uses, the bytes
    tests/_stream_rate.py's model counts per round, plus the flushed states, are Oracle.encode's stream size, and the model's
    final states are the stream's header -- on chunks cut out of the GPU file's own inputs;
  * the bounds reached, per 16-symbol group of one lane's chunk (16 / N rounds), over EVERY window of that many rounds: a
    frequency-1 symbol makes the decoder's step x = x >> scale_bits, so a group of them takes exactly 2 scale_bits bytes
    wherever the unit divides the bits a state loses (S.rare_group_bytes has the argument) -- 32 bytes for rans64 and the byte
    format at 16 bits, 28 at 14 bits, 24 for the 4-way word format and the 12-bit rans64 rows; 32 for the 8-way alias
    format at 16 bits, which its rule of at most two bytes per symbol cannot exceed.  k_decode_lanes_r64x2's header allows
    a valid stream 40 bytes per group ("5 renormalisations per state"): a looser bound than the format's -- a state that
    loses 8 x 16 bits and stays inside its 32-bit-wide interval takes at most four dwords -- so the kernel's ">= 48 B
    ahead" has a dword per state to spare; 32 is what a valid stream can reach, and what the GPU file feeds it;
  * silence: a common-only chunk takes no byte after its states;
  * bursts: a silent group and a group at the maximum in one chunk, wherever `lead` puts the runs;
  * coverage: LANE_CASES names every kernel the lane launchers can report under a rare-only, a common-only and a mixed
    wave, the patterns put every kind at every lane position of a quad, and the phases cover every offset."""
import numpy as np
import pytest

import _stream_rate as S
import test_gpu_lane_extremes as G
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD
from test_stream_rate_cpu import identity

IDS = [r["id"] for r in G.LANE_ROWS]
# The issue's table (bytes per 16-symbol group of a rare-only chunk), measured there with S.round_bytes on 1024-symbol
# streams; S.rare_group_bytes derives the same figures from the formats.
TABLE = {"r64-2-16bit": 32, "byte-1-16bit": 32, "byte-1-14bit": 28, "word-4-rate": 24, "word-4-quiet": 24}


def models_of(oracle, row, freqs=None):
    freqs = row["model"]() if freqs is None else freqs
    om = oracle.model(freqs, row["sb"], with_alias=(row["fmt"] == FMT_ALIAS))
    remap = om.table("alias_remap", 1 << row["sb"]) if row["fmt"] == FMT_ALIAS else None
    return freqs, om, remap


def section_a_input(row, chunk, freqs=None):
    """The GPU file's own input of section a -> (symbols, kind per chunk, name of every batch's pattern)."""
    freqs = row["model"]() if freqs is None else freqs
    h, kinds = G.lane_input(freqs, S.pattern_kinds, G.SMALL_BATCHES, chunk, 1000 + chunk)
    return h, kinds, [n for n, _ in S.lane_patterns()]


def chunks_of_kind(kinds, kind, limit):
    """`limit` chunks of a kind, spread over the batches (not the ragged last chunk)."""
    at = np.nonzero(kinds[:-1] == kind)[0]
    return at[::max(1, at.size // limit)][:limit]


# ---- the model against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.LANE_ROWS, ids=IDS)
def test_identity_on_the_lane_rows(oracle, row):
    """Two chunks of every kind and the ragged last chunk, of section a's input at 64, 256 and 256 + 5 symbols."""
    freqs, om, remap = models_of(oracle, row)
    for chunk in (64, 256, 261):
        if chunk not in G.small_sizes(row):
            continue
        h, kinds, _ = section_a_input(row, chunk)
        picks = [int(c) for kind in range(len(S.LANE_KINDS)) for c in chunks_of_kind(kinds, kind, 2)] + [kinds.size - 1]
        assert len(picks) == 2 * len(S.LANE_KINDS) + 1
        for c in picks:
            identity(oracle, row["fmt"], freqs, row["sb"], h[c * chunk:(c + 1) * chunk], row["ways"], om, remap)


@pytest.mark.parametrize("row", G.class_rows(), ids=[r["id"] for r in G.class_rows()])
def test_identity_under_the_model_classes(oracle, row):
    """Section c's input: every class, the four kinds in turn by chunk, and the ragged last chunk."""
    for name, f in G.classes_of(row):
        freqs, om, remap = models_of(oracle, row, f)
        h, kinds = G.lane_input(freqs, S.turn_kinds, G.SMALL_BATCHES, 64, 4000)
        assert kinds[:4].tolist() == [S.RARE, S.COMMON_K, S.BURSTS64, S.DRAWN]
        for c in (0, 1, 2, 3, kinds.size - 1):
            per_round = identity(oracle, row["fmt"], freqs, row["sb"], h[c * 64:(c + 1) * 64], row["ways"], om, remap)
            if name == "one-symbol":  # nothing but the flushed states leaves
                assert per_round.sum() == 0


def test_identity_on_the_threshold_models(oracle):
    """Section d: the models with a largest frequency of exactly 4095 / 4096, the 64-symbol models at scale_bits 7 and 16, the
    one-symbol model at 16 bits (two flushed states and nothing else), and the huge-chunk row's generator at 1024 + 2 symbols."""
    for sb, top in G.D_TOP:
        row = G.top_row(sb, top)
        freqs, om, remap = models_of(oracle, row)
        assert int(freqs.max()) == top and (row["decode"] == G.D_RXP) == (top == 4095)
        h, kinds = G.lane_input(freqs, G.rare_and_drawn, G.SMALL_BATCHES, 192, 6000 + top)
        for c in (0, 1, kinds.size - 1):
            identity(oracle, FMT_R64, freqs, sb, h[c * 192:(c + 1) * 192], 2, om)
        assert np.any(h[192:384] == 0), "no drawn symbol of the largest frequency"
    for sb, cls in G.D_BITS:
        row = G.bits_row(sb, cls)
        freqs, om, remap = models_of(oracle, row)
        assert freqs.size == 64 and int(freqs.sum()) == 1 << sb
        h, kinds = G.lane_input(freqs, G.rare_and_common, 2, 64, 7000 + sb)
        for c in (0, 1, kinds.size - 1):
            identity(oracle, FMT_R64, freqs, sb, h[c * 64:(c + 1) * 64], 2, om)
    row = G.one_symbol_row()
    freqs, om, remap = models_of(oracle, row)
    assert int(freqs.max()) == 1 << 16
    stream = oracle.encode(FMT_R64, om, np.full(64, 200, dtype=np.uint8), 2)
    assert stream.size == 16 and S.stream_states(FMT_R64, stream, 2).tolist() == [1 << 31, 1 << 31]
    row = G.ROW["byte-2-14bit"]
    freqs, om, remap = models_of(oracle, row)
    kinds = S.pattern_kinds(65, names=("quad-mates-differ-0",))
    grid = S.chunk_grid(freqs, kinds[:4], 1026, 9000)
    for c in range(4):
        identity(oracle, FMT_BYTE, freqs, 14, grid[c], 2, om)


# ---- the bounds reached ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.LANE_ROWS, ids=IDS)
def test_rare_only_chunks_take_the_most_in_every_group(oracle, row):
    """Every window of 16 / N rounds of a rare-only chunk of section a's all-rare wave, at 256 and 272 symbols: exactly
    2 scale_bits bytes where the unit divides the bits a state loses in a group; otherwise (the 2-way rans64 rows at 14 bits:
    112 bits, three or four dwords per state) between the floor and the ceiling, and the ceiling -- the format's 32 -- is
    reached: the two states of a rare-only chunk stay in lock-step, and two groups in a row take seven dwords per state."""
    freqs = row["model"]()
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    lo, hi = S.rare_group_bytes(fmt, sb, ways)
    assert hi <= 16 * 2 * S.UNIT[fmt] if fmt in (FMT_BYTE, FMT_ALIAS) else hi <= 16 * S.UNIT[fmt], "above the format's rule per symbol"
    if row["id"] in TABLE:
        assert (lo, hi) == (TABLE[row["id"]], TABLE[row["id"]])
    if fmt == FMT_ALIAS:  # derived the same way: two rounds of eight states, 16 bits each, a byte at a time -- and it is the
        assert (lo, hi) == (32, 32) and hi == 16 * 2  # most the format's rule of two bytes per symbol allows
    om_remap = models_of(oracle, row)[2]
    for chunk in (256, 272):
        if chunk not in G.small_sizes(row):
            continue
        h, kinds, names = section_a_input(row, chunk)
        first = 64 * names.index("all-rare")
        assert np.all(kinds[first:first + 64] == S.RARE)
        for c in (first, first + 1, first + 62, first + 63):
            w = S.group_bytes(S.round_bytes(fmt, freqs, sb, h[c * chunk:(c + 1) * chunk], ways, om_remap)[:chunk // ways], ways)
            assert w.size > 100 // ways and w.min() >= lo and w.max() == hi, (row["id"], chunk, c, w.min(), w.max())
            if lo == hi:
                assert w.min() == hi


@pytest.mark.parametrize("row", G.LANE_ROWS, ids=IDS)
def test_common_only_chunks_take_nothing(oracle, row):
    """Section a's all-common wave at 272 symbols (256 for the r64x2 rows): no byte after the flushed states -- under the byte,
    alias and rans64 models of 255 x 1 and one common symbol at 12, 14 and 16 bits, and under both word models (the quiet
    one: 0.011 bits a symbol).  The one exception is the 14-bit model of the packed slot records, whose commonest symbol is
    4033 / 16384 -- the record's 12-bit field allows no more -- and costs two bits: a dword per state every 16 symbols."""
    freqs = row["model"]()
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    chunk = 272 if 272 in G.small_sizes(row) else 256
    h, kinds, names = section_a_input(row, chunk)
    first = 64 * names.index("all-common")
    remap = models_of(oracle, row)[2]
    for c in (first, first + 63):
        rb = S.round_bytes(fmt, freqs, sb, h[c * chunk:(c + 1) * chunk], ways, remap)
        if row["id"] == "r64-2-14bit-packed":
            assert rb.sum() == 8 * (chunk // 32), rb.sum()
        else:
            assert rb.sum() == 0, (row["id"], rb.sum())


@pytest.mark.parametrize("row", G.LANE_ROWS, ids=IDS)
def test_burst_chunks_hold_both_extremes(oracle, row):
    """Every kind of burst chunk (runs of 64 and of 16) of section a's input at 192, 256 and 272 symbols, six chunks each -- their
    leads differ --: a window of 16 / N rounds that takes nothing and one that takes what a rare-only group takes.  (The
    14-bit rans64 rows: the unit does not divide a group's bits, a lone run of 16 may meet the floor -- at least the floor,
    then; and the packed-record model has no silent symbol.)"""
    freqs = row["model"]()
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    lo, hi = S.rare_group_bytes(fmt, sb, ways)
    remap = models_of(oracle, row)[2]
    leads = set()
    for chunk in (192, 256, 272):
        if chunk not in G.small_sizes(row):
            continue
        h, kinds, _ = section_a_input(row, chunk)
        for kind in (S.BURSTS64, S.BURSTS16):
            for c in chunks_of_kind(kinds, kind, 6):
                leads.add((kind, int(S.burst_lead(c))))
                w = S.group_bytes(S.round_bytes(fmt, freqs, sb, h[c * chunk:(c + 1) * chunk], ways, remap), ways)
                assert lo <= w.max() <= hi, (row["id"], chunk, c, w.max())
                if lo == hi or kind == S.BURSTS64:
                    assert w.max() == hi, (row["id"], chunk, c, w.max())
                if row["id"] != "r64-2-14bit-packed":
                    assert w.min() == 0, (row["id"], chunk, c, w.min())
    assert len(leads) >= 8, leads


def test_wrap_chunk_is_the_smallest_that_wraps_the_ring(oracle):
    """Section b's chunk size: a rare-only chunk of wrap_chunk(row) symbols is longer than the 128-byte ring of the staged
    kernels, one of 64 symbols fewer is not."""
    for row in G.LANE_ROWS:
        freqs, om, _ = models_of(oracle, row)
        chunk = G.wrap_chunk(row)
        assert oracle.encode(row["fmt"], om, S.rare_only(freqs, chunk, 1), row["ways"]).size > 128, row["id"]
        if chunk > 64:
            assert oracle.encode(row["fmt"], om, S.rare_only(freqs, chunk - 64, 1), row["ways"]).size <= 128, row["id"]


# ---- what the GPU file covers -------------------------------------------------------------------------------------------
def lane_kernel_names():
    """The names of decode_lanes.hip's and encode_lanes.hip's kernels: those of the registry's uniform family
    (tests/_kernel_rows.py) that say `_lanes`."""
    from _kernel_rows import UNIFORM, registry
    return {n for n in registry()[UNIFORM] if "_lanes" in n}


def test_no_lane_kernel_without_an_extreme_case():
    """Every kernel the lane launchers can report is asserted by a case of LANE_CASES under a rare-only, a common-only and a
    mixed wave: a later lane kernel needs a case.  (k_encode_lanes_r64x2 is two instantiations under one name: the models of
    255 x 1 and one common symbol have a record for every byte value and run the one without TRACK, every class of section c
    that has symbols without a record runs the other.)"""
    need = lane_kernel_names()
    assert need == {G.D_ST, G.D_RX, G.D_RXP, G.D_L, G.E_ST, G.E_RX, G.E_L16}, sorted(need)
    for inp in G.ALL_INPUTS:
        have = G.kernels_under(inp)
        assert not need - have, ("no lane case under a %s input" % inp, sorted(need - have))
    # the check has teeth: without its cases a kernel is reported missing
    less = [c for c in G.LANE_CASES if not c["id"].startswith("byte-2-huge-chunks")]
    assert all(G.D_L in need - G.kernels_under(inp, less) for inp in G.ALL_INPUTS)
    less = [c for c in G.LANE_CASES if G.D_RXP not in c["kernels"]]
    assert G.D_RXP in need - G.kernels_under("rare", less)
    # both instantiations of k_encode_lanes_r64x2
    dense = [r["id"] for r in G.LANE_ROWS if G.is_r64x2(r) and np.all(r["model"]() > 0)]
    sparse = [n for r in G.class_rows() if G.is_r64x2(r) for n, f in G.classes_of(r) if np.any(f == 0)]
    assert len(dense) == 4 and len(sparse) >= 9
    # and the table is what the tests run
    ids = {s: [c["id"] for c in G.LANE_CASES if c["section"] == s] for s in "abcd"}
    assert ids["a"] == [p.id for p in G._a_cases()] and ids["b"] == [p.id for p in G._b_cases()]
    assert ids["c"] == [p.id for p in G._c_cases()]
    assert len(ids["d"]) == len(G.D_TOP) + len(G.D_BITS) + 1 + len(G.HUGE_PATTERNS)


def test_lane_rows_are_the_shapes_the_launchers_take():
    """One row per (kernel, format, interleave) of the issue's table, with the decoder every chunk size of the row gets."""
    shapes = {(r["fmt"], r["sb"], r["ways"], r["decode"], r["big"]) for r in G.LANE_ROWS}
    for want in ((FMT_WORD, 12, 4, G.D_ST, G.E_ST), (FMT_BYTE, 14, 1, G.D_ST, G.E_ST), (FMT_BYTE, 16, 1, G.D_ST, G.E_ST),
                 (FMT_ALIAS, 16, 8, G.D_ST, G.E_ST), (FMT_R64, 14, 1, G.D_ST, G.E_ST), (FMT_BYTE, 14, 2, G.D_BP, G.E_ST),
                 (FMT_BYTE, 16, 2, G.D_BP, G.E_ST), (FMT_R64, 12, 2, G.D_RXP, G.E_RX), (FMT_R64, 14, 2, G.D_RXP, G.E_RX),
                 (FMT_R64, 14, 2, G.D_RX, G.E_RX), (FMT_R64, 16, 2, G.D_RX, G.E_RX)):
        assert want in shapes, want
    for r in G.LANE_ROWS:
        f = r["model"]()
        assert int(f.sum()) == 1 << r["sb"] and f.size == 256
        if G.is_r64x2(r):  # the rule of the packed slot records (model.h)
            assert (r["decode"] == G.D_RXP) == (r["sb"] <= 14 and int(f.max()) <= 4095), r["id"]
        assert [G.decoder_of(r, c) for c in (64, 261)] == ([r["decode"]] * 2 if r["lanes_decoder"] else [G.D_BP, G.D_ST])
        assert set(G.small_sizes(r)) >= {64, 192, 256} and G.wrap_chunk(r) in (64, 128)
        if not G.is_r64x2(r):
            assert {272, 261} <= set(G.small_sizes(r)) and 272 in G.big_sizes(r)


def test_patterns_put_every_kind_at_every_lane():
    """rotating: over its five waves every lane holds every kind, so every (lane mod 4, kind) pair is met; quad-mates-differ:
    the four lanes of every quad hold four different kinds, each lane of a quad each kind over the four rotations, runs of
    both lengths; one-rare / one-common: lane 0, 1, 2 and 3 of a first, a middle and the last quad is the odd one; and
    section a's geometry runs every pattern in a full wave, then a wave of 37 lanes with a ragged last chunk."""
    pats = dict(S.lane_patterns())
    assert len(pats) == 35 == G.SMALL_BATCHES
    rot = np.stack([pats["rotating-%d" % r] for r in range(5)])
    for lane in range(64):
        assert sorted(rot[:, lane].tolist()) == [0, 1, 2, 3, 4]
    assert {(l % 4, int(k)) for r in range(5) for l, k in enumerate(rot[r])} == {(m, k) for m in range(4) for k in range(5)}
    quad = np.stack([pats["quad-mates-differ-%d" % r] for r in range(4)])
    merged = np.where(quad == S.BURSTS16, S.BURSTS64, quad)
    for r in range(4):
        for q in range(16):
            assert sorted(merged[r, 4 * q:4 * q + 4].tolist()) == [S.RARE, S.COMMON_K, S.BURSTS64, S.DRAWN]
    for lane in range(64):
        assert sorted(merged[:, lane].tolist()) == [S.RARE, S.COMMON_K, S.BURSTS64, S.DRAWN]
    assert S.BURSTS64 in quad[0, :4] and S.BURSTS16 in quad[0, 4:8]
    odd = {"one-rare": set(), "one-common": set()}
    for name, k in pats.items():
        for what, one in (("one-rare", S.RARE), ("one-common", S.COMMON_K)):
            if name.startswith(what):
                at = np.nonzero(k == one)[0]
                assert at.size == 1 and np.all(np.delete(k, at[0]) == (S.COMMON_K if one == S.RARE else S.RARE))
                odd[what].add((int(at[0]) // 4, int(at[0]) % 4))
    assert odd["one-rare"] == odd["one-common"] == {(q, l) for q in (0, 7, 15) for l in range(4)}
    assert np.all(pats["all-rare"] == S.RARE) and np.all(pats["all-common"] == S.COMMON_K)
    nchunks, n = G.geometry(G.SMALL_BATCHES, 256)
    assert nchunks == 64 * 35 + 37 and nchunks % 64 == G.PART and 0 < n - (nchunks - 1) * 256 < 256
    kinds = S.pattern_kinds(nchunks)
    names = list(pats)
    for b in range(35):
        assert np.array_equal(kinds[64 * b:64 * b + 64], pats[names[b]])
    assert np.array_equal(kinds[64 * 35:], pats[names[0]][:37])
    # section c: the kinds in turn by chunk -- every quad holds the four kinds
    assert S.turn_kinds(8).tolist() == [S.RARE, S.COMMON_K, S.BURSTS64, S.DRAWN] * 2


def test_phases_cover_every_offset():
    """The phase-packed container: a wave's lanes at 64 different offsets modulo 128 (units of 1 and 2 bytes; 32 offsets of
    rans64's dword unit, every one twice), every multiple of the unit met over section a's batches, and the container
    pack_at_phases builds holds every stream at its phase."""
    nchunks, _ = G.geometry(G.SMALL_BATCHES, 64)
    for unit in (1, 2, 4):
        ph = S.lane_phases(nchunks, unit)
        assert sorted(set(ph.tolist())) == list(range(0, 128, unit))
        for b in range(G.SMALL_BATCHES):
            assert len(set(ph[64 * b:64 * b + 64].tolist())) == min(64, 128 // unit)
        assert np.all(ph % unit == 0)
    streams = [np.full(20 + c % 7, c % 251, dtype=np.uint8) for c in range(130)]
    cont, starts, used = S.pack_at_phases(streams, S.lane_phases(130, 4), 128)
    for c in range(130):
        assert starts[c] % 128 == S.lane_phases(130, 4)[c] and np.all(cont[starts[c]:starts[c] + streams[c].size] == c % 251)
    assert np.all(np.diff(starts) >= [s.size for s in streams[:-1]]) and used == starts[-1] + streams[-1].size


def test_chunk_grid_is_what_it_says():
    """The vectorised generator against the per-stream ones: rare chunks hold frequency-1 symbols alone, common chunks the
    commonest symbol, burst chunks S.bursts' pattern at burst_lead(c) with runs of 64 / 16, drawn chunks follow the model;
    all sixteen leads occur."""
    freqs = S.lane_model(14)
    kinds = S.pattern_kinds(64 * 35)
    grid = S.chunk_grid(freqs, kinds, 256, 5)
    rare, common = S.rare_and_common(freqs)
    assert np.all(freqs[grid[kinds == S.RARE]] == 1) and np.all(grid[kinds == S.COMMON_K] == common)
    for kind, run in ((S.BURSTS64, 64), (S.BURSTS16, 16)):
        for c in np.nonzero(kinds == kind)[0][:40]:
            want = S.bursts(freqs, 256, 0, lead=int(S.burst_lead(c)), run=run) == common
            assert np.array_equal(grid[c] == common, want), (kind, c)
    assert sorted({int(v) for v in S.burst_lead(np.arange(64 * 35))}) == list(range(0, 128, 8))
    drawn = grid[kinds == S.DRAWN]
    assert 0.97 < np.mean(drawn == common) < 0.995 and np.any(drawn != common)  # (16129 / 16384 = 0.984)
    assert grid.dtype == np.uint8 and grid.shape == (64 * 35, 256)
    # symbols without a record never appear
    q = S.quiet_model()
    assert np.all(q[S.chunk_grid(q, kinds, 64, 6)] > 0)
