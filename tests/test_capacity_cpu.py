"""tests/_capacity.py on the CPU: the reference functions against lists written by hand, and, with the oracle, that the case
table covers what it claims -- the frozen tails give the three residues, every row has a middle chunk that is no multiple of
16 bytes, caps_for reaches the zone T <= out_cap < E exactly when there is one, and the rows chosen are every (coding kernel,
placement) pair the compact layout can run.  No GPU."""
import numpy as np
import pytest

import _capacity as C


# ---- the reference against hand-written lists -----------------------------------------------------------------------------
HAND = [
    # lens, offsets (n + 1 entries), T, E
    ([37], [0, 37], 37, 48),                                   # a single chunk
    ([16, 32, 48], [0, 16, 48, 96], 96, 96),                   # all lengths multiples of 16
    ([100, 1], [0, 112, 113], 113, 128),                       # a last length of 1
    ([1, 17, 15, 16], [0, 16, 48, 64, 80], 80, 80),
    ([33, 64, 31], [0, 48, 112, 143], 143, 144),
]


@pytest.mark.parametrize("lens,offs,T,E", HAND)
def test_reference_by_hand(lens, offs, T, E):
    assert [int(v) for v in C.ref_offsets(lens)] == offs
    assert C.total(lens) == T and C.aligned_end(lens) == E
    assert E % 16 == 0 and 0 <= E - T < 16 and (E - T) % 16 == (-lens[-1]) % 16


def test_caps_by_hand():
    # last length 31: T = 143, E = 144; chunk 0 (33 bytes) is the first middle chunk that is no multiple of 16
    caps = C.caps_for([33, 64, 31], 1024)
    assert caps == [("bound", 1024, True), ("E", 144, True), ("E-1 = T", 143, False), ("T-1", 142, False),
                    ("offsets[last]", 112, False), ("offsets[0]+lens[0]", 33, False), ("16", 16, False)]
    # all multiples of 16: E == T, no middle chunk, no cap in [T, E)
    caps = C.caps_for([16, 32, 48], 96)
    assert caps == [("bound = E = T", 96, True), ("E-1 = T-1", 95, False), ("offsets[last]", 48, False), ("16", 16, False)]
    assert C.middle_chunk([16, 32, 48]) is None and C.middle_chunk([16, 33, 48]) == 1 and C.middle_chunk([37]) is None
    # a single chunk of 37 bytes: the last chunk has no room at out_cap 0
    caps = dict((label, (cap, fits)) for label, cap, fits in C.caps_for([37], 64))
    assert caps["offsets[last]"] == (0, False) and caps["E"] == (48, True) and caps["T"] == (37, False) and caps["16"] == (16, False)
    # a container of one granule fits out_cap 16
    assert C.caps_for([9], 32) == [("bound", 32, True), ("E = 16", 16, True), ("E-1", 15, False), ("T", 9, False), ("T-1", 8, False),
                                   ("offsets[last]", 0, False)]


def test_generator_slices(oracle):
    """zipf_slice: symbols [start, start + count) of the oracle's stream, u8 and u16 alphabets."""
    for K in (256, 4096):
        whole = oracle.gen_zipf(70000, K=K, s=1.0, seed=1)
        for start, count in ((0, 100), (1, 1), (4096 * 2, 227), (69000, 1000)):
            assert np.array_equal(C.zipf_slice(oracle, start, count, K), whole[start:start + count]), (K, start, count)


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_rows_cover_every_compact_placement():
    """The chosen rows' (kernel, placement) pairs are the list read from KERNEL_ROWS' encode column, each is what the matrix
    expects of the row in the regime named, and every pair the column can name is chosen or listed as no placement of the
    compact layout -- a new encoder row fails here until someone decides where it belongs."""
    assert len({c.id for c in C.CASES}) == len(C.CASES)
    chosen = {(c.kernel, c.placement) for c in C.CASES}
    assert chosen == C.MUST_COVER, (sorted(chosen - C.MUST_COVER), sorted(C.MUST_COVER - chosen))
    for c in C.CASES:
        assert C.expected_pair(c) == (c.kernel, c.placement), (c.id, C.expected_pair(c))
        assert tuple(C.row_of(c)["opts"]) == tuple(o for o in c.opts if o[0] != C.OPT_ENC_SCRATCH_RING), c.id
    named = C.encode_pairs()
    assert not (chosen & C.NOT_COMPACT_PLACEMENT)
    undecided = named - chosen - C.NOT_COMPACT_PLACEMENT
    assert not undecided, ("encode pairs of KERNEL_ROWS without a capacity case", sorted(undecided))
    assert not (chosen | C.NOT_COMPACT_PLACEMENT) - named, "a pair no row of KERNEL_ROWS names"
    # the check has teeth: a row with an encoder nobody has placed is reported
    extra = dict(C.KERNEL_ROWS[0], encode=("k_encode_new", 1))
    assert C.encode_pairs(C.KERNEL_ROWS + [extra]) - chosen - C.NOT_COMPACT_PLACEMENT == {("k_encode_new", 1)}
    # the variants the pair alone does not name: the alias encoder with its mailbox in LDS and in global memory, the scratch ring
    assert {C.row_of(c)["K"] for c in C.CASES if c.kernel == C.AL} == {256, 4096}
    assert [c.id for c in C.CASES if (C.OPT_ENC_SCRATCH_RING, 1) in c.opts] == ["word-64-scratch-ring"]
    assert sorted(c.id for c in C.CASES if C.is_adaptive(c)) == ["byte-64-per-chunk-models", "word-64-per-chunk-models"]


@pytest.mark.parametrize("cus", [C.FROZEN_CUS, 64])
def test_shapes_reach_the_dispatch_thresholds(cus):
    """The shapes restate the launchers' rules (encode_lanes.hip encode_lanes_staged_waves / encode_lanes_r64x2_shape,
    launchers.hpp lanes_applicable, api.cpp's ring condition); what the library then runs is asserted on the GPU."""
    for c in C.CASES:
        row, full = C.row_of(c), C.full_chunks(c, cus)
        nchunks, batches = full + 1, (full + 1 + 63) // 64
        assert nchunks >= 3, c.id  # (a first, a middle and the last chunk)
        if c.shape == "wave":
            assert row["ways"] >= 32 and nchunks < 64
        elif c.shape == "lanes16":
            assert nchunks >= 64 and batches < 6 * cus
        elif c.shape == "groups":
            assert row["ways"] == 8 and nchunks >= 64 and nchunks % 8 != 0
        elif c.shape == "staged":
            assert batches == 6 * cus and (full - 1 + 63) // 64 < 6 * cus, "the threshold itself"
        elif c.shape == "r64x2":
            assert full // 64 == cus and (full - 64) // 64 < cus
        else:
            assert c.shape == "ring" and nchunks == 64 * cus + 1  # > CUs x 32 waves x 2 ring slots
        if c.regime == "H":  # no larger than the matrix's "half the resident waves"
            assert nchunks <= C.regime_chunks(c, cus), (c.id, nchunks, C.regime_chunks(c, cus))


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_tails_residues_and_caps(oracle, case):
    """With the oracle alone: the frozen tails are what the search finds and give the three residues; a middle chunk that is
    no multiple of 16 exists; caps_for has a cap in [T, E) for the two non-zero residues and none for residue 0.  (lens: the
    first chunks and the tail chunk -- offsets in front of them do not change T mod 16.)"""
    cus = C.FROZEN_CUS
    assert C.find_tails(oracle, case, cus) == case.tails, "the frozen tails are not the search's"
    coder = C.Coder(oracle, case, cus)
    row = C.row_of(case)
    head = coder.head_lengths(4)
    assert len(head) >= 2
    unit = C.UNIT[row["fmt"]]
    assert C.residues_of(case) == (unit, 16 - unit, 0)
    for label, tail, residue in zip(C.RESIDUE_LABELS, case.tails, C.residues_of(case)):
        assert 1 <= tail <= row["chunk"]
        lens = head + [coder.tail_length(tail)]
        assert all(v % unit == 0 for v in lens), (case.id, lens)
        T, E = C.total(lens), C.aligned_end(lens)
        assert T % 16 == residue == lens[-1] % 16, (case.id, label, tail, lens[-1])
        m = C.middle_chunk(lens)
        assert m is not None and m < len(lens) - 1, (case.id, "no middle chunk with len % 16 != 0", lens)
        caps = C.caps_for(lens, C.align16(E) + 4096)
        offs = [int(v) for v in C.ref_offsets(lens)]
        zone = [cap for _, cap, fits in caps if T <= cap < E]
        assert bool(zone) == (residue != 0), (case.id, label, caps)
        assert all(not fits for _, cap, fits in caps if cap < E) and all(fits for _, cap, fits in caps if cap >= E)
        assert len({cap for _, cap, _ in caps}) == len(caps)
        # the middle cap: chunk m fits raw but not aligned, and nothing behind it fits
        mid = offs[m] + lens[m]
        assert mid in [cap for _, cap, _ in caps] and mid < offs[m] + C.align16(lens[m]) == offs[m + 1]
        assert {E, E - 1, T, T - 1, offs[-2], 16} <= {cap for _, cap, _ in caps}
