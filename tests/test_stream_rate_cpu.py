"""No GPU: the proof that the inputs of tests/test_gpu_rate_extremes.py sit at the bounds that file claims.

  * the byte-count identity: for every format and input the GPU tests use, the bytes tests/_stream_rate.py's model counts
    per round, plus the flushed states, are Oracle.encode's stream size, and the model's final states are the stream's
    header -- the model cannot drift from the oracle;
  * the input conditions, all of them consequences of the formats: 96 bytes in eight rounds of an 8-way word stream of
    frequency-1 symbols and the four lock-step phases, 32 bytes in every eight rounds of a 2-way byte stream at
    scale_bits = 16, 1024 and more silent rounds, and both extremes inside one burst stream;
  * the case table of the GPU file names every batch kernel the launchers can report, under a rare-only and under a
    common-only stream."""
import numpy as np
import pytest

import _stream_rate as S
import test_gpu_rate_extremes as G
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD


def identity(oracle, fmt, freqs, sb, syms, ways, om=None, remap=None):
    """sum(round_bytes) + the flushed states == Oracle.encode(...).size, and the states are the stream's header."""
    om = om or oracle.model(freqs, sb, with_alias=(fmt == FMT_ALIAS))
    stream = oracle.encode(fmt, om, syms, ways)
    per_round, states = S.simulate(fmt, freqs, sb, syms, ways, remap)
    assert int(per_round.sum()) + ways * S.STATE_BYTES[fmt] == stream.size, (fmt, sb, ways, syms.size)
    assert np.array_equal(states, S.stream_states(fmt, stream, ways)), (fmt, sb, ways, syms.size)
    return per_round


# ---- the model against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,sb,ways", [(FMT_WORD, 12, 8), (FMT_WORD, 12, 64), (FMT_BYTE, 14, 2), (FMT_BYTE, 8, 3), (FMT_BYTE, 16, 2),
                                         (FMT_R64, 14, 2), (FMT_R64, 20, 64), (FMT_ALIAS, 16, 64), (FMT_ALIAS, 12, 5)])
def test_identity_on_zipf_input(oracle, fmt, sb, ways):
    """The control: Zipf symbols under their own normalised model, lengths around a round and around many."""
    for n in (0, 1, ways - 1, ways, ways + 1, 37 * ways + 5):
        syms = oracle.gen_zipf(n, K=256, s=1.0, seed=3 + n)
        f, _ = oracle.normalize(oracle.count_freqs(oracle.gen_zipf(1 << 16, K=256, s=1.0, seed=9), 256), 1 << sb)
        om = oracle.model(f, sb, with_alias=(fmt == FMT_ALIAS))
        remap = om.table("alias_remap", 1 << sb) if fmt == FMT_ALIAS else None
        identity(oracle, fmt, f, sb, syms, ways, om, remap)


@pytest.mark.parametrize("model", list(G.A_MODELS))
def test_identity_section_a(oracle, model):
    om = oracle.model(G.A_MODELS[model](), 12)
    for j in range(G.A_BATCHES):
        freqs, counts, contents, _ = G.a_batch(model, j)
        for k in range(G.A_STREAMS):
            identity(oracle, FMT_WORD, freqs, 12, contents[k], 8, om)
    for name in G.A_WAVES:
        freqs, counts, contents, _ = G.a_wave(model, name)
        for k in range(8):
            identity(oracle, FMT_WORD, freqs, 12, contents[k], 8, om)


@pytest.mark.parametrize("bid", list(G.B_CASES))
def test_identity_section_b(oracle, bid):
    fmt, sb, ways = G.B_CASES[bid][:3]
    freqs, data, _ = G.b_case(bid)
    om = oracle.model(freqs, sb)
    for d in data:
        identity(oracle, fmt, freqs, sb, d, ways, om)


@pytest.mark.parametrize("row", G.C_ROWS, ids=[r["id"] for r in G.C_ROWS])
def test_identity_section_c(oracle, row):
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    for name, freqs in G.c_classes(row):
        om = oracle.model(freqs, sb, with_alias=(fmt == FMT_ALIAS))
        remap = om.table("alias_remap", 1 << sb) if fmt == FMT_ALIAS else None
        counts, contents = G.c_batch(row, freqs)
        for k in range(G.C_STREAMS):
            per_round = identity(oracle, fmt, freqs, sb, contents[k], ways, om, remap)
            if name == "one-symbol":  # nothing but the flushed states leaves
                assert per_round.sum() == 0


# ---- the input conditions --------------------------------------------------------------------------------------------
def test_word_rare_only_takes_96_bytes_per_eight_rounds_at_four_phases():
    """Frequency-1 symbols only, 8-way: every window of eight rounds takes 96 bytes -- the format's maximum: eight rounds
    remove at most 96 + 15 bits from a state, less than seven words --, the states renormalise in lock-step, 16, 16, 16, 0
    bytes per round, and p = 0..3 shifting symbols per state behind the rare ones put the round without a word at four
    different round numbers modulo 4: the burst moves against the decoders' fixed checkpoint rounds."""
    zero_at = []
    for model in (S.rate_model_16(), S.quiet_model()):
        for p in range(4):
            n = 8 * 132
            syms = S.rare_only(model, n, 5, shift=p)
            rb = S.round_bytes(FMT_WORD, model, 12, syms, 8)
            rare_rounds = rb[:132 - p]
            assert set(rare_rounds.tolist()) == {0, 16}, "not in lock-step"
            w = S.windows(rare_rounds)
            assert w.size > 100 and w.max() == 96 and w.min() == 96
            zeros = np.nonzero(rare_rounds == 0)[0]
            assert len(set((zeros % 4).tolist())) == 1 and np.all(np.diff(zeros) == 4)
            zero_at.append(int(zeros[0] % 4))
    assert sorted(zero_at[:4]) == [0, 1, 2, 3] and zero_at[4:] == zero_at[:4], zero_at
    # the inputs of the GPU file: every rare-only stream of sixteen rounds and more, of every batch and of the two single waves,
    # holds a 96-byte window (a stream of 77 symbols and three shifting ones per state has fewer than eight rare rounds)
    for model in G.A_MODELS:
        seen = 0
        sets = [(G.a_batch(model, j), [G.a_kind(j, k) for k in range(G.A_STREAMS)]) for j in range(G.A_BATCHES)]
        sets += [(G.a_wave(model, name), G.A_WAVES[name][1]) for name in G.A_WAVES]
        for (freqs, counts, contents, _), kinds in sets:
            for k in range(counts.size):
                if kinds[k].startswith("rare+") and counts[k] >= 128:
                    assert S.windows(S.round_bytes(FMT_WORD, freqs, 12, contents[k], 8)).max() == 96, (model, k)
                    seen += 1
        assert seen >= 7 * 16
    freqs, data, _ = G.b_case("word-groups-rare")
    patterns = [tuple(S.round_bytes(FMT_WORD, freqs, 12, d, 8)[8:24].tolist()) for d in data]
    assert len(set(patterns[:4])) == 4, "the four shifts give the same pattern"
    assert all(patterns[c] == patterns[c % 4] for c in range(G.B_CHUNKS))
    for d in data:
        assert S.windows(S.round_bytes(FMT_WORD, freqs, 12, d, 8)).max() == 96


def test_byte_pairs_take_32_bytes_in_every_eight_rounds():
    """2-way byte format, scale_bits = 16, frequency-1 symbols only: a state in [2^23, 2^31) becomes x >> 16 < 2^15 and takes
    two bytes, in every round -- k_decode_byte_pairs' bound of 8 x 2 x 2 bytes, sustained.  At 14 bits: 28 in every window."""
    for bid, want in (("byte-pairs-16bit-mod32", 32), ("byte-pairs-16bit-mod64", 32), ("byte-pairs-14bit-mod32", 28),
                      ("byte-pairs-14bit-mod64", 28)):
        fmt, sb, ways = G.B_CASES[bid][:3]
        freqs, data, _ = G.b_case(bid)
        for d in data:
            rb = S.round_bytes(fmt, freqs, sb, d, ways)
            w = S.windows(rb[:d.size // 2])
            assert w.size >= 120 and w.max() == want and w.min() == want, (bid, w.min(), w.max())
            if sb == 16:
                assert np.all(rb[:d.size // 2] == 4)


def test_common_only_is_silent_for_1024_rounds():
    """4065 + 16 + 15 x 1, the 4065-symbol only, 8-way: 1024 and more consecutive rounds take no byte, and the whole stream of
    65536 symbols is the flushed states and a few words.  Under 3841 + 255 x 1 the longest silence any input can have is
    172 rounds -- x' = x - 255 (x >> 12) loses 0.093 bits a round -- and 162 under 3826 + 16 + 254 x 1."""
    q = S.quiet_model()
    rb = S.round_bytes(FMT_WORD, q, 12, S.common_only(q, 65536), 8)
    assert S.longest_silence(rb) >= 1024
    assert rb.sum() <= 8 * 2 * 6, "more than a few words"
    for model in (S.rate_model(), S.rate_model_16()):
        rb = S.round_bytes(FMT_WORD, model, 12, S.common_only(model, 65536), 8)
        assert 160 <= S.longest_silence(rb) <= 176, S.longest_silence(rb)
        assert set(rb.tolist()) == {0, 16}  # (every state holds the same value)
    # the GPU file's stalled cursor: 65536 common-only symbols beside seven rare-only streams
    for model, least in (("4065-16-15x1", 1024), ("3826-16-254x1", 160)):
        freqs, counts, contents, _ = G.a_wave(model, "stalled-beside-draining")
        assert S.longest_silence(S.round_bytes(FMT_WORD, freqs, 12, contents[0], 8)) >= least
        for k in range(1, 8):
            assert S.windows(S.round_bytes(FMT_WORD, freqs, 12, contents[k], 8)).max() == 96


def test_bursts_hold_both_extremes():
    """Runs of 64 rare and 64 common symbols in turn: a window of eight rounds that takes nothing and one that takes 96 bytes
    in one stream, wherever the runs start."""
    for model in (S.rate_model_16(), S.quiet_model()):
        for lead in range(0, 64, 8):
            rb = S.round_bytes(FMT_WORD, model, 12, S.bursts(model, 1024 + 36, 7, lead=lead), 8)
            w = S.windows(rb)
            assert w.min() == 0 and w.max() == 96, (lead, w.min(), w.max())
    freqs, data, _ = G.b_case("word-groups-bursts")
    for d in data:
        w = S.windows(S.round_bytes(FMT_WORD, freqs, 12, d, 8))
        assert w.min() == 0 and w.max() == 96
    # section a: every burst stream of 640 symbols and more, of every batch (shorter ones hold two runs of each kind at most)
    for model in G.A_MODELS:
        seen = 0
        for j in range(G.A_BATCHES):
            freqs, counts, contents, _ = G.a_batch(model, j)
            for k in range(G.A_STREAMS):
                if G.a_kind(j, k) == "bursts" and counts[k] >= 640:
                    w = S.windows(S.round_bytes(FMT_WORD, freqs, 12, contents[k], 8))
                    assert w.min() == 0 and w.max() == 96, (model, j, k, w.min(), w.max())
                    seen += 1
        assert seen >= 8


# ---- what the GPU file covers ------------------------------------------------------------------------------------------
def test_section_a_meets_every_combination():
    """Over the seven batches every content kind meets every phase and every count; the phases are all 64 even ones; and
    eight states (32 bytes) straddle the first 128-byte block for the phases from 98 on."""
    phase_kind, kind_count, count_phase_classes = set(), set(), set()
    for j in range(G.A_BATCHES):
        for k in range(G.A_STREAMS):
            phase_kind.add((G.a_phase(k), G.a_kind(j, k)))
            kind_count.add((G.a_kind(j, k), G.a_count(j, k)))
            count_phase_classes.add((G.a_count(j, k), G.a_phase(k) + 32 > 128))
    assert len(phase_kind) == 64 * len(G.A_KINDS)
    assert len(kind_count) == len(G.A_KINDS) * len(G.A_COUNTS)
    assert len(count_phase_classes) == 2 * len(G.A_COUNTS)
    assert sorted({G.a_phase(k) for k in range(G.A_STREAMS)}) == list(range(0, 128, 2))
    assert sorted(G.A_COUNTS) == sorted(128 * b + t for b in (0, 1, 5) for t in (0, 1, 77, 127))
    for j in range(G.A_BATCHES):  # the groups of a wave differ: no octet of one kind or one count
        for o in range(8):
            ks = range(8 * o, 8 * o + 8)
            assert len({G.a_kind(j, k) for k in ks}) >= 7 and len({G.a_count(j, k) for k in ks}) >= 4


def test_no_batch_kernel_without_a_rate_case():
    """Every kernel name a batch launcher can report (the registry's batch and batch_word_groups_decode families,
    tests/_kernel_rows.py), every name of BATCH_ROWS and GROUP_ROWS, and the two uniform ring decoders are asserted by a case of
    RATE_CASES under a rare-only and under a common-only stream: a later batch kernel needs a rate-extreme case."""
    from _kernel_rows import BATCH, BATCH_ROWS, BATCH_WORD_GROUPS_DECODE, GROUP_ROWS, registry, row_batch_kernel_names
    need = registry()[BATCH] | registry()[BATCH_WORD_GROUPS_DECODE]
    need |= row_batch_kernel_names(BATCH_ROWS) | row_batch_kernel_names(GROUP_ROWS)
    need |= {"k_decode_word_groups", "k_decode_byte_pairs"}
    assert len(need) >= 16, sorted(need)
    for content in ("rare", "common"):
        have = G.kernels_under(content)
        assert not need - have, ("no rate-extreme case under a %s-only stream" % content, sorted(need - have))
    # the check has teeth: without its cases a kernel is reported missing
    less = {k for c in G.RATE_CASES if c["id"] != "alias256-64" for k in c["kernels"]}
    assert "k_decode_batch<alias>" in need - less
    # and the table is what the tests run: a case per parametrised test of sections b and c, one per model of section a
    assert {c["id"] for c in G.RATE_CASES if c["section"] == "b"} == set(G.B_CASES)
    assert [c["id"] for c in G.RATE_CASES if c["section"] == "c"] == [r["id"] for r in G.C_ROWS]
    assert [c["id"] for c in G.RATE_CASES if c["section"] == "a"] == ["groups-" + m for m in G.A_MODELS]
