"""The CPU side of the decoders' damage tests (tests/_verdict.py, tests/test_gpu_verdict.py): no GPU.

  * the reference decoder itself: on healthy oracle streams of every format and every interleave a verdict row uses it
    returns the oracle's symbols, verdict GOOD, consumed == len, and never needs a byte behind the stream -- against
    tests/_oracle.py's decoder (rans_amd_decode_host needs a context, that is a device: tests/test_gpu_verdict.py compares it);
  * every proof of the catalogue, for every row, entry and layout: index damage fails the header's rule on integers, model
    damage fails the sum rule, stream damage makes the reference's verdict BAD without a read at or behind the chunk's own
    last granule -- and there IS such an instance of every entry for every row (make_case raises where none is found);
  * the healthy edges are what they claim (H1: N * state_bytes long; H2: the container's end phases), R1 needs more than 16
    bytes behind container_bytes;
  * which start phases (off mod 16) the slot layout of every row reaches;
  * no chunked decoder kernel without a verdict row.
"""
import numpy as np
import pytest

import _verdict as V
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_NAMES, FMT_R64, FMT_WORD
from _kernel_rows import KERNEL_ROWS, UNIFORM, pick, registry

ROWS = V.VERDICT_ROWS
ROW_IDS = [r["id"] for r in ROWS]


@pytest.mark.parametrize("fmt,sb,K", [(FMT_BYTE, 14, 256), (FMT_BYTE, 12, 256), (FMT_WORD, 12, 256), (FMT_WORD, 12, 1024), (FMT_R64, 14, 256),
                                      (FMT_R64, 20, 256), (FMT_ALIAS, 16, 256), (FMT_ALIAS, 16, 4096)],
                         ids=lambda v: str(v))
def test_reference_equals_oracle(oracle, fmt, sb, K):
    for ways in (1, 2, 4, 8, 32, 64, 128):
        for n in (0, 1, ways - 1, ways, 5 * ways + 3, 1500):
            syms = oracle.gen_zipf(max(n, 1), K, 1.0, 7 + ways)[:n]
            freqs, _ = oracle.normalize(oracle.count_freqs(oracle.gen_zipf(4000, K, 1.0, 7 + ways), K), 1 << sb)
            syms = np.where(freqs[syms] == 0, int(np.argmax(freqs)), syms).astype(syms.dtype)
            om = oracle.model(freqs, sb, with_alias=fmt == FMT_ALIAS)
            stream = oracle.encode(fmt, om, syms, ways)
            v = V.ref_decode(V.RefModel(fmt, om), ways, stream, 0, n, stream.size, stream.size, "raise")
            what = (FMT_NAMES[fmt], sb, K, ways, n)
            assert v.good and v.consumed == stream.size and not v.needed_beyond and v.max_units <= 2, what
            assert np.array_equal(v.syms, syms), what
            assert np.array_equal(oracle.decode(fmt, om, stream, n, ways, dtype=syms.dtype), syms), what
            # ... and the verdict notices: a claimed length one unit short, a symbol fewer
            if n > ways:
                short = V.ref_decode(V.RefModel(fmt, om), ways, stream, 0, n, stream.size - V.UNIT[fmt], stream.size, "raise")
                assert not short.good and np.array_equal(short.syms, syms), what


@pytest.mark.parametrize("rid", ROW_IDS)
def test_reference_on_every_chunk_of_the_row(oracle, rid):
    """Every chunk of the row's container, in every layout (the 512 Ki-symbol chunks: the first and the last two)."""
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row)
    for layout in V.LAYOUTS:
        cont, offs, lens = V.lay_out(sh, layout)
        chunks = [0, sh.nchunks - 1] if row["big"] else range(sh.nchunks)
        for c in (chunks if layout == "compact" or not row["big"] else [sh.nchunks - 1]):
            off, ln = int(offs[c]), int(lens[c])
            assert V.index_rule(sh.fmt, sh.ways, off, ln, int(offs[-1]))
            v = V.ref_decode(sh.model_of(c), sh.ways, cont, off, sh.nsym_of(c), ln, V.granule_limit(off, ln), "raise")
            assert v.good and v.consumed == ln and v.max_units <= 2, (rid, layout, c, v)
            assert np.array_equal(v.syms, sh.syms[c * sh.chunk:c * sh.chunk + sh.nsym_of(c)]), (rid, layout, c)


def check_proofs(case, shape):
    """What a GPU test may assert of `case`: see the module docstring of tests/_verdict.py."""
    assert case.count == len(case.damaged) == len(case.rejected) + len(case.flagged)
    for c, entry, mode, good, beyond in case.proofs:
        assert good is False, (c, entry, "the reference's verdict is not BAD")
        assert beyond is False, (c, entry, "the reference needed a byte behind the chunk's last granule, or a third byte in one step")
    for c in range(shape.nchunks):  # every index entry left in the case: the rule says what the case says
        ok = V.index_rule(shape.fmt, shape.ways, int(case.offs[c]), int(case.lens[c]), case.total)
        rejected_by_index = c in case.rejected and not (case.rows is not None and not np.array_equal(case.rows[c], shape.rows[c]))
        assert ok == (not rejected_by_index), (c, ok)
        assert -V.MARGIN + 4096 <= int(case.offs[c]) and int(case.offs[c]) + int(case.lens[c]) <= case.total + V.MARGIN - 4096


@pytest.mark.parametrize("rid", ROW_IDS)
def test_every_entry_has_a_proven_instance(oracle, rid):
    """THE CAP: every catalogue entry of the row, in every layout, has an instance whose verdict is proved (make_case
    searches from the drawn position and raises when there is none)."""
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row)
    entries = V.entries_of(row)
    assert {"I2", "I3", "I4", "I5", "S1", "S2", "S3", "S4", "S5"} <= set(entries) and ("I6" in entries) == (not row["big"])
    assert ("I1" in entries) == (V.UNIT[row["fmt"]] > 1)
    assert ("S6" in entries) == (row["kernel"] in V.DESCRIPTOR_KERNELS)
    assert ("M1" in entries) == (row["kind"] == "adaptive")
    for layout in (V.LAYOUTS if not row["big"] else ("compact",)):
        for entry in V.entries_in(row, layout):
            sh = V.shape_of(oracle, row, V.entry_variant(row, entry))
            case = V.make_case(sh, layout, V.entry_damage(sh, layout, entry))
            assert case.count == 1 and len(case.proofs) == 1 and case.proofs[0][1] == entry, (rid, layout, entry)
            check_proofs(case, sh)
            c = case.damaged[0]
            first, nsym = c * sh.chunk, sh.nsym_of(c, case.n)
            if entry[0] in "IM":
                assert np.all(case.out[first:first + nsym] == V.POISON_OF(sh)), (rid, layout, entry)
            elif entry in ("S1", "S2"):  # the same bytes: the same symbols, the true length consumed
                assert np.array_equal(case.out[first:first + nsym], sh.syms[first:first + nsym]), (rid, layout, entry)
            assert (case.proofs[0][2] == "zeros") <= (row["kernel"] in V.DESCRIPTOR_KERNELS)
            others = np.ones(sh.n, dtype=bool)
            others[first:first + sh.chunk] = False
            assert np.array_equal(case.out[others[:case.out.size]], sh.syms[others])


@pytest.mark.parametrize("rid", ROW_IDS)
def test_every_placement_is_proved(oracle, rid):
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row)
    for name, chunks in V.placements(sh).items():
        case = V.make_case(sh, "compact", V.mixed(sh, "compact", chunks, index_only=name.startswith("rejected")), prove=not row["big"])
        assert case.count == len(chunks) and case.damaged == sorted(chunks), (rid, name)
        if not row["big"]:
            check_proofs(case, sh)
        if name == "every":
            assert case.count == sh.nchunks
        if row["unit"] >= 4 and name in ("one-whole-unit", "only-the-longest-healthy", "quad-mates"):
            assert case.rejected and case.flagged, (rid, name, "an index-rejected member beside stream-damaged ones")


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if r["kind"] == "static"])
def test_healthy_edges(oracle, rid):
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row, "h1")
    last = sh.streams[-1]
    assert last.size == sh.ways * V.STATE_BYTES[sh.fmt], (rid, last.size)  # H1: the states and nothing else
    v = V.ref_decode(sh.model_of(sh.nchunks - 1), sh.ways, last, 0, 3, last.size, last.size, "raise")
    assert v.good and np.all(v.syms == int(np.argmax(sh.freqs)))
    base = V.shape_of(oracle, row)
    for end_mod in V.h2_ends(row["fmt"]):
        case = V.make_case(base, "compact", [], end_mod=end_mod)
        assert case.total % 16 == end_mod and case.count == 0
        c = base.nchunks - 1
        assert int(case.offs[c]) + int(case.lens[c]) == case.total  # the last chunk ends on the container's last byte


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if not r["big"]])
def test_r1_needs_bytes_behind_the_container(oracle, rid):
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row, "r1")
    case, v = V.make_r1(sh)
    assert v.needed_beyond and not v.good and v.max_units <= 2
    assert v.last_read >= case.total + 16, (rid, v.last_read, case.total)
    # (the first half is the input: all states were L there)
    c = sh.nchunks - 1
    assert np.array_equal(v.syms[:sh.r1_half], sh.syms[c * sh.chunk:c * sh.chunk + sh.r1_half])


# The start phases (off mod 16) of the slot layout, whose chunks END on 16 bytes: recorded from the oracle's streams of
# each row -- a row reaches a phase iff one of its streams has that length mod 16, in steps of the format's unit.
def test_start_phases_of_the_slot_layout(oracle):
    for row in ROWS:
        sh = V.shape_of(oracle, row)
        _, offs, lens = V.lay_out(sh, "slots")
        phases = {int(o) & 15 for o in offs[:-1]}
        unit = V.UNIT[row["fmt"]]
        assert all(p % unit == 0 for p in phases) and phases == {(-int(ln)) & 15 for ln in lens}
        assert np.all((offs[:-1] + lens) % 16 == 0)
        # at least three phases everywhere, and every phase the unit allows where a row holds 80 chunks and more
        # (rans64 two-way: its stream is whole 4-byte units behind 16 bytes of states -- four phases)
        assert len(phases) >= 3, (row["id"], sorted(phases))
        if sh.nchunks >= 80 and unit < 4:
            assert len(phases) >= (16 // unit) - 4, (row["id"], sorted(phases))
        _, coffs, _ = V.lay_out(sh, "compact")
        assert {int(o) & 15 for o in coffs[:-1]} == {0}


def test_no_chunked_decoder_without_a_verdict_row():
    """Every kernel name rans_amd_decode / rans_amd_decode_adaptive[_fmt] can report (the names of the registry's uniform
    family, tests/_kernel_rows.py, that start with k_decode; the ragged-batch kernels are families of their own and have damage
    tests of their own) has a row in VERDICT_ROWS, the rows name no kernel that is gone, and every decoder of KERNEL_ROWS is there."""
    decoders = {n for n in registry()[UNIFORM] if n.startswith("k_decode")}
    assert len(decoders) >= 17 and not any("batch" in n for n in decoders), sorted(decoders)
    have = {r["kernel"] for r in ROWS}
    assert not decoders - have, ("decoder kernels without a verdict row", sorted(decoders - have))
    assert not have - decoders, ("verdict rows for kernels no launcher reports", sorted(have - decoders))
    matrix = {pick(r["decode"], g) for r in KERNEL_ROWS for g in r["regimes"]}
    assert matrix == have
    # the check has teeth
    assert "k_decode_lanes" in decoders - {r["kernel"] for r in ROWS if not r["big"]}
    # and the descriptor kernels are the wave-per-chunk ones: decode_wave.hip and decode_dual.hip
    assert set(V.DESCRIPTOR_KERNELS) == {n for n in have if n.startswith("k_decode<") or n in ("k_decode_word64", "k_decode_dual<alias>")}
