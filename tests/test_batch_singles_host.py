"""Ragged batches with sixty-four 1-way streams per wave (RANS_AMD_OPT_BATCH_SINGLES), the part that needs no GPU: the option's
constant in the header's fourth enum, the registry's fourth list held to the rows of tests/_batch_singles.py with the first
three lists left as they were, the proof that the rate inputs of tests/test_gpu_batch_singles.py reach each format's bound, the
counts and start phases of that file, and the verdict of every case of its damage catalogue, worked out by the plain reference
decoder of tests/_verdict.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import _batch_alias_pairs as A
import _batch_encode_alias_pairs as AE
import _batch_singles as N
import _stream_rate as S
import _verdict as V
import ryg_rans_amd as R
from _kernel_rows import CSRC, OPTIONS, ROOT, registry
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD


def test_batch_singles_option_constant():
    """RANS_AMD_OPT_BATCH_SINGLES is 13 in a NEW enum behind the third and in the package; the three earlier enums hold what
    they held, where they stood (three lines start with `enum rans_amd_option`); the version has not moved (additions only);
    and a NULL context is refused before the option is looked at."""
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    assert N.OPT_BATCH_SINGLES == R.OPT_BATCH_SINGLES == 13
    first = re.search(r"enum rans_amd_option \{(.*?)\n\};", header, re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", first, re.M)] == list(zip(OPTIONS, range(11)))
    more = re.search(r"\};\n[^\n]*\nenum rans_amd_option_more \{(.*?)\n\};\nint rans_amd_ctx_set_option", header, re.S)
    assert more and re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", more.group(1), re.M) == [("BATCH_ALIAS_PAIRS", "11")]
    third = re.search(r"int rans_amd_ctx_set_option[^\n]*\n[^\n]*\nenum rans_amd_option_third \{(.*?)\n\};\n", header, re.S)
    assert third and re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", third.group(1), re.M) == [("BATCH_ENCODE_ALIAS_PAIRS", "12")]
    fourth = re.search(r"enum rans_amd_option_third \{.*?\n\};\n[^\n]*\nenum rans_amd_batch_option \{(.*?)\n\};\n", header, re.S)
    assert fourth, "the new enum does not stand directly behind the third"
    assert re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", fourth.group(1), re.M) == [("BATCH_SINGLES", "13")]
    assert len(re.findall(r"^enum rans_amd_option", header, re.M)) == 3
    assert sorted(int(v) for v in re.findall(r"^    RANS_AMD_OPT_\w+\s*=\s*(\d+)", header, re.M)) == list(range(14))
    for v, n in enumerate(OPTIONS + A.OPTIONS_MORE + ("BATCH_ENCODE_ALIAS_PAIRS", "BATCH_SINGLES")):
        assert getattr(R, "OPT_" + n) == v, n
    assert re.search(r"#define\s+RANS_AMD_VERSION\s+600\b", header)
    assert R.lib().rans_amd_ctx_set_option(None, 13, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()


def test_no_singles_batch_kernel_without_a_row():
    """The fourth list is exactly the four names, ids 56..59, family batch_singles_decode (the driver itself fails on a name or
    family of the first three lists and on ids that do not follow them); rows and names match in both directions, every
    format's rows are 1-way with the format's wave encoder; and the check has teeth: without a format's rows its name is
    reported missing."""
    assert N.fourth_list() == [("batch_singles_decode", "k_decode_batch_singles<%s>" % f, 56 + k) for k, f in enumerate(N.FORMATS)]
    N.check_fourth_list_rows()
    for f in N.FORMATS:
        d = N.SINGLES[f]
        assert d.option == 13 and d.side == "decode" and d.fmt == N.FMT[f] and d.ways == 1 and d.streams == 64
        assert d.main is N.SINGLE_ROWS[f][0] and d.wave_kernel == "k_decode_batch<%s>" % f and d.family == "batch_singles_decode"
        assert d.graph == (N.FMT_NAME[f], d.main["sb"], "OPT_BATCH_SINGLES")
        try:
            N.check_fourth_list_rows(rows=[r for r in N.ALL_ROWS if r["fmt"] != d.fmt])
        except AssertionError as e:
            assert N.KERNEL[f] in str(e) and "kernels no row expects" in str(e)
        else:
            raise AssertionError("a name without a row went unnoticed")
    assert [(r["sb"], r["K"]) for r in N.SINGLE_ROWS["byte"]] == [(14, 256), (16, 256), (12, 256), (8, 256), (10, 64)]
    assert [(r["sb"], r["K"]) for r in N.SINGLE_ROWS["r64"]] == [(14, 256), (16, 256), (12, 256), (7, 64), (10, 64)]
    assert [(r["sb"], r["K"]) for r in N.SINGLE_ROWS["alias"]] == [(16, 256), (14, 256), (12, 256), (8, 256), (10, 64)]
    assert [(r["sb"], r["K"]) for r in N.SINGLE_ROWS["word"]] == [(12, 256)]
    src = open(os.path.join(CSRC, "kernel_names.hpp")).read()
    assert all(src.count('"%s"' % N.KERNEL[f]) == 1 for f in N.FORMATS)


def test_the_ids_follow_the_third_list(tmp_path):
    """Ids of all four lists lead to their rows, the fourth list's are 56..59, and an identifier in no list does not compile."""
    src = tmp_path / "id.cpp"
    src.write_text('#include "kernel_names.hpp"\nusing namespace rans_amd;\n'
                   'static_assert((int)KernelId::decode_batch_singles_byte == 56 && (int)KernelId::decode_batch_singles_word == 57, "id");\n'
                   'static_assert((int)KernelId::decode_batch_singles_r64 == 58 && (int)KernelId::decode_batch_singles_alias == 59, "id");\n'
                   'static_assert(kSinglesKernelEntryCount == 4 && kKernelEntryCount == 53, "entries");\n'
                   'static_assert(kernel_entry(KernelId::decode_batch_singles_r64).family == KernelFamily::batch_singles_decode, "row");\n'
                   'static_assert(kernel_entry(KernelId::encode_batch_alias_pairs).family == KernelFamily::batch_alias_pairs_encode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_batch_alias_pairs).family == KernelFamily::batch_alias_pairs_decode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_word64).family == KernelFamily::uniform, "row");\n'
                   'int main() { return 0; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)]).returncode == 0
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::decode_batch_singles_no_such; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "decode_batch_singles_no_such" in r.stderr


def test_the_first_three_lists_print_what_they_printed():
    """The first list's 53 lines, the second list's one and the third list's one are what they were, and the new names and
    family are not among them."""
    registry()
    exe = os.path.join(ROOT, "build", "kernel_names", "kernel_names_driver")
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 53 and not [ln for ln in lines if "singles" in ln]
    families = [ln.split("\t")[0] for ln in lines]
    assert families == ["uniform"] * 30 + ["batch"] * 13 + ["batch_models"] * 4 + [
        "batch_word_groups_decode", "batch_word_groups_encode", "batch_byte_pairs_decode", "batch_byte_pairs_encode", "batch_r64_lanes_decode",
        "batch_r64_lanes_encode"]
    assert lines[0] == "uniform\tk_decode_word64" and lines[37] == "batch\tk_decode_batch<alias>"
    assert lines[52] == "batch_r64_lanes_encode\tk_encode_batch_r64_lanes"
    assert A.second_list() == [("batch_alias_pairs_decode", "k_decode_batch_alias_pairs")]
    assert [tuple(t) for t in AE.third_list()] == [("batch_alias_pairs_encode", "k_encode_batch_alias_pairs")]


def test_counts_and_phases_cover_every_boundary():
    """The rate counts are 64 b + t for b in {0, 1, 5} and t in {0, 1, 31, 63}: no trip, one and several, with no tail, the
    shortest, a tail that ends inside a group of sixteen and the longest; every count meets every kind.  The hand-packed
    container puts stream k at k * unit (mod 64): every unit phase of a 64-byte line, per format.  The single wave-loads hold
    every trip/tail boundary: counts 0..3, 15..17, 63..65, 127..129, 191..193 in one wave."""
    assert set(N.RATE_COUNTS) == {64 * b + t for b in (0, 1, 5) for t in (0, 1, 31, 63)}
    for f in N.FORMATS:
        freqs, counts, contents, phases = N.rate_batch(f)
        unit = N.UNIT[N.FMT[f]]
        assert counts.size == 64 and sorted(set(p % 64 for p in phases)) == list(range(0, 64, unit))
        assert set(counts.tolist()) == set(N.RATE_COUNTS) and all(contents[k].size == counts[k] for k in range(64))
        kinds = [N.rate_kind(k) for k in range(64)]
        assert {(kinds[k], int(counts[k])) for k in range(64)} == {(kd, c) for kd in N.RATE_KINDS for c in N.RATE_COUNTS}
    b = N.WAVE_LOADS["boundaries"]
    assert len(b) == 64 and b[:16] == [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193]
    assert all(len(v) in (64, 65) for v in N.WAVE_LOADS.values()) and N.WAVE_LOADS["second-load-of-one"] == [300] * 65
    assert N.WAVE_LOADS["63-idle-1023-trips"] == [65536] + [127] * 63 and N.WAVE_LOADS["quad-mates-differ"] == [640, 0, 64, 385] * 16
    ends = N.WAVE_LOADS["every-lane-ends-elsewhere"]
    assert len({c >> 6 for c in ends}) == 16 and len({(c >> 6, c & 63) for c in ends}) == 64
    assert N.WAVE_LOADS["all-empty"] == [0] * 64 and N.WAVE_LOADS["mandatory-and-200s"][:7] == [0, 1, 0, 1, 2, 7, 65536]


def test_the_word_formats_bound_is_24_bytes():
    """The largest figure a valid 1-way WORD stream reaches in sixteen symbols, derived from the format alone
    (N.word_group_bound: at most three symbols in a row take a word): 12 words, 24 bytes -- the same figure
    tests/_stream_rate.py's rare_group_bytes gives for frequency-1 symbols (192 bits lost, 16 divides them)."""
    assert N.word_group_bound() == 24
    assert S.rare_group_bytes(FMT_WORD, 12, 1) == (24, 24)
    assert S.interval_bound(FMT_WORD, 12, 1, 16) == 24


@pytest.mark.parametrize("f", N.FORMATS)
def test_rate_inputs_reach_the_formats_bound(oracle, f):
    """255 x 1 and one common symbol, 1-way, the ORACLE's stream of every rate input decoded by plain integers (N.symbol_bytes)
    with the bytes behind every symbol counted:
      * byte, alias and rans64 under a 16-bit model: a frequency-1 symbol leaves x >> 16 whatever its slot, so a byte state in
        [2^23, 2^31) takes two bytes behind EVERY symbol and a rans64 state a dword behind every second one -- 32 bytes in every
        window of sixteen symbols, wherever it starts: half of what the ring's invariant (>= 64 bytes ahead) covers;
      * word at its 12 bits: 24 bytes in every window of sixteen, the largest figure a valid stream reaches (the test above);
      * a common-only stream takes nothing at all under the 16-bit models and one word per 172 symbols under the word format's
        12 bits (silent groups: a lane that requests nothing beside lanes at the bound);
      * the burst streams (runs of 16 rare and 16 common symbols) have windows at the bound and silent symbols in one stream.
    Where tests/_stream_rate.py models the format (all but alias) its per-symbol bytes are the same, symbol for symbol."""
    fmt, sb = N.FMT[f], N.RATE_SB[f]
    bound = 24 if f == "word" else 32
    assert N.RATE_ROW[f]["sb"] == sb and N.RATE_ROW[f]["fmt"] == fmt and N.RATE_ROW[f]["K"] == 256
    assert S.rare_group_bytes(fmt if f != "alias" else FMT_BYTE, sb, 1) == (bound, bound)
    freqs, counts, contents, _ = N.rate_batch(f)
    assert np.array_equal(freqs, S.lane_model(sb)) and int(freqs.sum()) == 1 << sb
    om = oracle.model(freqs, sb, with_alias=fmt == FMT_ALIAS)
    ref = V.RefModel(fmt, om)
    at_bound = silent = burst_both = 0
    for k in range(64):
        n, kind = int(counts[k]), N.rate_kind(k)
        out, taken = N.symbol_bytes(ref, oracle.encode(fmt, om, contents[k], 1), n)
        assert np.array_equal(out, contents[k])
        if fmt != FMT_ALIAS:
            assert np.array_equal(taken, S.round_bytes(fmt, freqs, sb, contents[k], 1)), (f, k)
        w = S.group_bytes(taken, 1)
        if kind == "rare":
            assert np.all(np.isin(contents[k], np.nonzero(freqs == 1)[0]))
            if n >= 16:
                assert w.min() == bound and w.max() == bound, (f, k, n, w.min(), w.max())
                at_bound += 1
        elif kind == "common":
            assert np.all(contents[k] == S.COMMON)
            if f == "word":  # 3841 / 4096 costs 0.093 bits: a word every 172 or 173 symbols (tests/_stream_rate.py quiet_model)
                assert taken.sum() <= 2 * (n // 172 + 1) and (n < 16 or w.min() == 0) and S.longest_silence(taken) >= min(n, 150), (f, k, n)
            else:
                assert taken.sum() == 0, (f, k, n)
            silent += n > 0
        elif n >= 64:
            assert w.max() == bound and S.longest_silence(taken) >= 15, (f, k, n, w.max(), S.longest_silence(taken))
            burst_both += 1
    assert at_bound >= 12 and silent >= 12 and burst_both >= 8, (at_bound, silent, burst_both)


@pytest.mark.parametrize("n", N.DAMAGE_LOADS)
@pytest.mark.parametrize("f", N.FORMATS)
def test_every_damage_case_has_a_decisive_verdict(oracle, f, n):
    """Every case of the catalogue -- per format, nine or ten kinds of damage, applied to one stream, to one lane of each quad
    position, to every second stream and to every stream, on one wave-load and on three -- gets its verdict here: the index
    rule of the header for the rejected kinds, the plain reference decoder for those that are decoded, which must say BAD
    without needing a byte behind the stream's own slack (zeros that no damage touches).  The GPU file asserts exactly these."""
    hb = N.HostBatch(oracle, f, n)
    fmt, unit, sbytes = N.FMT[f], N.UNIT[N.FMT[f]], N.STATE_BYTES[N.FMT[f]]
    assert hb.container_bytes % 16 == 0 and np.all(hb.offs % unit == 0) and hb.counts.min() >= 100 and hb.lens.min() > sbytes + 2 * unit
    assert len(set((hb.offs % 64).tolist())) >= min(n, 64 // unit) // 2
    for c in (0, n - 1):  # the undamaged batch is good
        v = V.ref_decode(hb.ref, 1, hb.cont, int(hb.offs[c]), int(hb.counts[c]), int(hb.lens[c]), V.granule_limit(int(hb.offs[c]), int(hb.lens[c])))
        assert v.good and np.array_equal(v.syms.astype(np.uint8), hb.syms[c])
    kinds = N.damage_kinds(f)
    assert ("misaligned" in kinds) == (unit > 1) and len(kinds) == (10 if unit > 1 else 9)
    for kind in kinds:
        for pname, which in N.damage_patterns(n).items():
            d = N.Damaged(hb, kind, which)
            assert d.bad == list(which) and set(d.proofs) == set(which), (kind, pname)
            assert all(bad for _, bad in d.proofs.values()), (kind, pname, "a verdict that is not BAD")
            assert all(what == ("index" if kind in N.REJECTED else "stream") for what, _ in d.proofs.values())
            assert set(d.written) == (set() if kind in N.REJECTED else set(which))
            want = d.expected(hb, 0xA5)
            for c in which:
                lo, cnt = int(hb.sym_offs[c]), int(hb.counts[c])
                if kind in N.REJECTED:
                    assert np.all(want[lo:lo + cnt] == 0xA5)
                elif kind in ("len-unit", "len+unit"):
                    assert np.array_equal(want[lo:lo + cnt], hb.syms[c])  # all symbols right, the length wrong
                elif kind in ("count-1", "count-64"):
                    k = cnt - (1 if kind == "count-1" else 64)
                    assert np.array_equal(want[lo:lo + k], hb.syms[c][:k]) and np.all(want[lo + k:lo + cnt] == 0xA5)
