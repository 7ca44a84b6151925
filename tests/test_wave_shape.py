"""ryg_rans_amd/csrc/wave_shape.hpp: which instance of the wave-per-chunk kernels a request gets.  The library reports
`k_decode<word>` whatever K and OUT were, so no GPU test can see these choices -- a slip that sends a full-wave aligned request
to the element stores costs only speed.  The header is host code: tests/wave_shape_driver.cpp (g++, no HIP) prints its answers
over the whole domain, and they are compared here with a second statement of every rule, written from the rule in words."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(ROOT, "build", "wave_shape")

FORMATS = ("word", "byte", "byte-fused", "r64", "r64-search", "word-u16", "byte-adaptive", "word-adaptive", "alias")
CHUNKS = (4096, 5000, 8192, 16384, 32768)


@pytest.fixture(scope="module")
def rows():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "wave_shape_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ryg_rans_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "wave_shape_driver.cpp")], check=True)
    out = {"K": {}, "D": {}, "L": {}, "E": {}, "A": {}}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, *f = line.split()
        if kind == "K":
            out["K"][int(f[0])] = int(f[1])
        elif kind == "D":  # (format, n_ways, sym_bytes, aligned, ragged) -> (K, store mode, word64 kernel, instantiated)
            out["D"][(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]))] = (int(f[5]), f[6], int(f[7]), int(f[8]))
        elif kind == "L":  # (format, output address, chunk_syms) -> aligned
            out["L"][(f[0], int(f[1]), int(f[2]))] = int(f[3])
        elif kind == "E":  # flags -> MODE
            out["E"][int(f[0])] = int(f[1])
        else:              # (n_ways, chunk_syms, symbols aligned, n >= chunk_syms, ragged) -> (K, RR)
            out["A"][tuple(int(v) for v in f[:5])] = (int(f[5]), int(f[6]))
    assert len(out["K"]) == 514 and len(out["D"]) == len(FORMATS) * 514 * 8 and len(out["E"]) == 128
    assert len(out["A"]) == 514 * len(CHUNKS) * 8 and len(out["L"]) == len(FORMATS) * 8 * 4
    assert {k[0] for k in out["D"]} == set(FORMATS)
    return out


def minimal_k(n_ways):
    """The fewest states per lane, of 1, 2, 4, 8, that give 64 lanes at least n_ways states; None where there are none."""
    fits = [k for k in (1, 2, 4, 8) if 64 * k >= n_ways >= 1]
    return min(fits) if fits else None


def test_states_per_lane_is_minimal_and_invalid_only_outside_1_to_512(rows):
    for n in range(514):
        want = minimal_k(n)
        assert (want is None) == (n == 0 or n > 512)
        assert rows["K"][n] == (want or 0), n
    for (fmt, n, sb, al, rg), (K, out, w64, exists) in rows["D"].items():
        assert K == rows["K"][n], (fmt, n)
    for (n, chunk, al, whole, rg), (K, rr) in rows["A"].items():
        assert K == rows["K"][n], (n, chunk)


def test_fast_stores_only_for_full_waves_and_only_kernels_that_exist(rows):
    for key, (K, out, w64, exists) in rows["D"].items():
        n = key[1]
        if K == 0:
            assert (out, w64, exists) == ("slow", 0, 0), key
            continue
        assert exists == 1, key  # the launcher has an instance for every valid answer
        if out != "slow" or w64:
            assert n == 64 * K, key


def decode_rule(fmt, n, sym_bytes, aligned, ragged):
    """The decoder's rule in words: full waves may store transposed -- u8 symbols four rounds a dword, u16 symbols two --
    where such a kernel exists; a uniform call only onto an aligned output, a ragged batch always (its kernel decides per
    stream).  The search decoder has element stores only.  The word-u16 format stores u16 whatever the call says, in the
    paired form up to 128 lanes.  The other formats have the paired form up to 256 lanes in uniform calls; in ragged
    batches only the alias format has it, up to 128 lanes.  The 64-way u8 word decoder is a kernel of its own."""
    K = minimal_k(n)
    if K is None:
        return (0, "slow", 0)
    slow = (K, "slow", 0)
    if n != 64 * K or fmt == "r64-search" or not (ragged or aligned):
        return slow
    if fmt == "word-u16":
        return (K, "fast16", 0) if n <= 128 else slow
    if sym_bytes == 2:
        limit = (128 if fmt == "alias" else 0) if ragged else 256
        return (K, "fast16", 0) if n <= limit else slow
    return (K, "fast8", 1 if fmt == "word" and n == 64 else 0)


def test_decode_shape_equals_the_rule_in_words(rows):
    for (fmt, n, sb, al, rg), (K, out, w64, exists) in rows["D"].items():
        assert (K, out, w64) == decode_rule(fmt, n, sb, al, rg), (fmt, n, sb, al, rg)


def test_output_alignment_counts_the_u16_only_format_in_bytes(rows):
    for (fmt, addr, chunk), aligned in rows["L"].items():
        chunk_bytes = chunk * 2 if fmt == "word-u16" else chunk
        assert aligned == int(addr % 4 == 0 and chunk_bytes % 4 == 0), (fmt, addr, chunk)


def encode_rule(fused, slot_layout, claims, slot_offsets, ovf_ctl, sym_ranges, worda):
    """k_encode's MODE in words: a status array means fused placement (1).  Otherwise the slot layout with claim counters is
    a slot mode: 4 when per-stream slot offsets come with it (which needs the streams' symbol ranges and excludes sized
    slots), 3 when an overflow control block does (sized slots), else 2.  Everything else is MODE 0, which knows no
    per-stream slots.  The per-chunk word models have MODE 0 only."""
    if fused:
        return -1 if worda else 1
    if slot_layout and claims:
        if worda:
            return -1
        if slot_offsets:
            return 4 if sym_ranges and not ovf_ctl else -1
        return 3 if ovf_ctl else 2
    return -1 if slot_offsets else 0


def test_encode_mode_equals_the_rule_in_words(rows):
    for b, mode in rows["E"].items():
        flags = [bool(b >> i & 1) for i in range(7)]
        assert mode == encode_rule(*flags), flags


def test_adaptive_shape_equals_the_rule_in_words(rows):
    """Register-resident chunks (RR = chunk / 1024) for uniform 64-way calls over whole, 4-byte aligned chunks of 4096, 8192
    or 16384 symbols; the two-pass form (RR = 0) for everything else, ragged batches always."""
    for (n, chunk, al, whole, rg), (K, rr) in rows["A"].items():
        resident = not rg and n == 64 and al and whole and chunk in (4096, 8192, 16384)
        assert (K, rr) == (minimal_k(n) or 0, chunk // 1024 if resident else 0), (n, chunk, al, whole, rg)


# (format, n_ways, sym_bytes, aligned, ragged) -> (K, store mode, word64): one row per asymmetry of the rules, by hand
PINNED = [
    (("byte", 64, 1, 0, 0), (1, "slow", 0)),      # a uniform call's fast stores need the alignment ...
    (("byte", 64, 1, 0, 1), (1, "fast8", 0)),     # ... a ragged batch's do not
    (("byte", 256, 2, 1, 0), (4, "fast16", 0)),   # paired u16 stores up to K = 4 in uniform calls ...
    (("byte", 512, 2, 1, 0), (8, "slow", 0)),     # ... not at K = 8
    (("alias", 128, 2, 1, 1), (2, "fast16", 0)),  # ragged: up to K = 2 ...
    (("alias", 256, 2, 1, 1), (4, "slow", 0)),
    (("byte", 128, 2, 1, 1), (2, "slow", 0)),     # ... and for the alias and the word-u16 format only
    (("word-u16", 128, 1, 0, 1), (2, "fast16", 0)),
    (("word-u16", 256, 2, 1, 0), (4, "slow", 0)),  # word-u16: K <= 2 in uniform calls too, and never u8 stores
    (("word-u16", 64, 1, 1, 0), (1, "fast16", 0)),
    (("r64-search", 64, 1, 1, 0), (1, "slow", 0)),  # the search decoder: element stores only
    (("r64-search", 64, 1, 1, 1), (1, "slow", 0)),
    (("word", 64, 1, 1, 0), (1, "fast8", 1)),     # word, 64-way, u8, fast: the kernel of its own, in both forms
    (("word", 64, 1, 0, 1), (1, "fast8", 1)),
    (("word", 64, 1, 0, 0), (1, "slow", 0)),
    (("word", 128, 1, 1, 0), (2, "fast8", 0)),
    (("word", 65, 1, 1, 0), (2, "slow", 0)),
    (("byte-adaptive", 512, 1, 1, 1), (8, "fast8", 0)),
]


def test_pinned_rows(rows):
    for key, want in PINNED:
        assert rows["D"][key][:3] == want, key
    # word-u16 aligns on chunk_syms * 2: an odd multiple of 2 symbols is a whole number of dwords there, and nowhere else
    assert rows["L"][("word-u16", 4, 4098)] == 1 and rows["L"][("word", 4, 4098)] == 0 and rows["L"][("word-u16", 4, 4097)] == 0
    # encode: status | slot_layout 2 | claims 4 | slot_offsets 8 | ovf_ctl 16 | symbol ranges 32 | word-adaptive 64
    for flags, mode in ((0, 0), (1, 1), (2, 0), (6, 2), (6 | 16, 3), (6 | 8 | 32, 4), (6 | 8, -1), (6 | 8 | 16 | 32, -1), (8, -1),
                        (1 | 8, 1), (64, 0), (64 | 1, -1), (64 | 6, -1)):
        assert rows["E"][flags] == mode, flags
    assert rows["A"][(64, 16384, 1, 1, 0)] == (1, 16) and rows["A"][(64, 16384, 1, 1, 1)] == (1, 0)
    assert rows["A"][(64, 5000, 1, 1, 0)] == (1, 0) and rows["A"][(64, 32768, 1, 1, 0)] == (1, 0) and rows["A"][(128, 4096, 1, 1, 0)] == (2, 0)
