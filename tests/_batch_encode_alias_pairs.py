"""What tests/test_batch_encode_alias_pairs_host.py and tests/test_gpu_batch_encode_alias_pairs.py share: the reader of the
registry's THIRD list (ryg_rans_amd/csrc/kernel_names.hpp, RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE), the rows and the descriptor
of the ragged 2-way alias ENCODER with thirty-two streams per wave (k_encode_batch_alias_pairs,
RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS), a plain-integer model of the kernel's put step beside the reference's formula on the
oracle's tables, a plain-integer 2-way alias coder built on that model which counts the bytes every round emits, and the
reader of the launcher's LDS plan.

Nothing here needs a GPU."""
import functools
import os
import subprocess

import numpy as np

import ryg_rans_amd as R
from _batch_alias_pairs import WAVE_DECODER, WAVE_ENCODER
from _kernel_rows import CSRC, HERE, PAIR_SHAPES, ROOT, Family, registry
from _oracle import FMT_ALIAS

BATCH_ALIAS_PAIRS_ENCODE = "batch_alias_pairs_encode"
KERNEL = "k_encode_batch_alias_pairs"
OPT_BATCH_ENCODE_ALIAS_PAIRS = R.OPT_BATCH_ENCODE_ALIAS_PAIRS
# RANS_AMD_OPT_*, by value, behind the first enum's eleven and the second enum's one
OPTIONS_THIRD = ("BATCH_ENCODE_ALIAS_PAIRS",)


def _driver(name, include=CSRC):
    build = os.path.join(ROOT, "build", "kernel_names")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", include, "-o", exe, os.path.join(HERE, name + ".cpp")], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


@functools.lru_cache(maxsize=None)
def third_list():
    """[(family, name)]: every entry of the third list, as tests/kernel_names_alias_pairs_encode_driver.cpp prints them (the
    driver fails on a name or a family of the first two lists, on an id that does not follow the second list's, and on an id
    that does not lead back to its row)."""
    return [tuple(ln.split("\t")) for ln in _driver("kernel_names_alias_pairs_encode_driver")]


def third_list_names(family):
    return {name for f, name in third_list() if f == family}


@functools.lru_cache(maxsize=None)
def lds_plan():
    """{scale_bits: (table_bytes, waves, lds_bytes, blocks_per_cu)} for scale_bits 0..17: pairs_plan.hpp's enc_alias_pairs_plan,
    as tests/enc_alias_pairs_plan_driver.cpp prints it."""
    return {int(f[0]): tuple(int(v) for v in f[1:]) for f in (ln.split("\t") for ln in _driver("enc_alias_pairs_plan_driver"))}


# ---- thirty-two 2-way alias streams per wave: encoder (tests/test_gpu_batch_encode_alias_pairs.py)
def _enc_alias_pair_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_ALIAS, "sb": sb, "K": K, "ways": 2, "decode": WAVE_DECODER, "encode": KERNEL}


ENC_ALIAS_PAIR_ROWS = [
    _enc_alias_pair_row("alias-2-encode-pairs", 16, 256),        # the reference's (main_alias.cpp: prob_bits 16): a block of 13 waves
    _enc_alias_pair_row("alias-2-encode-pairs-14bit", 14, 256),  # two blocks of 16 waves per CU
    _enc_alias_pair_row("alias-2-encode-pairs-12bit", 12, 256),
    _enc_alias_pair_row("alias-2-encode-pairs-8bit", 8, 256),    # every frequency 1: q = x, rem = 0
    _enc_alias_pair_row("alias-2-encode-pairs-64sym-10bit", 10, 64),  # byte values 64..255 have no record
]
EAROW = {r["id"]: r for r in ENC_ALIAS_PAIR_ROWS}
EAMAIN, EA14, EA8, EA64 = (EAROW["alias-2-encode-pairs"], EAROW["alias-2-encode-pairs-14bit"], EAROW["alias-2-encode-pairs-8bit"],
                           EAROW["alias-2-encode-pairs-64sym-10bit"])
ENC_ALIAS_PAIR_RATE_ROW = {16: EAMAIN, 14: EA14}  # the rows of _batch.rate_batch / rate_wave, by scale_bits
ENC_ALIAS_PAIRS = Family(OPT_BATCH_ENCODE_ALIAS_PAIRS, "encode", FMT_ALIAS, 2, 32, ENC_ALIAS_PAIR_ROWS, EAMAIN, WAVE_ENCODER,
                         BATCH_ALIAS_PAIRS_ENCODE, PAIR_SHAPES, ("FMT_ALIAS", 16, "OPT_BATCH_ENCODE_ALIAS_PAIRS"))

# shapes that keep the wave encoder with the option on (beside tests/_kernel_rows.py's ROW)
ALIAS_2_WAVE = dict(EAMAIN, id="alias-2", encode=WAVE_ENCODER)
ALIAS_U16_2_WAVE = {"id": "alias-u16-2", "fmt": FMT_ALIAS, "sb": 16, "K": 1024, "ways": 2, "decode": WAVE_DECODER, "encode": WAVE_ENCODER}


def ad_hoc_row(sb, K=256):
    """A row of the family's shape at any scale_bits (the every-scale_bits case builds its models ad hoc)."""
    return _enc_alias_pair_row("alias-2-encode-pairs-%dbit-%dsym" % (sb, K), sb, K)


def check_third_list_rows(d, rows=None):
    """tests/_kernel_rows.py check_family_rows for the family of the third list: the family's names are the kernels of the rows
    on the family's side, in both directions; the rows are the family's shapes and name the wave decoder; the name is in no
    family of the first list."""
    rows = d.rows if rows is None else rows
    names, kernel = third_list_names(d.family), d.main[d.side]
    got = {r[d.side] for r in rows}
    assert names == got, ("kernels no row expects", sorted(names - got), "names no launcher reports", sorted(got - names))
    assert kernel in names
    assert all(r["ways"] == d.ways and r["fmt"] == d.fmt and r["decode"] == WAVE_DECODER for r in rows)
    assert sorted((r["sb"], r["K"]) for r in rows) == d.shapes
    assert all(kernel not in ns for ns in registry().values()) and d.family not in registry()


# ---- the kernel's put step as plain integers --------------------------------------------------------------------------------
M32 = 0xffffffff


def device_records(om, sb):
    """The 256 records k_encode_batch_alias_pairs builds in its prologue (encode_groups.hip encode_batch_pairs<ALIAS>) from the
    ORACLE's frequencies and cumulative frequencies -- {rcp, (2^24 - freq) | rshift << 24, start | inc << 16, x_max}, the
    no-record form {0, ~0, 0, ~0} for a frequency of 0 and for byte values at and past nsyms -- and remap16 -> (uint64[4][256],
    uint64[1 << sb])."""
    ns = om.nsyms
    freqs, cum = om.table("freqs", ns), om.table("cum", ns + 1)
    rec = np.zeros((4, 256), dtype=np.uint64)
    rec[1, :] = rec[3, :] = M32
    for s in range(ns):
        f, start = int(freqs[s]), int(cum[s])
        if f == 0:
            continue
        assert f <= 0xffff and start <= 0xffff
        if f == 1:
            rec[:, s] = (M32, 0xffffff, start | 0x10000, 1 << (31 - sb))
        else:
            sh = (f - 1).bit_length()  # 32 - clz(freq - 1)
            rec[:, s] = ((((1 << (sh + 31)) + f - 1) // f) & M32, (0x1000000 - f) | ((sh - 1) << 24), start, f << (31 - sb))
    remap = om.table("alias_remap", 1 << sb).astype(np.uint64)
    assert int(remap.max()) < (1 << sb)
    return rec, remap


def kernel_put(tables, sb, sym, x):
    """The put of RANS_AE_ROUND (encode_groups.hip), the instructions in order with 32-bit wrapping, on arrays of byte values
    and of states that have been renormalised -> (next states, the gather's index into remap16).  numpy raises on an index
    outside remap16."""
    rec, remap = tables
    sym = np.asarray(sym, dtype=np.int64)
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    v56, v57, v58 = rec[0][sym], rec[1][sym], rec[2][sym]
    t0 = (x * v56) >> np.uint64(32)                                              # v_mul_hi_u32
    t0 = t0 >> ((v57 >> np.uint64(24)) & np.uint64(31))                          # v_lshrrev (SDWA: byte 3; the shifter takes 5 bits)
    t0 = (t0 + (v58 >> np.uint64(16))) & np.uint64(M32)                          # v_add (SDWA: word 1)
    t2 = ((t0 & np.uint64(0xffffff)) * (v57 & np.uint64(0xffffff)) + x) & np.uint64(M32)  # v_mad_u32_u24
    t2 = ((t2 + v58) << np.uint64(1)) & np.uint64(M32)                           # v_add_lshl_u32
    t2 = t2 & np.uint64(((1 << sb) - 1) << 1)                                    # v_and  mask2
    g = remap[(t2 >> np.uint64(1)).astype(np.int64)]                             # ds_read_u16 offset:4096
    return ((t0 << np.uint64(sb)) + g) & np.uint64(M32), t2 >> np.uint64(1)      # v_lshl_add_u32


def reference_put(om, sb, sym, x):
    """RansEncPutAlias behind its renormalisation (main_alias.cpp:249) on the oracle's tables, in 32 bits as RansState is."""
    ns = om.nsyms
    freqs, cum = om.table("freqs", ns).astype(np.uint64), om.table("cum", ns + 1).astype(np.uint64)
    remap = om.table("alias_remap", 1 << sb).astype(np.uint64)
    sym = np.asarray(sym, dtype=np.int64)
    x = np.asarray(x, dtype=np.uint64)
    f = freqs[sym]
    return (((x // f) << np.uint64(sb)) + remap[((x % f) + cum[sym]).astype(np.int64)]) & np.uint64(M32)


def encode_rounds(tables, sb, syms):
    """A 2-way alias stream coded with the kernel's records: the byte format's renormalisation against the record's x_max (a
    state's own two compares), kernel_put's arithmetic on plain ints, main_alias.cpp:306-330's order (an odd count's last
    symbol is state 0's alone and comes first; inside a round state 1 puts first; RansEncFlush(rans1), then rans0) -> (the
    stream, bytes emitted per round -- round r holds symbols 2 r and 2 r + 1; the coder runs from the last round to the first)."""
    rec, remap = tables
    r0, r1, r2, r3 = ([int(v) for v in rec[k]] for k in range(4))
    rm = [int(v) for v in remap]
    mask2 = ((1 << sb) - 1) << 1
    n = len(syms)
    x = [1 << 23, 1 << 23]
    emitted = bytearray()
    per_round = np.zeros((n + 1) // 2, dtype=np.int64)
    for k in range(n - 1, -1, -1):  # (an odd n: k = n - 1 is even, state 0 alone; then state 1, state 0, ...)
        s, i = int(syms[k]), k & 1
        v = x[i]
        nb = int(v >= r3[s]) + int((v >> 8) >= r3[s])
        for _ in range(nb):
            emitted.append(v & 0xff)
            v >>= 8
        per_round[k >> 1] += nb
        q = (((v * r0[s]) >> 32) >> ((r1[s] >> 24) & 31)) + (r2[s] >> 16)
        t = ((q & 0xffffff) * (r1[s] & 0xffffff) + v) & M32
        x[i] = ((q << sb) + rm[((((t + r2[s]) << 1) & M32) & mask2) >> 1]) & M32
    head = np.array([x[0], x[1]], dtype="<u4").view(np.uint8)
    return np.concatenate((head, np.frombuffer(bytes(emitted[::-1]), dtype=np.uint8))), per_round
