"""What tests/test_batch_alias_pairs_host.py and tests/test_gpu_batch_alias_pairs.py share: the reader of the registry's SECOND
list (ryg_rans_amd/csrc/kernel_names.hpp, RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS), the rows and the descriptor of the ragged 2-way
alias decoder with thirty-two streams per wave (k_decode_batch_alias_pairs, RANS_AMD_OPT_BATCH_ALIAS_PAIRS), a plain-integer
model of the kernel's symbol step over the oracle's tables, and a plain-integer decoder of a 2-way alias stream that counts
the bytes every round takes.

Nothing here needs a GPU."""
import functools
import os
import subprocess

import numpy as np

import ryg_rans_amd as R
from _kernel_rows import CSRC, HERE, PAIR_SHAPES, ROOT, Family, registry
from _oracle import FMT_ALIAS

BATCH_ALIAS_PAIRS_DECODE = "batch_alias_pairs_decode"
KERNEL = "k_decode_batch_alias_pairs"
WAVE_DECODER, WAVE_ENCODER = "k_decode_batch<alias>", "k_encode_batch<alias, LDS remap>"
OPT_BATCH_ALIAS_PAIRS = R.OPT_BATCH_ALIAS_PAIRS
# RANS_AMD_OPT_*, by value: the first enum's eleven (tests/_kernel_rows.py's OPTIONS) and the second enum's behind them
OPTIONS_MORE = ("BATCH_ALIAS_PAIRS",)


@functools.lru_cache(maxsize=None)
def second_list():
    """[(family, name)]: every entry of the second list, as tests/kernel_names_alias_pairs_driver.cpp prints them (the driver
    fails on a name or a family of the first list, and on an id that does not follow the first list's)."""
    build = os.path.join(ROOT, "build", "kernel_names")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "kernel_names_alias_pairs_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "kernel_names_alias_pairs_driver.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return [tuple(ln.split("\t")) for ln in out.splitlines()]


def second_list_names(family):
    return {name for f, name in second_list() if f == family}


# ---- thirty-two 2-way alias streams per wave: decoder (tests/test_gpu_batch_alias_pairs.py)
def _alias_pair_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_ALIAS, "sb": sb, "K": K, "ways": 2, "decode": KERNEL, "encode": WAVE_ENCODER}


ALIAS_PAIR_ROWS = [
    _alias_pair_row("alias-2-pairs", 16, 256),             # the reference's (main_alias.cpp: prob_bits 16): 256 slots per bucket
    _alias_pair_row("alias-2-pairs-14bit", 14, 256),
    _alias_pair_row("alias-2-pairs-12bit", 12, 256),       # 16 slots per bucket
    _alias_pair_row("alias-2-pairs-8bit", 8, 256),         # one slot per bucket, bucket shift 0, every frequency 1
    _alias_pair_row("alias-2-pairs-64sym-10bit", 10, 64),
]
AROW = {r["id"]: r for r in ALIAS_PAIR_ROWS}
AMAIN, A8 = AROW["alias-2-pairs"], AROW["alias-2-pairs-8bit"]
ALIAS_PAIR_RATE_ROW = {16: AMAIN, 14: AROW["alias-2-pairs-14bit"]}  # the rows of _batch.rate_batch / rate_wave, by scale_bits
ALIAS_PAIRS = Family(OPT_BATCH_ALIAS_PAIRS, "decode", FMT_ALIAS, 2, 32, ALIAS_PAIR_ROWS, AMAIN, WAVE_DECODER, BATCH_ALIAS_PAIRS_DECODE,
                     PAIR_SHAPES, ("FMT_ALIAS", 16, "OPT_BATCH_ALIAS_PAIRS"))

# shapes that keep the wave kernels with the option on (beside tests/_kernel_rows.py's ROW): fewer than 32 2-way alias streams
# run the main row's shape; u16 symbols are another shape
ALIAS_2_WAVE = dict(AMAIN, id="alias-2", decode=WAVE_DECODER)
ALIAS_U16_2_WAVE = {"id": "alias-u16-2", "fmt": FMT_ALIAS, "sb": 16, "K": 1024, "ways": 2, "decode": WAVE_DECODER, "encode": WAVE_ENCODER}


def check_second_list_rows(d, rows=None):
    """tests/_kernel_rows.py check_family_rows for a family of the second list (registry() knows the first list's families
    alone): the family's names are the kernels of the rows on the family's side, in both directions; the rows are the
    family's shapes and name the wave encoder; the name is in no family of the first list."""
    rows = d.rows if rows is None else rows
    names, kernel = second_list_names(d.family), d.main[d.side]
    got = {r[d.side] for r in rows}
    assert names == got, ("kernels no row expects", sorted(names - got), "names no launcher reports", sorted(got - names))
    assert kernel in names
    assert all(r["ways"] == d.ways and r["fmt"] == d.fmt and r["encode"] == WAVE_ENCODER for r in rows)
    assert sorted((r["sb"], r["K"]) for r in rows) == d.shapes
    assert all(kernel not in ns for ns in registry().values()) and d.family not in registry()


class AliasOracle:
    """The oracle with alias tables in every model it makes: tests/_batch.py's PoolBatch asks for a model without them."""

    def __init__(self, oracle):
        self._oracle = oracle

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def model(self, norm_freqs, scale_bits, with_alias=True):
        return self._oracle.model(norm_freqs, scale_bits, True)


# ---- the kernel's symbol step as plain integers -----------------------------------------------------------------------------
def device_tables(om):
    """The FMT_ALIAS tables the library builds (ryg_rans_amd/csrc/model.cpp) from the ORACLE's alias tables: the dividers and,
    per half bucket, {freq | sym << 16, adjust} -> (divider, lo, adjust), uint64 arrays."""
    ns = om.nsyms
    divider = om.table("divider", ns).astype(np.uint64)
    freq, sym = om.table("slot_freqs", 2 * ns).astype(np.uint64), om.table("sym_id", 2 * ns).astype(np.uint64)
    assert int(freq.max()) <= 0xffff and int(sym.max()) < ns <= 256
    return divider, freq | (sym << np.uint64(16)), om.table("slot_adjust", 2 * ns).astype(np.uint64)


def kernel_step(tables, sb, log2n, x):
    """k_decode_batch_alias_pairs' symbol step (decode_groups.hip RANS_A_ROUND, the instructions in order, 32-bit wrapping) on
    an array of states -> (symbols, next states).  Both half records of the bucket are read at once; the divider selects."""
    divider, lo, adjust = tables
    m32 = np.uint64(0xffffffff)
    x = np.asarray(x, dtype=np.uint64) & m32
    t0 = x & np.uint64((1 << sb) - 1)                          # v_and        xm
    t1 = t0 >> np.uint64(sb - log2n)                           # v_lshrrev    bucket
    t3 = divider[t1]                                           # v_lshl_add, ds_read_b32
    v56, v57 = lo[2 * t1], adjust[2 * t1]                      # v_lshlrev, ds_read_b128: the donor's half ...
    v58, v59 = lo[2 * t1 + 1], adjust[2 * t1 + 1]              # ... and the bucket's own symbol's
    t2 = x >> np.uint64(sb)                                    # v_lshrrev    q
    t3 = (t0 - t3) & m32                                       # v_sub        xm - divider, wrapping
    t3 = np.where(t3 >> np.uint64(31), m32, np.uint64(0))      # v_ashrrev    31: the sign as a mask
    v56 = (t3 & v58) | (~t3 & m32 & v56)                       # v_bfi
    v57 = (t3 & v59) | (~t3 & m32 & v57)                       # v_bfi
    nx = (v56 & np.uint64(0xffff)) * (t2 & np.uint64(0xffffff))  # v_mul_u32_u24, src0 the low word (sdwa)
    t0 = (t0 - v57) & m32                                      # v_sub        xm - adjust
    nx = (nx + t0) & m32                                       # v_add
    return (v56 >> np.uint64(16)) & np.uint64(0xff), nx        # v_perm: byte 2 of the record


def reference_step(om, sb, log2n, x):
    """RansDecGetAlias (main_alias.cpp:252-267) on the oracle's tables, in 32 bits as RansState is -> (symbols, next states)."""
    ns = om.nsyms
    divider = om.table("divider", ns).astype(np.uint64)
    freq, sym = om.table("slot_freqs", 2 * ns).astype(np.uint64), om.table("sym_id", 2 * ns).astype(np.uint64)
    adjust = om.table("slot_adjust", 2 * ns).astype(np.uint64)
    m32 = np.uint64(0xffffffff)
    x = np.asarray(x, dtype=np.uint64) & m32
    xm = x & np.uint64((1 << sb) - 1)
    bucket = xm >> np.uint64(sb - log2n)
    bucket2 = bucket * np.uint64(2) + (xm < divider[bucket]).astype(np.uint64)
    return sym[bucket2], (freq[bucket2] * (x >> np.uint64(sb)) + xm - adjust[bucket2]) & m32


def decode_rounds(om, sb, stream, n):
    """A 2-way alias stream of n symbols decoded with kernel_step and the byte format's renormalisation (rans_byte.h:307-318;
    state 0's bytes first) -> (symbols, bytes per round); the states must end at L and the cursor at the stream's end."""
    tables = device_tables(om)
    log2n = om.nsyms.bit_length() - 1
    s = np.ascontiguousarray(stream, dtype=np.uint8)
    x = [int(v) for v in s[:8].view(np.uint32)]
    cur, out, per_round = 8, np.zeros(n, dtype=np.uint8), np.zeros((n + 1) // 2, dtype=np.int64)
    for k in range(n):
        i = k & 1
        sy, nx = kernel_step(tables, sb, log2n, np.array([x[i]], dtype=np.uint64))
        out[k], v = int(sy[0]), int(nx[0])
        while v < (1 << 23):
            v = (v << 8) | int(s[cur])
            cur += 1
            per_round[k >> 1] += 1
        x[i] = v
    assert x == [1 << 23, 1 << 23] and cur == s.size, (x, cur, s.size)
    return out, per_round
