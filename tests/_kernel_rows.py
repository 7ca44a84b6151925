"""The rows of expectations of every kernel a launcher can report, and the one reader of the library's registry.

The library reports the kernel that served a call as an entry of one table, ryg_rans_amd/csrc/kernel_names.hpp: identifier,
name, family.  registry() compiles tests/kernel_names_driver.cpp (g++, no HIP) and returns {family: names}; each family's
`test_no_*_without_a_row` holds its names to its table below, in both directions.  The tables name, per shape, the kernels
the library must report for it; the GPU files run the rows.  Option numbers are ryg_rans_amd.OPT_*.
"""
import collections
import functools
import os
import re
import subprocess

import ryg_rans_amd as R
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ryg_rans_amd", "csrc")

# the registry's families
UNIFORM, BATCH, BATCH_MODELS = "uniform", "batch", "batch_models"
BATCH_WORD_GROUPS_DECODE, BATCH_WORD_GROUPS_ENCODE = "batch_word_groups_decode", "batch_word_groups_encode"
BATCH_BYTE_PAIRS_DECODE, BATCH_BYTE_PAIRS_ENCODE = "batch_byte_pairs_decode", "batch_byte_pairs_encode"
BATCH_R64_LANES_DECODE, BATCH_R64_LANES_ENCODE = "batch_r64_lanes_decode", "batch_r64_lanes_encode"
FAMILIES = (UNIFORM, BATCH, BATCH_MODELS, BATCH_WORD_GROUPS_DECODE, BATCH_WORD_GROUPS_ENCODE, BATCH_BYTE_PAIRS_DECODE,
            BATCH_BYTE_PAIRS_ENCODE, BATCH_R64_LANES_DECODE, BATCH_R64_LANES_ENCODE)


@functools.lru_cache(maxsize=None)
def registry():
    """{family: set of names}: every entry of kernel_names.hpp, as the driver prints them.  No name occurs twice, in one
    family or in two -- the pairwise disjointness the families' tests used to assert on their scans of the sources."""
    build = os.path.join(ROOT, "build", "kernel_names")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "kernel_names_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(HERE, "kernel_names_driver.cpp")],
                   check=True)
    lines = [ln.split("\t") for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    names = [name for _, name in lines]
    assert len(set(names)) == len(names), ("a name occurs twice in the registry", sorted(n for n in set(names) if names.count(n) > 1))
    out = {f: set() for f in FAMILIES}
    for family, name in lines:
        out[family].add(name)  # (a family this module does not know: KeyError)
    return out


# context options (the numbers are the ABI's, tests/test_abi.py)
LANE_FUSED, FUSED, DUAL = R.OPT_LANE_FUSED_PLACEMENT, R.OPT_FUSED_PLACEMENT, R.OPT_DUAL_DECODE
OPT_BATCH_GROUPS, OPT_BATCH_ENCODE_GROUPS = R.OPT_BATCH_GROUPS, R.OPT_BATCH_ENCODE_GROUPS
OPT_BATCH_PAIRS, OPT_BATCH_ENCODE_PAIRS = R.OPT_BATCH_PAIRS, R.OPT_BATCH_ENCODE_PAIRS
OPT_BATCH_LANES, OPT_BATCH_ENCODE_LANES = R.OPT_BATCH_LANES, R.OPT_BATCH_ENCODE_LANES
OPTIONS = ("LANE_KERNELS", "LANE_FUSED_PLACEMENT", "FUSED_PLACEMENT", "DUAL_DECODE", "ENC_SCRATCH_RING", "BATCH_GROUPS",
           "BATCH_ENCODE_GROUPS", "BATCH_PAIRS", "BATCH_ENCODE_PAIRS", "BATCH_LANES", "BATCH_ENCODE_LANES")  # RANS_AMD_OPT_*, by value


def check_option_constant(name, value):
    """RANS_AMD_OPT_<name> is `value` in the header and in the package, every option of OPTIONS is where it was and the
    header's enum holds no other, the version has not moved (additions only), and a NULL context is refused before the option is
    looked at (the values need a context: the family's GPU file)."""
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    assert OPTIONS[value] == name
    enum = re.search(r"enum rans_amd_option \{(.*?)\n\};", header, re.S).group(1)
    assert len(re.findall(r"^    RANS_AMD_OPT_\w+\s*=\s*\d+", enum, re.M)) == len(OPTIONS) == 11
    for v, n in enumerate(OPTIONS):
        m = re.search(r"RANS_AMD_OPT_%s\s*=\s*(\d+)" % n, header)
        assert m and int(m.group(1)) == v, n
        assert getattr(R, "OPT_" + n) == v, n
    assert re.search(r"#define\s+RANS_AMD_VERSION\s+600\b", header)
    assert R.lib().rans_amd_ctx_set_option(None, value, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()


# ---- uniform chunks (tests/test_gpu_kernel_matrix.py runs the rows) ---------------------------------------------------------
DEFAULT_ROUNDS_SYMBOLS = 1 << 28
REGIMES = ("U", "H", "R")


def _row(rid, fmt, sb, K, ways, chunk, unit, decode, encode, slots, sized, opts=(), regimes=REGIMES, n=None, kind="static"):
    return {"id": rid, "fmt": fmt, "sb": sb, "K": K, "ways": ways, "chunk": chunk, "unit": unit, "decode": decode, "encode": encode,
            "slots": slots, "sized": sized, "opts": tuple(opts), "regimes": tuple(regimes), "n": n, "kind": kind}


def _by(U, H, R=None):
    """An expectation that depends on the regime (the lane encoders take their staged form from six batches per CU on)."""
    return {"U": U, "H": H, "R": H if R is None else R}


W, B = "k_encode<word>", "k_encode<byte>"
WG, ST, L16, RX = "k_encode_word_groups", "k_encode_lanes_staged", "k_encode_lanes16", "k_encode_lanes_r64x2"

# One table: the shape (format, scale_bits, alphabet -- u16 symbols above 256 --, interleave, chunk size, work unit in
# chunks, context options) and the kernels the library must report for it: the decoder, and the coding kernel + placement
# flag of the compact layout, the slot layout and sized slots.
KERNEL_ROWS = [
    # ---- wave per chunk (decode_wave.hip / encode_wave.hip): one chunk per unit
    _row("word-64", FMT_WORD, 12, 256, 64, 4096, 1, "k_decode_word64", (W, 1), (W, 2), (W, 2)),
    _row("word-128", FMT_WORD, 12, 256, 128, 8192, 1, "k_decode<word>", (W, 1), (W, 2), (W, 2)),
    _row("word-32", FMT_WORD, 12, 256, 32, 4096, 1, "k_decode<word>", (W, 1), (W, 2), (W, 2)),
    _row("word-64-unfused", FMT_WORD, 12, 256, 64, 4096, 1, "k_decode_word64", (W, 0), (W, 2), (W, 2), opts=((FUSED, 0),)),
    _row("word-u16-64", FMT_WORD, 12, 1024, 64, 4096, 1, "k_decode<word, u16 symbols>", (W, 1), (W, 2), (W, 2)),
    _row("byte-64-14bit", FMT_BYTE, 14, 256, 64, 4096, 1, "k_decode<byte>", (B, 1), (B, 2), (B, 2)),
    _row("byte-64-12bit", FMT_BYTE, 12, 256, 64, 4096, 1, "k_decode<byte, slot records>", (B, 1), (B, 2), (B, 2)),
    _row("r64-64", FMT_R64, 14, 256, 64, 4096, 1, "k_decode<r64>", ("k_encode<r64>", 1), ("k_encode<r64>", 2), ("k_encode<r64>", 2)),
    _row("r64-search-64", FMT_R64, 20, 256, 64, 4096, 1, "k_decode<r64 search>", ("k_encode<r64 full-width>", 1),
         ("k_encode<r64 full-width>", 2), ("k_encode<r64 full-width>", 2)),
    _row("alias256-64", FMT_ALIAS, 16, 256, 64, 4096, 1, "k_decode<alias>", ("k_encode<alias, LDS remap>", 1),
         ("k_encode<alias, LDS remap>", 2), ("k_encode<alias, LDS remap>", 2)),
    # ---- two chunks per wave (decode_dual.hip): u16 symbols (config 4's model), and u8 symbols where the option asks for it
    _row("alias4096-64", FMT_ALIAS, 16, 4096, 64, 4096, 1, "k_decode_dual<alias>", ("k_encode<alias, LDS remap>", 1),
         ("k_encode<alias, LDS remap>", 2), ("k_encode<alias, LDS remap>", 2)),
    _row("alias256-64-dual", FMT_ALIAS, 16, 256, 64, 4096, 1, "k_decode_dual<alias>", ("k_encode<alias, LDS remap>", 1),
         ("k_encode<alias, LDS remap>", 2), ("k_encode<alias, LDS remap>", 2), opts=((DUAL, 2),)),
    # ---- eight chunks per wave (decode_groups.hip / encode_groups.hip).  The compact layout of fewer than 64 chunks goes to the
    #      wave encoder and its fused placement; without it (OPT_FUSED_PLACEMENT = 0) 8..63 chunks run the group encoder
    #      WITHOUT claim counters (second finding): regime U of the second row is that shape (12 chunks)
    _row("word-8", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", _by((W, 1), (WG, 0)), (WG, 2), (WG, 2)),
    _row("word-8-unfused", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", (WG, 0), (WG, 2), (WG, 2), opts=((FUSED, 0),)),
    # ---- 32 chunks per wave (k_decode_byte_pairs); its encoders are the lane encoders, staged from six batches per CU on
    _row("byte-2", FMT_BYTE, 14, 256, 2, 256, 32, "k_decode_byte_pairs", _by((B, 1), (ST, 0)), _by((B, 2), (ST, 2)), _by((B, 2), (ST, 2))),
    _row("byte-2-lane-fused", FMT_BYTE, 14, 256, 2, 256, 32, "k_decode_byte_pairs", _by((B, 1), (ST, 1)), _by((B, 2), (ST, 2)),
         _by((B, 2), (ST, 2)), opts=((LANE_FUSED, 1),)),
    # ---- one chunk per lane (decode_lanes.hip, encode_lanes.hip): 64 chunks per unit
    _row("r64-2-packed", FMT_R64, 14, 256, 2, 128, 64, "k_decode_lanes_r64x2<packed slots>", _by((L16, 0), (RX, 0)),
         _by((L16, 2), (RX, 2)), _by(("k_encode<r64>", 2), (RX, 2))),
    _row("r64-2-16bit", FMT_R64, 16, 256, 2, 128, 64, "k_decode_lanes_r64x2", _by((L16, 0), (RX, 0)), _by((L16, 2), (RX, 2)),
         _by(("k_encode<r64>", 2), (RX, 2))),
    _row("r64-2-lane-fused", FMT_R64, 14, 256, 2, 128, 64, "k_decode_lanes_r64x2<packed slots>", _by((L16, 0), (RX, 1)),
         _by((L16, 2), (RX, 2)), _by(("k_encode<r64>", 2), (RX, 2)), opts=((LANE_FUSED, 1),)),
    _row("word-4", FMT_WORD, 12, 256, 4, 128, 64, "k_decode_lanes_staged", _by((L16, 0), (ST, 0)), _by((L16, 2), (ST, 2)),
         _by((W, 2), (ST, 2))),
    _row("byte-1", FMT_BYTE, 14, 256, 1, 128, 64, "k_decode_lanes_staged", _by((L16, 0), (ST, 0)), _by((L16, 2), (ST, 2)),
         _by((B, 2), (ST, 2))),
    _row("alias256-8", FMT_ALIAS, 16, 256, 8, 128, 64, "k_decode_lanes_staged", _by((L16, 0), (ST, 0)), _by((L16, 2), (ST, 2)),
         _by(("k_encode<alias, LDS remap>", 2), (ST, 2))),
    # (chunks that are no multiple of 4 symbols: not the group kernels'; no multiple of 16: the per-lane encoder at every size,
    #  and sized slots, which it cannot take, go to the wave encoder)
    _row("word-8-chunk-130", FMT_WORD, 12, 256, 8, 130, 64, "k_decode_lanes_staged", (L16, 0), (L16, 2), (W, 2)),
    # (the per-lane decoder is the fallback for chunks of 512 Ki symbols and more: a wave holds 64 of them, 32 Mi symbols --
    #  "half the resident waves" would be 2^36 symbols, so this row has regime U alone)
    _row("byte-2-huge-chunks", FMT_BYTE, 14, 256, 2, (1 << 19) + 2, 64, "k_decode_lanes", (L16, 0), (L16, 2), (B, 2), regimes=("U",)),
    # ---- one model per chunk (decode_wave.hip, encode_wave.hip, encode_adaptive.hip): Oracle.compare_container_adaptive
    _row("byte-64-per-chunk-models", FMT_BYTE, 12, 256, 64, 4096, 1, "k_decode<byte, per-chunk models>", "k_encode<byte, per-chunk models>",
         None, "k_encode_adaptive<byte>", kind="adaptive"),
    _row("word-64-per-chunk-models", FMT_WORD, 12, 256, 64, 4096, 1, "k_decode<word, per-chunk models>", "k_encode<word, per-chunk models>",
         None, "k_encode_adaptive<word>", kind="adaptive"),
    # ---- either side of every applicability threshold of the group kernels (fixed sizes; chunks this small have no sized
    #      slot below the worst case, so the sized steps are left out).  Word groups: chunks of 32 symbols and more ...
    _row("word-8-chunk-28", FMT_WORD, 12, 256, 8, 28, 8, "k_decode_lanes_staged", (L16, 0), (L16, 2), None, regimes=("F",), n=28 * 1000 + 9),
    _row("word-8-chunk-32", FMT_WORD, 12, 256, 8, 32, 8, "k_decode_word_groups", (WG, 0), (WG, 2), None, regimes=("F",), n=32 * 1000 + 9),
    _row("word-8-chunk-36", FMT_WORD, 12, 256, 8, 36, 8, "k_decode_word_groups", (WG, 0), (WG, 2), None, regimes=("F",), n=36 * 1000 + 9),
    # ... and eight full chunks and more (with and without the fused placement of the wave encoder that takes fewer than 64)
    _row("word-8-7-chunks", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode<word>", (W, 1), (W, 2), None, regimes=("F",), n=7 * 1024),
    _row("word-8-8-chunks", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", (W, 1), (WG, 2), None, regimes=("F",), n=8 * 1024),
    _row("word-8-9-chunks", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", (W, 1), (WG, 2), None, regimes=("F",), n=9 * 1024),
    _row("word-8-7-chunks-unfused", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode<word>", (W, 0), (W, 2), None, opts=((FUSED, 0),),
         regimes=("F",), n=7 * 1024),
    _row("word-8-8-chunks-unfused", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", (WG, 0), (WG, 2), None, opts=((FUSED, 0),),
         regimes=("F",), n=8 * 1024),
    _row("word-8-63-chunks-unfused", FMT_WORD, 12, 256, 8, 1024, 8, "k_decode_word_groups", (WG, 0), (WG, 2), None, opts=((FUSED, 0),),
         regimes=("F",), n=63 * 1024),
    # byte pairs: chunks of 64 symbols and more ...
    _row("byte-2-chunk-60", FMT_BYTE, 14, 256, 2, 60, 32, "k_decode_lanes_staged", (L16, 0), (L16, 2), None, regimes=("F",), n=60 * 1000 + 9),
    _row("byte-2-chunk-64", FMT_BYTE, 14, 256, 2, 64, 32, "k_decode_byte_pairs", (L16, 0), (L16, 2), None, regimes=("F",), n=64 * 1000 + 9),
    _row("byte-2-chunk-68", FMT_BYTE, 14, 256, 2, 68, 32, "k_decode_byte_pairs", (L16, 0), (L16, 2), None, regimes=("F",), n=68 * 1000 + 9),
    # ... and 32 full chunks and more
    _row("byte-2-31-chunks", FMT_BYTE, 14, 256, 2, 256, 32, "k_decode<byte>", (B, 1), (B, 2), None, regimes=("F",), n=31 * 256),
    _row("byte-2-32-chunks", FMT_BYTE, 14, 256, 2, 256, 32, "k_decode_byte_pairs", (B, 1), (B, 2), None, regimes=("F",), n=32 * 256),
    _row("byte-2-33-chunks", FMT_BYTE, 14, 256, 2, 256, 32, "k_decode_byte_pairs", (B, 1), (B, 2), None, regimes=("F",), n=33 * 256),
]


def pick(value, regime):
    return value.get(regime) if isinstance(value, dict) else value


def row_kernel_names(rows=None):
    """Every kernel name KERNEL_ROWS expects, in any regime."""
    names = set()
    for r in KERNEL_ROWS if rows is None else rows:
        for key in ("decode", "encode", "slots", "sized"):
            v = r[key]
            for w in (v.values() if isinstance(v, dict) else (v,)):
                if w is not None:
                    names.add(w if isinstance(w, str) else w[0])
    return names


def regime_symbols(row, regime, resident):
    """-> (n, whole units before the partial one)"""
    chunk, unit = row["chunk"], row["unit"]
    ragged = chunk // 3 + 1
    if regime == "F":
        return row["n"], row["n"] // (chunk * unit)
    if regime == "U":
        units = 1
    elif regime == "H":
        units = resident // 2
    else:
        per_unit = chunk * unit
        units = max(4 * resident, (DEFAULT_ROUNDS_SYMBOLS + per_unit - 1) // per_unit)
    return (units * unit + unit // 2) * chunk + ragged, units


# ---- ragged batches, one stream per wave (tests/test_gpu_batch.py) -----------------------------------------------------------
def _batch_row(rid, fmt, sb, K, ways, decode, encode):
    return {"id": rid, "fmt": fmt, "sb": sb, "K": K, "ways": ways, "decode": decode, "encode": encode}


BATCH_ROWS = [
    _batch_row("word-64", FMT_WORD, 12, 256, 64, "k_decode_batch_word64", "k_encode_batch<word>"),
    _batch_row("word-128", FMT_WORD, 12, 256, 128, "k_decode_batch<word>", "k_encode_batch<word>"),
    _batch_row("word-8", FMT_WORD, 12, 256, 8, "k_decode_batch<word>", "k_encode_batch<word>"),
    _batch_row("word-u16-64", FMT_WORD, 12, 1024, 64, "k_decode_batch<word, u16 symbols>", "k_encode_batch<word>"),
    _batch_row("byte-64-14bit", FMT_BYTE, 14, 256, 64, "k_decode_batch<byte>", "k_encode_batch<byte>"),
    _batch_row("byte-64-12bit", FMT_BYTE, 12, 256, 64, "k_decode_batch<byte, slot records>", "k_encode_batch<byte>"),
    _batch_row("byte-2", FMT_BYTE, 14, 256, 2, "k_decode_batch<byte>", "k_encode_batch<byte>"),
    _batch_row("r64-64", FMT_R64, 14, 256, 64, "k_decode_batch<r64>", "k_encode_batch<r64>"),
    _batch_row("r64-2", FMT_R64, 14, 256, 2, "k_decode_batch<r64>", "k_encode_batch<r64>"),
    _batch_row("r64-search-64", FMT_R64, 20, 256, 64, "k_decode_batch<r64 search>", "k_encode_batch<r64 full-width>"),
    _batch_row("alias256-64", FMT_ALIAS, 16, 256, 64, "k_decode_batch<alias>", "k_encode_batch<alias, LDS remap>"),
]
ROW = {r["id"]: r for r in BATCH_ROWS}


def row_batch_kernel_names(rows):
    return {r[k] for r in rows for k in ("decode", "encode")}


# ---- ... with one model per stream (tests/test_gpu_batch_models.py) ----------------------------------------------------------
def _model_row(rid, fmt, sb, ways):
    f = "word" if fmt == FMT_WORD else "byte"
    return {"id": rid, "fmt": fmt, "sb": sb, "ways": ways, "decode": "k_decode_batch_models<%s>" % f,
            "encode": "k_encode_batch_models<%s>" % f}


MODEL_ROWS = [
    _model_row("word-64", FMT_WORD, 12, 64),
    _model_row("word-8", FMT_WORD, 12, 8),
    _model_row("word-128", FMT_WORD, 12, 128),
    _model_row("byte-64-12bit", FMT_BYTE, 12, 64),
    _model_row("byte-2-12bit", FMT_BYTE, 12, 2),
    _model_row("byte-64-8bit", FMT_BYTE, 8, 64),
]
MODEL_ROW = {r["id"]: r for r in MODEL_ROWS}

# ---- eight 8-way word streams per wave: decoder (tests/test_gpu_batch_groups.py), encoder (tests/test_gpu_batch_encode_groups.py)
GROUP_ROWS = [
    {"id": "word-8-groups", "fmt": FMT_WORD, "sb": 12, "K": 256, "ways": 8,
     "decode": "k_decode_batch_word_groups", "encode": "k_encode_batch<word>"},
]
GROW = GROUP_ROWS[0]
ENC_GROUP_ROWS = [
    {"id": "word-8-enc-groups", "fmt": FMT_WORD, "sb": 12, "K": 256, "ways": 8,
     "decode": "k_decode_batch<word>", "encode": "k_encode_batch_word_groups"},
]
EROW = ENC_GROUP_ROWS[0]


# ---- thirty-two 2-way byte streams per wave: decoder (tests/test_gpu_batch_pairs.py) ...
def _pair_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_BYTE, "sb": sb, "K": K, "ways": 2, "decode": "k_decode_batch_byte_pairs", "encode": "k_encode_batch<byte>"}


PAIR_ROWS = [
    _pair_row("byte-2-pairs", 14, 256),           # the reference's scale_bits (main.cpp:139)
    _pair_row("byte-2-pairs-16bit", 16, 256),     # 64 KiB of cum2sym: one block per CU
    _pair_row("byte-2-pairs-12bit", 12, 256),     # (the wave kernel would take the fused slot records here)
    _pair_row("byte-2-pairs-8bit", 8, 256),
    _pair_row("byte-2-pairs-64sym-10bit", 10, 64),
]
PROW = {r["id"]: r for r in PAIR_ROWS}
PMAIN = PROW["byte-2-pairs"]
PAIR_RATE_ROW = {16: PROW["byte-2-pairs-16bit"], 14: PMAIN}  # the rows of _batch.rate_batch / rate_wave, by scale_bits


# ... and encoder (tests/test_gpu_batch_encode_pairs.py)
def _enc_pair_row(rid, sb, K, decode):
    return {"id": rid, "fmt": FMT_BYTE, "sb": sb, "K": K, "ways": 2, "decode": decode, "encode": "k_encode_batch_byte_pairs"}


# decode None: the decoder the default context reports for the shape (test_gpu_batch_encode_pairs.decoder_of)
ENC_PAIR_ROWS = [
    _enc_pair_row("byte-2-enc-pairs", 14, 256, "k_decode_batch<byte>"),       # the reference's scale_bits (main.cpp:139)
    _enc_pair_row("byte-2-enc-pairs-16bit", 16, 256, "k_decode_batch<byte>"),
    _enc_pair_row("byte-2-enc-pairs-12bit", 12, 256, None),
    _enc_pair_row("byte-2-enc-pairs-8bit", 8, 256, None),
    _enc_pair_row("byte-2-enc-pairs-64sym-10bit", 10, 64, None),                # (the record table is padded to 256)
]
EROWS = {r["id"]: r for r in ENC_PAIR_ROWS}
EMAIN, E16 = EROWS["byte-2-enc-pairs"], EROWS["byte-2-enc-pairs-16bit"]


# ---- sixty-four 2-way rans64 streams per wave: decoder (tests/test_gpu_batch_lanes.py)
def _lane_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_R64, "sb": sb, "K": K, "ways": 2, "decode": "k_decode_batch_r64_lanes", "encode": "k_encode_batch<r64>"}


LANE_ROWS = [
    _lane_row("r64-2-lanes", 14, 256),            # the reference's scale_bits (main64.cpp)
    _lane_row("r64-2-lanes-16bit", 16, 256),      # 64 KiB of cum2sym: eleven waves per block
    _lane_row("r64-2-lanes-12bit", 12, 256),
    _lane_row("r64-2-lanes-64sym-7bit", 7, 64),   # the smallest cum2sym table (2^7 slots hold no 256 symbols)
    _lane_row("r64-2-lanes-64sym-10bit", 10, 64),
]
LROW = {r["id"]: r for r in LANE_ROWS}
LMAIN, LANE16 = LROW["r64-2-lanes"], LROW["r64-2-lanes-16bit"]  # (L16 is the lane ENCODER's name above)
LANE_RATE_ROW = {14: LMAIN, 16: LANE16}  # the rows of _batch_lanes.rate_batch, by scale_bits


# ... and encoder (tests/test_gpu_batch_encode_lanes.py)
def _enc_lane_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_R64, "sb": sb, "K": K, "ways": 2, "decode": "k_decode_batch<r64>", "encode": "k_encode_batch_r64_lanes"}


ENC_LANE_ROWS = [
    _enc_lane_row("r64-2-enc-lanes", 14, 256),            # the reference's scale_bits (main64.cpp)
    _enc_lane_row("r64-2-enc-lanes-16bit", 16, 256),      # a frequency of 2^16 is inside the working range
    _enc_lane_row("r64-2-enc-lanes-12bit", 12, 256),
    _enc_lane_row("r64-2-enc-lanes-64sym-7bit", 7, 64),   # the smallest scale_bits; the record table is padded to 256
    _enc_lane_row("r64-2-enc-lanes-64sym-10bit", 10, 64),
]
ELROW = {r["id"]: r for r in ENC_LANE_ROWS}
ELMAIN, EL16 = ELROW["r64-2-enc-lanes"], ELROW["r64-2-enc-lanes-16bit"]
ENC_LANE_RATE_ROW = {14: ELMAIN, 16: EL16}

# ---- the six streams-per-wave families, one descriptor each: what their GPU and host files differ in -----------------------
# side: the row key of the family's own kernel; streams: per wave; wave_kernel: what the main row's shape reports with the option
# off; shapes: the (sb, K) of the rows; graph: the captured-graph child's format, scale_bits and option, by name
Family = collections.namedtuple("Family", "option side fmt ways streams rows main wave_kernel family shapes graph")
PAIR_SHAPES, LANE_SHAPES = [(8, 256), (10, 64), (12, 256), (14, 256), (16, 256)], [(7, 64), (10, 64), (12, 256), (14, 256), (16, 256)]
GROUPS = Family(OPT_BATCH_GROUPS, "decode", FMT_WORD, 8, 8, GROUP_ROWS, GROW, "k_decode_batch<word>", BATCH_WORD_GROUPS_DECODE,
                [(12, 256)], ("FMT_WORD", 12, "OPT_BATCH_GROUPS"))
PAIRS = Family(OPT_BATCH_PAIRS, "decode", FMT_BYTE, 2, 32, PAIR_ROWS, PMAIN, "k_decode_batch<byte>", BATCH_BYTE_PAIRS_DECODE,
               PAIR_SHAPES, ("FMT_BYTE", 14, "OPT_BATCH_PAIRS"))
LANES = Family(OPT_BATCH_LANES, "decode", FMT_R64, 2, 64, LANE_ROWS, LMAIN, "k_decode_batch<r64>", BATCH_R64_LANES_DECODE,
               LANE_SHAPES, ("FMT_R64", 14, "OPT_BATCH_LANES"))
ENC_GROUPS = Family(OPT_BATCH_ENCODE_GROUPS, "encode", FMT_WORD, 8, 8, ENC_GROUP_ROWS, EROW, "k_encode_batch<word>",
                    BATCH_WORD_GROUPS_ENCODE, [(12, 256)], ("FMT_WORD", 12, "OPT_BATCH_ENCODE_GROUPS"))
ENC_PAIRS = Family(OPT_BATCH_ENCODE_PAIRS, "encode", FMT_BYTE, 2, 32, ENC_PAIR_ROWS, EMAIN, "k_encode_batch<byte>",
                   BATCH_BYTE_PAIRS_ENCODE, PAIR_SHAPES, ("FMT_BYTE", 14, "OPT_BATCH_ENCODE_PAIRS"))
ENC_LANES = Family(OPT_BATCH_ENCODE_LANES, "encode", FMT_R64, 2, 64, ENC_LANE_ROWS, ELMAIN, "k_encode_batch<r64>",
                   BATCH_R64_LANES_ENCODE, LANE_SHAPES, ("FMT_R64", 14, "OPT_BATCH_ENCODE_LANES"))
STREAM_FAMILIES = (GROUPS, ENC_GROUPS, PAIRS, ENC_PAIRS, LANES, ENC_LANES)
WAVE_ENCODER = {FMT_WORD: "k_encode_batch<word>", FMT_BYTE: "k_encode_batch<byte>", FMT_R64: "k_encode_batch<r64>"}


def check_family_rows(d):
    """Every name of the registry's family is the kernel of a row of the family's table on its side, and the table names no
    kernel the registry does not hold; the rows are the family's shapes (a decoder's rows name the wave encoder); and the check
    has teeth: without the family's rows its kernel is reported missing.  (Disjointness from the other families: registry()
    asserts that no name occurs twice.)"""
    names, kernel = registry()[d.family], d.main[d.side]
    assert kernel in names
    rows = {r[d.side] for r in d.rows}
    assert names == rows, ("kernels no row expects", sorted(names - rows), "names no launcher reports", sorted(rows - names))
    assert all(r["ways"] == d.ways and r["fmt"] == d.fmt for r in d.rows)
    assert d.side == "encode" or all(r["encode"] == WAVE_ENCODER[d.fmt] for r in d.rows)
    assert sorted((r["sb"], r["K"]) for r in d.rows) == d.shapes
    less = {r[d.side] for r in d.rows if not r["id"].startswith(d.main["id"])}
    assert kernel in names - less
