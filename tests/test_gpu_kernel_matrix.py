"""Every kernel the launchers can report, over several rounds of its persistent grid, every chunk against the oracle.

Every coder kernel is a persistent grid: waves claim work units from counters, place chunks by look-back over status words
and re-zero the counter slot a later launch will use.  Mistakes in that machinery show only when a launch holds more units
than the grid has waves, so every row of KERNEL_ROWS runs in three regimes, sized from the device's CU count and the row's
work unit (word groups: 8 chunks, byte pairs: 32, lane kernels: 64, everything else: 1):

  U  one unit and a partial one, the last chunk ragged
  H  about half as many units as there are resident waves (part of one round)
  R  at least 4 x (CUs x 2 blocks x 16 waves per block) units, a partial unit, a ragged last chunk (several rounds) -- 16
     waves is the largest block any launcher uses, so the count is an upper bound of the resident waves of every kernel

Input is bench.gen_zipf with seed 1 (test_gpu_scale.py proves it equal to the oracle's generator); the checker is
tests/_every_chunk.py: every chunk of every layout is compared with the CPU oracle, the decoders also get a container the
oracle made, and after every call the kernel the library reports must be the one the row names -- a change of dispatch
that moves a shape to another kernel fails here instead of leaving a kernel without a test.

test_no_kernel_without_a_row runs without a GPU: every kernel-name literal of the launchers in ryg_rans_amd/csrc/*.hip
must appear in KERNEL_ROWS, and KERNEL_ROWS must name no kernel the sources do not contain.
"""
import glob
import os
import re

import pytest

from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ryg_rans_amd", "csrc")

# context options (ryg_rans_amd.OPT_*; the numbers are the ABI's, tests/test_abi.py)
LANE_FUSED, FUSED, DUAL = 1, 2, 3

WAVES_PER_BLOCK = 16  # kDecBlockThreads / 64: no launcher uses a larger block
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


_LITERAL = re.compile(r'"((?:[^"\\]|\\.)*)"')


def source_kernel_names(csrc=CSRC):
    """The kernel-name literals of the launchers: every string literal of a statement `*name = ...;` (a ternary chain has one
    per arm), and the literal passed as `kname` at every call of launch_dual_t (decode_dual.hip assigns `*name = kname`).
    Returns (names, number of assignment statements)."""
    names, sites = set(), 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        text = open(path).read()
        for m in re.finditer(r"\*name\s*=\s*([^;]*);", text):
            sites += 1
            names.update(_LITERAL.findall(m.group(1)))
        for m in re.finditer(r"\blaunch_dual_t<[^;(]*>\(([^;]*)\);", text):
            lits = _LITERAL.findall(m.group(1))
            assert lits, (path, m.group(0))  # (a caller that passes no literal: this extraction must learn its form)
            names.update(lits)
    return names, sites


def test_no_kernel_without_a_row():
    """Runs without a GPU.  All 13 statements that assign `*name` in ryg_rans_amd/csrc/*.hip are found -- the seven arms of
    encode_wave.hip's chain, the ten of decode_wave.hip's (k_decode_word64 is its first), every caller of launch_dual_t -- and the
    set of names they can report equals the set KERNEL_ROWS expects: a new kernel needs a row, and a row cannot name a kernel
    that is gone."""
    names, sites = source_kernel_names()
    assert sites >= 13, sites
    for must in ("k_encode<word>", "k_encode<byte>", "k_encode<byte, per-chunk models>", "k_encode<word, per-chunk models>", "k_encode<r64>",
                 "k_encode<r64 full-width>", "k_encode<alias, LDS remap>", "k_decode_dual<alias>", "k_decode<word, u16 symbols>",
                 "k_decode_lanes_r64x2<packed slots>", "k_decode_lanes_r64x2", "k_encode_adaptive<word>", "k_encode_adaptive<byte>"):
        assert must in names, must
    assert all(n.startswith("k_") for n in names), names
    rows = row_kernel_names()
    assert not names - rows, ("kernels no row of KERNEL_ROWS expects", sorted(names - rows))
    assert not rows - names, ("KERNEL_ROWS names kernels no launcher reports", sorted(rows - names))
    # the check has teeth: without its row a kernel is reported missing
    less = [r for r in KERNEL_ROWS if r["decode"] != "k_decode_lanes"]
    assert "k_decode_lanes" in names - row_kernel_names(less)


# ---- the GPU part ---------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def resident_waves(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * WAVES_PER_BLOCK


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


def _cases():
    for r in KERNEL_ROWS:
        for regime in r["regimes"]:
            yield pytest.param(r, regime, id="%s-%s" % (r["id"], regime), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,regime", list(_cases()))
def test_kernel_row_every_chunk_equals_oracle(gpu, oracle, row, regime):
    R, shared, torch = gpu
    from _every_chunk import check_every_chunk, check_every_chunk_adaptive
    resident = resident_waves(torch)
    n, units = regime_symbols(row, regime, resident)
    if regime == "R":  # a bigger part must not turn "several rounds" into one round unnoticed
        assert units >= 4 * resident and n >= units * row["unit"] * row["chunk"], (units, resident)
    if regime == "H":
        assert 0 < units < resident
    ctx = R.Context(0) if row["opts"] else shared  # (options must not leak into the other rows)
    try:
        for opt, val in row["opts"]:
            ctx.set_option(opt, val)
        kernels = {k: pick(row[k], regime) for k in ("decode", "encode", "slots", "sized")}
        if row["kind"] == "adaptive":
            check_every_chunk_adaptive(R, ctx, torch, oracle, row["fmt"], row["sb"], row["ways"], row["chunk"], n, kernels)
        else:
            small = row["chunk"] < 512
            # (the sized container against the compact one: a statement about many full chunks in whole 64-byte lines -- not
            #  about regime U, where the ragged last chunk is one of two and still gets a slot of the full size)
            ratio = None if small or regime == "U" else 1.35
            check_every_chunk(R, ctx, torch, row["fmt"], row["sb"], row["K"], row["ways"], row["chunk"], n, kernels=kernels, damaged=False,
                              sized=row["sized"] is not None, sized_ratio=ratio, all_overflow_at_half=not small)
    finally:
        if ctx is not shared:
            ctx.close()


# ---- the counter ring, on purpose --------------------------------------------------------------------------------------

RING_DECODE_LAUNCHES = 136  # two wraps of the 64-slot ring and a bit


@pytest.mark.gpu
def test_counter_ring_two_wraps_on_a_fresh_context(oracle):
    """A fresh context, RING_DECODE_LAUNCHES eager decode launches without a synchronisation in between, cycling through the
    decode rows of the matrix at their "part of one round" size in a FIXED order (launch i runs item i % items: a failure
    names its position in the ring).  The three decode entry points share the one ring, so the cycle holds all of them:
    the static rows through ctx.decode, the two per-chunk-model rows through ctx.decode_adaptive, and one ragged batch
    (tests/test_gpu_batch.py's Batch) through ctx.decode_batch.  Launch i claims from counter slot i % 64 and re-zeroes slot
    (i + 32) % 64 for the launch 32 calls later (api.cpp take_counter_slot): a kernel family or an entry point that forgot
    would leave a used counter to a launch of ANOTHER one.  Every launch has its own pre-poisoned output; afterwards every
    output == its input and decode_errors() == 0.
    Then the encoders that claim from the encode status workspace, the three placements mixed, rans_amd_encode_status after
    every call and every chunk of every container against the oracle."""
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import bench
    import ryg_rans_amd as R
    from test_gpu_batch import ROW as BATCH_ROW, Batch, draw_lengths
    resident = resident_waves(torch)
    rows = [r for r in KERNEL_ROWS if "H" in r["regimes"] and not r["opts"]]
    assert len({pick(r["decode"], "H") for r in rows if r["kind"] == "static"}) >= 10
    assert sorted(r["id"] for r in rows if r["kind"] == "adaptive") == ["byte-64-per-chunk-models", "word-64-per-chunk-models"]
    ctx = R.Context(0)
    try:
        prepared = []
        for r in rows:
            n, _ = regime_symbols(r, "H", resident)
            d_syms = bench.gen_zipf(torch, n, r["K"], 1.0, 1, "cuda")
            if r["kind"] == "adaptive":  # (its own container and frequency rows: one model per chunk, built by the encoder)
                cont, offs, lens, freqs, total = ctx.encode_adaptive(d_syms, r["ways"], r["chunk"], r["sb"], fmt=r["fmt"])
                gm = None
            else:
                freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, r["K"]), 1 << r["sb"])
                gm = ctx.model(r["fmt"], freqs, r["sb"])
                cont, offs, lens, total = ctx.encode(gm, d_syms, r["ways"], r["chunk"])
            prepared.append((r, n, d_syms, freqs, gm, cont, offs, lens, total))
        # the ragged batch: 300 streams of 0 .. 64 Ki symbols, laid out on 4-symbol boundaries in a poison-filled buffer
        brow = BATCH_ROW["word-64"]
        b = Batch(R, ctx, torch, oracle, brow, draw_lengths(300, brow["ways"], 7))
        b_buf, b_sym_offs, b_slot_offs = b.laid_out(4)
        b_sym, b_slot = b.dev(b_sym_offs, np.int64), b.dev(b_slot_offs, np.int64)
        b_cont, b_offs, b_lens = ctx.encode_batch(b.gm, b_buf, b_sym, b.d_counts, brow["ways"], b_slot)
        ctx.encode_status()
        items = prepared + [(dict(brow, kind="batch", id="batch-" + brow["id"]), None, b_buf)]
        torch.cuda.synchronize()
        outs = []
        for i in range(RING_DECODE_LAUNCHES):
            r, n, d_syms = items[i % len(items)][:3]
            if r["kind"] == "batch":
                out = torch.full_like(d_syms, b.poison())
                ctx.decode_batch(b.gm, b_cont, int(b_slot_offs[-1]), b_offs, b_lens, b_sym, b.d_counts, r["ways"], out, sync=False)
            else:
                freqs, gm, cont, offs, lens, total = items[i % len(items)][3:]
                out = torch.full_like(d_syms, 0x5A)
                if r["kind"] == "adaptive":
                    ctx.decode_adaptive(cont, total, offs, lens, freqs, n, r["ways"], r["chunk"], r["sb"], d_out=out, sync=False, fmt=r["fmt"])
                else:
                    ctx.decode(gm, cont, total, offs, lens, n, r["ways"], r["chunk"], d_out=out, sync=False)
            assert ctx.last_decode_kernel() == pick(r["decode"], "H"), (i, r["id"], ctx.last_decode_kernel())
            outs.append(out)
        assert {items[i % len(items)][0]["kind"] for i in range(RING_DECODE_LAUNCHES)} == {"static", "adaptive", "batch"}
        assert ctx.decode_errors() == 0
        for i, out in enumerate(outs):
            r, n, d_syms = items[i % len(items)][:3]
            assert torch.equal(out, d_syms), ("launch", i, "ring slot", i % 64, r["id"])
        del outs
        # the encoders: wave encoders (status words + claims), the group encoder (claims), lane encoders -- compact, slots, sized
        enc_rows = [p for p in prepared if p[0]["id"] in ("word-64", "byte-64-14bit", "r64-64", "alias256-64", "word-8", "byte-2", "word-4")]
        assert len(enc_rows) == 7  # (7 rows x 3 placements: launch i runs row i % 7 in placement i % 3 -- all 21 pairs)
        for i in range(63):
            r, n, d_syms, freqs, gm, cont, offs, lens, total = enc_rows[i % 7]
            fmt, ways, chunk = r["fmt"], r["ways"], r["chunk"]
            nchunks = (n + chunk - 1) // chunk
            art = {"fmt": fmt, "sb": r["sb"], "K": r["K"], "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms}
            key = ("encode", "slots", "sized")[i % 3]
            if key == "encode":
                e_cont, e_offs, e_lens, _ = ctx.encode(gm, d_syms, ways, chunk, sync=False)
            elif key == "slots":
                e_cont, e_offs, e_lens, _ = ctx.encode_slots(gm, d_syms, ways, chunk, sync=False)
                art["slot"] = R.slot_bytes(fmt, n, ways, chunk)
            else:
                e_cont, e_offs, e_lens, _, slot = ctx.encode_sized(gm, d_syms, ways, chunk, sync=False)
                art["slot"], art["worst"] = slot, R.slot_bytes(fmt, n, ways, chunk)
            got = (ctx.last_encode_kernel()[0], ctx.last_encode_placement())
            assert got == pick(r[key], "H"), (i, r["id"], key, got)
            ctx.encode_status()
            assert torch.equal(e_lens, lens), (i, r["id"], key)
            art.update(cont=e_cont, offs=e_offs, lens=e_lens, total=int(e_offs[nchunks].item()))
            assert bench.oracle_check_chunks(art) == nchunks, (i, r["id"], key)
    finally:
        ctx.close()
