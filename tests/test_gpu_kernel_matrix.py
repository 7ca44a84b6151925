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

test_no_kernel_without_a_row runs without a GPU: every name of the registry's uniform family (tests/_kernel_rows.py reads
ryg_rans_amd/csrc/kernel_names.hpp) must appear in KERNEL_ROWS, and KERNEL_ROWS must name no kernel the registry does not hold.
"""
import pytest

from _batch import resident_waves
from _kernel_rows import KERNEL_ROWS, UNIFORM, pick, regime_symbols, registry, row_kernel_names


def test_no_kernel_without_a_row():
    """Runs without a GPU.  The set of names the uniform launchers can report -- the registry's uniform family -- equals the set
    KERNEL_ROWS expects: a new kernel needs a row, and a row cannot name a kernel that is gone.  (A count of the assignment
    statements and a special case for launch_dual_t's argument once guarded the completeness of a scan of the sources; the
    launchers now report a KernelId, and a name outside the registry does not compile.)"""
    names = registry()[UNIFORM]
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
    (tests/_batch.py's Batch) through ctx.decode_batch.  Launch i claims from counter slot i % 64 and re-zeroes slot
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
    from _batch import Batch, draw_lengths
    from _kernel_rows import ROW as BATCH_ROW
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
