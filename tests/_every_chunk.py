"""The "every chunk" checker shared by tests/test_gpu_scale.py and tests/test_gpu_kernel_matrix.py.

One call takes a shape through the whole device path and compares EVERY chunk with the CPU oracle -- nothing is sampled:

  1.  GPU encode (compact layout): every chunk == the oracle's stream, the index == the prefix sums
      (bench.oracle_check_chunks); GPU decode of the GPU's own container
  2.  GPU decode of a container the ORACLE made (bench.decode_oracle_container)
  3.  the encoder's scratch ring (64-way wave encoders)
  4.  the slot layout, then its compaction
  4b. sized slots at the tight size and at half of it
  5.  (optional) one damaged chunk

`kernels` names what the library must report for the shape (rans_amd_last_decode_kernel / rans_amd_last_encode_kernel):
a dict with any of
    "decode": name
    "encode": (name, placement)   the compact layout  -- placement 0: layout + compaction kernels behind the coder,
    "slots":  (name, placement)   the slot layout        1: the coder placed its chunks itself, 2: slots (nothing moved)
    "sized":  (name, placement)   sized slots
A key that is missing is not asserted.  The names are checked right after every call that launches the kernel in question,
so a change of dispatch.cpp that moves a shape to another kernel fails here and does not leave a kernel untested.
"""
import numpy as np

from _oracle import FMT_ALIAS


def expect_encode(ctx, kernels, key, what):
    if kernels and kernels.get(key) is not None:
        name, placement = kernels[key]
        got = (ctx.last_encode_kernel()[0], ctx.last_encode_placement())
        assert got == (name, placement), (what, key, "the library ran", got, "the row expects", (name, placement))


def expect_decode(ctx, kernels, what):
    if kernels and kernels.get("decode") is not None:
        assert ctx.last_decode_kernel() == kernels["decode"], (what, "the library ran", ctx.last_decode_kernel(),
                                                               "the row expects", kernels["decode"])


def check_every_chunk(R, ctx, torch, fmt, sb, K, ways, chunk, n, kernels=None, seed=1, damaged=True, sized=True,
                      sized_ratio=1.35, all_overflow_at_half=True, d_syms=None, freqs=None):
    """See the module docstring.  sized_ratio: the sized container against the compact one (None: small chunks, whose slots
    of whole 64-byte lines outweigh the compact layout's 16-byte grid -- only rans_amd_encode_sized_bound() holds there).
    all_overflow_at_half: chunks large enough that every full one is longer than half its tight slot.  Returns the artifact
    dict of the compact container (d_syms, freqs, cont, offs, lens, total ...).
    freqs: a normalised model in place of the one counted from the input (tests/test_gpu_lane_extremes.py: input that does not
    follow its model -- frequency-1 symbols only, say, whose histogram would normalise to a flat model).  Chunks of such
    input overflow a tight slot by design, so the sized steps then get overflow room for every chunk."""
    import bench
    if d_syms is None:
        d_syms = bench.gen_zipf(torch, n, K, 1.0, seed, "cuda")
    if freqs is None:
        counts = ctx.count_freqs_device(d_syms, K)
        assert int(counts.sum()) == n
        freqs, _ = R.normalize_freqs(counts, 1 << sb)
        room = None
    else:
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        assert freqs.size == K and int(freqs.sum()) == 1 << sb
        room = (n + chunk - 1) // chunk
    gm = ctx.model(fmt, freqs, sb)
    cont, offs, lens, total = ctx.encode(gm, d_syms, ways, chunk)
    expect_encode(ctx, kernels, "encode", "compact encode")
    art = {"fmt": fmt, "sb": sb, "K": K, "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms,
           "cont": cont, "offs": offs, "lens": lens, "total": total}
    # 1. EVERY chunk of the GPU encoder's container == the oracle's stream for it; the index == prefix sums
    assert bench.oracle_check_chunks(art) == (n + chunk - 1) // chunk
    out = ctx.decode(gm, cont, total, offs, lens, n, ways, chunk)
    assert torch.equal(out, d_syms)
    expect_decode(ctx, kernels, "decode of the GPU's container")
    del out
    # 2. the decoder on a container made by the ORACLE alone (host, threaded), not by the GPU encoder
    assert bench.decode_oracle_container(torch, R, ctx, gm, art, "cuda")
    expect_decode(ctx, kernels, "decode of the oracle's container")
    # 3. the encoder with its scratch ring (RANS_AMD_OPT_ENC_SCRATCH_RING; wave-per-chunk encoders): the same container
    if ways == 64 and fmt != FMT_ALIAS:
        ctx2 = R.Context(0)
        ctx2.set_option(R.OPT_ENC_SCRATCH_RING, 1)
        gm2 = ctx2.model(fmt, freqs, sb)
        cont_r, offs_r, lens_r, total_r = ctx2.encode(gm2, d_syms, ways, chunk)
        assert total_r == total and torch.equal(offs_r, offs) and torch.equal(lens_r, lens)
        art_r = dict(art, cont=cont_r)
        assert bench.oracle_check_chunks(art_r) == (n + chunk - 1) // chunk
        del cont_r, gm2
        ctx2.close()
    # 4. the slot layout (rans_amd_encode_slots: every chunk written once, where it was coded): every chunk == the
    #    oracle's stream again, index == (c + 1) * slot - length, the slot container decodes as it is, and its compaction
    #    is the container of step 1
    s_cont, s_offs, s_lens, s_total = ctx.encode_slots(gm, d_syms, ways, chunk)
    assert ctx.last_encode_placement() == 2 and torch.equal(s_lens, lens)
    expect_encode(ctx, kernels, "slots", "slot layout")
    art_s = dict(art, cont=s_cont, offs=s_offs, lens=s_lens, total=s_total, slot=R.slot_bytes(fmt, n, ways, chunk))
    assert bench.oracle_check_chunks(art_s) == (n + chunk - 1) // chunk
    out = ctx.decode(gm, s_cont, s_total, s_offs, s_lens, n, ways, chunk)
    assert torch.equal(out, d_syms)
    expect_decode(ctx, kernels, "decode of the slot container")
    del out
    c_cont, c_offs, c_total = ctx.compact(s_cont, s_total, s_offs, s_lens, lens.numel())
    assert c_total == total and torch.equal(c_offs, offs)
    assert bench.oracle_check_chunks(dict(art, cont=c_cont, offs=c_offs)) == (n + chunk - 1) // chunk
    del s_cont, c_cont
    # 4b. SIZED slots (rans_amd_encode_slots_sized, slot = rans_amd_tight_slot_bytes()): every chunk == the oracle's stream
    #     wherever it lies (its slot or the overflow region), the index follows the layout's rule, the container is about
    #     the compact one's size and decodes as it is.  Then the same with slots of HALF that size: every chunk overflows
    #     into the region behind them (the redo launch codes the whole shard) and still equals the oracle's.
    if sized:
        nchunks = (n + chunk - 1) // chunk
        worst = R.slot_bytes(fmt, n, ways, chunk)
        t_cont, t_offs, t_lens, t_total, t_slot = ctx.encode_sized(gm, d_syms, ways, chunk, overflow_chunks=room)
        assert torch.equal(t_lens, lens) and t_slot < worst
        expect_encode(ctx, kernels, "sized", "sized slots")
        if sized_ratio is not None:
            assert t_total <= sized_ratio * total, (t_total, total)  # (config 2's 512-symbol chunks in whole 64-byte lines: 1.23 x)
        assert t_total <= R.encode_sized_bound(fmt, n, ways, chunk, t_slot, nchunks // 64 + 4 if room is None else room), t_total
        assert bench.oracle_check_chunks(dict(art, cont=t_cont, offs=t_offs, lens=t_lens, total=t_total, slot=t_slot, worst=worst)) == nchunks
        out = ctx.decode(gm, t_cont, t_total, t_offs, t_lens, n, ways, chunk)
        assert torch.equal(out, d_syms)
        expect_decode(ctx, kernels, "decode of the sized container")
        del out, t_cont
        half = max(64, (t_slot // 2) & ~63)
        h_cont, h_offs, h_lens, h_total, _ = ctx.encode_sized(gm, d_syms, ways, chunk, slot=half, overflow_chunks=nchunks)
        expect_encode(ctx, kernels, "sized", "sized slots, half the tight size")
        assert torch.equal(h_lens, lens)
        if all_overflow_at_half:
            assert h_total >= nchunks * half + (nchunks - 1) * worst  # (a ragged last chunk may fit)
        # (whatever the chunk size: a chunk longer than its slot cannot lie in it)
        assert h_total >= nchunks * half + int((lens.to(torch.int64) > half).sum().item()) * worst
        assert bench.oracle_check_chunks(dict(art, cont=h_cont, offs=h_offs, lens=h_lens, total=h_total, slot=half, worst=worst)) == nchunks
        out = ctx.decode(gm, h_cont, h_total, h_offs, h_lens, n, ways, chunk)
        assert torch.equal(out, d_syms)
        del out, h_cont
    # 5. a corrupted chunk is flagged (or at least does not decode to the input)
    if damaged:
        bad = cont.clone()
        bad[int(offs[0].item()) + int(lens[0].item()) // 2] ^= 0x10
        out2 = torch.empty_like(d_syms)
        ctx.decode(gm, bad, total, offs, lens, n, ways, chunk, d_out=out2, sync=False)
        assert ctx.decode_errors() >= 1 or not torch.equal(out2, d_syms)
    return art


def check_every_chunk_adaptive(R, ctx, torch, oracle, fmt, sb, ways, chunk, n, kernels, seed=1):
    """Per-chunk models: the one-kernel encoder (rans_amd_encode_adaptive_sized) and the three-launch path
    (rans_amd_encode_adaptive) -- EVERY chunk's row == the oracle's normalize(count(chunk)) and EVERY chunk's stream == the
    oracle's stream of that chunk under its own model (Oracle.compare_container_adaptive); both containers decode as they
    are, and so does a container (streams AND rows) the ORACLE made.
    kernels: {"decode": name, "encode": name of the three-launch coder, "sized": name of the one-kernel encoder}."""
    import bench
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, seed, "cuda")
    h_syms = d_syms.cpu().numpy()
    nchunks = (n + chunk - 1) // chunk
    cont, offs, lens, rows, total = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt)
    assert ctx.last_encode_kernel()[0] == kernels["sized"], ctx.last_encode_kernel()
    h_offs, h_lens = offs.cpu().numpy().astype(np.uint64), lens.cpu().numpy().astype(np.uint32)
    h_rows = rows.cpu().numpy()
    count, bad = oracle.compare_container_adaptive(fmt, h_syms, ways, chunk, sb, cont[:total].cpu().numpy(), h_offs, h_lens, h_rows)
    assert count == nchunks and bad == -1, bad
    ends = h_offs[:nchunks] + h_lens
    assert np.all(ends % np.uint64(64) == 0) and np.all(ends[:-1] <= h_offs[1:nchunks]) and int(ends[-1]) == total == int(h_offs[nchunks])
    out = ctx.decode_adaptive(cont, total, offs, lens, rows, n, ways, chunk, sb, fmt=fmt)
    assert ctx.last_decode_kernel() == kernels["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_syms) and ctx.decode_errors() == 0
    del out, cont
    # the three-launch path: the same rows and the same streams (its container: the compact layout)
    c0, o0, l0, r0, t0 = ctx.encode_adaptive(d_syms, ways, chunk, sb, fmt=fmt)
    assert ctx.last_encode_kernel()[0] == kernels["encode"], ctx.last_encode_kernel()
    assert torch.equal(r0, rows) and torch.equal(l0, lens)
    count, bad = oracle.compare_container_adaptive(fmt, h_syms, ways, chunk, sb, c0[:t0].cpu().numpy(), o0.cpu().numpy(), h_lens, h_rows)
    assert count == nchunks and bad == -1, bad
    out = ctx.decode_adaptive(c0, t0, o0, l0, r0, n, ways, chunk, sb, fmt=fmt)
    assert ctx.last_decode_kernel() == kernels["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_syms) and ctx.decode_errors() == 0
    del out, c0
    # the decoder on a container (streams AND rows) made by the oracle alone
    o_cont, o_offs, o_lens, o_rows = oracle.encode_chunked_adaptive(fmt, h_syms, ways, chunk, sb)
    assert np.array_equal(o_lens, h_lens) and np.array_equal(o_rows.reshape(-1), h_rows.view(np.uint16))
    d_cont = torch.zeros(o_cont.size + 64, dtype=torch.uint8, device="cuda")
    d_cont[:o_cont.size] = torch.from_numpy(o_cont).cuda()
    out = ctx.decode_adaptive(d_cont, o_cont.size, torch.from_numpy(o_offs.astype(np.int64)).cuda(),
                              torch.from_numpy(o_lens.astype(np.int32)).cuda(), torch.from_numpy(o_rows.reshape(-1).view(np.int16)).cuda(),
                              n, ways, chunk, sb, fmt=fmt)
    assert ctx.last_decode_kernel() == kernels["decode"], ctx.last_decode_kernel()
    assert torch.equal(out, d_syms) and ctx.decode_errors() == 0
