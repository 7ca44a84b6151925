"""Every chunked encode entry point at its capacity's edge: where it writes, and what it reports.

The rule under test (include/ryg_rans_amd.h, rans_amd_encode): a compact-layout call succeeds iff out_cap >= E =
d_offsets[n_chunks] rounded up to 16, and whatever the status no byte outside [d_out, d_out + out_cap) is written.  The
reference is plain integers (tests/_capacity.py: ref_offsets, total, aligned_end, caps_for); the streams are the CPU
oracle's (bench.oracle_check_chunks / Oracle.compare_container_adaptive on the ample run, every other run compared with the
ample one on the device through a mask of stream bytes).  Every comparison is exact.

Every call encodes into an ARENA: d_out is a slice of exactly out_cap bytes of a poisoned tensor with 4 KiB of poison on
both sides, d_offsets exactly n_chunks + 1 and d_lengths exactly n_chunks entries of sentinel-filled tensors with eight guard
entries on both sides.  A stray write lands in the test's own memory and is found there; the library is never told of more
room than lies behind d_out.

  test_compact_capacity          one test per row of _capacity.CASES -- every (coding kernel, placement) pair of the compact
                                 layout, the scratch-ring variant, both per-chunk-model rows (rans_amd_encode_adaptive) --
                                 with three last-chunk sizes (T mod 16 = smallest, largest, 0) x the caps of caps_for
  test_adaptive_sized_capacity   rans_amd_encode_adaptive_sized at out_cap = P (the total of its pieces), P - 1 and P - 64
  test_slots_capacity            rans_amd_encode_slots at out_cap = n_chunks * slot and one byte less
  test_sized_slots_capacity      rans_amd_encode_slots_sized at out_cap = rans_amd_encode_sized_bound(.., room) exactly
  test_container_compact_capacity rans_amd_container_compact at dst_cap = T (T % 16 != 0: E_SPACE) and E (OK)

Seconds per test on an MI355X (256 CUs; the whole file: 23 tests in 4.4 s):
test_compact_capacity[word-64] 1.02 (the first launches of the process), [word-64-scratch-ring] 0.20 (16 385 chunks, 67 M
symbols), [byte-2] and [byte-2-lane-fused] 0.13 (98 241 chunks), [r64-2-lane-fused] 0.12, [r64-2-packed] 0.08, [word-8]
and [word-4] 0.03, every other case 0.01-0.02; test_adaptive_sized_capacity, test_slots_capacity,
test_sized_slots_capacity and test_container_compact_capacity 0.01 or less each.
"""
import time

import numpy as np
import pytest

import _capacity as C

pytestmark = pytest.mark.gpu

# No performance bound: it tells a refused call that returns at once from one that waits for the placement protocols' watchdog
# (30 s and more: a wave of the placement waiting for something a refused chunk never sends).  A call here takes milliseconds.
STALL_SECONDS = 10.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    yield R, torch, torch.cuda.get_device_properties(0).multi_processor_count


def context_for(R, opts):
    ctx = R.Context(0)
    for opt, val in opts:
        ctx.set_option(opt, val)
    return ctx


class Run:
    """One encode into fresh arenas.  call(d_out, d_offsets, d_lengths, sync) makes the library call."""

    def __init__(self, R, torch, nchunks, cap, call, sync=True, rows=False):
        self.cap, self.nchunks = cap, nchunks
        self.whole, self.d_out = C.arena(torch, cap)
        self.offs_whole, self.d_offs = C.index_arena(torch, nchunks + 1, torch.int64)
        self.lens_whole, self.d_lens = C.index_arena(torch, nchunks, torch.int32)
        self.rows_whole = self.d_rows = None
        extra = ()
        if rows:  # per-chunk models: the frequency rows, 256 entries per chunk (8-byte aligned: 8 guard entries of 2 bytes)
            self.rows_whole, self.d_rows = C.arena(torch, nchunks * 256, C.GUARD_ENTRIES, C.GUARD_ENTRIES, torch.int16, C.SENTINEL)
            extra = (self.d_rows,)
        assert self.d_out.numel() == cap and self.d_offs.numel() == nchunks + 1 and self.d_lens.numel() == nchunks
        self.total = None
        t0 = time.perf_counter()
        try:
            self.total = call(self.d_out, self.d_offs, self.d_lens, sync, *extra)
            self.status = R.OK
        except R.RansAmdError as e:
            self.status = e.status
        self.seconds = time.perf_counter() - t0

    def assert_guards(self, what):
        """The front guard, every byte of the arena from out_cap on, the guard entries around the index arrays."""
        assert C.guards_intact(self.whole, self.d_out, C.POISON), (what, "a byte outside [d_out, d_out + out_cap) was written")
        assert C.guards_intact(self.offs_whole, self.d_offs, C.SENTINEL), (what, "written outside d_offsets[0 .. n_chunks]")
        assert C.guards_intact(self.lens_whole, self.d_lens, C.SENTINEL), (what, "written outside d_lengths[0 .. n_chunks)")
        if self.rows_whole is not None:
            assert C.guards_intact(self.rows_whole, self.d_rows, C.SENTINEL), (what, "written outside the frequency rows")

    def host_index(self):
        return self.d_offs.cpu().numpy().astype(np.uint64), self.d_lens.cpu().numpy().astype(np.uint32)


def same_stream_bytes(torch, got, want, mask, size):
    """Every stream byte below `size` equal (the gaps between the chunks are not compared)."""
    return bool(((got[:size] == want[:size]) | ~mask[:size]).all())


# ---- the compact layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_compact_capacity(gpu, oracle, case):
    import bench
    R, torch, cus = gpu
    row = C.row_of(case)
    fmt, sb, K, ways, chunk = row["fmt"], row["sb"], row["K"], row["ways"], row["chunk"]
    adaptive = C.is_adaptive(case)
    full = C.full_chunks(case, cus)
    nchunks = full + 1
    tails = C.tails_for(oracle, case, cus)
    ctx = context_for(R, case.opts)
    try:
        gm = freqs = None
        if not adaptive:
            freqs = C.model_freqs(oracle, case, cus)
            gm = ctx.model(fmt, freqs, sb)

        def is_the_rows(what):
            got = (ctx.last_encode_kernel()[0], ctx.last_encode_placement())
            assert got == (case.kernel, case.placement), (case.id, what, "the library ran", got)

        async_done = False
        for label, tail, residue in zip(C.RESIDUE_LABELS, tails, C.residues_of(case)):
            n = full * chunk + tail
            d_syms = bench.gen_zipf(torch, n, K, 1.0, 1, "cuda")
            h_tail = d_syms[full * chunk:].cpu().numpy()
            assert np.array_equal(h_tail.view(np.uint16) if h_tail.dtype == np.int16 else h_tail, C.zipf_slice(oracle, full * chunk, tail, K))
            bound = R.encode_bound(fmt, n, ways, chunk)

            def call(d_out, d_offs, d_lens, sync, d_rows=None):
                if adaptive:
                    return ctx.encode_adaptive(d_syms, ways, chunk, sb, sync=sync, fmt=fmt, d_out=d_out, d_offsets=d_offs,
                                               d_lengths=d_lens, d_freqs=d_rows)[4]
                return ctx.encode(gm, d_syms, ways, chunk, d_out=d_out, sync=sync, d_offsets=d_offs, d_lengths=d_lens)[3]

            def run(cap, sync=True):
                return Run(R, torch, nchunks, cap, call, sync=sync, rows=adaptive)

            # the ample run: against the oracle, once
            ample = run(bound)
            what = (case.id, label, "ample")
            assert ample.status == R.OK, what
            is_the_rows(what)
            ample.assert_guards(what)
            offs, lens = ample.host_index()
            T, E = C.total(lens), C.aligned_end(lens)
            assert np.array_equal(offs, C.ref_offsets(lens)) and ample.total == T == int(offs[nchunks]), what
            assert T % 16 == residue, (what, T, "the tail does not give the residue the table claims")
            if adaptive:
                h_rows = ample.d_rows.cpu().numpy()
                count, bad = oracle.compare_container_adaptive(fmt, d_syms.cpu().numpy(), ways, chunk, sb, ample.d_out[:T].cpu().numpy(),
                                                               offs, lens, h_rows)
                assert count == nchunks and bad == -1, (what, bad)
            else:
                art = {"fmt": fmt, "sb": sb, "K": K, "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms,
                       "cont": ample.d_out, "offs": ample.d_offs, "lens": ample.d_lens, "total": T}
                assert bench.oracle_check_chunks(art) == nchunks, what
            mask = C.stream_mask(torch, offs[:nchunks], lens, E, "cuda")
            assert int(mask.sum()) == int(lens.astype(np.int64).sum())

            def assert_as_ample(r, what):
                assert r.status == R.OK and r.total == T, (what, r.status, r.total, T)
                assert torch.equal(r.d_offs, ample.d_offs) and torch.equal(r.d_lens, ample.d_lens), what
                assert same_stream_bytes(torch, r.d_out, ample.d_out, mask, E), (what, "stream bytes differ from the ample run's")
                if adaptive:
                    assert torch.equal(r.d_rows, ample.d_rows), what
                is_the_rows(what)

            caps = C.caps_for(lens, bound)
            assert any(T <= cap < E for _, cap, _ in caps) == (residue != 0)
            failed = 0
            for cap_label, cap, fits in caps:
                what = (case.id, label, "out_cap = " + cap_label, cap, "T", T, "E", E)
                assert cap <= bound
                r = run(cap)
                r.assert_guards(what)
                if fits:
                    assert_as_ample(r, what)
                else:
                    failed += 1
                    assert r.status == R.E_SPACE, (what, "status", r.status)
                    # (a placement wave that waits for something a refused chunk never sends ends at the watchdog's half minute)
                    assert r.seconds < STALL_SECONDS, (what, "the refused call took", r.seconds, "s")
                    assert int(r.d_offs[nchunks].item()) == T, (what, "d_offsets[n_chunks] is how a caller learns what to allocate")
                    if not async_done and T - 1 <= cap < E:  # the asynchronous form, once per row, at the edge itself
                        a = run(cap, sync=False)
                        with pytest.raises(R.RansAmdError) as e:
                            ctx.encode_status()
                        assert e.value.status == R.E_SPACE, (what, "encode_status", e.value.status)
                        a.assert_guards(what + ("asynchronous",))
                        # (a.status says only that the launch call returned: the verdict is what encode_status() raised above)
                        assert a.status == R.OK and int(a.d_offs[nchunks].item()) == T, what
                        async_done = True
            assert failed >= 4
            # a healthy call on the same context: flags, status words and claim counters of the failed launches did not leak
            again = run(bound)
            what = (case.id, label, "ample call behind the failed ones")
            again.assert_guards(what)
            assert_as_ample(again, what)
            ctx.encode_status()
        assert async_done
    finally:
        ctx.close()


# ---- per-chunk models in one kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in C.CASES if C.is_adaptive(c)], ids=[c.id for c in C.CASES if C.is_adaptive(c)])
def test_adaptive_sized_capacity(gpu, oracle, case):
    """rans_amd_encode_adaptive_sized.  The piece sizes are the kernel's own (tests/test_gpu_model_extremes.py pins them): the
    reference for the cap is the total P the ample run reported, a multiple of 64.  out_cap = P: OK and index, rows and bytes
    as the ample run's; P - 1 and P - 64: E_SPACE, a chunk with d_lengths[c] != 0 lies where the ample run put it with the
    same bytes, a chunk with d_lengths[c] == 0 left its piece poison, nothing at or behind out_cap is written; then a
    healthy call."""
    import bench
    R, torch, cus = gpu
    row = C.row_of(case)
    fmt, sb, ways, chunk = row["fmt"], row["sb"], row["ways"], row["chunk"]
    full = C.full_chunks(case, cus)
    nchunks = full + 1
    n = full * chunk + C.tails_for(oracle, case, cus)[0]
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    ctx = R.Context(0)
    try:
        def call(d_out, d_offs, d_lens, sync, d_rows):
            return ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt, d_out=d_out, sync=sync, d_offsets=d_offs, d_lengths=d_lens,
                                             d_freqs=d_rows)[4]

        def run(cap):
            return Run(R, torch, nchunks, cap, call, rows=True)

        bound = int(R.lib().rans_amd_encode_adaptive_sized_bound(fmt, n, ways, chunk))
        ample = run(bound)
        assert ample.status == R.OK and ctx.last_encode_kernel()[0] == row["sized"], ctx.last_encode_kernel()
        ample.assert_guards((case.id, "ample"))
        offs, lens = ample.host_index()
        P = ample.total
        ends = offs[:nchunks] + lens
        starts = np.concatenate([[np.uint64(0)], ends[:-1]])  # chunk c's piece: [the end of the piece before it, its own end)
        assert P % 64 == 0 and int(ends[-1]) == P == int(offs[nchunks]) and np.all(ends % np.uint64(64) == 0) and P <= bound
        count, bad = oracle.compare_container_adaptive(fmt, d_syms.cpu().numpy(), ways, chunk, sb, ample.d_out[:P].cpu().numpy(), offs, lens,
                                                       ample.d_rows.cpu().numpy())
        assert count == nchunks and bad == -1, bad

        def assert_as_ample(r, what):
            r.assert_guards(what)
            assert r.status == R.OK and r.total == P, (what, r.status, r.total)
            assert torch.equal(r.d_offs, ample.d_offs) and torch.equal(r.d_lens, ample.d_lens) and torch.equal(r.d_rows, ample.d_rows), what
            for c in range(nchunks):
                a, e = int(offs[c]), int(ends[c])
                assert torch.equal(r.d_out[a:e], ample.d_out[a:e]), (what, "chunk", c)
            assert ctx.last_encode_kernel()[0] == row["sized"], what

        assert_as_ample(run(P), (case.id, "out_cap = P", P))
        for cap in (P - 1, P - 64):
            what = (case.id, "out_cap", cap, "P", P)
            r = run(cap)
            r.assert_guards(what)
            assert r.status == R.E_SPACE, (what, r.status)
            g_offs, g_lens = r.host_index()
            dropped = 0
            for c in range(nchunks):
                s, e = int(starts[c]), int(ends[c])
                if g_lens[c] != 0:
                    assert e <= cap and int(g_offs[c]) == int(offs[c]) and int(g_lens[c]) == int(lens[c]), (what, "chunk", c)
                    assert torch.equal(r.d_out[int(offs[c]):e], ample.d_out[int(offs[c]):e]), (what, "chunk", c)
                else:
                    dropped += 1
                    assert e > cap, (what, "chunk", c, "fits and was not coded")
                    assert bool((r.d_out[s:min(e, cap)] == C.POISON).all()), (what, "chunk", c, "has no length and its piece was written")
            assert dropped >= 1, what
        assert_as_ample(run(bound), (case.id, "ample call behind the failed ones"))
        ctx.encode_status()
    finally:
        ctx.close()


# ---- slots ------------------------------------------------------------------------------------------------------------------
SLOT_CASES = ["word-64", "word-8", "word-4"]  # a wave row, the group encoder, a lane row


def static_input(R, torch, oracle, ctx, case, cus):
    import bench
    row = C.row_of(case)
    full = C.full_chunks(case, cus)
    n = full * row["chunk"] + C.tails_for(oracle, case, cus)[0]
    d_syms = bench.gen_zipf(torch, n, row["K"], 1.0, 1, "cuda")
    freqs = C.model_freqs(oracle, case, cus)
    return row, n, full + 1, d_syms, freqs, ctx.model(row["fmt"], freqs, row["sb"])


@pytest.mark.parametrize("cid", SLOT_CASES)
def test_slots_capacity(gpu, oracle, cid):
    """rans_amd_encode_slots.  out_cap = n_chunks * slot exactly: both guards intact (a write in front of slot 0 is what the
    front guard is for), every chunk the oracle's; one byte less: E_SPACE and the whole arena still poison (nothing is
    launched)."""
    import bench
    R, torch, cus = gpu
    case = next(c for c in C.CASES if c.id == cid)
    ctx = R.Context(0)
    try:
        row, n, nchunks, d_syms, freqs, gm = static_input(R, torch, oracle, ctx, case, cus)
        fmt, ways, chunk = row["fmt"], row["ways"], row["chunk"]
        slot = R.slot_bytes(fmt, n, ways, chunk)
        cap = nchunks * slot
        assert cap == R.encode_slots_bound(fmt, n, ways, chunk)

        def call(d_out, d_offs, d_lens, sync):
            return ctx.encode_slots(gm, d_syms, ways, chunk, d_out=d_out, sync=sync, d_offsets=d_offs, d_lengths=d_lens)[3]

        r = Run(R, torch, nchunks, cap, call)
        what = (cid, "out_cap = n_chunks * slot", cap)
        assert r.status == R.OK and r.total == cap, what
        assert (ctx.last_encode_kernel()[0], ctx.last_encode_placement()) == C.pick(row["slots"], case.regime), ctx.last_encode_kernel()
        r.assert_guards(what)
        art = {"fmt": fmt, "sb": row["sb"], "K": row["K"], "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms,
               "cont": r.d_out, "offs": r.d_offs, "lens": r.d_lens, "total": cap, "slot": slot}
        assert bench.oracle_check_chunks(art) == nchunks
        less = Run(R, torch, nchunks, cap - 1, call)
        assert less.status == R.E_SPACE, (cid, less.status)
        assert bool((less.whole == C.POISON).all()), "E_SPACE up front, and the arena was written"
        assert bool((less.offs_whole == C.SENTINEL).all()) and bool((less.lens_whole == C.SENTINEL).all())
        again = Run(R, torch, nchunks, cap, call)
        again.assert_guards((cid, "behind the refused call"))
        assert again.status == R.OK and torch.equal(again.d_offs, r.d_offs) and torch.equal(again.d_lens, r.d_lens)
        # (what a slot holds in front of its stream is unspecified -- the group encoder stores whole lines -- so: the oracle again)
        assert bench.oracle_check_chunks(dict(art, cont=again.d_out, offs=again.d_offs, lens=again.d_lens)) == nchunks
    finally:
        ctx.close()


def test_sized_slots_capacity(gpu, oracle):
    """rans_amd_encode_slots_sized at out_cap = rans_amd_encode_sized_bound(.., room) exactly, room taken from a first run (as
    tests/test_gpu_wave_extremes.py section d does, which also pins the verdict at room - 1): slots of half the tight size,
    so that chunks overflow into the region that ends at out_cap."""
    import bench
    R, torch, cus = gpu
    case = next(c for c in C.CASES if c.id == "word-64")
    ctx = R.Context(0)
    try:
        row, n, nchunks, d_syms, freqs, gm = static_input(R, torch, oracle, ctx, case, cus)
        fmt, ways, chunk = row["fmt"], row["ways"], row["chunk"]
        worst = R.slot_bytes(fmt, n, ways, chunk)
        slot = max(64, (ctx.tight_slot_bytes(gm, ways, chunk) // 2) & ~63)
        assert slot < worst
        _, f_offs, _, _, _ = ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, overflow_chunks=nchunks)
        room = int((f_offs.cpu().numpy()[:nchunks].astype(np.int64) >= nchunks * slot).sum())
        assert 1 <= room <= nchunks
        cap = R.encode_sized_bound(fmt, n, ways, chunk, slot, room)
        assert cap == nchunks * slot + room * worst

        def call(d_out, d_offs, d_lens, sync):
            return ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, d_out=d_out, sync=sync, d_offsets=d_offs, d_lengths=d_lens)[3]

        r = Run(R, torch, nchunks, cap, call)
        what = ("sized slots, out_cap = the bound for exactly the chunks that overflow", cap, room)
        assert r.status == R.OK and r.total == cap, (what, r.status, r.total)
        assert (ctx.last_encode_kernel()[0], ctx.last_encode_placement()) == C.pick(row["sized"], case.regime)
        r.assert_guards(what)
        art = {"fmt": fmt, "sb": row["sb"], "K": row["K"], "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms,
               "cont": r.d_out, "offs": r.d_offs, "lens": r.d_lens, "total": cap, "slot": slot, "worst": worst}
        assert bench.oracle_check_chunks(art) == nchunks
    finally:
        ctx.close()


# ---- rans_amd_container_compact -------------------------------------------------------------------------------------------
def test_container_compact_capacity(gpu):
    """dst_cap = T with T % 16 != 0: E_SPACE, nothing copied, the offsets complete; dst_cap = E: OK, nothing behind it."""
    R, torch, cus = gpu
    lens = np.array([33, 64, 31], dtype=np.uint32)
    from_ = np.array([5, 100, 200], dtype=np.uint64)
    src = np.random.default_rng(7).integers(0, 256, size=256, dtype=np.uint8)
    T, E = C.total(lens), C.aligned_end(lens)
    assert (T, E) == (143, 144)
    d_src = torch.from_numpy(src).cuda()
    d_from = torch.from_numpy(from_.astype(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    ctx = R.Context(0)
    try:
        for cap, fits in ((T, False), (E, True)):
            whole, dst = C.arena(torch, cap)
            offs_whole, d_offs = C.index_arena(torch, 4, torch.int64)
            status, total = R.OK, None
            try:
                _, _, total = ctx.compact(d_src, src.size, d_from, d_lens, 3, d_dst=dst, d_dst_offsets=d_offs)
            except R.RansAmdError as e:
                status = e.status
            assert C.guards_intact(whole, dst, C.POISON) and C.guards_intact(offs_whole, d_offs, C.SENTINEL), cap
            assert np.array_equal(d_offs.cpu().numpy().astype(np.uint64), C.ref_offsets(lens)), cap
            if fits:
                assert status == R.OK and total == T
                got = dst.cpu().numpy()
                for c, o in enumerate(C.ref_offsets(lens)[:3]):
                    assert np.array_equal(got[int(o):int(o) + int(lens[c])], src[int(from_[c]):int(from_[c]) + int(lens[c])]), c
            else:
                assert status == R.E_SPACE, status
                assert bool((whole == C.POISON).all()), "E_SPACE, and the destination was written"
    finally:
        ctx.close()
