"""The kernels AROUND every coder call at their edges: the offset scan (k_layout_sums, k_layout), the compaction (k_compact,
k_compact_small), the whole-input histogram (k_histogram_u8, k_histogram_u16, k_zero before them) and the order of a
ragged batch (k_order_hist, k_order_scan, k_order_scatter).  They build every model and every compact index and move every
compressed byte; the rest of the suite sees them on well-behaved inputs only.

tests/_around_coders.py holds the references (numpy, integers only) and the case tables, tests/test_around_coders_cpu.py
proves without a GPU that the tables reach what they claim and that every compaction case lands on its kernel.  Every
comparison here is exact -- against numpy on the host, against torch indexing on the device where gigabytes are compared.
No case is meant to fault: every input is valid or cleanly rejected.

  layout      through ctx.compact with an explicit d_dst_offsets.  nchunks 0 .. 1025 * 8192 + 9 (the first size at which the
              carry loop of k_layout takes a second trip), lengths all 0 / all 1 / c % 33 (the copy runs, exact fit and 16
              bytes less) and all 0xFFFFFFFF / random u32 / one 0xFFFFFFF1 among zeros at the first and last chunk of a
              thread, a wave, a block: a 16-byte poisoned destination, RANS_AMD_E_SPACE, the poison intact, the offsets
              complete (include/ryg_rans_amd.h promises both)
  compaction  both kernels: every source phase x every length around the granule, the pass and the kernels' thresholds,
              chunks on the source's last byte (src_limit, load16_below's bytewise tail), length 0, more than one trip over
              the grid, a 1 MiB chunk among short ones; destination offsets, source offsets and one length beyond 32 bits;
              entries outside the source at odd phases.  The source is exactly src_bytes long (src_bytes % 16 == 5), the
              destination a poisoned slice with poison behind it; the up to 15 bytes of padding behind a chunk are
              unspecified and not compared
  histogram   every start phase x every n around one vector, the pipelined loop's steady state (n = 2 T + 53 and 3 T + 53 at
              phase 3), a symbol outside the alphabet in the head, in a second-trip vector, in the tail, alone; a counter at
              2^32 - 1; u16 at every boundary of the copy count and at the ABI's largest alphabet; k_zero's 16-byte body
              plus 4-byte tail on the shared workspace
  order       n around the 2048-stream tile, one bucket for all (every block on one cursor), both sides of every key's
              boundary, one stream per bucket; two calls in a row; n = 0

What the cases are tight against, by reading the kernels (no mutated kernel was built or run); each of these passes the
suite as it was before this file:
  * k_layout: the carry loop as one trip (`if (threadIdx.x < blockIdx.x)` for the `for`): spike@8388608 -- the sum of block
    1024, which only thread 0 of block 1025 reads, in its second trip -- and every other class at 1025 * 8192 + 9 chunks.
    `mine` or the wave scan's `v` in 32 bits: all_ff (2^35 per thread) and every spike (2^32 in one thread) wrap to 0.
    The spikes at the first and last chunk of a thread, a wave and a block put one large term where a carry added to the
    wrong neighbour shows in every offset behind it.
  * k_compact: funnel16<DSH> picked one instance too low: every phase >= 4 of phases-wave; bsh taken from the wrong
    address: every phase that is no multiple of 4 (the old suite's sources all start on a granule: dsh = bsh = 0).  The
    src_limit guard one granule too strict: the chunks that end on the source's last byte at phases 5..15, whose last piece
    straddles the source's last two granules, get zeros for real bytes.  The guard DROPPED is not visible in bytes: what
    b then holds is shifted in behind the chunk's end; the guard protects the read, not the result.
  * k_compact_small: the high half of `off` not shuffled: (b); of `from`: (c).  The pass loop as one pass: every length
    above 512 of phases-small and the 1 MiB chunk of mixed-small.  load16_below's bytewise tail returning zeros: the chunks
    on the last byte at phases 1..4 of phases-small (their last piece starts in the source's last 4 bytes).  Its `a + b <
    limit` as `<=` is not visible: the byte lies in the padding.
  * both: n16 in 32 bits: (d).  The parent commit fails it -- nothing is copied, the call reports OK; run once on each build.
  * k_histogram_u8: `v = nv` dropped (every thread counts its first vector again for each later one: the sum stays n, which
    is all the 1 GiB tests ask, and the exact 1 MiB test never enters the loop): the steady-state cases with uniform and
    Zipf bytes.  One count4 of the loop's body dropped: the same cases, by exact counts (and by the sum).  Phase x short n:
    head >= n, head only, exactly one vector, a tail -- `n - nhead` and the tail's start off by one vector or one byte.
  * k_histogram_u16: count1's `sym < nsyms` as `<=`: the symbol equal to nsyms is counted into the padding between the
    copies and no error is reported -- every nsyms case.  The launches with 4, 2 and 1 copies and the 65 568-byte LDS request
    at 16384 symbols had never run.  Not visible: `cstride = nsyms` (the copies then share banks, the counts stay exact).
  * k_zero: the 4-byte tail dropped: the residue case (counter 4 of 5 keeps the 16384-symbol call's count).
  * batch_order: the totals not cleared between calls: test_order_two_calls_in_a_row (per_bucket, then all_ff, ..) and every
    test_order case, whose classes follow each other on one context.  The reservation of a block's piece as a read and a
    write instead of an atomicAdd: all_ff from 2049 streams on (every block on the cursor of bucket 32).  Keys by a float
    log2 in the REFERENCE: pow2_edges (2^k - 2, 2^k - 1, 2^k) is checked in integers.
Still invisible: which of the two compaction kernels ran (no name is reported; tests/test_around_coders_cpu.py pins the
rule to the source text and every case to its kernel instead), and the up to 15 padding bytes behind a chunk.

Wall time on an MI355X (256 CUs), one run of this file, 69 cases in 7.1 s, 1.7 s of it the first case's setup (it loads the
kernels).  Per case, seconds:
  test_compact_one_chunk_of_almost_4_gib (d)     1.93   (4 GiB through one wave; the estimate was 4 to 8 s)
  test_layout[8396809]                           0.84   (16 length classes, 67 MB of offsets to the host for each)
  test_histogram_u8_steady_state[2-zipf]         0.43   (the host draws 16.8 M Zipf bytes); [3-uniform] 0.09, [2-uniform]
                                                        0.06, [2-constant] 0.03
  test_compact_source_beyond_4_gib[small] (c)    0.34   (2.1 M chunks checked on the host); [wave] < 0.005, the shared
                                                        4 GiB source is drawn in 0.01
  test_compact[trips-wave] / [trips-small]       0.20 / 0.17
  test_histogram_u8_symbol_outside_the_alphabet  0.17
  test_histogram_u16_two_rounds                  0.16
  test_layout_of_nothing                         0.12   (the first launches of the file)
  test_layout[8191]                              0.09
  test_compact_wave_destination_beyond_4_gib (a) 0.06;  test_compact_small_destination_beyond_4_gib (b) 0.02
  test_histogram_u8_every_phase_and_short_n      0.04   (656 calls);  test_compact[phases-wave] 0.04
  test_compact[mixed-small] 0.02; [mixed-wave], [phases-small], [small-n1 / n63 / n64 / n65], the u16 phases and
  test_histogram_u16_one_counter_of_16384 0.01 each
  every other case (the other test_layout sizes, test_layout_exact_fit, the rejected entries, test_histogram_u16_nsyms,
  test_histogram_u8_counter_ceiling, the residue case, every order case) below 0.005
"""
import numpy as np
import pytest

import _around_coders as A
from _around_coders import GUARD, POISON

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def cus_of(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(torch, a, dtype):
    """A numpy index array on the device, reinterpreted as the signed type torch has."""
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def dev_lens(torch, lens):
    return torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda()


def poisoned(torch, cap):
    """A destination of exactly `cap` bytes (at least one granule) as a slice of a poisoned tensor: -> (whole, slice)."""
    cap = max(int(cap), 16)
    whole = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole, whole[:cap]


def run_compact(gpu, d_src, src_bytes, from_, lens, cap=None):
    """ctx.compact into an exactly fitting poisoned destination -> (whole, cap, d_offsets, total)."""
    R, ctx, torch = gpu
    n = len(lens)
    cap = A.aligned_total(lens) if cap is None else cap
    whole, dst = poisoned(torch, cap)
    d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    _, _, total = ctx.compact(d_src, src_bytes, dev(torch, from_, np.int64), dev_lens(torch, lens), n, d_dst=dst, d_dst_offsets=d_offs)
    return whole, dst.numel(), d_offs, total


def check_offsets(d_offs, total, lens):
    want = A.ref_offsets(lens)
    got = d_offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), "offsets differ first at chunk %d" % int(np.argmax(got != want))
    assert total is None or total == int(want[-1])
    return want


def check_chunks(got, h_src, from_, lens, offs, skip=()):
    """Every chunk's bytes in the host copy `got` of the destination against the source."""
    if len(lens) <= 5000:
        for c, want in enumerate(A.ref_compact(h_src, from_, lens)):
            if c not in skip:
                a = int(offs[c])
                assert np.array_equal(got[a:a + want.size], want), "chunk %d (from %d, %d bytes)" % (c, int(from_[c]), want.size)
        return
    assert not skip
    want, have = A.ref_compact_flat(h_src, from_, lens), got[A.flat_index(offs[:-1], lens)]
    if not np.array_equal(want, have):
        at = int(np.argmax(want != have))
        c = int(np.searchsorted(np.cumsum(np.asarray(lens, dtype=np.int64)), at, side="right"))
        raise AssertionError("chunk %d (from %d, %d bytes) differs" % (c, int(from_[c]), int(lens[c])))


# ---------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------

def test_layout_of_nothing(gpu):
    """nchunks == 0: no error, offsets[0] == 0, total 0, no source needed, the destination untouched."""
    R, ctx, torch = gpu
    whole, dst = poisoned(torch, 16)
    d_offs = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    nothing8, nothing32, nothing64 = (torch.empty(0, dtype=t, device="cuda") for t in (torch.uint8, torch.int32, torch.int64))
    assert nothing8.data_ptr() == 0
    _, _, total = ctx.compact(nothing8, 0, nothing64, nothing32, 0, d_dst=dst, d_dst_offsets=d_offs)
    assert total == 0 and d_offs.tolist() == [0]
    assert bool((whole == POISON).all())


@pytest.mark.parametrize("n", [n for n in A.LAYOUT_NCHUNKS if n])
def test_layout(gpu, n):
    R, ctx, torch = gpu
    h_src = A.source_bytes(A.LAYOUT_SRC_BYTES, 3)
    d_src = torch.from_numpy(h_src).cuda()
    d_from = dev(torch, A.layout_from(n), np.int64)
    for name in A.layout_classes(n):
        lens = A.layout_lengths(name, n)
        d_lens = dev_lens(torch, lens)
        d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        if A.layout_is_big(name):
            # the sum fits no destination: one poisoned granule, RANS_AMD_E_SPACE, nothing copied, the offsets complete
            whole, dst = poisoned(torch, 16)
            with pytest.raises(R.RansAmdError) as e:
                ctx.compact(d_src, A.LAYOUT_SRC_BYTES, d_from, d_lens, n, d_dst=dst, d_dst_offsets=d_offs)
            assert e.value.status == R.E_SPACE, (n, name)
            assert bool((whole == POISON).all()), (n, name, "the destination was written")
            check_offsets(d_offs, None, lens)
            continue
        cap = A.aligned_total(lens)
        whole, dst = poisoned(torch, cap)
        _, _, total = ctx.compact(d_src, A.LAYOUT_SRC_BYTES, d_from, d_lens, n, d_dst=dst, d_dst_offsets=d_offs)
        offs = check_offsets(d_offs, total, lens)
        assert bool((whole[dst.numel():] == POISON).all()), (n, name, "written behind dst_cap")
        if n <= 16385:
            check_chunks(whole.cpu().numpy(), h_src, A.layout_from(n), lens, offs)
        del whole, dst


@pytest.mark.parametrize("n", [513, 8193])
def test_layout_exact_fit(gpu, n):
    """dst_cap == the aligned total succeeds (test_layout runs every small class that way); 16 bytes less is
    RANS_AMD_E_SPACE with the destination untouched and the offsets complete."""
    R, ctx, torch = gpu
    h_src = A.source_bytes(A.LAYOUT_SRC_BYTES, 3)
    d_src = torch.from_numpy(h_src).cuda()
    for name in ("ones", "mod33"):
        lens = A.layout_lengths(name, n)
        cap = A.aligned_total(lens)
        whole, cap_used, d_offs, total = run_compact(gpu, d_src, A.LAYOUT_SRC_BYTES, A.layout_from(n), lens)
        assert cap_used == cap
        offs = check_offsets(d_offs, total, lens)
        got = whole.cpu().numpy()
        assert np.all(got[cap:] == POISON)
        check_chunks(got, h_src, A.layout_from(n), lens, offs)
        whole, dst = poisoned(torch, cap - 16)
        d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        with pytest.raises(R.RansAmdError) as e:
            ctx.compact(d_src, A.LAYOUT_SRC_BYTES, dev(torch, A.layout_from(n), np.int64), dev_lens(torch, lens), n, d_dst=dst,
                        d_dst_offsets=d_offs)
        assert e.value.status == R.E_SPACE and dst.numel() == cap - 16
        assert bool((whole == POISON).all()), "the destination was written"
        check_offsets(d_offs, None, lens)


# ---------------------------------------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------------------------------------
CASE_NAMES = [c.name for c in A.compact_cases(1)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_compact(gpu, name):
    R, ctx, torch = gpu
    case = {c.name: c for c in A.compact_cases(cus_of(torch))}[name]
    assert A.compact_kernel(case.src_bytes, case.lens.size) == case.kernel
    h_src = A.source_bytes(case.src_bytes, case.seed)
    d_src = torch.from_numpy(h_src).cuda()  # exactly src_bytes long
    assert d_src.numel() == case.src_bytes and case.src_bytes % 16 == 5
    whole, cap, d_offs, total = run_compact(gpu, d_src, case.src_bytes, case.from_, case.lens)
    offs = check_offsets(d_offs, total, case.lens)
    got = whole.cpu().numpy()
    assert np.all(got[cap:] == POISON), "written behind dst_cap"
    check_chunks(got, h_src, case.from_, case.lens, offs)


@pytest.mark.parametrize("kernel", ["wave", "small"])
def test_compact_rejects_at_odd_phases(gpu, kernel):
    """from + len == src_bytes + 1 at an odd phase: RANS_AMD_E_CORRUPT, that chunk neither read nor written, the others
    copied; from == src_bytes with len == 0 lies inside the source and is accepted."""
    R, ctx, torch = gpu
    src_bytes, from_, lens, victims = A.reject_cases(kernel)
    h_src = A.source_bytes(src_bytes, 70)
    d_src = torch.from_numpy(h_src).cuda()
    for victim, f, ln, accepted in victims:
        f2, l2 = from_.copy(), lens.copy()
        f2[victim], l2[victim] = f, ln
        if accepted:
            whole, cap, d_offs, total = run_compact(gpu, d_src, src_bytes, f2, l2)
        else:
            whole, dst = poisoned(torch, A.aligned_total(l2))
            cap = dst.numel()
            d_offs = torch.full((l2.size + 1,), -1, dtype=torch.int64, device="cuda")
            with pytest.raises(R.RansAmdError) as e:
                ctx.compact(d_src, src_bytes, dev(torch, f2, np.int64), dev_lens(torch, l2), l2.size, d_dst=dst, d_dst_offsets=d_offs)
            assert e.value.status == R.E_CORRUPT
            total = None
        offs = check_offsets(d_offs, total, l2)
        got = whole.cpu().numpy()
        assert np.all(got[cap:] == POISON)
        check_chunks(got, h_src, f2, l2, offs, skip=() if accepted else (victim,))
        if not accepted:
            a = int(offs[victim])
            assert np.all(got[a:a + A.align16(ln)] == POISON), "the rejected chunk was written"


def equal_in_pieces(torch, a, b, piece=256 << 20):
    """torch.equal over two flat views of the same length without a temporary of their size."""
    assert a.numel() == b.numel()
    return all(torch.equal(a[i:i + piece], b[i:i + piece]) for i in range(0, a.numel(), piece))


def test_compact_wave_destination_beyond_4_gib(gpu):
    """(a) 66 chunks of 64 MiB + 16 k from 66 places of an 80 MiB source: the last two start above 2^32 in the destination."""
    R, ctx, torch = gpu
    from_, lens = A.big_a()
    g = torch.Generator(device="cuda").manual_seed(11)
    d_src = torch.randint(0, 256, (A.BIG_A_SRC,), dtype=torch.uint8, device="cuda", generator=g)
    whole, cap, d_offs, total = run_compact(gpu, d_src, A.BIG_A_SRC, from_, lens)
    offs = check_offsets(d_offs, total, lens)
    assert int(offs[-2]) > 1 << 32
    assert bool((whole[cap:] == POISON).all())
    for c in range(lens.size):
        a, f, ln = int(offs[c]), int(from_[c]), int(lens[c])
        assert torch.equal(whole[a:a + ln], d_src[f:f + ln]), c


def test_compact_small_destination_beyond_4_gib(gpu):
    """(b) 8192 chunks of 520 KiB + 7 through k_compact_small, from = 37 k: 4.06 GiB; the rows are src.unfold(0, L, 37)."""
    R, ctx, torch = gpu
    from_, lens = A.big_b()
    g = torch.Generator(device="cuda").manual_seed(12)
    d_src = torch.randint(0, 256, (A.BIG_B_SRC,), dtype=torch.uint8, device="cuda", generator=g)
    whole, cap, d_offs, total = run_compact(gpu, d_src, A.BIG_B_SRC, from_, lens)
    offs = check_offsets(d_offs, total, lens)
    assert int(offs[-2]) > 1 << 32
    assert bool((whole[cap:] == POISON).all())
    pitch = A.align16(A.BIG_B_LEN)
    assert cap == A.BIG_B_N * pitch
    rows = whole[:cap].view(A.BIG_B_N, pitch)[:, :A.BIG_B_LEN]
    want = d_src.unfold(0, A.BIG_B_LEN, A.BIG_B_STEP)[:A.BIG_B_N]
    for r in range(0, A.BIG_B_N, 256):
        assert torch.equal(rows[r:r + 256], want[r:r + 256]), "rows %d .. %d" % (r, r + 255)


@pytest.fixture(scope="module")
def big_src(gpu):
    """4 GiB + 1 MiB + 5 random bytes on the device, shared by (c) and (d) and never written; the host keeps the first and
    the last MiB."""
    R, ctx, torch = gpu
    g = torch.Generator(device="cuda").manual_seed(13)
    d_src = torch.empty(A.BIG_SRC, dtype=torch.uint8, device="cuda")
    for i in range(0, A.BIG_SRC, 1 << 30):
        part = d_src[i:i + (1 << 30)]
        part.copy_(torch.randint(0, 256, (part.numel(),), dtype=torch.uint8, device="cuda", generator=g))
    ends = torch.cat([d_src[:A.MIB], d_src[A.BIG_SRC - A.MIB:]]).cpu().numpy()
    yield d_src, ends
    del d_src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", ["wave", "small"])
def test_compact_source_beyond_4_gib(gpu, big_src, kernel):
    """(c) chunks in the first and in the last MiB of a 4 GiB + 1 MiB source, the last one on its last byte."""
    R, ctx, torch = gpu
    d_src, ends = big_src
    from_, lens = A.big_c(kernel)
    assert A.compact_kernel(A.BIG_SRC, lens.size) == kernel
    whole, cap, d_offs, total = run_compact(gpu, d_src, A.BIG_SRC, from_, lens)
    offs = check_offsets(d_offs, total, lens)
    got = whole.cpu().numpy()
    assert np.all(got[cap:] == POISON)
    check_chunks(got, ends, A.big_c_local(from_), lens, offs)


def test_compact_one_chunk_of_almost_4_gib(gpu, big_src):
    """(d) one chunk of 2^32 - 8 bytes at from = 3: len + 15 wraps in 32 bits, and the chunk must arrive whole (before the
    64-bit sum in both compaction kernels nothing was copied and the call reported OK).  4 GiB through one wave."""
    R, ctx, torch = gpu
    d_src, _ = big_src
    f, ln = A.BIG_D_FROM, A.BIG_D_LEN
    from_, lens = np.array([f], dtype=np.uint64), np.array([ln], dtype=np.uint32)
    whole, cap, d_offs, total = run_compact(gpu, d_src, A.BIG_SRC, from_, lens)
    check_offsets(d_offs, total, lens)
    assert total == ln and cap == 1 << 32
    assert bool((whole[cap:] == POISON).all())
    tail = 64 << 10
    assert torch.equal(whole[ln - tail:ln], d_src[f + ln - tail:f + ln]), "the last 64 KiB"
    assert torch.equal(whole[:ln:65521], d_src[f:f + ln:65521]), "a strided sample"
    assert equal_in_pieces(torch, whole[:ln], d_src[f:f + ln])


# ---------------------------------------------------------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------------------------------------------------------

def placed(torch, h_syms, phase):
    """The symbols `phase` elements behind a 16-byte aligned address, poison around them."""
    t_dtype = torch.uint8 if h_syms.dtype == np.uint8 else torch.int16
    big = torch.full((h_syms.size + 64,), 0x6E, dtype=t_dtype, device="cuda")
    view = big[phase:phase + h_syms.size]
    view.copy_(torch.from_numpy(h_syms.view(np.uint8 if h_syms.dtype == np.uint8 else np.int16)))
    assert big.data_ptr() % 16 == 0 and view.numel() == h_syms.size
    return view


def check_hist(gpu, view, h_syms, nsyms, what):
    R, ctx, torch = gpu
    want = A.ref_hist(h_syms, nsyms)
    if isinstance(want, str):
        with pytest.raises(R.RansAmdError) as e:
            ctx.count_freqs_device(view, nsyms)
        assert e.value.status == R.E_ARG, what
        return
    got = ctx.count_freqs_device(view, nsyms).astype(np.int64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d counters differ, first %d: %d for %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]]))


def test_histogram_u8_every_phase_and_short_n(gpu):
    R, ctx, torch = gpu
    h = A.hist_data("uniform", 64 + 40, 21)
    big = placed(torch, h, 0)
    for ph in A.U8_PHASES:
        for n in A.U8_NS:
            view = big[ph:ph + n]
            assert n == 0 or view.data_ptr() % 16 == ph
            check_hist(gpu, view, h[ph:ph + n], 256, "phase %d, n %d" % (ph, n))


@pytest.mark.parametrize("rounds,name", [(2, "uniform"), (2, "zipf"), (2, "constant"), (3, "uniform")])
def test_histogram_u8_steady_state(gpu, rounds, name):
    """n = rounds * T + 53 at phase 3: the pipelined loop's body runs (rounds 3: twice in every thread), then a ragged tail."""
    R, ctx, torch = gpu
    n = rounds * A.hist_t8(cus_of(torch)) + 53
    h = A.hist_data(name, n, 22)
    check_hist(gpu, placed(torch, h, 3), h, 256, "%s, n %d" % (name, n))


def test_histogram_u8_symbol_outside_the_alphabet(gpu):
    """nsyms 200, one symbol >= 200 in the head bytes only, in a vector of the second trip only, in the tail only, alone:
    RANS_AMD_E_ARG each time, and the good call right behind is exact."""
    R, ctx, torch = gpu
    stride = 8 * cus_of(torch) * 256
    n = 2 * A.hist_t8(cus_of(torch)) + 53
    good = A.hist_data("uniform", n, 23, nsyms=200)
    d_good = placed(torch, good, 3)
    head = 13
    for what, at in (("head", 5), ("second trip", head + (stride + 7) * 16 + 9), ("tail", n - 1)):
        assert at < n and (what != "head" or at < head) and (what != "tail" or at >= head + (n - head) // 16 * 16)
        bad = good.copy()
        bad[at] = 233
        check_hist(gpu, placed(torch, bad, 3), bad, 200, what)
        check_hist(gpu, d_good, good, 200, "the good call behind " + what)
    alone = np.array([200], dtype=np.uint8)
    for ph in (0, 3):
        check_hist(gpu, placed(torch, alone, ph), alone, 200, "alone")
        check_hist(gpu, d_good, good, 200, "the good call behind the lone symbol")


def test_histogram_u8_counter_ceiling(gpu):
    """2^32 - 1 symbols of one value: the last size the entry point accepts, the counter's last value."""
    R, ctx, torch = gpu
    n = (1 << 32) - 1
    d = torch.full((n,), 0xA7, dtype=torch.uint8, device="cuda")
    got = ctx.count_freqs_device(d, 256)
    assert int(got[0xA7]) == 4294967295 and int(got.astype(np.uint64).sum()) == n
    del d
    torch.cuda.empty_cache()


def test_histogram_u16_every_phase_and_short_n(gpu):
    R, ctx, torch = gpu
    h = A.hist_data("uniform", 64, 24, nsyms=4096, dtype=np.uint16)
    big = placed(torch, h, 0)
    for ph in A.U16_PHASES:
        for n in A.U16_NS:
            view = big[ph:ph + n]
            assert n == 0 or view.data_ptr() % 16 == 2 * ph
            check_hist(gpu, view, h[ph:ph + n], 4096, "phase %d, n %d" % (ph, n))


def test_histogram_u16_two_rounds(gpu):
    R, ctx, torch = gpu
    n = 2 * A.hist_t16(cus_of(torch)) + 21
    for name in ("uniform", "zipf"):
        h = A.hist_data(name, n, 25, nsyms=4096, dtype=np.uint16)
        check_hist(gpu, placed(torch, h, 3), h, 4096, "%s, n %d" % (name, n))


@pytest.mark.parametrize("nsyms", A.U16_NSYMS)
def test_histogram_u16_nsyms(gpu, nsyms):
    """Every symbol present, the last one a quarter of the input; then one symbol == nsyms: rejected."""
    R, ctx, torch = gpu
    h = A.u16_nsyms_input(nsyms, 100 + nsyms)
    check_hist(gpu, placed(torch, h, 1), h, nsyms, "nsyms %d" % nsyms)
    bad = h.copy()
    bad[bad.size // 3] = nsyms
    check_hist(gpu, placed(torch, bad, 1), bad, nsyms, "nsyms %d, one symbol outside" % nsyms)
    check_hist(gpu, placed(torch, h, 0), h, nsyms, "nsyms %d, the good call behind" % nsyms)


def test_histogram_u16_one_counter_of_16384(gpu):
    """nsyms 16384 (65 568 bytes of LDS), 2^22 times one symbol: every lane of every wave on one counter."""
    R, ctx, torch = gpu
    for sym in (16383, 0):
        h = np.full(1 << 22, sym, dtype=np.uint16)
        check_hist(gpu, placed(torch, h, 0), h, 16384, "constant %d" % sym)


def test_histogram_workspace_residue(gpu):
    """16384 counters all non-zero, then 5 counters on the same workspace: k_zero's 16-byte body and 4-byte tail."""
    R, ctx, torch = gpu
    full = A.u16_nsyms_input(16384, 31)
    d_full = placed(torch, full, 0)
    for dtype in (np.uint8, np.uint16):
        check_hist(gpu, d_full, full, 16384, "every counter")
        h = A.hist_data("uniform", 1000, 32, nsyms=5, dtype=dtype)
        check_hist(gpu, placed(torch, h, 0), h, 5, "5 counters behind 16384")


# ---------------------------------------------------------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------------------------------------------------------

def run_order(gpu, counts):
    R, ctx, torch = gpu
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    whole = torch.full((counts.size + 64,), -1, dtype=torch.int32, device="cuda")
    order = ctx.batch_order(d_counts, d_order=whole[:counts.size])
    got = whole.cpu().numpy()
    assert np.all(got[counts.size:] == -1), "written behind the order"
    return A.check_order(order.cpu().numpy().view(np.uint32), counts)


@pytest.mark.parametrize("n", A.ORDER_NS)
def test_order(gpu, n):
    for name in A.ORDER_CLASSES:
        counts = A.order_counts(name, n)
        keys = run_order(gpu, counts)
        assert sorted(keys.tolist(), reverse=True) == keys.tolist()
        if name == "per_bucket" and n >= 33:
            assert set(keys.tolist()) == set(range(33))


def test_order_two_calls_in_a_row(gpu):
    """The workspace (33 totals, 33 cursors) starts clean each time: every bucket used, then one bucket for all, then
    every bucket again."""
    for name, n in (("per_bucket", 4097), ("all_ff", 2049), ("pow2_edges", 4097), ("zeros", 257), ("log_uniform", 3 * 2048)):
        run_order(gpu, A.order_counts(name, n, seed=1))


def test_order_of_nothing(gpu):
    R, ctx, torch = gpu
    whole = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    order = ctx.batch_order(torch.empty(0, dtype=torch.int32, device="cuda"), d_order=whole)
    assert order.numel() == 0 and bool((whole == -1).all())
