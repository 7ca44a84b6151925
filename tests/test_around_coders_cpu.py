"""The kernels around the coders (tests/test_gpu_around_coders.py), the part that needs no GPU: the references of
tests/_around_coders.py against the library's host entry points and the oracle, the proof that the case tables cover what
they claim, and the kernel-choice rule pinned to the source text -- if the rule moves, the GPU cases must not silently all
land on one compaction kernel."""
import os
import re

import numpy as np
import pytest

import _around_coders as A
import ryg_rans_amd as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ryg_rans_amd", "csrc")
CUS_TRIED = (4, 104, 256, 304)


@pytest.mark.parametrize("n", A.LAYOUT_NCHUNKS)
def test_ref_offsets_is_the_host_entry_point(n):
    if n == 0:
        assert A.ref_offsets(np.zeros(0, dtype=np.uint32)).tolist() == [0]
        assert R.offsets_from_lengths(np.zeros(0, dtype=np.uint32)).tolist() == [0]
        return
    names = A.layout_classes(n)
    assert set(A.LAYOUT_SMALL + A.LAYOUT_BIG) <= set(names) and "spike@%d" % (n - 1) in names
    for name in names:
        lens = A.layout_lengths(name, n)
        assert lens.dtype == np.uint32 and lens.size == n
        want = A.ref_offsets(lens)
        assert np.array_equal(want, R.offsets_from_lengths(lens)), (n, name)
        if A.layout_is_big(name):  # no 16-byte destination holds it: the GPU case must end in RANS_AMD_E_SPACE
            assert A.aligned_total(lens) > 16, (n, name)
        else:
            assert int(lens.max()) + 4 <= A.LAYOUT_SRC_BYTES - 1
    # plain Python on one vector, the arithmetic spelled out
    lens = A.layout_lengths("random", n)[:1000]
    at, want = 0, []
    for v in lens.tolist():
        want.append(at)
        at += (v + 15) & ~15
    want.append(want[-1] + int(lens[-1]))
    assert A.ref_offsets(lens).tolist() == want


def test_layout_table_reaches_the_carry_loops_second_trip():
    n = max(A.LAYOUT_NCHUNKS)
    blocks = (n + A.LAYOUT_PER_BLOCK - 1) // A.LAYOUT_PER_BLOCK
    assert blocks - 1 > 1024, "no block whose carry loop (b = threadIdx.x; b < blockIdx.x; b += 1024) takes a second trip"
    assert (n - 9 + A.LAYOUT_PER_BLOCK - 1) // A.LAYOUT_PER_BLOCK - 1 == 1024, "9 chunks fewer and no block takes it"
    assert n == 1025 * 8192 + 9
    pos = A.spike_positions(n)
    assert A.LAYOUT_CARRY_TRIP in pos and A.LAYOUT_CARRY_TRIP // A.LAYOUT_PER_BLOCK == 1024  # read only by that second trip
    for p in (67 * 8, 67 * 8 + 7, 3 * 512, 3 * 512 + 511, 0, 8191, 8192, n - 1):
        assert p in pos
    # the all-0xFFFFFFFF vector: per-thread sums of 2^35 through the shuffles, the total inside 64 bits
    assert 8 * A.align16(0xFFFFFFFF) == 1 << 35 and n * A.align16(0xFFFFFFFF) < 1 << 64


def test_ref_hist_is_count_freqs(oracle):
    seen = set()
    for what, syms, nsyms in A.small_hist_inputs():
        want = A.ref_hist(syms, nsyms)
        seen.add((syms.dtype.itemsize, nsyms, isinstance(want, str)))
        if isinstance(want, str):
            with pytest.raises(R.RansAmdError) as e:
                R.count_freqs(syms, nsyms)
            assert e.value.status == R.E_ARG, what
            continue
        assert int(want.sum()) == syms.size
        assert np.array_equal(R.count_freqs(syms, nsyms).astype(np.int64), want), what
        assert np.array_equal(oracle.count_freqs(syms, nsyms).astype(np.int64), want), what
    for nsyms in A.U16_NSYMS:
        assert (2, nsyms, False) in seen and (2, nsyms, True) in seen
        syms = A.u16_nsyms_input(nsyms, 100 + nsyms)
        h = A.ref_hist(syms, nsyms)
        assert h.min() >= 1 and 4 * int(h[nsyms - 1]) >= syms.size, nsyms
    assert (1, 256, False) in seen and (1, 200, False) in seen and (1, 200, True) in seen and (1, 5, False) in seen


def test_u16_nsyms_sit_on_the_copy_boundaries():
    """8, 4, 2 and 1 counter copies, both sides of every boundary, and the one launch above 64 KiB of LDS."""
    copies = {n: A.u16_copies(n) for n in A.U16_NSYMS}
    assert (copies[1048], copies[1049], copies[2104], copies[2105], copies[4216], copies[4217]) == (8, 4, 4, 2, 2, 1)
    assert copies[1] == 8 and copies[16384] == 1 and (16384 + 8) * 4 == 65568
    launcher = open(os.path.join(CSRC, "container_kernels.hip")).read()
    assert "(size_t)copies * (nsyms + 8) * 4 > 33 * 1024" in launcher  # u16_copies restates this line
    assert "nsyms > 16384" in open(os.path.join(CSRC, "api.cpp")).read()


def test_histogram_sizes_reach_the_steady_state_body():
    src = open(os.path.join(CSRC, "container_kernels.hip")).read()
    assert "kHistCopies = 32, kHistBlocksPerCu = 8;" in src and "(sym_bytes == 1 ? kHistBlocksPerCu : 4)" in src
    for cus in CUS_TRIED:
        stride = 8 * cus * 256  # threads of k_histogram_u8's grid = 16-byte vectors per round
        assert A.hist_t8(cus) == stride * 16
        nvec = (2 * A.hist_t8(cus) + 53 - 13) // 16  # phase 3: 13 head bytes
        assert nvec > 2 * stride  # a first load, the loop's body once in every thread and twice in some
        assert (3 * A.hist_t8(cus) + 53 - 13) // 16 > 3 * stride  # ... twice in every thread
        assert (2 * A.hist_t16(cus) + 21) // 8 > 2 * (4 * cus * 256)


def test_ref_order_keys_is_bit_length():
    vals = np.concatenate([A.POW2_EDGES.astype(np.uint32), A.order_counts("log_uniform", 3000), np.array([0, 1, 2, 3], dtype=np.uint32)])
    assert A.ref_order_keys(vals).tolist() == [(int(v) + 1).bit_length() - 1 for v in vals]
    with pytest.raises(AssertionError):
        A.check_order(np.array([0, 1]), np.array([1, 3], dtype=np.uint32))  # keys 1, 2: increasing
    with pytest.raises(AssertionError):
        A.check_order(np.array([0, 0]), np.array([3, 3], dtype=np.uint32))  # no permutation
    A.check_order(np.array([1, 0]), np.array([1, 3], dtype=np.uint32))


def test_order_cases_hit_every_key_and_the_tile_boundary():
    keys = set()
    for n in A.ORDER_NS:
        for name in A.ORDER_CLASSES:
            c = A.order_counts(name, n)
            assert c.dtype == np.uint32 and c.size == n
            keys |= set(A.ref_order_keys(c).tolist())
    assert keys == set(range(33))
    assert set(A.ref_order_keys(A.order_counts("per_bucket", 33)).tolist()) == set(range(33))
    assert set(A.ref_order_keys(A.order_counts("all_ff", 5)).tolist()) == {32}
    for n in (A.ORDER_TILE - 1, A.ORDER_TILE, A.ORDER_TILE + 1, 2 * A.ORDER_TILE + 1, 3 * A.ORDER_TILE):
        assert n in A.ORDER_NS
    assert "kOrderThreads = 256;" in open(os.path.join(CSRC, "batch_order.hip")).read()
    assert "kOrderItems = 8;" in open(os.path.join(CSRC, "batch_order.hip")).read()


@pytest.mark.parametrize("src_bytes", [A.WAVE_SRC, A.SMALL_SRC])
def test_phase_length_table_is_complete(src_bytes):
    from_, lens = A.phase_length_table(src_bytes, 41)
    assert src_bytes % 16 == 5
    assert np.all(from_.astype(np.int64) + lens.astype(np.int64) <= src_bytes)
    have = set(zip((from_ % np.uint64(16)).tolist(), lens.tolist()))
    for ln in A.LENGTHS:
        for ph in range(16):
            assert (ph, ln) in have, (ph, ln)
    ends = from_.astype(np.int64) + lens.astype(np.int64) == src_bytes
    assert set((from_[ends] % np.uint64(16)).tolist()) == set(range(16)), "a start phase is missing among the chunks on the last byte"
    assert int(ends.sum()) >= 17 and src_bytes in lens.tolist() and 0 in from_.tolist()
    # both forms of the reference agree
    src = A.source_bytes(src_bytes, 41)
    assert np.array_equal(np.concatenate(A.ref_compact(src, from_, lens)), A.ref_compact_flat(src, from_, lens))


@pytest.mark.parametrize("cus", CUS_TRIED)
def test_every_compaction_case_selects_its_kernel(cus):
    cases = A.compact_cases(cus)
    assert {c.kernel for c in cases} == {"wave", "small"}
    for c in cases:
        n = c.lens.size
        assert c.from_.size == n and c.src_bytes % 16 == 5, c.name
        assert np.all(c.from_.astype(np.int64) + c.lens.astype(np.int64) <= c.src_bytes), c.name
        assert A.compact_kernel(c.src_bytes, n) == c.kernel, c.name
    by = {c.name: c for c in cases}
    assert by["trips-wave"].lens.size > 2 * 32 * cus      # launch_compact: 8 blocks of four waves per CU
    assert by["trips-small"].lens.size > 2 * 2048 * cus   # ... each wave 64 chunks per trip
    assert int(by["mixed-small"].lens.max()) == (1 << 20) + 3 and {0, 1} <= set(by["mixed-wave"].lens.tolist())
    assert [by["small-n%d" % n].lens.size for n in (1, 63, 64, 65)] == [1, 63, 64, 65]


def test_the_cases_beyond_32_bits():
    from_, lens = A.big_a()
    assert A.compact_kernel(A.BIG_A_SRC, from_.size) == "wave" and len(set(from_.tolist())) == 66
    assert set((from_ % np.uint64(16)).tolist()) == set(range(16))
    assert int((from_ + lens.astype(np.uint64)).max()) <= A.BIG_A_SRC and int(A.ref_offsets(lens)[-2]) > 1 << 32
    from_, lens = A.big_b()
    assert A.compact_kernel(A.BIG_B_SRC, from_.size) == "small"
    assert int((from_ + lens.astype(np.uint64)).max()) <= A.BIG_B_SRC and int(A.ref_offsets(lens)[-2]) > 1 << 32
    for kernel in ("wave", "small"):
        from_, lens = A.big_c(kernel)
        assert A.compact_kernel(A.BIG_SRC, from_.size) == kernel
        ends = from_.astype(np.int64) + lens.astype(np.int64)
        assert int(ends.max()) == A.BIG_SRC and int(from_.max()) > 1 << 32 and int(from_.min()) < A.MIB
        local = A.big_c_local(from_)
        assert np.all((local >= 0) & (local + lens.astype(np.int64) <= 2 * A.MIB))
    assert A.BIG_C_SMALL_N == (1 << 21) + 512 and A.compact_kernel(A.BIG_SRC, A.BIG_C_SMALL_N - 1100) == "wave"
    # (d): one chunk whose length + 15 wraps in 32 bits, inside the source
    assert A.BIG_D_LEN >= (1 << 32) - 15 and (A.BIG_D_LEN + 15) & 0xFFFFFFFF < 16
    assert A.BIG_D_FROM + A.BIG_D_LEN <= A.BIG_SRC and A.compact_kernel(A.BIG_SRC, 1) == "wave" and A.BIG_SRC % 16 == 5


@pytest.mark.parametrize("kernel", ["wave", "small"])
def test_rejected_entries_sit_on_odd_phases(kernel):
    src, from_, lens, victims = A.reject_cases(kernel)
    assert A.compact_kernel(src, lens.size) == kernel and src % 16 == 5
    (v0, f0, l0, ok0), (v1, f1, l1, ok1) = victims
    assert f0 + l0 == src + 1 and f0 % 16 not in (0, 5) and not ok0
    assert f1 == src and l1 == 0 and ok1 and f1 % 2 == 1


def test_kernel_choice_rule_is_the_sources():
    api = open(os.path.join(CSRC, "api.cpp")).read()
    assert "src_bytes / n_chunks <= 2048" in api
    m = re.search(r"cp\.slot_bytes = \(src_bytes / n_chunks <= 2048\) \? (\d+) : (1u << 20);", api)
    assert m and int(m.group(1)) <= 8192 < (1 << 20), "the two slot sizes no longer straddle launch_compact's threshold"
    hip = open(os.path.join(CSRC, "container_kernels.hip")).read()
    body = hip[hip.index("hipError_t launch_compact("):]
    body = body[:body.index("\n}\n")]
    assert "slot_bytes <= 8192" in body
    assert body.index("slot_bytes <= 8192") < body.index("k_compact_small") < body.index("RANS_LAUNCH(k_compact,")
    assert A.compact_kernel(2048 * 7 + 6, 7) == "small" and A.compact_kernel(2049 * 7, 7) == "wave"
