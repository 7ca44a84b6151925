"""References and case tables for the kernels that run AROUND every coder call: the offset scan (k_layout_sums, k_layout),
the compaction (k_compact, k_compact_small), the whole-input histogram (k_histogram_u8, k_histogram_u16, and k_zero before
them) of container_kernels.hip and the three kernels of batch_order.hip.  Plain numpy: no GPU, no call into the library
or the oracle -- tests/test_around_coders_cpu.py holds everything here to the host entry points and to the oracle and proves
that the tables cover what they claim, tests/test_gpu_around_coders.py holds the kernels to it.

Every comparison built on this file is exact: integers and bytes, no tolerance, no float in a reference.

Sizes that depend on the part are functions of `cus` (the GPU's compute units): the GPU tests pass what the device reports,
the CPU tests several values."""
from collections import namedtuple

import numpy as np

POISON = 0xEE
GUARD = 4096

U64 = np.uint64


def align16(x):
    return (int(x) + 15) & ~15


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------

def ref_offsets(lengths):
    """offsets[c] = sum_{i<c} align16(lengths[i]) in uint64; offsets[n] = offsets[n - 1] + lengths[n - 1]; [0] for n == 0."""
    ln = np.ascontiguousarray(lengths).astype(U64)
    n = ln.size
    out = np.zeros(n + 1, dtype=U64)
    if n:
        aligned = (ln + U64(15)) & ~U64(15)
        np.cumsum(aligned[:-1], dtype=U64, out=out[1:n])
        out[n] = out[n - 1] + ln[n - 1]
    return out


def aligned_total(lengths):
    """The capacity a destination needs: the sum of every chunk's length rounded up to 16."""
    ln = np.ascontiguousarray(lengths).astype(U64)
    return int(((ln + U64(15)) & ~U64(15)).sum(dtype=U64))


def ref_compact(src, from_, lens):
    """The bytes every chunk must hold, one array per chunk."""
    return [src[int(f):int(f) + int(ln)] for f, ln in zip(from_, lens)]


def flat_index(starts, lens):
    """The byte positions start[c] .. start[c] + lens[c] - 1 of every chunk, one after the other (int64)."""
    lens = np.ascontiguousarray(lens).astype(np.int64)
    starts = np.ascontiguousarray(starts).astype(np.int64)
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def ref_compact_flat(src, from_, lens):
    """np.concatenate(ref_compact(..)) without a Python loop, for the cases with 10^6 chunks."""
    return src[flat_index(from_, lens)]


def ref_hist(syms, nsyms):
    """np.bincount, or "error" when a symbol lies outside the alphabet."""
    syms = np.ascontiguousarray(syms)
    if syms.size and int(syms.max()) >= nsyms:
        return "error"
    return np.bincount(syms, minlength=nsyms).astype(np.int64)


def ref_order_keys(counts):
    """bit_length(count + 1) - 1 = floor(log2(count + 1)) in integers: the number of k in 1..32 with 2^k <= count + 1."""
    x = np.ascontiguousarray(counts).astype(U64) + U64(1)
    keys = np.zeros(x.size, dtype=np.int64)
    for k in range(1, 33):
        keys += x >= U64(1 << k)
    return keys


def check_order(order, counts):
    """`order` is a permutation of the stream indices along which the bucket key never increases."""
    order = np.ascontiguousarray(order).astype(np.int64)
    n = len(counts)
    assert order.size == n, (order.size, n)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.int64)), "not a permutation"
    keys = ref_order_keys(np.asarray(counts)[order])
    assert np.all(np.diff(keys) <= 0), "bucket keys increase along the order"
    return keys


def compact_kernel(src_bytes, n_chunks):
    """The rule of rans_amd_container_compact (api.cpp) and launch_compact (container_kernels.hip), restated once: the
    source cannot hold chunks longer than src_bytes / n_chunks on average; up to 2048 the 16-lanes-per-chunk kernel."""
    return "small" if src_bytes // n_chunks <= 2048 else "wave"


def source_bytes(src_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=src_bytes, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# section 3: the offset scan.  A thread of k_layout takes 8 consecutive chunks, a wave 512, a block 8192; the carry loop
# of block b walks block_sums[threadIdx.x], [threadIdx.x + 1024], ..: its second trip needs b > 1024.
# ---------------------------------------------------------------------------------------------------------------------------
LAYOUT_PER_THREAD, LAYOUT_PER_WAVE, LAYOUT_PER_BLOCK = 8, 512, 8192
LAYOUT_CARRY_TRIP = 1024 * LAYOUT_PER_BLOCK  # the first chunk of block 1024: block 1025's thread 0 reads its sum in trip 2
LAYOUT_NCHUNKS = (0, 1, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 16385, 1025 * 8192 + 9)
SPIKE = 0xFFFFFFF1
LAYOUT_SMALL = ("zeros", "ones", "mod33")  # the destination holds them: the copy runs
LAYOUT_BIG = ("all_ff", "random")          # sums no destination holds: RANS_AMD_E_SPACE, the offsets still complete


def spike_positions(n):
    """First and last chunk of a thread (thread 67: wave 1, lane 3), of a wave (wave 3), of a block (blocks 0, 1 and 1024:
    the one only a second trip of the carry loop reaches) and the last chunk of all."""
    t, w = 67, 3
    want = {t * LAYOUT_PER_THREAD, t * LAYOUT_PER_THREAD + 7, w * LAYOUT_PER_WAVE, w * LAYOUT_PER_WAVE + 511,
            0, LAYOUT_PER_BLOCK - 1, LAYOUT_PER_BLOCK, 2 * LAYOUT_PER_BLOCK - 1,
            LAYOUT_CARRY_TRIP, LAYOUT_CARRY_TRIP + LAYOUT_PER_BLOCK - 1, n - 1}
    return sorted(p for p in want if 0 <= p < n)


def layout_classes(n):
    """The length classes that make sense at n chunks (none at 0: test_layout_of_nothing)."""
    if n == 0:
        return ()
    return LAYOUT_SMALL + LAYOUT_BIG + tuple("spike@%d" % p for p in spike_positions(n))


def layout_lengths(name, n):
    if name == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if name == "ones":
        return np.ones(n, dtype=np.uint32)
    if name == "mod33":  # every residue around the 16-byte round-up
        return (np.arange(n, dtype=np.int64) % 33).astype(np.uint32)
    if name == "all_ff":  # per-thread sums of 2^35
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    if name == "random":
        return np.random.default_rng(1000 + n % 9973).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert name.startswith("spike@"), name
    out = np.zeros(n, dtype=np.uint32)
    out[int(name[6:])] = SPIKE
    return out


def layout_is_big(name):
    return name in LAYOUT_BIG or name.startswith("spike@")


LAYOUT_SRC_BYTES = 37  # the small classes copy from here: from = c % 5, lengths <= 32


def layout_from(n):
    return (np.arange(n, dtype=np.int64) % 5).astype(U64)


# ---------------------------------------------------------------------------------------------------------------------------
# section 4: compaction
# ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kernel src_bytes seed from_ lens")

LENGTHS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1008, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 8191, 8192, 8193)
WAVE_SRC = (2 << 20) + 5
SMALL_SRC = (256 << 10) + 5
END_GRANULES = (0, 1, 2, 5, 64)  # whole granules in front of the ragged piece of the chunks that end on the last byte


def phase_length_table(src_bytes, seed):
    """Every source phase 0..15 x every length of LENGTHS (anywhere in the source), 16 chunks that end exactly on the
    source's last byte and start on phases 0..15, one chunk that starts at 0, one that is the whole source; shuffled."""
    assert src_bytes % 16 == 5
    rng = np.random.default_rng(seed)
    rows = []
    for ln in LENGTHS:
        for ph in range(16):
            base = int(rng.integers(0, (src_bytes - ln - 15) // 16 + 1))
            rows.append((16 * base + ph, ln))
    for ph in range(16):
        ln = (src_bytes - ph) % 16 + 16 * END_GRANULES[ph % 5]
        rows.append((src_bytes - ln, ln))
    rows.append((0, 77))
    rows.append((0, src_bytes))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return np.array([r[0] for r in rows], dtype=U64), np.array([r[1] for r in rows], dtype=np.uint32)


def random_chunks(seed, n, src_bytes, lo, hi):
    """n chunks with lengths in [lo, hi] anywhere in the source (random phases)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, min(hi, src_bytes) + 1, size=n, dtype=np.int64)
    from_ = rng.integers(0, src_bytes - lens + 1, dtype=np.int64)
    return from_.astype(U64), lens.astype(np.uint32)


def src_for(n, per_chunk):
    """The smallest source of at least n * per_chunk bytes with src_bytes % 16 == 5."""
    s = n * per_chunk
    return s + (5 - s) % 16


def compact_cases(cus):
    """The cases of section 4 that are compared on the host."""
    out = [Case("phases-wave", "wave", WAVE_SRC, 41, *phase_length_table(WAVE_SRC, 41)),
           Case("phases-small", "small", SMALL_SRC, 42, *phase_length_table(SMALL_SRC, 42))]
    for n in (1, 63, 64, 65):  # a part of a wave's 64 chunks, all of them, one more
        src = 2048 * n - 11
        out.append(Case("small-n%d" % n, "small", src, 50 + n, *random_chunks(50 + n, n, src, 0, 700)))
    # more than one trip over the grid: 32 cus waves of k_compact, 2048 cus chunks per trip of k_compact_small
    n = 64 * cus + 3
    src = src_for(n, 2049)
    out.append(Case("trips-wave", "wave", src, 61, *random_chunks(61, n, src, 0, 4096)))
    n = 4096 * cus + 67
    out.append(Case("trips-small", "small", (1 << 20) + 5, 62, *random_chunks(62, n, (1 << 20) + 5, 0, 48)))
    # mixed: a long chunk in k_compact_small's 512-bytes-per-pass loop, lengths 0 and 1 among long chunks in k_compact
    src = (2 << 20) + 5
    from_, lens = random_chunks(63, 4097, src, 0, 40)
    from_[2000], lens[2000] = 9, (1 << 20) + 3
    out.append(Case("mixed-small", "small", src, 63, from_, lens))
    src = (4 << 20) + 5
    from_, lens = random_chunks(64, 40, src, 50000, 150000)
    lens[0::3], lens[1::3] = 0, 1
    out.append(Case("mixed-wave", "wave", src, 64, from_, lens))
    return out


REJECT_SRC = {"wave": (2 << 20) + 5, "small": 2048 * 65 - 11}


def reject_cases(kernel):
    """65 healthy chunks; chunk 31 replaced by (a) from + len == src_bytes + 1 at an odd phase: outside, rejected, and
    (b) from == src_bytes, len == 0: inside, accepted.  -> (src_bytes, from_, lens, [(victim, from, len, accepted)])"""
    src = REJECT_SRC[kernel]
    from_, lens = random_chunks(70, 65, src, 1, 700)
    return src, from_, lens, [(31, src + 1 - 37, 37, False), (31, src, 0, True)]


# beyond 32 bits: compared on the device
BIG_A_SRC, BIG_A_N = (80 << 20) + 5, 66
BIG_B_SRC, BIG_B_N, BIG_B_LEN, BIG_B_STEP = (16 << 20) + 5, 8192, (520 << 10) + 7, 37
BIG_SRC = (4 << 30) + (1 << 20) + 5  # cases (c) and (d) share one source
BIG_C_SMALL_N = (1 << 21) + 512
BIG_D_FROM, BIG_D_LEN = 3, (1 << 32) - 8
MIB = 1 << 20


def big_a():
    """Wave kernel, destination offsets above 2^32: 66 chunks of 64 MiB + 16 k bytes from 66 places (every phase)."""
    k = np.arange(BIG_A_N, dtype=np.int64)
    return (17 * k).astype(U64), ((64 << 20) + 16 * k).astype(np.uint32)


def big_b():
    """Small kernel, destination offsets above 2^32: 8192 chunks of 520 KiB + 7 bytes, from = 37 k."""
    k = np.arange(BIG_B_N, dtype=np.int64)
    return (BIG_B_STEP * k).astype(U64), np.full(BIG_B_N, BIG_B_LEN, dtype=np.uint32)


def big_c(kernel):
    """Source offsets above 2^32: chunks in the first and in the last MiB of BIG_SRC, alternating; the last chunk ends on
    the source's last byte."""
    n, hi = (64, 8193) if kernel == "wave" else (BIG_C_SMALL_N, 48)
    from_, lens = random_chunks(80 if kernel == "wave" else 81, n, MIB, 0, hi)
    from_[1::2] += U64(BIG_SRC - MIB)
    from_[n - 1] = BIG_SRC - int(lens[n - 1])
    return from_, lens


def big_c_local(from_):
    """Positions of big_c's chunks in first MiB + last MiB laid side by side (what the host keeps of BIG_SRC)."""
    f = from_.astype(np.int64)
    return np.where(f >= BIG_SRC - MIB, f - (BIG_SRC - 2 * MIB), f)


# ---------------------------------------------------------------------------------------------------------------------------
# section 5: histogram
# ---------------------------------------------------------------------------------------------------------------------------
U8_PHASES, U8_NS = range(16), range(41)
U16_PHASES, U16_NS = range(8), range(25)
U16_NSYMS = (1, 2, 255, 256, 257, 1048, 1049, 2104, 2105, 4096, 4216, 4217, 16383, 16384)
HIST_CLASSES = ("uniform", "zipf", "constant")


def hist_t8(cus):
    """Bytes one round of 16-byte loads of k_histogram_u8's grid takes: above it the pipelined loop's body runs."""
    return 8 * cus * 256 * 16


def hist_t16(cus):
    """Symbols one round of k_histogram_u16's grid takes."""
    return 4 * cus * 256 * 8


def u16_copies(nsyms):
    """launch_histogram's rule: as many counter copies (8, 4, 2, 1) as fit 33 KiB."""
    copies = 8
    while copies > 1 and copies * (nsyms + 8) * 4 > 33 * 1024:
        copies >>= 1
    return copies


def hist_data(name, n, seed, nsyms=256, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return rng.integers(0, nsyms, size=n, dtype=np.int64).astype(dtype)
    if name == "constant":
        return np.full(n, min(0xA7, nsyms - 1), dtype=dtype)
    assert name == "zipf", name
    # p(s) ~ 1 / (s + 1) through an integer table of cumulative weights: the top symbol is a sixth of the input
    weights = (1 << 40) // np.arange(1, nsyms + 1, dtype=np.int64)
    edges = np.cumsum(weights)
    return np.searchsorted(edges, rng.integers(0, int(edges[-1]), size=n, dtype=np.int64), side="right").astype(dtype)


def u16_nsyms_input(nsyms, seed):
    """Every symbol at least once, symbol nsyms - 1 a quarter of the input and more, the rest uniform; shuffled."""
    rng = np.random.default_rng(seed)
    n = 4 * nsyms + 21
    quarter = (n + 3) // 4
    syms = np.concatenate([np.arange(nsyms, dtype=np.int64), np.full(quarter, nsyms - 1, dtype=np.int64),
                           rng.integers(0, nsyms, size=n - nsyms - quarter, dtype=np.int64)])
    return rng.permutation(syms).astype(np.uint16)


def small_hist_inputs():
    """The small inputs of section 5, for the CPU comparison of ref_hist: (what, symbols, nsyms)."""
    base8 = hist_data("uniform", 64, 5)
    for ph in U8_PHASES:
        for n in U8_NS:
            yield "u8 phase %d n %d" % (ph, n), base8[ph:ph + n], 256
    in200 = hist_data("uniform", 300, 6, nsyms=200)
    yield "u8 nsyms 200", in200, 200
    for at in (0, 150, 299):
        bad = in200.copy()
        bad[at] = 200 + at % 56
        yield "u8 nsyms 200, symbol %d at %d" % (int(bad[at]), at), bad, 200
    yield "u8 nsyms 200, the only symbol outside", np.array([255], dtype=np.uint8), 200
    base16 = hist_data("uniform", 40, 7, nsyms=4096, dtype=np.uint16)
    for ph in U16_PHASES:
        for n in U16_NS:
            yield "u16 phase %d n %d" % (ph, n), base16[ph:ph + n], 4096
    for nsyms in U16_NSYMS:
        good = u16_nsyms_input(nsyms, 100 + nsyms)
        yield "u16 nsyms %d" % nsyms, good, nsyms
        bad = good.copy()
        bad[bad.size // 3] = nsyms
        yield "u16 nsyms %d, one symbol %d" % (nsyms, nsyms), bad, nsyms
    yield "u8 data in 0..4, nsyms 5", hist_data("uniform", 1000, 8, nsyms=5), 5
    yield "u16 data in 0..4, nsyms 5", hist_data("uniform", 1000, 9, nsyms=5, dtype=np.uint16), 5


# ---------------------------------------------------------------------------------------------------------------------------
# section 6: order.  A block of k_order_hist / k_order_scatter takes a tile of 2048 streams.
# ---------------------------------------------------------------------------------------------------------------------------
ORDER_TILE = 2048
ORDER_NS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 3 * 2048)
ORDER_CLASSES = ("zeros", "ones", "all_ff", "pow2_edges", "per_bucket", "log_uniform")
POW2_EDGES = np.array([v for k in range(1, 33) for v in ((1 << k) - 2, (1 << k) - 1, 1 << k)], dtype=np.uint64).clip(0, 0xFFFFFFFF)


def order_counts(name, n, seed=0):
    if name == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if name == "ones":
        return np.ones(n, dtype=np.uint32)
    if name == "all_ff":  # one bucket: every block takes the same cursor
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    if name == "pow2_edges":  # both sides of every key's boundary
        return np.resize(POW2_EDGES, n).astype(np.uint32)
    if name == "per_bucket":  # one stream per bucket, repeated across the tiles
        return np.array([(1 << (i % 33)) - 1 for i in range(n)], dtype=np.uint64).astype(np.uint32)
    assert name == "log_uniform", name
    rng = np.random.default_rng(2000 + seed + n)
    return (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) >> rng.integers(0, 33, size=n, dtype=np.uint64)).astype(np.uint32)
