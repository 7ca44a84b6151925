"""Inputs and plain models for the per-chunk-model builders (device_common.hpp adapt_normalize / adapt_build_dec, the count
passes of k_chunk_models and k_encode_adaptive, the piece-size bound of encode_adaptive.hip step 3) at the extremes of the
HISTOGRAM.  Plain numpy: no GPU, no call into the library or the oracle -- tests/test_model_extremes_cpu.py holds everything
here to the oracle, tests/test_gpu_model_extremes.py holds the kernels to the oracle and to need_model.

A class is a function (nsym, seed) -> u8[nsym]: a seeded shuffle of EXACT counts (counts_of), so the histogram of a chunk
is known without counting.  supports(name, nsym) says where a class is defined.

  dom_first / dom_last / dom_mid   symbol 0 / 255 / 128 takes nsym - 255, every other symbol occurs once (chunks shorter than
                                   256: the lowest nsym - 1 other symbols once, the dominant one once)
  tie_chain                        symbols 0..199 once, 200..254 sixteen times, 255 the rest (nsym >= 1081)
  exact_2048 / _2049 / _4095       nsym = 4096 k: {2048 k, 2048 k} at symbols 7 and 250, {2049 k at 7, 2047 k at 250},
                                   {4095 k at 0, k at 255}: at 12 bits the width is the count / k, no repair
  constant_0 / constant_255        one value
  all_once                         every value nsym / 256 times (the first nsym mod 256 values once more)
  lane_edges                       nine symbols whose counts are whole 64ths of nsym (LANE_EDGES: symbol, 64ths): every
                                   occupied symbol starts on lane * (M >> 6) of the decode-table builder, at 12 and at 8
                                   bits, behind at least four symbols of count 0; the last occupied symbol is 199
  sparse_16                        symbols 3, 7, .., 63 with equal counts: a symbol every four lanes of the builder
"""
import numpy as np

from _oracle import FMT_BYTE, FMT_WORD

STATE_BYTES = 4  # both formats flush 32-bit states

LANE_EDGES = ((5, 3), (12, 1), (20, 7), (33, 5), (64, 16), (100, 1), (131, 11), (150, 2), (199, 18))
assert sum(w for _, w in LANE_EDGES) == 64
SPARSE_16 = tuple(range(3, 64, 4))


def _dom(x):
    def counts(nsym):
        if nsym < 1:
            return None
        c = np.zeros(256, dtype=np.int64)
        others = [s for s in range(256) if s != x][:min(255, nsym - 1)]
        c[others] = 1
        c[x] = nsym - len(others)
        return c
    return counts


def _tie_chain(nsym):
    if nsym < 200 + 55 * 16 + 1:
        return None
    c = np.zeros(256, dtype=np.int64)
    c[:200] = 1
    c[200:255] = 16
    c[255] = nsym - 200 - 55 * 16
    return c


def _exact(pairs):
    def counts(nsym):
        if nsym < 4096 or nsym % 4096:
            return None
        c = np.zeros(256, dtype=np.int64)
        for s, w in pairs:
            c[s] = w * (nsym // 4096)
        return c
    return counts


def _constant(x):
    def counts(nsym):
        if nsym < 1:
            return None
        c = np.zeros(256, dtype=np.int64)
        c[x] = nsym
        return c
    return counts


def _all_once(nsym):
    if nsym < 1:
        return None
    return nsym // 256 + (np.arange(256) < nsym % 256).astype(np.int64)


def _weights(pairs, den):
    def counts(nsym):
        if nsym < den or nsym % den:
            return None
        c = np.zeros(256, dtype=np.int64)
        for s, w in pairs:
            c[s] = w * (nsym // den)
        return c
    return counts


_COUNTS = {
    "dom_first": _dom(0), "dom_last": _dom(255), "dom_mid": _dom(128),
    "tie_chain": _tie_chain,
    "exact_2048": _exact(((7, 2048), (250, 2048))), "exact_2049": _exact(((7, 2049), (250, 2047))), "exact_4095": _exact(((0, 4095), (255, 1))),
    "constant_0": _constant(0), "constant_255": _constant(255),
    "all_once": _all_once,
    "lane_edges": _weights(LANE_EDGES, 64),
    "sparse_16": _weights(tuple((s, 1) for s in SPARSE_16), 16),
}


def counts_of(name, nsym):
    """The exact histogram of class `name` at nsym symbols (i64[256]); None where the class is not defined."""
    return _COUNTS[name](int(nsym))


def supports(name, nsym):
    return counts_of(name, nsym) is not None


def _histogram(name):
    def make(nsym, seed):
        c = counts_of(name, nsym)
        assert c is not None and int(c.sum()) == nsym, (name, nsym)
        out = np.repeat(np.arange(256), c).astype(np.uint8)
        np.random.default_rng(seed).shuffle(out)
        return out
    make.__name__ = name
    return make


HISTOGRAMS = {name: _histogram(name) for name in _COUNTS}


# ---- what the GPU tests feed: shared with the CPU tests, which prove the conditions on exactly these chunks --------------------
CHUNKS = (4096, 8192, 16384)                     # 64-way, 4-aligned: the register-resident kernels RR = 4 / 8 / 16
OTHER_WAYS = {4096: 2, 8192: 128, 16384: 512}    # the second interleave of a uniform call, by chunk size


def class_plan(chunk, last="dom_last"):
    """[(class, nsym)] of a uniform call: every class defined at `chunk` symbols as one chunk each, then `last` as the ragged
    chunk of chunk / 3 + 1 symbols."""
    return [(name, chunk) for name in HISTOGRAMS if supports(name, chunk)] + [(last, chunk // 3 + 1)]


NATURAL = (("dom_first", 16384), ("dom_last", 16384), ("dom_mid", 16384), ("tie_chain", 16384), ("exact_2048", 4096), ("exact_2049", 4096),
           ("exact_4095", 4096), ("constant_0", 5127), ("constant_255", 1031), ("all_once", 4100), ("lane_edges", 5120), ("sparse_16", 1024))


# all_once at sizes where lo sits a few bytes below a line for every row of tests/test_gpu_batch_models.py MODEL_ROWS (22 906: the
# 64- and 128-way rows; 20 787: the 8- and 2-way rows): the 1 + 2^-12 factor of the estimate, 5 bytes here, buys another line and
# need_floor is lo + 64 (found by search over the model, held by tests/test_model_extremes_cpu.py)
FACTOR_SIZES = (22906, 20787)


def batch_plan():
    """[(class, nsym)] of a ragged batch: every class at the size its condition is stated for, then every size of the count-path
    table with the classes in turn (the next one defined at that size), all_once at FACTOR_SIZES, then an empty stream between
    two dom_* streams."""
    names = tuple(HISTOGRAMS)
    plan = list(NATURAL)
    for i, size in enumerate(COUNT_SIZES):
        defined = [name for name in names if supports(name, size)]
        plan.append((defined[(5 * i) % len(defined)], size))
    plan += [("all_once", n) for n in FACTOR_SIZES]
    return plan + [("dom_first", 17415), ("empty", 0), ("dom_last", 12289)]


def normalize_model(counts, target):
    """normalize_freqs, width-based: edge[s] = target * (counts[0] + .. + counts[s]) div total, width[s] = edge[s] - edge[s - 1];
    then every symbol that occurs but got width 0, in ascending order, takes one slot from the narrowest symbol wider than 1
    (lowest index on ties).  -> (widths i64[256], [(squeezed, victim), ..]); None in place of the widths where nobody can give."""
    counts = np.asarray(counts, dtype=np.int64)
    edges = (int(target) * np.cumsum(counts)) // int(counts.sum())
    width = np.diff(np.concatenate(([0], edges)))
    pairs = []
    for s in np.nonzero((counts > 0) & (width == 0))[0]:
        wide = np.nonzero(width > 1)[0]
        if wide.size == 0:
            return None, pairs
        victim = int(wide[np.argmin(width[wide])])  # (argmin: the first of equal widths)
        width[victim] -= 1
        width[s] = 1
        pairs.append((int(s), victim))
    return width, pairs


def align64(x):
    return (int(x) + 63) & ~63


def worst_slot(nsym, n_ways):
    """rans_amd_chunk_bound in whole 64-byte lines: two bytes a symbol and the flushed states (api.cpp encode_slot_bytes; the
    ragged form of encode_adaptive.hip computes the same from the stream's own count)."""
    return align64(2 * int(nsym) + n_ways * STATE_BYTES)


def need_model(fmt, row, counts, nsym, n_ways, sb, ragged, chunk_syms=None):
    """Step 3 of encode_adaptive.hip in f64 -> (lo, hi): the piece a chunk of `nsym` symbols with histogram `counts` and
    normalised row `row` may be given.  chunk_syms: the full chunk of a uniform call, min(n, chunk size) -- its worst-case slot
    (rans_amd_encode_adaptive_sized's worst_slot) caps every piece of the call, the shorter last one included; default nsym.

      B     = sum counts[s] * (sb - log2 row[s])                         bits, f64
      slack = (nsym * 23) >> 11 (word) | nsym >> 12 (byte), + n_ways * 4 state bytes + 64
      lo    = align64(floor(B / 8) + slack)
      hi    = align64(floor((B + E) / 8 * (1 + 2^-12)^2) + slack),       E = nsym * 3 * 2^-21
      both capped by the worst-case slot, and equal to it when row.max() == 1 << sb in the word format (`always`).

    Where hi comes from.  The kernel computes est = fl(bits * c) in f32, c = (1 + 2^-12) / 8 exactly, and says that 2^-12 of
    the sum covers the rounding: est <= B / 8 * (1 + 2^-12)^2 is its own budget.  That holds for the RELATIVE part of the f32
    error: bits is a sum of 256 products fl(cnt) * fl(sb - l) added up in 3 + 6 steps (four terms in a lane, six butterfly
    levels), each rounding within 2^-24, and one more for est: (1 + 2^-24)^12 < 1 + 2^-20, far inside 1 + 2^-12.  The ABSOLUTE
    part it does not cover: l = __log2f(width) is the hardware logarithm, documented as accurate to 1 ULP of its result, and
    the result lies in [0, 12], so |l - log2 width| <= 2^-20 (the ULP in [8, 16)); sb - l is rounded once more, by at most
    half an ULP of a value below 16, 2^-21.  A term is thus off by up to cnt * 3 * 2^-21 bits whatever its size, the sum by
    E = nsym * 3 * 2^-21 -- and on a chunk that codes to less than 3 * 2^-9 bits a symbol (exact_4095: 0.0033) E is more than
    2^-12 of B.  Hence B + E in hi: at most 0.012 bytes for 65 536 symbols, it moves hi only where B / 8 sits that close
    below a multiple of 64.  lo is the issue's: the real-valued bound, which the kernel's margin is meant to stay above."""
    lo, _, hi = _need(fmt, row, counts, nsym, n_ways, sb, ragged, chunk_syms)
    return lo, hi


def need_floor(fmt, row, counts, nsym, n_ways, sb, ragged, chunk_syms=None):
    """What the kernel's estimate cannot fall below if it multiplies by 1 + 2^-12 as it says: with the error terms of
    need_model's derivation taken the other way, bits >= (B - E) (1 - 2^-24)^11 and est >= (B - E) (1 + 2^-12) (1 - 2^-20) / 8,
    so need >= align64(floor(that) + slack), capped like lo.  Not below lo on any piece the tests look at but those where E
    counts (a chunk of a few bits); a kernel that drops the factor returns lo itself and misses this floor on every piece
    where the factor's B / 32768 bytes cross a line (tests/test_model_extremes_cpu.py counts them)."""
    return _need(fmt, row, counts, nsym, n_ways, sb, ragged, chunk_syms)[1]


def _need(fmt, row, counts, nsym, n_ways, sb, ragged, chunk_syms):
    assert fmt in (FMT_WORD, FMT_BYTE)
    row = np.asarray(row, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    nsym = int(nsym)
    assert int(counts.sum()) == nsym
    worst = worst_slot(nsym if ragged else int(chunk_syms or nsym), n_ways)
    if fmt == FMT_WORD and nsym and int(row.max()) == 1 << sb:
        return worst, worst, worst
    occ = counts > 0
    B = float(np.sum(counts[occ] * (sb - np.log2(row[occ]))))
    slack = ((nsym * 23) >> 11 if fmt == FMT_WORD else nsym >> 12) + n_ways * STATE_BYTES + 64
    E = nsym * 3.0 * 2.0 ** -21
    lo = align64(int(np.floor(B / 8.0)) + slack)
    floor_ = align64(int(np.floor(max(B - E, 0.0) / 8.0 * (1.0 + 2.0 ** -12) * (1.0 - 2.0 ** -20))) + slack)
    hi = align64(int(np.floor((B + E) / 8.0 * (1.0 + 2.0 ** -12) ** 2)) + slack)
    return min(lo, worst), min(floor_, worst), min(hi, worst)


# ---- the count passes ------------------------------------------------------------------------------------------------------
TRIP, LOOP, DWORD, TAIL = "4096-trip", "1024-loop", "4-byte", "byte tail"


def count_paths(nsym, base, trip=4096):
    """The loops the count pass of k_encode_adaptive enters for a chunk of nsym symbols at byte address `base` (modulo 16), from
    the kernel's loop bounds: 16-byte loads in trips of `trip` = 4 x 1024 symbols while whole trips remain, then by 1024; dwords
    behind that on a 4-aligned address; bytes for the rest -- all of it on an odd address.  trip = 0: k_chunk_models, which has
    the 1024-loop alone for its 16-byte loads."""
    paths, done = set(), 0
    if base % 16 == 0:
        big = nsym & ~(trip - 1) if trip else 0
        body16 = nsym & ~1023
        if big:
            paths.add(TRIP)
        if body16 > big:
            paths.add(LOOP)
        done = body16
    body = (nsym & ~3) if base % 4 == 0 else done
    if body > done:
        paths.add(DWORD)
    if nsym > body:
        paths.add(TAIL)
    return paths


# chunk size -> the paths at a 16-aligned, a 4-aligned and an odd base (T: 4096-trip, L: 1024-loop, 4: 4-byte, b: byte tail).
# 4096 k + 1024 j + 4 i + t; 8192 and up run the trip loop's prefetch branch (a next trip exists), 2052 and 11270 the
# 1024-loop more than once, 4100 the dword loop right behind a trip, 12289 the byte tail right behind three trips.
COUNT_TABLE = {
    1:     ("b",    "b",  "b"),
    3:     ("b",    "b",  "b"),
    4:     ("4",    "4",  "b"),
    64:    ("4",    "4",  "b"),
    67:    ("4b",   "4b", "b"),
    1024:  ("L",    "4",  "b"),
    1027:  ("Lb",   "4b", "b"),
    1031:  ("L4b",  "4b", "b"),
    2052:  ("L4",   "4",  "b"),
    4095:  ("L4b",  "4b", "b"),
    4096:  ("T",    "4",  "b"),
    4100:  ("T4",   "4",  "b"),
    5120:  ("TL",   "4",  "b"),
    5127:  ("TL4b", "4b", "b"),
    8192:  ("T",    "4",  "b"),
    11270: ("TL4b", "4b", "b"),
    12289: ("Tb",   "4b", "b"),
    16384: ("T",    "4",  "b"),
    17415: ("TL4b", "4b", "b"),
}
COUNT_SIZES = tuple(COUNT_TABLE)
COUNT_BASES = (0, 4, 1)  # 16-aligned, 4-aligned, odd -- the columns of COUNT_TABLE
_LETTER = {"T": TRIP, "L": LOOP, "4": DWORD, "b": TAIL}


def table_paths(nsym, base):
    return {_LETTER[ch] for ch in COUNT_TABLE[nsym][COUNT_BASES.index(base)]}
