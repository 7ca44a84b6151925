"""Where the chunked encode entry points may write, and what they report when out_cap is just too small: the plain-integer
reference and the case tables.  numpy, the package's option numbers and the kernel matrix's table only (the CPU oracle is
handed in): tests/test_capacity_cpu.py proves on the CPU what the tables claim, tests/test_gpu_capacity.py holds the encoders
to them.

The rule (include/ryg_rans_amd.h, rans_amd_encode): with lens the chunk stream lengths,

    offsets[c] = sum_{i<c} align16(lens[i])        T = offsets[last] + lens[last]       (= d_offsets[n_chunks])
    E = offsets[last] + align16(lens[last])        (= T rounded up to 16: every offset is a multiple of 16)

a call succeeds iff out_cap >= E, and whatever the status no byte outside [d_out, d_out + out_cap) is written.  The caps
with T <= out_cap < E are where a placement that compares the RAW length of the last chunk says OK and then stores whole
16-byte granules behind out_cap; they exist iff T % 16 != 0, and T % 16 == lens[last] % 16: only the last chunk's symbol
count matters.  Every row of CASES therefore runs with three last-chunk sizes ("tails"), found with the oracle alone
(find_tails) and frozen in the table: the smallest non-zero residue the format's unit allows, the largest, and 0.

Input: the oracle's generator (orc_gen_zipf; tests/test_gpu_scale.py proves bench.gen_zipf equal to it).  Its state is a
counter (splitmix64), so symbols [start, start + count) are gen_zipf(count, seed + start * GAMMA) -- the tail of a row with
10^5 chunks costs one chunk.  The static rows' model is counted from the first min(n, MODEL_SYMBOLS) symbols, every count + 1
(every symbol codable whatever the tail holds): it does not depend on the tail, so the search codes the last chunk only.

Shapes are the rows' smallest ones (full_chunks): the wave rows two chunks of 4096 symbols and the tail; the lane and group
rows the fewest chunks at which the library reports the row's kernel -- a dispatch fact the GPU test asserts through
last_encode_kernel(), not a workload size.  Those depend on the part's compute units (`cus`); the frozen tails are the ones
of 256 CUs (MI355X), another part searches its own (tails_for)."""
from collections import namedtuple

import numpy as np

from _around_coders import align16, aligned_total, ref_offsets  # (the offset scan's reference says it already)
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD
from ryg_rans_amd import OPT_ENC_SCRATCH_RING
from _batch import WAVES_PER_BLOCK
from _kernel_rows import B, FUSED, KERNEL_ROWS, L16, LANE_FUSED, RX, ST, W, WG, pick, regime_symbols

POISON = 0xA5
GUARD_BYTES = 4096
GUARD_ENTRIES = 8
SENTINEL = -1
GAMMA = 0x9E3779B97F4A7C15  # splitmix64's increment
MODEL_SYMBOLS = 1 << 16
FROZEN_CUS = 256

UNIT = {FMT_BYTE: 1, FMT_WORD: 2, FMT_R64: 4, FMT_ALIAS: 1}  # bytes a stream grows by


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------

def aligned_end(lens):
    """E: the capacity a compact container of these chunk lengths needs."""
    return aligned_total(lens)


def total(lens):
    """T: the container size the call reports, offsets[last] + lens[last]."""
    return int(ref_offsets(lens)[-1])


def caps_for(lens, bound):
    """The capacities a compact-layout case runs: [(label, out_cap, fits)], fits = out_cap >= E; duplicates removed, their
    labels joined.  `bound` is rans_amd_encode_bound() (the ample cap, a multiple of 16)."""
    lens = [int(v) for v in lens]
    offs = [int(v) for v in ref_offsets(lens)]
    last = len(lens) - 1
    T, E = offs[-1], aligned_end(lens)
    assert E == align16(T) and bound >= E and bound % 16 == 0, (T, E, bound)
    caps = [("bound", bound), ("E", E), ("E-1", E - 1), ("T", T), ("T-1", T - 1), ("offsets[last]", offs[last])]
    m = middle_chunk(lens)
    if m is not None:  # fits raw but not aligned, and nothing behind it fits
        caps.append(("offsets[%d]+lens[%d]" % (m, m), offs[m] + lens[m]))
    caps.append(("16", 16))
    out = []
    for label, cap in caps:
        for i, (l0, c0, f0) in enumerate(out):
            if c0 == cap:
                out[i] = (l0 + " = " + label, c0, f0)
                break
        else:
            out.append((label, cap, cap >= E))
    return out


def middle_chunk(lens):
    """The first chunk in front of the last whose length is no multiple of 16, or None."""
    for c in range(len(lens) - 1):
        if int(lens[c]) % 16:
            return c
    return None


def stream_mask(torch, offs, lens, size, device):
    """bool[size] on the device: True at the stream bytes [offs[c], offs[c] + lens[c]) -- the alignment gaps between the
    chunks are unspecified and stay False.  offs: the nchunks starts, lens: the nchunks lengths (host arrays)."""
    starts = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(device)
    ends = starts + torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).to(device)
    assert int(ends.max()) <= size
    delta = torch.zeros(size + 1, dtype=torch.int32, device=device)
    one = torch.ones(starts.numel(), dtype=torch.int32, device=device)
    delta.index_add_(0, starts, one)
    delta.index_add_(0, ends, -one)
    return torch.cumsum(delta[:size], 0, dtype=torch.int32) > 0


def arena(torch, count, front=GUARD_BYTES, back=GUARD_BYTES, dtype=None, fill=POISON, device="cuda"):
    """-> (whole, slice): `slice` is exactly `count` elements of `whole`, with `front` / `back` elements of `fill` on its
    sides (and `fill` inside).  A stray write lands in the test's own memory: the allocation never ends where the slice does."""
    dtype = torch.uint8 if dtype is None else dtype
    assert front > 0 and back > 0 and count >= 0
    whole = torch.full((front + count + back,), fill, dtype=dtype, device=device)
    part = whole[front:front + count]
    if dtype == torch.uint8:
        assert part.data_ptr() % 16 == 0
    assert part.numel() == count
    return whole, part


def index_arena(torch, count, dtype, device="cuda"):
    """d_offsets (exactly n_chunks + 1 entries) / d_lengths (exactly n_chunks): a slice of a sentinel-filled tensor."""
    return arena(torch, count, GUARD_ENTRIES, GUARD_ENTRIES, dtype, SENTINEL, device)


def guards_intact(whole, part, fill):
    """Nothing in front of the slice and nothing from its end on has changed."""
    front = part.storage_offset() - whole.storage_offset()
    return bool((whole[:front] == fill).all()) and bool((whole[front + part.numel():] == fill).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id row regime shape kernel placement opts tails")

# (W, B, WG, ST, L16, RX: the matrix's names of the word, byte, group and lane encoders)
R64, R64F, AL = "k_encode<r64>", "k_encode<r64 full-width>", "k_encode<alias, LDS remap>"
PCB, PCW = "k_encode<byte, per-chunk models>", "k_encode<word, per-chunk models>"

# tails: the last chunk's symbol count for (smallest non-zero residue, largest residue, residue 0) of T mod 16, at
# FROZEN_CUS compute units -- found by find_tails, re-derived by tests/test_capacity_cpu.py
CASES = [
    Case("word-64", "word-64", "U", "wave", W, 1, (), (84, 119, 1)),
    Case("word-64-unfused", "word-64-unfused", "U", "wave", W, 0, ((FUSED, 0),), (84, 119, 1)),
    Case("byte-64-14bit", "byte-64-14bit", "U", "wave", B, 1, (), (1, 53, 54)),
    Case("r64-64", "r64-64", "U", "wave", R64, 1, (), (194, 227, 1)),
    Case("r64-search-64", "r64-search-64", "U", "wave", R64F, 1, (), (194, 227, 1)),
    Case("alias256-64", "alias256-64", "U", "wave", AL, 1, (), (1, 53, 54)),
    Case("alias4096-64", "alias4096-64", "U", "wave", AL, 1, (), (1, 33, 35)),  # the mailbox in global memory
    Case("word-8", "word-8", "H", "groups", WG, 0, (), (11, 27, 1)),
    Case("word-4", "word-4", "U", "lanes16", L16, 0, (), (10, 25, 1)),
    Case("byte-2", "byte-2", "H", "staged", ST, 0, (), (12, 9, 11)),
    Case("byte-2-lane-fused", "byte-2-lane-fused", "H", "staged", ST, 1, ((LANE_FUSED, 1),), (12, 9, 11)),
    Case("r64-2-packed", "r64-2-packed", "H", "r64x2", RX, 0, (), (10, 20, 1)),
    Case("r64-2-lane-fused", "r64-2-lane-fused", "H", "staged", RX, 1, ((LANE_FUSED, 1),), (8, 21, 1)),
    Case("word-64-scratch-ring", "word-64", "R", "ring", W, 1, ((OPT_ENC_SCRATCH_RING, 1),), (68, 94, 1)),
    Case("byte-64-per-chunk-models", "byte-64-per-chunk-models", "U", "wave", PCB, 0, (), (65, 83, 1)),
    Case("word-64-per-chunk-models", "word-64-per-chunk-models", "U", "wave", PCW, 0, (), (1, 143, 2)),
]

# the (coding kernel, placement) pairs the compact layout can run, from reading KERNEL_ROWS' encode column: CASES must cover
# exactly these (tests/test_capacity_cpu.py) ...
MUST_COVER = {(W, 1), (W, 0), (B, 1), (R64, 1), (R64F, 1), (AL, 1), (WG, 0), (L16, 0), (ST, 0), (ST, 1), (RX, 0), (RX, 1),
              (PCB, 0), (PCW, 0)}
# ... and a pair the encode column names that is neither covered nor listed here fails there: a new encoder row must be
# given its place.  (Empty today: every pair the column names is a placement of the compact layout.)
NOT_COMPACT_PLACEMENT = set()

RESIDUE_LABELS = ("smallest", "largest", "zero")


def row_of(case):
    return next(r for r in KERNEL_ROWS if r["id"] == case.row)


def is_adaptive(case):
    return row_of(case)["kind"] == "adaptive"


def encode_pairs(rows=None):
    """Every (kernel, placement) the encode column of KERNEL_ROWS can name (the per-chunk-model rows name the coder of the
    three-launch path: layout + compaction behind it, placement 0)."""
    out = set()
    for r in KERNEL_ROWS if rows is None else rows:
        v = r["encode"]
        for w in (v.values() if isinstance(v, dict) else (v,)):
            out.add((w, 0) if isinstance(w, str) else tuple(w))
    return out


def expected_pair(case):
    """What KERNEL_ROWS says the library reports for the case's row in the case's regime."""
    row = row_of(case)
    v = pick(row["encode"], case.regime if case.regime in row["regimes"] else row["regimes"][0])
    return (v, 0) if isinstance(v, str) else tuple(v)


def full_chunks(case, cus):
    """Whole chunks in front of the tail chunk: the smallest shape that reaches the case's kernel and placement.
      wave     two chunks (and the tail: a middle chunk exists)
      lanes16  96: the lane encoders take 64 chunks and more, the per-lane one below six batches of 64 per CU
      groups   72: the group encoder takes the compact layout from 64 chunks on (nine octets and the tail's partial one)
      staged   64 (6 cus - 1): with the tail chunk exactly six batches per CU, the staged kernels' (and the lane-fused
               placement's) dispatch threshold itself
      r64x2    64 cus: one whole batch per CU, from which the unfused 2-way rans64 encoder runs
      ring     64 cus: with the tail one chunk more than two ring slots for each of a CU's 32 waves"""
    return {"wave": 2, "lanes16": 96, "groups": 72, "staged": 64 * (6 * cus - 1), "r64x2": 64 * cus, "ring": 64 * cus}[case.shape]


def symbols(case, cus, tail):
    return full_chunks(case, cus) * row_of(case)["chunk"] + tail


def zipf_slice(oracle, start, count, K, seed=1):
    """Symbols [start, start + count) of the oracle's gen_zipf(.., seed)."""
    return oracle.gen_zipf(count, K=K, s=1.0, seed=(seed + start * GAMMA) & 0xFFFFFFFFFFFFFFFF)


def model_freqs(oracle, case, cus):
    """The static rows' model: counts of the first min(full chunks, MODEL_SYMBOLS) symbols + 1, normalised."""
    row = row_of(case)
    head = zipf_slice(oracle, 0, min(full_chunks(case, cus) * row["chunk"], MODEL_SYMBOLS), row["K"])
    freqs, _ = oracle.normalize(oracle.count_freqs(head, row["K"]) + np.uint32(1), 1 << row["sb"])
    return freqs


class Coder:
    """The oracle's stream lengths of a case's chunks (static model or one model per chunk)."""

    def __init__(self, oracle, case, cus):
        self.oracle, self.case, self.cus, self.row = oracle, case, cus, row_of(case)
        self.adaptive = is_adaptive(case)
        if not self.adaptive:
            self.freqs = model_freqs(oracle, case, cus)
            self.model = oracle.model(self.freqs, self.row["sb"], with_alias=self.row["fmt"] == FMT_ALIAS)

    def length(self, syms):
        r = self.row
        if self.adaptive:
            return int(self.oracle.encode_chunked_adaptive(r["fmt"], syms, r["ways"], r["chunk"], r["sb"], threads=1)[2][0])
        return int(self.oracle.encode(r["fmt"], self.model, syms, r["ways"]).size)

    def chunk_syms(self, c, count=None):
        chunk = self.row["chunk"]
        return zipf_slice(self.oracle, c * chunk, chunk if count is None else count, self.row["K"])

    def tail_length(self, tail):
        return self.length(self.chunk_syms(full_chunks(self.case, self.cus), tail))

    def head_lengths(self, chunks):
        """The first min(chunks, full chunks) chunk lengths."""
        return [self.length(self.chunk_syms(c)) for c in range(min(chunks, full_chunks(self.case, self.cus)))]


def residues_of(case):
    """(smallest non-zero, largest, 0): T mod 16 moves in steps of the format's unit."""
    unit = UNIT[row_of(case)["fmt"]]
    return unit, 16 - unit, 0


def find_tails(oracle, case, cus):
    """The smallest last-chunk sizes whose oracle stream lengths have the three residues of residues_of(case)."""
    coder = Coder(oracle, case, cus)
    want = residues_of(case)
    found = {}
    start = full_chunks(case, cus) * coder.row["chunk"]
    syms = zipf_slice(oracle, start, coder.row["chunk"], coder.row["K"])
    for t in range(1, coder.row["chunk"] + 1):
        r = coder.length(syms[:t]) % 16
        if r in want and r not in found:
            found[r] = t
            if len(found) == len(set(want)):
                break
    assert len(found) == len(set(want)), (case.id, "residues reached", sorted(found), "wanted", want)
    return tuple(found[r] for r in want)


def tails_for(oracle, case, cus):
    return case.tails if cus == FROZEN_CUS else find_tails(oracle, case, cus)


def regime_chunks(case, cus):
    """Chunks of the matrix's regime for the case's row: the case's own shape is no larger (except the wave rows' second
    chunk, there for the middle cap)."""
    row = row_of(case)
    n, _ = regime_symbols(row, case.regime, cus * 2 * WAVES_PER_BLOCK)
    return (n + row["chunk"] - 1) // row["chunk"]
