"""What tests/test_batch_lanes_host.py and tests/test_gpu_batch_lanes.py share: the single wave-loads of the ragged 2-way rans64
lane decoder (k_decode_batch_r64_lanes, RANS_AMD_OPT_BATCH_LANES; its rows are tests/_kernel_rows.py's LANE_ROWS), the rate inputs
whose bounds the host file proves, and the damage catalogue with every verdict worked out on the CPU.

Nothing here needs a GPU: symbols are Oracle.gen_zipf's (bit-identical to bench.gen_zipf), streams the oracle's, verdicts
tests/_verdict.py's plain reference decoder's."""
import numpy as np

import _stream_rate as S
import _verdict as V
from _batch import mandatory_lengths, padded
from _oracle import FMT_R64

# ---- single wave-loads: the smallest shapes at which the parking can go wrong ---------------------------------------------
WAVE_LOADS = {
    "one-trip-each": [64] * 64,
    "boundaries": padded(64, [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193]),
    "63-parked-1023-trips": [65536] + [127] * 63,
    "every-lane-parks-elsewhere": [64 * (l % 16 + 1) + l for l in range(64)],
    "quad-mates-differ": [640, 0, 64, 385] * 16,
    "all-empty": [0] * 64,
    "second-load-of-one": [300] * 65,
    "mandatory-and-200s": padded(64, mandatory_lengths(2)),
}
ALIGNS = (1, 4, 64)

# ---- rate x phase x parking ------------------------------------------------------------------------------------------------
RATE_BITS = (14, 16)
RATE_STREAMS = 64
RATE_COUNTS = tuple(64 * b + t for b in (0, 1, 5) for t in (0, 1, 31, 63))
RATE_KINDS = ("rare", "common", "bursts")


def rate_kind(k):
    return RATE_KINDS[k % 3]


def rate_count(k):
    """Every count meets every kind: 12 counts against the period 3 of the kinds."""
    return RATE_COUNTS[(5 * k + k // 12) % len(RATE_COUNTS)]


def rate_content(freqs, kind, n, seed):
    if kind == "common":
        return S.common_only(freqs, n)
    if kind == "rare":
        return S.rare_only(freqs, n, seed)
    return S.bursts(freqs, n, seed, lead=8 * (seed % 8), run=16)


def rate_batch(sb):
    """-> (freqs, counts, {stream: symbols}, phases): 255 x 1 and one common symbol at 2^sb; stream k rare-only, common-only or
    bursts of 16 in turn, at offset == 4 k (mod 64) of a container packed by hand: every 4-byte phase of a 64-byte line."""
    freqs = S.lane_model(sb)
    counts = np.array([rate_count(k) for k in range(RATE_STREAMS)], dtype=np.uint32)
    contents = {k: rate_content(freqs, rate_kind(k), int(counts[k]), 800 + k) for k in range(RATE_STREAMS)}
    return freqs, counts, contents, [(4 * k) % 64 for k in range(RATE_STREAMS)]


# ---- the damage catalogue --------------------------------------------------------------------------------------------------
DAMAGE_KINDS = ("misaligned", "len-12", "behind", "len-4", "len+4", "state-bit", "stream-dword", "count-1", "count-64", "range")
REJECTED = ("misaligned", "len-12", "behind", "range")  # refused on the index entry: nothing read, nothing written
DAMAGE_LOADS = (64, 192)  # one wave-load and three


def damage_patterns(n):
    """Which streams are damaged -> {name: indices}: one stream, one lane of each quad position (in four different quads),
    every second stream, every stream."""
    return {"one": [min(n - 1, 37)], "quad-positions": [4 * 1 + 0, 4 * 6 + 1, 4 * 9 + 2, 4 * 14 + 3],
            "every-second": list(range(0, n, 2)), "every": list(range(n))}


class HostBatch:
    """n 2-way rans64 streams of 100..400 symbols (every stream has stream dwords behind its states and more than 64 symbols)
    under a 14-bit model, coded by the oracle, laid out by hand in a shuffled order: stream c at a 4-byte aligned offset (every
    phase of a 64-byte line) with SLACK zero bytes of its own behind it, which no damage touches (container_bytes counts the
    last stream's: a multiple of 16), the symbols of stream c at sym_offs[c] (sym_align 4, the mixed store paths) of an
    output of out_syms symbols."""
    SLACK = 512

    def __init__(self, oracle, n, seed=17):
        self.n, self.sb = n, 14
        rng = np.random.default_rng(seed + n)
        self.counts = rng.integers(100, 401, n).astype(np.uint32)
        dense = np.concatenate(([0], np.cumsum(self.counts.astype(np.int64))))
        syms = oracle.gen_zipf(int(dense[-1]), K=256, s=1.0, seed=1)
        sample = oracle.gen_zipf(1 << 20, K=256, s=1.0, seed=1)
        self.freqs, _ = oracle.normalize(oracle.count_freqs(sample, 256), 1 << self.sb)
        self.om = oracle.model(self.freqs, self.sb)
        self.ref = V.RefModel(FMT_R64, self.om)
        self.syms = [syms[dense[c]:dense[c + 1]] for c in range(n)]
        self.streams = [oracle.encode(FMT_R64, self.om, s, 2) for s in self.syms]
        self.lens = np.array([s.size for s in self.streams], dtype=np.uint32)
        self.offs = np.zeros(n, dtype=np.int64)
        at = 4
        for k, c in enumerate(rng.permutation(n)):
            at += 4 * int(rng.integers(1, 4))
            self.offs[c] = at
            at += int(self.lens[c]) + self.SLACK
        self.container_bytes = (at + 15) & ~15
        self.cont = np.zeros(self.container_bytes, dtype=np.uint8)
        for c in range(n):
            self.cont[self.offs[c]:self.offs[c] + self.lens[c]] = self.streams[c]
        self.sym_offs = np.concatenate(([0], np.cumsum((self.counts.astype(np.int64) + 3) & ~3)))
        self.out_syms = int(self.sym_offs[-1])


class Damaged:
    """One damage kind applied to the streams `which` of a HostBatch -> the arrays a decode_batch call takes, and per damaged
    stream what a correct decoder leaves: `bad` (the streams that must be counted), `written` {stream: symbols} for the
    damaged streams that ARE decoded (the reference decoder's symbols on the very bytes the kernel sees), the rest of the
    damaged streams untouched.  Stream damage is decisive only where the plain reference decoder (mode "raise") says BAD
    without needing a byte behind the stream's own slack -- zero bytes that belong to no stream and that no damage touches, so
    a kernel whose window is the container (the lane kernels') sees the bytes the reference saw whatever is done to the
    neighbours; positions that fail that are replaced by the next that pass, and `proofs` keeps every verdict."""

    def __init__(self, hb, kind, which):
        self.kind = kind
        self.cont, self.offs, self.lens = hb.cont.copy(), hb.offs.copy(), hb.lens.astype(np.int64).copy()
        self.counts, self.sym_offs = hb.counts.astype(np.int64).copy(), hb.sym_offs[:-1].copy()
        self.bad, self.written, self.proofs = [], {}, {}
        for c in which:
            off, ln, cnt = int(hb.offs[c]), int(hb.lens[c]), int(hb.counts[c])
            if kind == "misaligned":
                self.offs[c] = off + 2
            elif kind == "len-12":
                self.lens[c] = 12
            elif kind == "behind":
                self.offs[c] = hb.container_bytes + 16
            elif kind == "range":
                self.sym_offs[c] = hb.out_syms - cnt + 1  # one symbol past the end
            elif kind in ("len-4", "len+4"):
                self.lens[c] = ln + (4 if kind == "len+4" else -4)
                self._prove(hb, c, self.cont, off, cnt, int(self.lens[c]))
            elif kind in ("count-1", "count-64"):
                self.counts[c] = cnt - (1 if kind == "count-1" else 64)
                self._prove(hb, c, self.cont, off, int(self.counts[c]), ln)
            else:
                # state-bit: a bit of the low half of a flushed state, state 0 first (the state stays >= L); stream-dword: a bit in the
                # middle of the stream -- the first position whose verdict is decisive
                spots = [(off + 8 * (b // 32) + (b % 32) // 8, b % 8) for b in range(0, 64)] if kind == "state-bit" else \
                    [(off + 16 + 4 * ((ln - 16) // 8) + d // 8, d % 8) for d in range(0, 64)]
                for at, bit in spots:
                    trial = self.cont.copy()
                    trial[at] ^= 1 << bit
                    if self._prove(hb, c, trial, off, cnt, ln, keep=False):
                        self.cont[at] ^= 1 << bit
                        self._prove(hb, c, self.cont, off, cnt, ln)
                        break
                else:
                    raise AssertionError(("no decisive position", kind, c))
            if kind in REJECTED:
                self.proofs[c] = ("index", not V.index_rule(FMT_R64, 2, int(self.offs[c]), int(self.lens[c]), hb.container_bytes)
                                  or kind == "range")
            self.bad.append(c)

    def _prove(self, hb, c, cont, off, cnt, ln, keep=True):
        try:
            v = V.ref_decode(hb.ref, 2, cont, off, cnt, ln, off + int(hb.lens[c]) + hb.SLACK, mode="raise")
        except V.BeyondLimit:
            assert not keep, ("the reference needs bytes behind the stream's slack", self.kind, c)
            return False
        if keep:
            self.proofs[c] = ("stream", not v.good)
            self.written[c] = v.syms.astype(np.uint8)
        return not v.good

    def expected(self, hb, poison):
        """The output buffer a correct decode leaves (out_syms symbols)."""
        want = np.full(hb.out_syms, poison, dtype=np.uint8)
        for c in range(hb.n):
            lo = int(hb.sym_offs[c])
            if c in self.written:
                want[lo:lo + self.written[c].size] = self.written[c]
            elif c not in self.bad:
                want[lo:lo + int(hb.counts[c])] = hb.syms[c]
        return want
