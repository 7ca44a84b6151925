"""What tests/test_batch_singles_host.py and tests/test_gpu_batch_singles.py share: the reader of the registry's FOURTH list
(ryg_rans_amd/csrc/kernel_names.hpp, RANS_AMD_KERNEL_NAMES_SINGLES), the rows and one descriptor per format of the ragged 1-way
decoder with sixty-four streams per wave (k_decode_batch_singles<byte|word|r64|alias>, RANS_AMD_OPT_BATCH_SINGLES), its single
wave-loads, the rate inputs whose bounds the host file proves, a plain-integer 1-way decoder that counts the bytes of every
symbol, and the damage catalogue with every verdict worked out on the CPU by tests/_verdict.py's plain reference decoder.

Nothing here needs a GPU: symbols are Oracle.gen_zipf's (bit-identical to bench.gen_zipf), streams the oracle's."""
import functools
import os
import subprocess

import numpy as np

import _batch_lanes as L
import _stream_rate as S
import _verdict as V
import ryg_rans_amd as R
from _batch import mandatory_lengths, padded
from _kernel_rows import CSRC, HERE, ROOT, Family, registry
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

BATCH_SINGLES_DECODE = "batch_singles_decode"
OPT_BATCH_SINGLES = R.OPT_BATCH_SINGLES
FORMATS = ("byte", "word", "r64", "alias")
FMT = {"byte": FMT_BYTE, "word": FMT_WORD, "r64": FMT_R64, "alias": FMT_ALIAS}
FMT_NAME = {"byte": "FMT_BYTE", "word": "FMT_WORD", "r64": "FMT_R64", "alias": "FMT_ALIAS"}
KERNEL = {f: "k_decode_batch_singles<%s>" % f for f in FORMATS}
WAVE_DECODER = {f: "k_decode_batch<%s>" % f for f in FORMATS}
WAVE_ENCODER = {"byte": "k_encode_batch<byte>", "word": "k_encode_batch<word>", "r64": "k_encode_batch<r64>",
                "alias": "k_encode_batch<alias, LDS remap>"}
FIRST_ID = 56  # the third list ends at 55
UNIT, STATE_BYTES = V.UNIT, V.STATE_BYTES


@functools.lru_cache(maxsize=None)
def fourth_list():
    """[(family, name, id)]: every entry of the fourth list, as tests/kernel_names_singles_driver.cpp prints them (the driver
    fails on a name or a family of the first three lists, and on ids that do not follow the third list's)."""
    build = os.path.join(ROOT, "build", "kernel_names")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "kernel_names_singles_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "kernel_names_singles_driver.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return [(f, n, int(i)) for f, n, i in (ln.split("\t") for ln in out.splitlines())]


def fourth_list_names(family=BATCH_SINGLES_DECODE):
    return {name for f, name, _ in fourth_list() if f == family}


# ---- sixty-four 1-way streams per wave, every format: the decoder's rows (tests/test_gpu_batch_singles.py)
def _row(f, suffix, sb, K):
    return {"id": "%s-1-singles%s" % (f, suffix), "fmt": FMT[f], "sb": sb, "K": K, "ways": 1, "decode": KERNEL[f], "encode": WAVE_ENCODER[f]}


SINGLE_ROWS = {
    "byte": [_row("byte", "", 14, 256),            # the reference's scale_bits (main.cpp:139)
             _row("byte", "-16bit", 16, 256),      # 64 KiB of cum2sym: ten waves per block
             _row("byte", "-12bit", 12, 256),      # (the wave kernel would take the fused slot records here)
             _row("byte", "-8bit", 8, 256),
             _row("byte", "-64sym-10bit", 10, 64)],
    "word": [_row("word", "", 12, 256)],           # rans_word_sse41.h:37 fixes 12 bits
    "r64": [_row("r64", "", 14, 256),              # the reference's (main64.cpp)
            _row("r64", "-16bit", 16, 256),
            _row("r64", "-12bit", 12, 256),
            _row("r64", "-64sym-7bit", 7, 64),     # the smallest cum2sym table
            _row("r64", "-64sym-10bit", 10, 64)],
    "alias": [_row("alias", "", 16, 256),          # the reference's (main_alias.cpp: prob_bits 16)
              _row("alias", "-14bit", 14, 256),
              _row("alias", "-12bit", 12, 256),
              _row("alias", "-8bit", 8, 256),      # one slot per bucket, bucket shift 0
              _row("alias", "-64sym-10bit", 10, 64)],
}
ALL_ROWS = [r for f in FORMATS for r in SINGLE_ROWS[f]]
MAIN = {f: SINGLE_ROWS[f][0] for f in FORMATS}
SHAPES = {f: sorted((r["sb"], r["K"]) for r in SINGLE_ROWS[f]) for f in FORMATS}
# the rows of rate_batch: the scale_bits at which a frequency-1 symbol costs the most a valid stream can pay
RATE_SB = {"byte": 16, "word": 12, "r64": 16, "alias": 16}
RATE_ROW = {f: next(r for r in SINGLE_ROWS[f] if r["sb"] == RATE_SB[f] and r["K"] == 256) for f in FORMATS}
SINGLES = {f: Family(OPT_BATCH_SINGLES, "decode", FMT[f], 1, 64, SINGLE_ROWS[f], MAIN[f], WAVE_DECODER[f], BATCH_SINGLES_DECODE, SHAPES[f],
                     (FMT_NAME[f], MAIN[f]["sb"], "OPT_BATCH_SINGLES")) for f in FORMATS}
# shapes that keep the wave kernels with the option on, beside tests/_kernel_rows.py's ROW
ALIAS_U16_1_WAVE = {"id": "alias-u16-1", "fmt": FMT_ALIAS, "sb": 16, "K": 1024, "ways": 1, "decode": WAVE_DECODER["alias"],
                    "encode": WAVE_ENCODER["alias"]}
ALIAS_2_WAVE = {"id": "alias-2", "fmt": FMT_ALIAS, "sb": 16, "K": 256, "ways": 2, "decode": WAVE_DECODER["alias"], "encode": WAVE_ENCODER["alias"]}


def check_fourth_list_rows(rows=None):
    """tests/_kernel_rows.py check_family_rows for the fourth list (registry() knows the first list's families alone): the
    family's names are the decode kernels of the rows, in both directions; every format's rows are its shapes, 1-way, and name
    its wave encoder; no name is in a family of the first list."""
    rows = ALL_ROWS if rows is None else rows
    names = fourth_list_names()
    got = {r["decode"] for r in rows}
    assert names == got, ("kernels no row expects", sorted(names - got), "names no launcher reports", sorted(got - names))
    for f in FORMATS:
        d = SINGLES[f]
        mine = [r for r in rows if r["fmt"] == d.fmt]
        assert all(r["ways"] == 1 and r["decode"] == KERNEL[f] and r["encode"] == WAVE_ENCODER[f] for r in mine)
        assert d.main["decode"] in names
    assert all(not (names & ns) for ns in registry().values()) and BATCH_SINGLES_DECODE not in registry()


# ---- single wave-loads: the smallest shapes at which the exec masking of trips and tails can go wrong -------------------------
WAVE_LOADS = {
    "one-trip-each": [64] * 64,
    "boundaries": padded(64, [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193]),
    "63-idle-1023-trips": [65536] + [127] * 63,
    "every-lane-ends-elsewhere": [64 * (l % 16 + 1) + l for l in range(64)],
    "quad-mates-differ": [640, 0, 64, 385] * 16,
    "all-empty": [0] * 64,
    "second-load-of-one": [300] * 65,
    "mandatory-and-200s": padded(64, mandatory_lengths(1)),
}
ALIGNS = (1, 4, 64)

# ---- rate x phase ----------------------------------------------------------------------------------------------------------
RATE_STREAMS, RATE_COUNTS, RATE_KINDS = L.RATE_STREAMS, L.RATE_COUNTS, L.RATE_KINDS
rate_kind, rate_count = L.rate_kind, L.rate_count


def rate_batch(f):
    """-> (freqs, counts, {stream: symbols}, phases): 255 x 1 and one common symbol at 2^RATE_SB[f]; stream k rare-only,
    common-only or bursts of 16 in turn, its count one of 64 b + t, at offset == k * unit (mod 64) of a container packed by hand:
    every unit phase of a 64-byte line."""
    freqs = S.lane_model(RATE_SB[f])
    counts = np.array([rate_count(k) for k in range(RATE_STREAMS)], dtype=np.uint32)
    contents = {k: L.rate_content(freqs, rate_kind(k), int(counts[k]), 800 + k) for k in range(RATE_STREAMS)}
    return freqs, counts, contents, [(UNIT[FMT[f]] * k) % 64 for k in range(RATE_STREAMS)]


def symbol_bytes(ref, stream, n):
    """A 1-way stream of n symbols decoded by plain integers (the reference's per-symbol loops, as tests/_verdict.py's
    ref_decode writes them) -> (symbols, stream bytes taken behind every symbol).  The state must end at L and the cursor at
    the stream's end."""
    fmt, sb = ref.fmt, ref.sb
    s = bytes(memoryview(np.ascontiguousarray(stream, dtype=np.uint8)))
    sbytes, Lv, unit, mask = STATE_BYTES[fmt], V.L_OF[fmt], UNIT[fmt], (1 << sb) - 1
    x = int.from_bytes(s[:sbytes], "little")
    cur, out, taken = sbytes, np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.int64)
    import bisect
    for i in range(n):
        if fmt == FMT_ALIAS:  # main_alias.cpp:252-267
            xm = x & mask
            bucket = xm >> (sb - ref.log2nsyms)
            half = 2 * bucket + (1 if xm < ref.divider[bucket] else 0)
            out[i] = ref.sym_id[half]
            x = (ref.slot_freqs[half] * (x >> sb) + xm - ref.slot_adjust[half]) & 0xffffffff
        else:
            cf = x & mask
            sy = bisect.bisect_right(ref.cum, cf) - 1
            out[i] = sy
            x = ref.freqs[sy] * (x >> sb) + cf - ref.cum[sy]
        while x < Lv:  # `if` in the word and rans64 formats: one unit always brings a valid state back
            x = (x << (8 * unit)) | int.from_bytes(s[cur:cur + unit], "little")
            cur += unit
            taken[i] += unit
        assert taken[i] <= (2 if unit == 1 else unit), (i, int(taken[i]))
    assert x == Lv and cur == len(s), (x, cur, len(s))
    return out, taken


def word_group_bound():
    """The most bytes sixteen symbols of a valid 1-way WORD stream take, from the format alone (rans_word_sse41.h:123-141): a
    symbol removes at most 12 bits from the state (frequency 1: x = x >> 12), a word comes in when the state is below 2^16 and
    brings it to 2^16 times what it was at the least.  Behind a symbol that took no word the state is >= 2^16; then >= 2^4,
    a word, >= 2^20; >= 2^8, a word, >= 2^24; >= 2^12, a word, >= 2^28; >= 2^16: NO word.  So at most three symbols in a row
    take a word, a group starts no better than behind a symbol without one (its state is >= 2^16 as well), and sixteen symbols
    take at most 12 words.  The walk below is that argument on the least bit length a state can have."""
    most = 0
    for start in range(16, 32):  # bit length - 1 of the state in front of the group: x in [2^16, 2^32)
        k, words = start, 0
        for _ in range(16):
            k -= 12
            if k < 16:
                k += 16
                words += 1
        most = max(most, words)
    return 2 * most


# ---- the damage catalogue --------------------------------------------------------------------------------------------------
DAMAGE_KINDS = ("misaligned", "len-short", "behind", "len-unit", "len+unit", "state-bit", "stream-unit", "count-1", "count-64", "range")
REJECTED = ("misaligned", "len-short", "behind", "range")  # refused on the index entry: nothing read, nothing written
DAMAGE_LOADS = L.DAMAGE_LOADS  # one wave-load and three
damage_patterns = L.damage_patterns


def damage_kinds(f):
    """A misaligned offset exists where the unit is more than a byte."""
    return tuple(k for k in DAMAGE_KINDS if k != "misaligned" or UNIT[FMT[f]] > 1)


class HostBatch:
    """n 1-way streams of format f of 100..400 symbols (every stream has stream units behind its state and more than 64
    symbols) under the main row's model, coded by the oracle, laid out by hand in a shuffled order: stream c at a unit-aligned
    offset (every phase of a 64-byte line) with SLACK zero bytes of its own behind it, which no damage touches
    (container_bytes counts the last stream's: a multiple of 16), the symbols of stream c at sym_offs[c] (sym_align 4: the
    mixed store paths) of an output of out_syms symbols."""
    SLACK = 512

    def __init__(self, oracle, f, n, seed=17):
        self.f, self.fmt, self.n, self.sb = f, FMT[f], n, MAIN[f]["sb"]
        unit = UNIT[self.fmt]
        rng = np.random.default_rng(seed + n)
        self.counts = rng.integers(100, 401, n).astype(np.uint32)
        dense = np.concatenate(([0], np.cumsum(self.counts.astype(np.int64))))
        syms = oracle.gen_zipf(int(dense[-1]), K=256, s=1.0, seed=1)
        sample = oracle.gen_zipf(1 << 20, K=256, s=1.0, seed=1)
        self.freqs, _ = oracle.normalize(oracle.count_freqs(sample, 256), 1 << self.sb)
        self.om = oracle.model(self.freqs, self.sb, with_alias=self.fmt == FMT_ALIAS)
        self.ref = V.RefModel(self.fmt, self.om)
        self.syms = [syms[dense[c]:dense[c + 1]] for c in range(n)]
        self.streams = [oracle.encode(self.fmt, self.om, s, 1) for s in self.syms]
        self.lens = np.array([s.size for s in self.streams], dtype=np.uint32)
        self.offs = np.zeros(n, dtype=np.int64)
        at = unit
        for k, c in enumerate(rng.permutation(n)):
            at += unit * int(rng.integers(1, 4))
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
    damaged streams untouched.  tests/_batch_lanes.py's rule: stream damage is decisive only where the plain reference decoder
    (mode "raise") says BAD without needing a byte behind the stream's own slack -- zero bytes that belong to no stream and
    that no damage touches -- and, in the byte formats, without a step that wants more than the two bytes the reference's loop
    can need on a stream of the format; positions that fail that are replaced by the next that pass, and `proofs` keeps every
    verdict."""

    def __init__(self, hb, kind, which):
        self.kind = kind
        fmt = hb.fmt
        unit, sbytes = UNIT[fmt], STATE_BYTES[fmt]
        self.cont, self.offs, self.lens = hb.cont.copy(), hb.offs.copy(), hb.lens.astype(np.int64).copy()
        self.counts, self.sym_offs = hb.counts.astype(np.int64).copy(), hb.sym_offs[:-1].copy()
        self.bad, self.written, self.proofs = [], {}, {}
        for c in which:
            off, ln, cnt = int(hb.offs[c]), int(hb.lens[c]), int(hb.counts[c])
            if kind == "misaligned":
                assert unit > 1
                self.offs[c] = off + unit // 2
            elif kind == "len-short":
                self.lens[c] = sbytes - unit
            elif kind == "behind":
                self.offs[c] = hb.container_bytes + 16
            elif kind == "range":
                self.sym_offs[c] = hb.out_syms - cnt + 1  # one symbol past the end
            elif kind in ("len-unit", "len+unit"):
                self.lens[c] = ln + (unit if kind == "len+unit" else -unit)
                self._prove(hb, c, self.cont, off, cnt, int(self.lens[c]))
            elif kind in ("count-1", "count-64"):
                self.counts[c] = cnt - (1 if kind == "count-1" else 64)
                self._prove(hb, c, self.cont, off, int(self.counts[c]), ln)
            else:
                # state-bit: a bit of the low half of the flushed state (the state stays >= L); stream-unit: a bit in the middle
                # of the stream -- the first position whose verdict is decisive
                half = 4 * sbytes
                spots = [(off + b // 8, b % 8) for b in range(0, half)] if kind == "state-bit" else \
                    [(off + sbytes + unit * ((ln - sbytes) // (2 * unit)) + d // 8, d % 8) for d in range(0, 64)]
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
                self.proofs[c] = ("index", not V.index_rule(fmt, 1, int(self.offs[c]), int(self.lens[c]), hb.container_bytes)
                                  or kind == "range")
            self.bad.append(c)

    def _prove(self, hb, c, cont, off, cnt, ln, keep=True):
        try:
            v = V.ref_decode(hb.ref, 1, cont, off, cnt, ln, off + int(hb.lens[c]) + hb.SLACK, mode="raise")
        except V.BeyondLimit:
            assert not keep, ("the reference needs bytes behind the stream's slack", self.kind, c)
            return False
        if v.max_units > 2:
            assert not keep, ("a step that wants more than two bytes", self.kind, c)
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
