"""A plain reference decoder WITH A VERDICT, and the damage catalogue of tests/test_verdict_cpu.py / tests/test_gpu_verdict.py.

ref_decode is integer-only Python over the reference's per-symbol loops (rans_byte.h:125-128 / :291-298 / :307-318,
rans_word_sse41.h:123-141, rans64.h:118-121 / :286-316, main_alias.cpp:252-267) at N-way interleave: initial states in
RansDecInit order (lane 0 first), symbol i on lane i mod N, the stream read forward.  Besides the symbols it says what the
header's rule (include/ryg_rans_amd.h, rans_amd_decode) says of the chunk: GOOD iff every final state == L and the bytes
consumed == the claimed length.  Reads at or behind `limit` either raise (mode "raise": the proofs) or return zeros (mode
"zeros": what a buffer descriptor whose num_records is the chunk's 16-byte rounded length returns -- the stream windows of
decode_common.hpp).  The model's tables (freqs, cum, the alias tables) are the oracle's; everything that is decoding is here.

A CASE is a container, an index, a symbol count and what a correct decoder must do with them, made on the CPU alone:

    make_case(shape, layout, damage)    damage: a list of (chunk, entry), at most one entry per chunk

Every chunk's verdict is PROVED here before a GPU test may assert it (Case.proofs, checked by test_verdict_cpu.py):

  index damage   I1 off + unit / 2 (word, rans64: no multiple of the unit)      the header's rule evaluated on integers says
                 I2 len = N * state_bytes - unit                                 "rejected": no byte of such a chunk is read
                 I3 off + len one unit behind container_bytes                    and, by the reading of every kernel, none of
                 I4 off == container_bytes, len > 0                              its symbols written: its output stays poison
                 I5 off = container_bytes + 16
                 I6 len = 2^20 (the containers here are smaller)
  stream damage  S1 len - unit, S2 len + unit, both ending in the chunk's own last 16-byte granule and inside the container
                 S3 one bit of the low half of a flushed state flipped (the state stays >= L, as in every stream)
                 S4 one byte in the middle of the stream flipped
                 S5 (the call's n lowered: the last chunk is told fewer symbols than it was coded for)
                 -> ref_decode in mode "raise" with limit = the end of the chunk's own last granule, (skip + len' + 15) & ~15
                    from the granule that holds `off`: the verdict must be BAD and no byte at or behind the limit needed --
                    every kernel then sees the bytes the reference saw, must count the chunk once, and must write the
                    reference's garbage symbols.  A position that fails the proof is replaced by the next one that passes.
                 S6 len shortened by whole granules: ref_decode in mode "zeros" -- asserted on the kernels whose window is a
                    descriptor of the chunk (DESCRIPTOR_KERNELS) only
  model damage   M1 / M2 / M3 a per-chunk model row that sums to M - 1, to M + 1, or holds one frequency > M: the rule of
                 tests/_model_extremes.py's CPU side (a row is a model iff it sums to M) rejects all three; adapt_build_dec
                 (device_common.hpp) checks exactly the sum
  healthy edges  H1 a last chunk of N * state_bytes (a few symbols of the most probable symbol), H2 a container that ends
                 1 / 15 / 0 bytes (word: 2 / 14, rans64: 4 / 12) behind a 16-byte boundary with its last chunk: count 0
  R1             the last chunk holds the stream of HALF its symbols and is told all: the reference (zeros) needs more
                 than 16 bytes behind container_bytes
"""
import bisect

import numpy as np

from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

L_OF = {FMT_BYTE: 1 << 23, FMT_ALIAS: 1 << 23, FMT_WORD: 1 << 16, FMT_R64: 1 << 31}
UNIT = {FMT_BYTE: 1, FMT_ALIAS: 1, FMT_WORD: 2, FMT_R64: 4}
STATE_BYTES = {FMT_BYTE: 4, FMT_ALIAS: 4, FMT_WORD: 4, FMT_R64: 8}
POISON = 0x5A
GAP = 0xA5           # what lies between the streams of a hand-laid container
MARGIN = (1 << 20) + 8192  # arena on both sides of the container: more than the largest len used (2^20) + 4 KiB

# the kernels whose stream window is a buffer descriptor of the CHUNK (decode_common.hpp StreamWindow::stream_rsrc,
# decode_wave.hip chunk_rsrc): reads behind the chunk's own last granule return zeros.  The lane kernels read the container up
# to ITS last granule (decode_lanes.hip glimit / the batch window of k_decode_lanes_r64x2), the group kernels likewise
# (decode_groups.hip glimit): behind a shortened chunk they see the next chunk's bytes, which S6 does not model.
DESCRIPTOR_KERNELS = ("k_decode_word64", "k_decode<word>", "k_decode<byte>", "k_decode<byte, slot records>", "k_decode<r64>",
                      "k_decode<r64 search>", "k_decode<word, u16 symbols>", "k_decode<alias>", "k_decode_dual<alias>",
                      "k_decode<byte, per-chunk models>", "k_decode<word, per-chunk models>")


class BeyondLimit(Exception):
    pass


class RefModel:
    """The oracle's tables as Python integers."""

    def __init__(self, fmt, om):
        self.fmt, self.sb, self.nsyms = fmt, om.scale_bits, om.nsyms
        self.freqs = [int(v) for v in om.table("freqs", om.nsyms)]
        self.cum = [int(v) for v in om.table("cum", om.nsyms + 1)]
        if fmt == FMT_ALIAS:
            self.log2nsyms = int(om.ptr.contents.log2nsyms)
            self.divider = [int(v) for v in om.table("divider", om.nsyms)]
            self.slot_adjust = [int(v) for v in om.table("slot_adjust", 2 * om.nsyms)]
            self.slot_freqs = [int(v) for v in om.table("slot_freqs", 2 * om.nsyms)]
            self.sym_id = [int(v) for v in om.table("sym_id", 2 * om.nsyms)]


class Verdict:
    __slots__ = ("syms", "states", "consumed", "needed_beyond", "good", "max_units", "last_read")

    def __repr__(self):
        return "Verdict(good=%s consumed=%d beyond=%s)" % (self.good, self.consumed, self.needed_beyond)


def ref_decode(model, ways, buf, off, nsym, length, limit, mode="raise"):
    """Decode nsym symbols of the chunk at buf[off:]; `length` is the CLAIMED length (the verdict's), `limit` >= off + length
    the absolute position from which on reads raise BeyondLimit / return zeros."""
    fmt = model.fmt
    assert limit >= off + length and mode in ("raise", "zeros")
    data = bytes(memoryview(np.ascontiguousarray(buf[off:min(limit, len(buf))])))
    if limit > len(buf):  # the padding of the container's last granule: the GPU test's arena holds GAP there
        assert limit - len(buf) < 16
        data += bytes([GAP]) * (limit - len(buf))
    span = limit - off
    assert len(data) == span, "the limit lies outside the buffer"
    v = Verdict()
    v.needed_beyond, v.max_units, v.last_read = False, 0, -1
    pos = 0

    def take(k):
        nonlocal pos
        got = data[pos:pos + k]
        if len(got) < k:
            v.needed_beyond = True
            if mode == "raise":
                raise BeyondLimit(pos + off)
            got = got + bytes(k - len(got))
        pos += k
        v.last_read = off + pos - 1
        return int.from_bytes(got, "little")

    sbytes, Lv, sb = STATE_BYTES[fmt], L_OF[fmt], model.sb
    mask = (1 << sb) - 1
    x = [take(sbytes) for _ in range(ways)]
    out = np.zeros(nsym, dtype=np.uint16)
    freqs, cum = model.freqs, model.cum
    for i in range(nsym):
        lane = i % ways
        xv = x[lane]
        if fmt == FMT_ALIAS:  # main_alias.cpp:252-267 (32-bit wrap-around is intended)
            xm = xv & mask
            bucket = xm >> (sb - model.log2nsyms)
            half = 2 * bucket + (1 if xm < model.divider[bucket] else 0)
            s = model.sym_id[half]
            xv = (model.slot_freqs[half] * (xv >> sb) + xm - model.slot_adjust[half]) & 0xffffffff
        else:
            cf = xv & mask
            s = bisect.bisect_right(cum, cf) - 1
            xv = freqs[s] * (xv >> sb) + cf - cum[s]
            if fmt != FMT_R64:
                xv &= 0xffffffff
        out[i] = s
        if fmt == FMT_R64:  # rans64.h:305-316
            if xv < Lv:
                xv = ((xv << 32) | take(4)) & 0xffffffffffffffff
        elif fmt == FMT_WORD:  # rans_word_sse41.h:134-141
            if xv < Lv:
                xv = ((xv << 16) | take(2)) & 0xffffffff
        else:  # rans_byte.h:307-318; a stream's states never need more than two bytes (x >= 2^7 behind D): four is "damaged"
            units = 0
            while xv < Lv and units < 4:
                xv = ((xv << 8) | take(1)) & 0xffffffff
                units += 1
            v.max_units = max(v.max_units, units)
        x[lane] = xv
    v.syms, v.states, v.consumed = out, x, pos
    v.good = all(s == Lv for s in x) and pos == length
    return v


def granule_limit(off, length):
    """The end of the chunk's own last 16-byte granule: (skip + len + 15) & ~15 from the granule that holds off."""
    skip = off & 15
    return (off - skip) + ((skip + length + 15) & ~15)


def index_rule(fmt, ways, off, length, container_bytes):
    """The header's rule for an index entry, in the two-compare form that cannot wrap."""
    return off % UNIT[fmt] == 0 and length >= ways * STATE_BYTES[fmt] and off <= container_bytes and length <= container_bytes - off


# ---- shapes -----------------------------------------------------------------------------------------------------------

def _row(rid, fmt, sb, K, ways, chunk, unit, kernel, chunks, kind="static", big=False, opts=()):
    return {"id": rid, "fmt": fmt, "sb": sb, "K": K, "ways": ways, "chunk": chunk, "unit": unit, "kernel": kernel,
            "chunks": chunks, "kind": kind, "big": big, "opts": tuple(opts)}


# One row for every decoder rans_amd_decode / rans_amd_decode_adaptive[_fmt] can report: the shapes of
# tests/test_gpu_kernel_matrix.py KERNEL_ROWS at small chunks that still hold a stream behind their states (a lane's first
# symbols renormalise nothing: 16 symbols per lane for the wave kernels).  `chunks`: full chunks (a ragged one
# of chunk // 3 + 1 symbols follows); `unit`: chunks per work unit.  k_decode_word64 has two rows: 256 symbols are one group
# of four rounds (groups <= kClaimAhead: both hand-over steps are issued behind the loop), 4096 are sixteen (issued inside).
VERDICT_ROWS = [
    _row("word-64-short", FMT_WORD, 12, 256, 64, 256, 1, "k_decode_word64", 11),
    _row("word-64-long", FMT_WORD, 12, 256, 64, 4096, 1, "k_decode_word64", 11),
    _row("word-128", FMT_WORD, 12, 256, 128, 2048, 1, "k_decode<word>", 9),
    _row("word-u16-64", FMT_WORD, 12, 1024, 64, 1024, 1, "k_decode<word, u16 symbols>", 9),
    _row("byte-64-14bit", FMT_BYTE, 14, 256, 64, 1024, 1, "k_decode<byte>", 9),
    _row("byte-64-12bit", FMT_BYTE, 12, 256, 64, 1024, 1, "k_decode<byte, slot records>", 9),
    _row("r64-64", FMT_R64, 14, 256, 64, 1024, 1, "k_decode<r64>", 9),
    _row("r64-search-64", FMT_R64, 20, 256, 64, 1024, 1, "k_decode<r64 search>", 9),
    _row("alias256-64", FMT_ALIAS, 16, 256, 64, 1024, 1, "k_decode<alias>", 9),
    # (the paired path of k_decode_dual takes chunks that are whole groups of four rounds: 256 symbols)
    # (11 chunks: the ragged last one is unpaired; 10 chunks: the last pair's B is the ragged one and both go singly)
    _row("alias4096-64-11-chunks", FMT_ALIAS, 16, 4096, 64, 256, 2, "k_decode_dual<alias>", 10),
    _row("alias4096-64-10-chunks", FMT_ALIAS, 16, 4096, 64, 256, 2, "k_decode_dual<alias>", 9),
    # (u8 symbols through the same kernel's four-round groups: RANS_AMD_OPT_DUAL_DECODE = 2, as tests/test_gpu_kernel_matrix.py)
    _row("alias256-64-dual", FMT_ALIAS, 16, 256, 64, 256, 2, "k_decode_dual<alias>", 10, opts=((3, 2),)),
    _row("word-8", FMT_WORD, 12, 256, 8, 32, 8, "k_decode_word_groups", 28),
    _row("byte-2", FMT_BYTE, 14, 256, 2, 64, 32, "k_decode_byte_pairs", 80),
    _row("r64-2-packed", FMT_R64, 14, 256, 2, 64, 64, "k_decode_lanes_r64x2<packed slots>", 160),
    _row("r64-2-16bit", FMT_R64, 16, 256, 2, 64, 64, "k_decode_lanes_r64x2", 160),
    _row("word-4", FMT_WORD, 12, 256, 4, 36, 64, "k_decode_lanes_staged", 160),
    _row("byte-2-huge-chunks", FMT_BYTE, 14, 256, 2, (1 << 19) + 2, 64, "k_decode_lanes", 65, big=True),
    _row("byte-64-per-chunk-models", FMT_BYTE, 12, 256, 64, 1024, 1, "k_decode<byte, per-chunk models>", 9, kind="adaptive"),
    _row("word-64-per-chunk-models", FMT_WORD, 12, 256, 64, 1024, 1, "k_decode<word, per-chunk models>", 9, kind="adaptive"),
]
ROW_BY_ID = {r["id"]: r for r in VERDICT_ROWS}

_SHAPES = {}


class Shape:
    """A row's input, model and the oracle's stream of every chunk (made once per process)."""

    def __init__(self, oracle, row, variant=None):
        """variant "h1": the last chunk is three symbols of the most probable symbol (H1); "r1": the last chunk is a full
        one whose stream codes only the first half of its symbols (R1)."""
        self.row = row
        fmt, sb, K, ways, chunk = row["fmt"], row["sb"], row["K"], row["ways"], row["chunk"]
        if variant == "r1":  # (the second half must renormalise more than 16 bytes' worth: 256 symbols and more)
            chunk = max(chunk, 256)
        self.fmt, self.sb, self.ways, self.chunk = fmt, sb, ways, chunk
        self.n = row["chunks"] * chunk + (chunk if variant == "r1" else chunk // 3 + 1)
        syms = oracle.gen_zipf(self.n, K, 1.0, 1)
        self.adaptive = row["kind"] == "adaptive"
        self._oracle = oracle
        self._ref_models, self._oms = {}, {}
        if not self.adaptive:
            self.freqs, _ = oracle.normalize(oracle.count_freqs(syms, K), 1 << sb)
            if variant == "h1":
                self.n = row["chunks"] * chunk + 3
                syms = syms[:self.n].copy()
                syms[row["chunks"] * chunk:] = int(np.argmax(self.freqs))
            self.om = oracle.model(self.freqs, sb, with_alias=fmt == FMT_ALIAS)
            self.ref_model = RefModel(fmt, self.om)
            cont, offs, lens = oracle.encode_chunked_mt(fmt, self.om, syms, ways, chunk)
            self.rows = None
        else:
            assert variant != "h1"
            cont, offs, lens, rows = oracle.encode_chunked_adaptive(fmt, syms, ways, chunk, sb)
            self.rows = rows.copy()
            self.freqs = None
        self.syms = syms
        self.nchunks = (self.n + chunk - 1) // chunk
        self.streams = [cont[int(offs[c]):int(offs[c]) + int(lens[c])].copy() for c in range(self.nchunks)]
        self.r1_half = None
        if variant == "r1":
            c = self.nchunks - 1
            self.r1_half = chunk // 2
            self.streams[c] = oracle.encode(fmt, self.oracle_model_of(c), syms[c * chunk:c * chunk + self.r1_half], ways)

    def oracle_model_of(self, c):
        if not self.adaptive:
            return self.om
        if c not in self._oms:
            self._oms[c] = self._oracle.model(self.rows[c].astype(np.uint32), self.sb)
        return self._oms[c]

    def model_of(self, c):
        if not self.adaptive:
            return self.ref_model
        if c not in self._ref_models:
            self._ref_models[c] = RefModel(self.fmt, self.oracle_model_of(c))
        return self._ref_models[c]

    def nsym_of(self, c, n=None):
        n = self.n if n is None else n
        return max(0, min(self.chunk, n - c * self.chunk))


def shape_of(oracle, row, variant=None):
    key = (row["id"], variant)
    if key not in _SHAPES:
        _SHAPES[key] = Shape(oracle, row, variant)
    return _SHAPES[key]


def make_r1(shape, layout="compact"):
    """R1 (shape variant "r1"): the case, and the verdict of the reference in mode "zeros" on its last chunk."""
    case = make_case(shape, layout, [])
    c = shape.nchunks - 1
    off, ln = int(case.offs[c]), int(case.lens[c])
    v = ref_decode(shape.model_of(c), shape.ways, case.cont, off, shape.chunk, ln, granule_limit(off, ln), "zeros")
    case.out[c * shape.chunk:] = v.syms
    case.flagged.append(c)
    case.count = 1
    case.damaged = [c]
    case.proofs.append((c, "R1", "zeros", v.good, v.max_units > 2))
    return case, v


# ---- layouts ----------------------------------------------------------------------------------------------------------

def lay_out(shape, layout, end_mod=None):
    """-> (container u8[total], offs int64[nchunks + 1], lens int64[nchunks]).
    "compact": 16-byte starts (rans_amd_encode); "slots": 16-byte ENDS in slots of one size (rans_amd_encode_slots);
    "sized": slots of whole 64-byte lines that hold the median stream, longer streams in worst-case slots behind them
    (rans_amd_encode_slots_sized).  end_mod (compact): the last chunk is moved down so that the container ends end_mod bytes
    behind a 16-byte boundary."""
    lens = np.array([s.size for s in shape.streams], dtype=np.int64)
    nc = lens.size
    offs = np.zeros(nc + 1, dtype=np.int64)
    if layout == "compact":
        pos = 0
        for c in range(nc):
            pos = (pos + 15) & ~15
            if end_mod is not None and c == nc - 1:
                pos += (end_mod - (pos + int(lens[c]))) % 16
                assert pos % UNIT[shape.fmt] == 0
            offs[c] = pos
            pos += int(lens[c])
        total = pos
    elif layout == "slots":
        S = ((int(lens.max()) + 15) & ~15) + 16
        offs[:nc] = (np.arange(nc) + 1) * S - lens
        total = nc * S
    else:
        assert layout == "sized"
        worst = ((int(lens.max()) + 15) & ~15) + 16
        slot = max(64, (int(np.median(lens)) + 63) & ~63)
        k = 0
        for c in range(nc):
            if lens[c] <= slot:
                offs[c] = (c + 1) * slot - lens[c]
            else:
                offs[c] = nc * slot + (k + 1) * worst - lens[c]
                k += 1
        total = nc * slot + k * worst
    offs[nc] = total
    cont = np.full(total, GAP, dtype=np.uint8)
    for c in range(nc):
        cont[int(offs[c]):int(offs[c]) + int(lens[c])] = shape.streams[c]
    return cont, offs, lens


# ---- cases ------------------------------------------------------------------------------------------------------------

INDEX_ENTRIES = ("I1", "I2", "I3", "I4", "I5", "I6")
STREAM_ENTRIES = ("S1", "S2", "S3", "S4")
MODEL_ENTRIES = ("M1", "M2", "M3")


def entries_of(row):
    e = [x for x in INDEX_ENTRIES if x != "I1" or UNIT[row["fmt"]] > 1] + list(STREAM_ENTRIES) + ["S5"]
    if row["big"]:  # (I6 is a statement about a SMALL container: 2^20 bytes lie inside this one)
        e.remove("I6")
    if row["kernel"] in DESCRIPTOR_KERNELS:
        e.append("S6")
    if row["kind"] == "adaptive":
        e += list(MODEL_ENTRIES)
    return e


def entry_variant(row, entry):
    """The shape an entry is shown on.  A damaged STATE garbles the whole chunk, and over the 170 Ki symbols of the smallest
    chunk of the 512 Ki row the consumption never ends within 16 bytes of the stream's: that row takes S3 on the three-symbol
    last chunk of its H1 variant."""
    return "h1" if row["big"] and entry == "S3" else None


class Case:
    """What the decoder is given (cont, total, offs, lens, n, rows) and what it must do (count, out)."""


def _arena_ok(off, length, total):
    return -MARGIN + 4096 <= off and off + length <= total + MARGIN - 4096


def make_case(shape, layout, damage, end_mod=None, prove=True):
    """damage: [(chunk, entry)] -- at most one entry per chunk; S5 names the last chunk and lowers the call's n.
    Stream entries search from their drawn position for the next one whose proof passes (Case.searched counts the steps)."""
    fmt, ways, unit, sbytes = shape.fmt, shape.ways, UNIT[shape.fmt], STATE_BYTES[shape.fmt]
    cont, offs, lens = lay_out(shape, layout, end_mod)
    total = int(offs[-1])
    nc = shape.nchunks
    case = Case()
    case.n = shape.n
    case.rows = None if shape.rows is None else shape.rows.copy()
    out = shape.syms.astype(np.uint16).copy()
    case.rejected, case.flagged, case.proofs, case.searched = [], [], [], 0
    seen = set()
    # the call's n first: every other entry's symbol count depends on it
    for c, entry in damage:
        if entry == "S5":
            assert c == nc - 1
            true_len = int(lens[c])
            for cut in range(1, shape.nsym_of(c)):
                v = _try(shape, cont, c, int(offs[c]), true_len, shape.nsym_of(c) - cut, "raise")
                case.searched += 1
                if v is not None and not v.good and v.max_units <= 2:
                    break
            else:
                raise AssertionError("S5: no proven instance")
            case.n = shape.n - cut
            first = c * shape.chunk
            out[first:first + v.syms.size] = v.syms
            out[case.n:] = POISON_OF(shape)
            case.flagged.append(c)
            case.proofs.append((c, "S5", "zeros" if v.needed_beyond else "raise", v.good, v.max_units > 2))
            seen.add(c)
    for c, entry in damage:
        if entry == "S5":
            continue
        assert c not in seen and 0 <= c < nc, (c, entry)
        seen.add(c)
        off, ln, nsym = int(offs[c]), int(lens[c]), shape.nsym_of(c, case.n)
        first = c * shape.chunk
        if entry in INDEX_ENTRIES:
            if entry == "I1":
                assert unit > 1
                off += unit // 2
            elif entry == "I2":
                ln = ways * sbytes - unit
            elif entry == "I3":
                ln = total - off + unit
            elif entry == "I4":
                off = total
                assert ln > 0
            elif entry == "I5":
                off = total + 16
            else:
                assert total < (1 << 20) and 0 < c < nc - 1
                ln = 1 << 20
            assert not index_rule(fmt, ways, off, ln, total), (c, entry)
            assert _arena_ok(off, ln, total), (c, entry, off, ln)
            offs[c], lens[c] = off, ln
            out[first:first + nsym] = POISON_OF(shape)
            case.rejected.append(c)
            case.proofs.append((c, entry, "rule", False, False))
        elif entry in MODEL_ENTRIES:
            M = 1 << shape.sb
            row = case.rows[c].astype(np.int64)
            top = int(np.argmax(row))
            if entry == "M1":
                row[top] -= 1
            elif entry == "M2":
                row[top] += 1
            else:
                row[top] = M + 1
            assert int(row.sum()) != M and row.max() < 65536 and row.min() >= 0  # (the rule of tests/_model_extremes.py: a row is a model iff it sums to M)
            case.rows[c] = row.astype(np.uint16)
            out[first:first + nsym] = POISON_OF(shape)
            case.rejected.append(c)
            case.proofs.append((c, entry, "rule", False, False))
        else:
            v, mode = None, "raise"
            if entry in ("S1", "S2"):
                new = ln - unit if entry == "S1" else ln + unit
                same = granule_limit(off, new) == granule_limit(off, ln)
                assert same and new >= ways * sbytes and off + new <= total, (c, entry, "not applicable here", off, ln)
                lens[c] = new
                v = _try(shape, cont, c, off, new, nsym, "raise") if prove else None
                if not prove:  # the streams are the oracle's: the same bytes decode to the same symbols and consume ln != new
                    case.flagged.append(c)
                    continue
            elif entry == "S3":
                for k in range(ways * 16):
                    j, b = (c + k // 16) % ways, (5 + k) % 16
                    at = off + j * sbytes + b // 8
                    cont[at] ^= 1 << (b % 8)
                    v = _try(shape, cont, c, off, ln, nsym, "raise")
                    case.searched += 1
                    if v is not None and not v.good and v.max_units <= 2:
                        break
                    cont[at] ^= 1 << (b % 8)
                    v = None
            elif entry == "S4":
                body = ln - ways * sbytes
                for k in range(max(body, 1)):
                    if body <= 0:
                        break
                    at = off + ways * sbytes + (body // 2 if k == 0 else body - k)  # the middle, then from the end backwards
                    cont[at] ^= 0x10
                    v = _try(shape, cont, c, off, ln, nsym, "raise")
                    case.searched += 1
                    if v is not None and not v.good and v.max_units <= 2:
                        break
                    cont[at] ^= 0x10
                    v = None
            else:
                assert entry == "S6", entry
                mode = "zeros"
                new = ln - 16
                assert new >= ways * sbytes, (c, "S6 needs a stream longer than its states by a granule", ln)
                lens[c] = new
                v = _try(shape, cont, c, off, new, nsym, "zeros")
            assert v is not None, (c, entry, "no proven instance")
            out[first:first + nsym] = v.syms
            case.flagged.append(c)
            if v.needed_beyond:
                mode = "zeros"
                assert shape.row["kernel"] in DESCRIPTOR_KERNELS
            case.proofs.append((c, entry, mode, v.good, v.max_units > 2))
    case.cont, case.total, case.offs, case.lens = cont, total, offs, lens
    case.count = len(case.rejected) + len(case.flagged)
    case.out = out
    case.damaged = sorted(seen)
    return case


def POISON_OF(shape):
    return POISON if shape.row["K"] <= 256 else (POISON | (POISON << 8))


def _try(shape, cont, c, off, length, nsym, mode):
    """The reference's verdict in mode "raise"; None where it needs a byte behind the chunk's last granule -- unless the row's
    kernel fetches through a descriptor of the chunk: what lies behind is zeros to it, and the verdict of mode "zeros" holds
    (Verdict.needed_beyond then says that this happened)."""
    try:
        return ref_decode(shape.model_of(c), shape.ways, cont, off, nsym, length, granule_limit(off, length), mode)
    except BeyondLimit:
        if shape.row["kernel"] in DESCRIPTOR_KERNELS:
            return ref_decode(shape.model_of(c), shape.ways, cont, off, nsym, length, granule_limit(off, length), "zeros")
        return None


def s1_applies(off, ln, fmt, ways):
    """S1 without a decode (vectorised over numpy arrays): the shorter length ends in the same granule and still holds the states."""
    unit = UNIT[fmt]
    skip = off & 15
    return (((skip + ln + 15) & ~15) == ((skip + ln - unit + 15) & ~15)) & (ln - unit >= ways * STATE_BYTES[fmt])


def s2_applies(off, ln, fmt, total):
    unit = UNIT[fmt]
    skip = off & 15
    return (((skip + ln + 15) & ~15) == ((skip + ln + unit + 15) & ~15)) and off + ln + unit <= total


# ---- where the damage sits ----------------------------------------------------------------------------------------------

def placements(shape):
    """name -> chunks.  The last FULL chunk is nchunks - 2, the ragged one nchunks - 1."""
    nc, u = shape.nchunks, shape.row["unit"]
    mid = nc // 2
    p = {"first": [0], "middle": [mid], "last-full": [nc - 2], "ragged-last": [nc - 1], "neighbours": [mid, mid + 1],
         "every-second": list(range(0, nc, 2)), "every": list(range(nc)), "all-but-one": [c for c in range(nc) if c != mid]}
    # runs of rejected index entries (k_decode_word64's hand-over ladder looks further one step after the other)
    p["rejected-run-2"] = [mid, mid + 1]
    p["rejected-run-3"] = [mid - 1, mid, mid + 1]
    p["rejected-first-two"] = [0, 1]
    p["rejected-last-two"] = [nc - 2, nc - 1]
    if u > 1:
        units = nc // u
        p["unit-first-members"] = [k * u for k in range(units)]
        p["unit-last-members"] = [k * u + u - 1 for k in range(units)]
        p["quad-mates"] = [k * u + q for k in range(units) for q in ((1, 2) if u >= 4 else (1,))]
        p["one-whole-unit"] = list(range(u * (units - 1), u * units))
        longest = max(range(u), key=lambda c: shape.streams[c].size)
        p["only-the-longest-healthy"] = [c for c in range(u) if c != longest]
    return p


def mixed(shape, layout, chunks, index_only=False, offs=None, lens=None, total=None):
    """Cheap entries for a placement: S1 where it applies (S2 next, then I2) on every even member, I2 / I3 / I5 on the odd
    ones -- an index-rejected member beside stream-damaged ones in every work unit that holds two."""
    if offs is None:
        _, offs, lens = lay_out(shape, layout)
        total = int(offs[-1])
    dmg = []
    for k, c in enumerate(chunks):
        off, ln = int(offs[c]), int(lens[c])
        if index_only:
            dmg.append((c, ("I2", "I3", "I5", "I4")[k % 4]))
        elif k % 2 == 0 and s1_applies(off, ln, shape.fmt, shape.ways):
            dmg.append((c, "S1"))
        elif k % 2 == 0 and s2_applies(off, ln, shape.fmt, total):
            dmg.append((c, "S2"))
        else:
            dmg.append((c, ("I2", "I3", "I5")[(k // 2) % 3]))
    return dmg


def entry_damage(shape, layout, entry):
    """One catalogue entry on one chunk: the middle one, or for S1 / S2 the next chunk (upwards, wrapping) whose lengths end in
    the same granule.  The 512 Ki-symbol chunks of the per-lane fallback take their stream damage in the short ragged chunk."""
    nc, big = shape.nchunks, shape.row["big"]
    mid = nc // 2
    if entry == "S5":
        return [(nc - 1, "S5")]
    if entry in ("S1", "S2"):
        _, offs, lens = lay_out(shape, layout)
        total = int(offs[-1])
        order = list(range(nc - 1, -1, -1)) if big else [(mid + k) % nc for k in range(nc)]
        for c in order:
            off, ln = int(offs[c]), int(lens[c])
            if (entry == "S1" and s1_applies(off, ln, shape.fmt, shape.ways)) or (entry == "S2" and s2_applies(off, ln, shape.fmt, total)):
                return [(c, entry)]
        raise AssertionError((shape.row["id"], layout, entry, "applies to no chunk"))
    if entry in ("S3", "S4", "S6") and big:
        return [(nc - 1, entry)]
    return [(mid, entry)]


LAYOUTS = ("compact", "slots", "sized")


def h2_ends(fmt):
    """H2: how many bytes behind a 16-byte boundary the container ends (1, 15 and 0, in the format's units)."""
    unit = UNIT[fmt]
    return (unit, 16 - unit, 0)


def entries_in(row, layout):
    """S2 needs a stream that ends inside a granule: the slot layouts end every stream ON a 16-byte boundary, one unit more is
    another granule (and another chunk's slot) -- there the entry does not exist."""
    return [e for e in entries_of(row) if e != "S2" or layout == "compact"]
