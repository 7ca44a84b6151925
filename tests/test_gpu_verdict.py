"""Every chunked decoder's verdict on damage: the count exact, the damage contained.

One row (tests/_verdict.py VERDICT_ROWS) for every kernel rans_amd_decode / rans_amd_decode_adaptive[_fmt] can report.  The
containers are laid out on the CPU from the ORACLE's streams (compact: 16-byte starts; slots: 16-byte ends, every start phase
the row's lengths reach; sized: 64-byte slots and an overflow region), the damage is the catalogue of tests/_verdict.py, and
nothing is asserted here that tests/test_verdict_cpu.py has not proved on the CPU: how many chunks a correct decoder must
flag, and which symbols it must write -- the input for every undamaged chunk, the REFERENCE's garbage for a chunk whose
stream is damaged (tests/_verdict.py ref_decode), and nothing at all for a chunk whose index entry or model row is rejected.

RULE ON REJECTED CHUNKS (read in every kernel, stated in include/ryg_rans_amd.h, asserted here): a chunk whose index entry
fails the header's rule, or whose per-chunk model row does not sum to M, is counted once and SKIPPED -- none of its bytes is
read, none of its symbols written (k_decode / k_decode_word64: `continue` / the hand-over looks further; k_decode_dual:
decode_single runs for the partner only; the lane kernels: the lane turns invalid, its stores are masked by vq / nsym = 0;
the group kernels: groups_common.hpp's `valid`).  The output range of such a chunk is still poison afterwards.

Every case asserts
  count        synchronous: RANS_AMD_E_CORRUPT and h_bad_chunks == the proved number (Context.decode attaches it to the error
               as `bad_chunks`); asynchronous: the case queued twice, rans_amd_decode_errors returns the sum once, then 0
  containment  d_out lies in a poisoned buffer between guards of 4096 symbols: the whole buffer equals the expectation
               (undamaged chunks == input, damaged ones as above, guards intact), after each of the three launches
  recovery     a healthy decode on the same context right behind the failed ones is exact and counts 0
  the kernel   rans_amd_last_decode_kernel after every call
  safety       every index entry keeps [off, off + len) inside the test's own arena: the container lies 1 MiB + 8 KiB from
               either end, the largest len used is 2^20 (asserted on the CPU side for every entry of every case)

Where the damage sits: every catalogue entry on one chunk in every layout (test_entries); the placements of
tests/_verdict.py placements() with the cheap entries -- single chunks, neighbours, every second, every, all but one, runs
of rejected entries (k_decode_word64's hand-over ladder at chunks of one group, both steps issued behind the loop, and of
sixteen, issued inside), and for the 2 / 8 / 32 / 64-chunk work units one member per unit in every position class, a whole
unit, a unit whose only healthy member is its longest, index-rejected members beside stream-damaged ones (test_placements);
H1 / H2 (test_healthy_edges); R1 with two different patterns behind the container's last granule (test_read_bound); and one
row per unit kind over four rounds of the persistent grid, every third chunk damaged (test_rounds: the chunk count is
4 x resident_waves() units as in regime R of tests/test_gpu_kernel_matrix.py -- without that regime's floor of 2^28 symbols,
which small chunks are there to avoid).

Not asserted, on purpose: S6 and the symbols of R1 on the lane and group kernels (they read the container up to ITS last
granule: behind a shortened chunk they see its neighbour, profiles/verdict_record.md says what they do); offsets and lengths
only a 64-bit wrap would admit (not run on a GPU at all: the two-compare form `off <= container_bytes && len <=
container_bytes - off` is in every kernel, by reading).

Wall times on an MI355X (pytest --durations=0, seconds, as measured): the file's 129 cases take 25.4 s in all.  Every case
of the rows with small chunks takes 0.05 s or less (test_entries 0.01, test_placements 0.02 - 0.05, test_healthy_edges and
test_read_bound 0.01, test_rounds 0.04), but for the first one of the file (0.15 + 1.7 s of set-up: the context) and
test_rounds[word-64] (0.48: the first launches of the encoder).  The row of 512 Ki-symbol chunks (k_decode_lanes takes nothing
smaller) moves a 35 MB container per case and pays a second of Python per reference decode: its test_entries cases take
1.15 - 2.0 s each, test_healthy_edges 3.5, test_placements 4.6 -- which is why it has one entry per case and four placements.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _verdict as V
from _batch import resident_waves
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

pytestmark = pytest.mark.gpu

GUARD = 4096
BEHIND = 0xC3  # the arena outside the container's granules


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


@contextlib.contextmanager
def row_context(R, shared, row):
    """The shared context, or one of the row's own where it sets options (they must not leak into the other rows)."""
    if not row["opts"]:
        yield shared
        return
    ctx = R.Context(0)
    try:
        for opt, val in row["opts"]:
            ctx.set_option(opt, val)
        yield ctx
    finally:
        _HEALTHY.clear()
        ctx.close()


class Rig:
    """A case on the device: the arena with the container in its middle, the index, the guarded output buffers."""

    def __init__(self, R, ctx, torch, sh, case, behind=BEHIND):
        self.R, self.ctx, self.torch, self.sh, self.case = R, ctx, torch, sh, case
        total16 = (case.total + 15) & ~15
        arena = np.full(V.MARGIN + total16 + V.MARGIN, behind, dtype=np.uint8)
        arena[V.MARGIN:V.MARGIN + case.total] = case.cont
        arena[V.MARGIN + case.total:V.MARGIN + total16] = V.GAP
        self.arena = torch.from_numpy(arena).cuda()
        self.d_cont = self.arena[V.MARGIN:]
        assert self.d_cont.data_ptr() % 16 == 0
        self.d_offs = torch.from_numpy(np.ascontiguousarray(case.offs, dtype=np.int64)).cuda()
        self.d_lens = torch.from_numpy(np.ascontiguousarray(case.lens, dtype=np.int64).astype(np.int32)).cuda()
        self.d_rows = None if case.rows is None else torch.from_numpy(case.rows.reshape(-1).view(np.int16).copy()).cuda()
        self.u16 = sh.row["K"] > 256
        poison = V.POISON_OF(sh)
        want = np.full(GUARD + sh.n + GUARD, poison, dtype=np.uint16)
        want[GUARD:GUARD + sh.n] = case.out
        self.want = torch.from_numpy(want.view(np.int16).copy() if self.u16 else want.astype(np.uint8)).cuda()
        self.gm = None if sh.adaptive else ctx.model(sh.fmt, sh.freqs, sh.sb)

    def fresh_out(self):
        return self.torch.full_like(self.want, self.want[0].item())

    def launch(self, buf, sync):
        """-> (status, bad chunks or None)"""
        R, ctx, sh, case = self.R, self.ctx, self.sh, self.case
        d_out = buf[GUARD:GUARD + sh.n]
        assert d_out.data_ptr() % 64 == 0
        if self.gm is not None:
            try:
                ctx.decode(self.gm, self.d_cont, case.total, self.d_offs, self.d_lens, case.n, sh.ways, sh.chunk, d_out=d_out, sync=sync)
                rc, bad = R.OK, 0
            except R.RansAmdError as e:
                rc, bad = e.status, e.bad_chunks
        else:  # (the wrapper's decode_adaptive drops the count: the C ABI directly)
            h_bad = C.c_uint64(0)
            args = (self.d_cont.data_ptr(), case.total, self.d_offs.data_ptr(), self.d_lens.data_ptr(), self.d_rows.data_ptr(), case.n,
                    sh.ways, sh.chunk, sh.sb, d_out.data_ptr(), C.byref(h_bad) if sync else None, R._torch_stream())
            lib = R.lib()
            rc = lib.rans_amd_decode_adaptive(ctx._h, *args) if sh.fmt == FMT_BYTE else lib.rans_amd_decode_adaptive_fmt(ctx._h, sh.fmt, *args)
            bad = int(h_bad.value)
        assert ctx.last_decode_kernel() == sh.row["kernel"], (ctx.last_decode_kernel(), sh.row["kernel"])
        return rc, (bad if sync else None)

    def diff(self, buf):
        """'' or where the buffer differs from the expectation, in chunks."""
        if self.torch.equal(buf, self.want):
            return ""
        at = (buf != self.want).nonzero().flatten().cpu().numpy() - GUARD
        chunks = sorted({int(a) // self.sh.chunk if 0 <= a < self.sh.n else ("guard below" if a < 0 else "guard above") for a in at[:4096]},
                        key=str)
        return "differs in %d symbols; chunks %s (damaged: %s)" % (at.size, chunks[:12], self.case.damaged[:12])


def run_case(R, ctx, torch, sh, case, what, healthy=None, behind=BEHIND):
    """The assertions every case makes (module docstring).  healthy: the rig of the row's undamaged container."""
    rig = Rig(R, ctx, torch, sh, case, behind)
    assert ctx.decode_errors() == 0, (what, "a count left over from before")
    # asynchronous, queued twice: the sum once, then nothing
    a, b = rig.fresh_out(), rig.fresh_out()
    assert rig.launch(a, False)[0] == R.OK and rig.launch(b, False)[0] == R.OK
    got = ctx.decode_errors()
    assert got == 2 * case.count, (what, "asynchronous count of two launches", got, "proved", 2 * case.count)
    assert ctx.decode_errors() == 0, (what, "the count was not reset")
    assert rig.diff(a) == "" and rig.diff(b) == "", (what, rig.diff(a), rig.diff(b))
    # synchronous: status and the stored value
    c = rig.fresh_out()
    rc, bad = rig.launch(c, True)
    assert (rc, bad) == ((R.E_CORRUPT if case.count else R.OK), case.count), (what, "synchronous", rc, bad, "proved", case.count)
    assert rig.diff(c) == "", (what, rig.diff(c))
    assert ctx.decode_errors() == 0, (what, "the synchronous call left its count behind")
    # a healthy decode right behind the failed ones
    if healthy is not None and case.count:
        d = healthy.fresh_out()
        rc, bad = healthy.launch(d, True)
        assert (rc, bad) == (R.OK, 0) and healthy.diff(d) == "", (what, "healthy decode behind the failed ones", rc, bad, healthy.diff(d))
    return rig, c


_HEALTHY = {}


def healthy_rig(R, ctx, torch, sh, layout):
    key = (sh.row["id"], layout, id(ctx))
    if key not in _HEALTHY:
        _HEALTHY.clear()  # (one at a time: the 512 Ki row's arena is 35 MB)
        _HEALTHY[key] = Rig(R, ctx, torch, sh, V.make_case(sh, layout, []))
    return _HEALTHY[key]


def _entry_params():
    for r in V.VERDICT_ROWS:
        if r["big"]:  # (its Python reference costs a second per chunk: one entry per case)
            for e in V.entries_in(r, "compact"):
                yield pytest.param(r["id"], "compact", (e,), id="%s-compact-%s" % (r["id"], e))
        else:
            for layout in V.LAYOUTS:
                yield pytest.param(r["id"], layout, None, id="%s-%s" % (r["id"], layout))


@pytest.mark.parametrize("rid,layout,only", list(_entry_params()))
def test_entries(gpu, oracle, rid, layout, only):
    """Every catalogue entry on one chunk; the healthy container first (count 0, exact)."""
    R, shared, torch = gpu
    row = V.ROW_BY_ID[rid]
    base = V.shape_of(oracle, row)
    with row_context(R, shared, row) as ctx:
        healthy = healthy_rig(R, ctx, torch, base, layout)
        if only is None:
            run_case(R, ctx, torch, base, healthy.case, (rid, layout, "healthy"))
        for entry in only or V.entries_in(row, layout):
            sh = V.shape_of(oracle, row, V.entry_variant(row, entry))
            case = V.make_case(sh, layout, V.entry_damage(sh, layout, entry))
            assert case.count == 1
            run_case(R, ctx, torch, sh, case, (rid, layout, entry, case.damaged), healthy if sh is base else None)


# (the row of 512 Ki-symbol chunks moves 35 MB per case: the placements that differ for a kernel that strides over chunks)
BIG_PLACEMENTS = ("ragged-last", "every", "unit-first-members", "rejected-run-3")


@pytest.mark.parametrize("rid", [r["id"] for r in V.VERDICT_ROWS])
def test_placements(gpu, oracle, rid):
    R, shared, torch = gpu
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row)
    with row_context(R, shared, row) as ctx:
        healthy = healthy_rig(R, ctx, torch, sh, "compact")
        for name, chunks in V.placements(sh).items():
            if row["big"] and name not in BIG_PLACEMENTS:
                continue
            case = V.make_case(sh, "compact", V.mixed(sh, "compact", chunks, index_only=name.startswith("rejected")), prove=not row["big"])
            assert case.count == len(chunks)
            run_case(R, ctx, torch, sh, case, (rid, name, chunks[:16]), healthy)
        # the slot layout (every start phase) under the two densest placements
        for name in ("every-second", "all-but-one") if not row["big"] else ():
            chunks = V.placements(sh)[name]
            case = V.make_case(sh, "slots", V.mixed(sh, "slots", chunks), prove=not row["big"])
            run_case(R, ctx, torch, sh, case, (rid, "slots", name), None)


@pytest.mark.parametrize("rid", [r["id"] for r in V.VERDICT_ROWS if r["kind"] == "static"])
def test_healthy_edges(gpu, oracle, rid):
    """H1: a last chunk that is its states and nothing else; H2: the last chunk ends on the container's last byte, which lies
    one unit / 16 - unit / 0 bytes behind a 16-byte boundary.  Count 0, every symbol exact."""
    R, shared, torch = gpu
    row = V.ROW_BY_ID[rid]
    h1 = V.shape_of(oracle, row, "h1")
    assert h1.streams[-1].size == h1.ways * V.STATE_BYTES[h1.fmt]
    with row_context(R, shared, row) as ctx:
        for layout in ("compact", "slots") if not row["big"] else ("compact",):
            run_case(R, ctx, torch, h1, V.make_case(h1, layout, []), (rid, "H1", layout))
        sh = V.shape_of(oracle, row)
        for end_mod in V.h2_ends(row["fmt"]):
            case = V.make_case(sh, "compact", [], end_mod=end_mod)
            assert case.total % 16 == end_mod
            run_case(R, ctx, torch, sh, case, (rid, "H2", end_mod))


@pytest.mark.parametrize("rid", [r["id"] for r in V.VERDICT_ROWS if not r["big"]])
def test_read_bound(gpu, oracle, rid):
    """R1: the last chunk's stream ends after half its symbols; the reference then needs more than 16 bytes behind
    container_bytes (proved on the CPU).  Two decodes with different bytes behind the container's last granule: the count,
    every symbol written (the damaged chunk's included) and the guards are the same; on the kernels that fetch through a
    descriptor of the chunk the count is 1 and the symbols are the reference's with zeros behind the limit."""
    R, shared, torch = gpu
    row = V.ROW_BY_ID[rid]
    sh = V.shape_of(oracle, row, "r1")
    case, v = V.make_r1(sh)
    assert v.needed_beyond and v.last_read >= case.total + 16
    with row_context(R, shared, row) as ctx:
        _read_bound(R, ctx, torch, row, rid, sh, case)


def _read_bound(R, ctx, torch, row, rid, sh, case):
    if row["kernel"] in V.DESCRIPTOR_KERNELS:
        _, out1 = run_case(R, ctx, torch, sh, case, (rid, "R1", hex(BEHIND)))
        _, out2 = run_case(R, ctx, torch, sh, case, (rid, "R1", "0x3c"), behind=0x3C)
        assert torch.equal(out1, out2)
        return
    outs, counts = [], []
    for behind in (BEHIND, 0x3C):
        rig = Rig(R, ctx, torch, sh, case, behind)
        buf = rig.fresh_out()
        rc, bad = rig.launch(buf, True)
        assert rc in (R.OK, R.E_CORRUPT)
        outs.append(buf)
        counts.append(bad)
    first = GUARD + (sh.nchunks - 1) * sh.chunk
    assert counts[0] == counts[1] and torch.equal(outs[0], outs[1]), (rid, counts)
    assert torch.equal(outs[0][:first], rig.want[:first]) and torch.equal(outs[0][GUARD + sh.n:], rig.want[GUARD + sh.n:]), rid
    print("R1 %s: count %d, the damaged chunk's symbols %s the zeros reference" % (rid, counts[0], "==" if torch.equal(outs[0], rig.want) else "!="))


# ---- several rounds of the persistent grid ---------------------------------------------------------------------------------
# (format, scale_bits, interleave, chunk, chunks per unit, kernel): the smallest chunks each unit kind takes
ROUNDS = [
    ("word-64", FMT_WORD, 12, 64, 64, 1, "k_decode_word64"),
    ("word-8", FMT_WORD, 12, 8, 32, 8, "k_decode_word_groups"),
    ("byte-2", FMT_BYTE, 14, 2, 64, 32, "k_decode_byte_pairs"),
    ("word-4", FMT_WORD, 12, 4, 4, 64, "k_decode_lanes_staged"),
    ("r64-2", FMT_R64, 14, 2, 64, 64, "k_decode_lanes_r64x2<packed slots>"),
]


@pytest.mark.parametrize("rid,fmt,sb,ways,chunk,unit,kernel", ROUNDS, ids=[r[0] for r in ROUNDS])
def test_rounds(gpu, rid, fmt, sb, ways, chunk, unit, kernel):
    """4 x resident_waves() units, half a unit and a ragged chunk, under two patterns.
    "every-third": every third chunk damaged -- S1 where the shorter length ends in the same granule (the same bytes decode
    to the same symbols and consume the true length: flagged, output == input), I2 elsewhere (rejected: output poison).
    "head": the first 2 x resident_waves() units rejected (I2) and nothing else -- whatever a wave claims FIRST is a rejected
    entry, and every chunk behind the head must still be decoded by someone.
    The container is the GPU encoder's (every chunk of it is held to the oracle by tests/test_gpu_kernel_matrix.py).  The
    count is exact, through both paths."""
    R, ctx, torch = gpu
    import bench
    resident = resident_waves(torch)
    units = 4 * resident
    nchunks_full = units * unit + unit // 2
    n = nchunks_full * chunk + chunk // 3 + 1
    nchunks = nchunks_full + 1
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, 256), 1 << sb)
    gm = ctx.model(fmt, freqs, sb)
    cont, offs, lens, total = ctx.encode(gm, d_syms, ways, chunk)
    out = ctx.decode(gm, cont, total, offs, lens, n, ways, chunk)
    assert ctx.last_decode_kernel() == kernel and torch.equal(out, d_syms)
    h_offs, h_lens = offs[:nchunks].cpu().numpy().astype(np.int64), lens[:nchunks].cpu().numpy().astype(np.int64)
    for pattern in ("every-third", "head"):
        damaged = np.zeros(nchunks, dtype=bool)
        if pattern == "head":
            damaged[:2 * resident * unit] = True
            s1 = np.zeros(nchunks, dtype=bool)
        else:
            damaged[::3] = True
            s1 = damaged & V.s1_applies(h_offs, h_lens, fmt, ways)
            # (one symbol per lane renormalises nothing: the streams of word-64 and word-4 are their states, S1 applies nowhere)
            assert s1.any() == (rid not in ("word-64", "word-4")), int(s1.sum())
        i2 = damaged & ~s1
        new = h_lens.copy()
        new[s1] -= V.UNIT[fmt]
        new[i2] = ways * V.STATE_BYTES[fmt] - V.UNIT[fmt]
        count = int(damaged.sum())
        assert count == ((nchunks + 2) // 3 if pattern == "every-third" else 2 * resident * unit) and i2.any()
        d_lens = torch.from_numpy(new.astype(np.int32)).cuda()
        rejected = torch.from_numpy(i2).cuda().repeat_interleave(chunk)[:n]
        want = torch.full((GUARD + n + GUARD,), V.POISON, dtype=torch.uint8, device="cuda")
        want[GUARD:GUARD + n] = torch.where(rejected, torch.full_like(d_syms, V.POISON), d_syms)
        bufs = [torch.full_like(want, V.POISON) for _ in range(3)]
        for b in bufs[:2]:
            ctx.decode(gm, cont, total, offs, d_lens, n, ways, chunk, d_out=b[GUARD:GUARD + n], sync=False)
            assert ctx.last_decode_kernel() == kernel
        got = ctx.decode_errors()
        assert got == 2 * count and ctx.decode_errors() == 0, (rid, pattern, got, 2 * count)
        with pytest.raises(R.RansAmdError) as e:
            ctx.decode(gm, cont, total, offs, d_lens, n, ways, chunk, d_out=bufs[2][GUARD:GUARD + n])
        assert e.value.status == R.E_CORRUPT and e.value.bad_chunks == count, (rid, pattern, e.value.bad_chunks, count)
        for b in bufs:
            assert torch.equal(b, want), (rid, pattern, int((b != want).sum().item()))
        out = ctx.decode(gm, cont, total, offs, lens, n, ways, chunk)
        assert torch.equal(out, d_syms) and ctx.decode_errors() == 0


def test_reference_equals_host_decoder(gpu, oracle):
    """The reference decoder of tests/_verdict.py against rans_amd_decode_host (which needs a context): healthy streams of
    every format at the interleaves the rows use."""
    R, ctx, torch = gpu
    for fmt, sb, K in ((FMT_BYTE, 14, 256), (FMT_WORD, 12, 256), (FMT_WORD, 12, 1024), (FMT_R64, 14, 256), (FMT_R64, 20, 256),
                       (FMT_ALIAS, 16, 256), (FMT_ALIAS, 16, 4096)):
        for ways in (1, 2, 4, 8, 64, 128):
            n = 5 * ways + 3
            syms = oracle.gen_zipf(4000, K, 1.0, 7 + ways)
            freqs, _ = oracle.normalize(oracle.count_freqs(syms, K), 1 << sb)
            syms = syms[:n]
            om = oracle.model(freqs, sb, with_alias=fmt == FMT_ALIAS)
            stream = oracle.encode(fmt, om, syms, ways)
            v = V.ref_decode(V.RefModel(fmt, om), ways, stream, 0, n, stream.size, stream.size, "raise")
            host = ctx.decode_host(ctx.model(fmt, freqs, sb), stream, n, ways)
            assert v.good and np.array_equal(v.syms, host) and np.array_equal(host, syms), (fmt, sb, K, ways)
