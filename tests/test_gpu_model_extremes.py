"""The per-chunk-model BUILDERS at the extremes of the histogram: the device code that makes a model from the data it is about
to code -- adapt_normalize (device_common.hpp; k_chunk_models and k_encode_adaptive in its uniform, register-resident and
ragged forms), the count passes that feed it, the record builder and the f32 piece-size bound of k_encode_adaptive
(encode_adaptive.hip steps 3 and 4) and adapt_build_dec (k_decode<.., per-chunk models>, k_decode_batch_models<..>).

tests/_model_extremes.py holds the inputs (seeded shuffles of exact counts), the width-based normalisation, the f64 model
of the bound (need_model, with the derivation of its window) and the table of count paths; tests/test_model_extremes_cpu.py
proves without a GPU what each class reaches (191 / 192 repairs against one victim, 150 repairs over 50 victims in
ascending order, a victim worn down to width 1, widths 2048 / 2049 / 4095 / 4096, symbols that start on a lane's first
position behind runs of width 0) and that the oracle's stream fits lo.  No number here comes from the library: rows, streams and
lengths are the oracle's, the window of a piece is need_model's from the oracle's row.

  section a  every class as one chunk each and a ragged last chunk, chunks of 4096 / 8192 / 16 384 symbols (64-way: the
             register-resident kernels RR = 4 / 8 / 16), 64 ways and 2 / 128 / 512 ways, through the one-kernel encoder and the
             three-launch one (k_chunk_models), the input at base + 0, + 1 and + 4 bytes (+ 1 / + 4: the two-pass form, + 1:
             counting byte by byte): every row and every stream == the oracle's, the two encoders' lengths equal
  section b  the count passes: every chunk size of COUNT_TABLE at base + 0, + 4 and + 1, one chunk per call, dom_last and
             all_once (a miscount of one symbol changes the row), 64 ways (base + 0, 4096 / 8192 / 16 384: counted from the
             registers) and 128 ways (the same sizes in trips of 4096)
  section c  the piece a chunk gets: need[c] = end of piece c - end of piece c - 1, a multiple of 64 inside need_model's
             window, the stream at its top, pieces in index order, the same container on a second call
  section d  ragged batches (tests/_batch.py ModelBatch / run_model_row): the classes at the sizes of section b,
             neighbours at different alignments (sym_align 1 and 16), an empty stream between two dom_* streams; rows, streams,
             kernel names, exact decode into poison; the window of section c with the ragged cap
  section e  adapt_build_dec alone: the oracle's containers and rows, decode_adaptive at 64 and 2 ways and
             decode_batch_adaptive into guarded buffers

What the cases are tight against, by reading the kernels (no mutated kernel was built):
  * adapt_normalize taking the HIGHEST index on ties: tie_chain at 16 384 symbols, 12 bits -- the victims become 254, 253, ..
    and the five symbols left at width 4 are 200..204, not 250..254: a row differs (sections a, c, d).  A victim of width 1
    allowed: the repair robs the lowest symbol of width 1, which occurs and is squeezed in turn -- every dom_* chunk that needs
    a repair (12 bits from 8192 symbols on, 8 bits always) and tie_chain end with another row or never end: a, b, d.
  * small = wmax < 2048 and small = wmax <= 2049: NOT visible in the bytes, and no test can make them so.  At frequency
    2048 the round-up reciprocal is m' = 1, sh = 10: q = (x >> 1) >> 10, exact.  At 2049 Alverson's reciprocal is
    (2^43 + 1024) / 2049 (2^11 = -1 modulo 2049, so 2^43 = -1024): mulhi(x, rcp) >> 11 is exact while 1024 x < 2^43, i.e.
    for every 32-bit x.  Both sides of `small` give the oracle's stream at both frequencies; exact_2048 / exact_2049 pin
    that the switch, wherever it sits between them, changes nothing -- in the two-pass form (base + 1, + 4; sections c, d),
    the register-resident kernels code with the round-up records whatever the frequencies.  exact_4095 and constant_* are
    one below and on `always`, where a wrong side IS visible: 2 n + 4 N bytes against a few.
  * the (1 + 1/4096) factor dropped: need is then lo itself, inside the issue's window on every piece; what notices is
    need_floor (the estimate cannot fall below (B - E)(1 + 2^-12)(1 - 2^-20) / 8 if the factor is there): missed on every piece
    where B / 32768 bytes cross a line -- tests/test_model_extremes_cpu.py counts them in the plans of sections c and d.
    slack halved: need falls by 32 + 2 N bytes and more, two lines and more at 64 ways: below lo on every piece that is not
    capped by the worst-case slot (c, d).
  * counting only nsym & ~3 symbols on the unaligned path: the sizes of section b that are no multiple of 4 at base + 1
    (1, 3, 67, 1027, 1031, 4095, ..): symbols missing from a histogram that is still divided by nsym, a row differs.
  * adapt_build_dec starting its search at s = 1: constant_0 (lane 0.. would find symbol 1, whose end is M: symbol 1 in
    every slot), exact_4095, dom_first; the step-over stopping at 254: exact_4095 (slot 4095, the only one of symbol 255,
    is reached by stepping over 254 symbols of width 0 -- it would hold 254, and symbol 255 occurs in every chunk) and
    dom_last at 8 bits (slot 255 likewise, symbol 255 being most of the chunk): section e and the decodes of d.
    constant_255 is found by the search itself (every start is 0) and pins that the search may answer 255.

Wall time on an MI355X: 4.4 s for the 39 cases of this file, 1.8 s of it the first case's setup (it loads the kernels); the
slowest case is a ragged batch at 0.5 s, every other one takes 0.02 to 0.1 s."""
import numpy as np
import pytest

import _model_extremes as X
from _batch import GUARD, POISON
from _oracle import FMT_BYTE, FMT_WORD

FORMATS = {"word-12": (FMT_WORD, 12), "byte-12": (FMT_BYTE, 12), "byte-8": (FMT_BYTE, 8)}
CHUNKS, OTHER_WAYS = X.CHUNKS, X.OTHER_WAYS
OFFSETS = (0, 1, 4)
NAMES = tuple(X.HISTOGRAMS)
F = {FMT_WORD: "word", FMT_BYTE: "byte"}
E_SIZED = {f: "k_encode_adaptive<%s>" % F[f] for f in F}
E_MODELS = {f: "k_encode<%s, per-chunk models>" % F[f] for f in F}
D_MODELS = {f: "k_decode<%s, per-chunk models>" % F[f] for f in F}
D_BATCH = {f: "k_decode_batch_models<%s>" % F[f] for f in F}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def class_input(chunk, last="dom_last"):
    """X.class_plan: every class defined at `chunk` symbols as one chunk each, then `last` at chunk / 3 + 1 symbols
    -> (symbols, [(class, nsym)])."""
    plan = X.class_plan(chunk, last)
    parts = [X.HISTOGRAMS[name](n, 100 + c) for c, (name, n) in enumerate(plan)]
    return np.concatenate(parts), plan


_ORACLE = {}


def oracle_of(oracle, fmt, sb, ways, chunk, last="dom_last"):
    """The oracle's container of class_input(chunk) -- computed once, shared, never written."""
    key = (fmt, sb, ways, chunk, last)
    if key not in _ORACLE:
        h_syms, plan = class_input(chunk, last)
        _ORACLE[key] = (h_syms, plan) + tuple(oracle.encode_chunked_adaptive(fmt, h_syms, ways, chunk, sb))
        for a in _ORACLE[key][2:]:
            a.setflags(write=False)
    return _ORACLE[key]


def place(torch, h_syms, off):
    """The symbols at base + off of an allocation of their own, poison around them."""
    big = torch.full((h_syms.size + 64,), POISON, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    view = big[off:off + h_syms.size]
    view.copy_(torch.from_numpy(h_syms))
    assert view.data_ptr() % 16 == off and view.numel() == h_syms.size
    return view


def host(t, dtype, count=None):
    a = t.cpu().numpy().view(dtype)
    return a if count is None else a[:count]


def check_against_oracle(oracle, what, plan, fmt, sb, ways, chunk, h_syms, enc, o_lens, o_rows):
    """Rows, lengths and every stream of one encode (the tuple the library returns) against the oracle."""
    cont, offs, lens, rows, total = enc
    nchunks = len(plan)
    h_rows = host(rows, np.uint16).reshape(-1, 256)[:nchunks]
    h_lens = host(lens, np.uint32, nchunks)
    bad = np.nonzero((h_rows != o_rows).any(axis=1))[0]
    assert bad.size == 0, (what, "rows differ from the oracle's", [plan[c] for c in bad[:4]])
    bad = np.nonzero(h_lens != o_lens)[0]
    assert bad.size == 0, (what, "lengths differ from the oracle's", [plan[c] for c in bad[:4]], h_lens[bad[:4]], o_lens[bad[:4]])
    count, first = oracle.compare_container_adaptive(fmt, h_syms, ways, chunk, sb, host(cont, np.uint8)[:total], host(offs, np.uint64), h_lens,
                                                     h_rows, threads=1)
    assert count == nchunks and first == -1, (what, first, plan[first[0]] if first != -1 else None)
    return h_lens


def _chunk_cases():
    for fid in FORMATS:
        for chunk in CHUNKS:
            yield pytest.param(fid, chunk, id="%s-%d" % (fid, chunk), marks=pytest.mark.gpu)


# ---- section a ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid,chunk", list(_chunk_cases()))
def test_every_builder_on_every_class(gpu, oracle, fid, chunk):
    """Section a."""
    R, ctx, torch = gpu
    fmt, sb = FORMATS[fid]
    for ways in (64, OTHER_WAYS[chunk]):
        h_syms, plan, o_cont, o_offs, o_lens, o_rows = oracle_of(oracle, fmt, sb, ways, chunk)
        for off in OFFSETS:
            what = (fid, chunk, ways, "base + %d" % off)
            d_syms = place(torch, h_syms, off)
            enc = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt)
            assert ctx.last_encode_kernel()[0] == E_SIZED[fmt], (what, ctx.last_encode_kernel())
            l1 = check_against_oracle(oracle, what + ("one kernel",), plan, fmt, sb, ways, chunk, h_syms, enc, o_lens, o_rows)
            enc = ctx.encode_adaptive(d_syms, ways, chunk, sb, fmt=fmt)
            assert ctx.last_encode_kernel()[0] == E_MODELS[fmt], (what, ctx.last_encode_kernel())
            l3 = check_against_oracle(oracle, what + ("k_chunk_models",), plan, fmt, sb, ways, chunk, h_syms, enc, o_lens, o_rows)
            assert np.array_equal(l1, l3), what


# ---- section b ----------------------------------------------------------------------------------------------------------
def _count_cases():
    for fid in FORMATS:
        for base in X.COUNT_BASES:
            yield pytest.param(fid, base, id="%s-base+%d" % (fid, base), marks=pytest.mark.gpu)


@pytest.mark.parametrize("fid,base", list(_count_cases()))
def test_count_paths(gpu, oracle, fid, base):
    """Section b.  One chunk per call, so that the chunk's address is the base's."""
    R, ctx, torch = gpu
    fmt, sb = FORMATS[fid]
    for size in X.COUNT_SIZES:
        assert X.table_paths(size, base) == X.count_paths(size, base)
        for k, name in enumerate(("dom_last", "all_once")):
            h_syms = X.HISTOGRAMS[name](size, 7 * size + k)
            plan = [(name, size)]
            d_syms = place(torch, h_syms, base)
            for ways in (64, 128):
                _, _, o_lens, o_rows = oracle.encode_chunked_adaptive(fmt, h_syms, ways, size, sb, threads=1)
                assert np.array_equal(o_rows[0], oracle.normalize(X.counts_of(name, size).astype(np.uint32), 1 << sb)[0])
                what = (fid, name, size, "base + %d" % base, ways, sorted(X.table_paths(size, base)))
                enc = ctx.encode_adaptive_sized(d_syms, ways, size, sb, fmt=fmt)
                assert ctx.last_encode_kernel()[0] == E_SIZED[fmt], (what, ctx.last_encode_kernel())
                check_against_oracle(oracle, what + ("one kernel",), plan, fmt, sb, ways, size, h_syms, enc, o_lens, o_rows)
                enc = ctx.encode_adaptive(d_syms, ways, size, sb, fmt=fmt)
                assert ctx.last_encode_kernel()[0] == E_MODELS[fmt], (what, ctx.last_encode_kernel())
                check_against_oracle(oracle, what + ("k_chunk_models",), plan, fmt, sb, ways, size, h_syms, enc, o_lens, o_rows)


# ---- section c ----------------------------------------------------------------------------------------------------------
def check_pieces(what, plan, fmt, sb, ways, is_ragged, chunk, offs, lens, total, o_lens, o_rows):
    """offs[n + 1], lens[n] of a one-kernel container -> every piece inside need_model's window (the oracle's row), the stream at
    its top, pieces in index order."""
    n = len(plan)
    ends = offs[:n].astype(np.int64) + lens.astype(np.int64)
    need = np.diff(np.concatenate(([0], ends)))
    assert int(offs[n]) == int(ends[-1]) == total, (what, "the container's end", int(offs[n]), int(ends[-1]), total)
    assert np.array_equal(lens, o_lens), (what, "lengths differ from the oracle's")
    for c, (name, nsym) in enumerate(plan):
        counts = X.counts_of(name, nsym) if nsym else np.zeros(256, dtype=np.int64)
        lo, hi = X.need_model(fmt, o_rows[c], counts, nsym, ways, sb, is_ragged, chunk_syms=chunk)
        floor = X.need_floor(fmt, o_rows[c], counts, nsym, ways, sb, is_ragged, chunk_syms=chunk)
        print("%s chunk %2d %-12s %6d symbols: stream %6d  need %6d  window [%d, %d]  floor %d" % (what, c, name, nsym, int(lens[c]), int(need[c]), lo, hi,
                                                                                                    floor))
        assert need[c] > 0 and need[c] % 64 == 0, (what, c, name, "a piece is no whole number of lines", int(need[c]))
        assert lo <= need[c] <= hi, (what, c, name, nsym, "need outside the window", int(need[c]), lo, hi)
        assert need[c] >= floor, (what, c, name, nsym, "need below what the 1 + 2^-12 factor gives", int(need[c]), floor)
        assert int(lens[c]) <= need[c], (what, c, name, "the stream is longer than its piece")
    assert np.all(np.diff(ends) > 0), (what, "pieces out of index order")


@pytest.mark.parametrize("fid,chunk", list(_chunk_cases()))
def test_piece_sizes_inside_the_window(gpu, oracle, fid, chunk):
    """Section c, uniform calls (the ragged cap: section d).  A chunk that overflowed its piece (flag 1024) or a container
    without room (flag 2) makes the call raise; the calls here return."""
    R, ctx, torch = gpu
    fmt, sb = FORMATS[fid]
    for ways in (64, OTHER_WAYS[chunk]):
        h_syms, plan, o_cont, o_offs, o_lens, o_rows = oracle_of(oracle, fmt, sb, ways, chunk)
        n = len(plan)
        for off in (0, 1):  # (register-resident / two-pass at 64 ways: the bound is the same code, the coding loop is not)
            what = "%s %d %d-way base + %d" % (fid, chunk, ways, off)
            d_syms = place(torch, h_syms, off)
            cap = int(R._lib.rans_amd_encode_adaptive_sized_bound(fmt, h_syms.size, ways, chunk))
            d_out = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
            cont, offs, lens, rows, total = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt, d_out=d_out, cap=cap)
            h_offs, h_lens, h_cont = host(offs, np.uint64), host(lens, np.uint32, n), host(cont, np.uint8)
            check_pieces(what, plan, fmt, sb, ways, False, chunk, h_offs, h_lens, total, o_lens, o_rows)
            assert total <= cap and np.all(h_cont[total:] == POISON), (what, "written behind the bytes in use")
            for c in range(n):
                a = int(h_offs[c])
                assert np.array_equal(h_cont[a:a + int(h_lens[c])], o_cont[int(o_offs[c]):int(o_offs[c]) + int(o_lens[c])]), (what, plan[c])
            d_out2 = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
            cont2, offs2, lens2, rows2, total2 = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt, d_out=d_out2, cap=cap)
            assert total2 == total and torch.equal(offs2, offs) and torch.equal(lens2, lens) and torch.equal(rows2, rows), (what, "second call")
            live = np.zeros(total, dtype=bool)  # (what lies below a stream inside its piece is never written: compare the streams)
            for c in range(n):
                live[int(h_offs[c]):int(h_offs[c]) + int(h_lens[c])] = True
            assert np.array_equal(host(cont2, np.uint8)[:total][live], h_cont[:total][live]), (what, "second call: the streams differ")


# ---- section d ----------------------------------------------------------------------------------------------------------
def _batch_cases():
    from _kernel_rows import MODEL_ROWS
    for row in MODEL_ROWS:
        yield pytest.param(row, id=row["id"], marks=pytest.mark.gpu)


@pytest.mark.parametrize("row", list(_batch_cases()))
def test_ragged_batches_of_the_classes(gpu, oracle, row):
    """Section d."""
    from _batch import ModelBatch
    from _batch import run_model_row as run_row
    R, ctx, torch = gpu
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    plan = X.batch_plan()
    assert {name for name, _ in plan} == set(NAMES) | {"empty"} and {n for _, n in plan} >= set(X.COUNT_SIZES)
    counts = np.array([n for _, n in plan], dtype=np.uint32)
    contents = {c: X.HISTOGRAMS[name](n, 300 + c) for c, (name, n) in enumerate(plan) if n}
    b = ModelBatch(R, ctx, torch, oracle, row, counts, contents=contents)
    for c, (name, n) in enumerate(plan):  # (the oracle's rows are what the CPU tests hold the classes to)
        if n:
            assert np.array_equal(b.rows[c], oracle.normalize(X.counts_of(name, n).astype(np.uint32), 1 << sb)[0]), (name, n)
    for align in (1, 16):
        run_row(b, align)  # rows, lengths, streams, layout, kernel names, a second run, exact decode of both containers into poison
        assert ctx.decode_errors() == 0
        d_buf, sym_offs = b.laid_out(align)
        starts = sym_offs[:-1][counts > 0] % 16
        assert (np.unique(starts).size >= 8 and np.any(np.diff(starts) != 0)) if align == 1 else np.all(starts == 0), (align, starts)
        (cont, offs, lens, rows, total), _ = b.encode(d_buf, b.dev(sym_offs, np.int64))
        assert ctx.last_encode_kernel()[0] == row["encode"], ctx.last_encode_kernel()
        check_pieces("%s sym_align %d" % (row["id"], align), plan, fmt, sb, ways, True, None, offs, lens, total, b.lens, b.rows)


# ---- section e ----------------------------------------------------------------------------------------------------------
def _decode_cases():
    for fid in FORMATS:
        for ways in (64, 2):
            yield pytest.param(fid, ways, id="%s-%dway" % (fid, ways), marks=pytest.mark.gpu)


@pytest.mark.parametrize("fid,ways", list(_decode_cases()))
def test_decode_table_builder_alone(gpu, oracle, fid, ways):
    """Section e.  Every class at 4096 symbols and constant_255 as the ragged last chunk, the oracle's container and rows: no
    device encoder is involved.  decode_adaptive, then the same streams as a ragged batch whose streams start one symbol
    further apart than they are long (every alignment)."""
    from test_gpu_wave_extremes import exact_container
    R, ctx, torch = gpu
    fmt, sb = FORMATS[fid]
    chunk = 4096
    h_syms, plan, o_cont, o_offs, o_lens, o_rows = oracle_of(oracle, fmt, sb, ways, chunk, last="constant_255")
    assert {"constant_0", "constant_255", "lane_edges", "exact_4095", "dom_last", "sparse_16"} <= {name for name, _ in plan}
    n, nchunks = h_syms.size, len(plan)
    d_cont = exact_container(torch, o_cont.copy(), o_cont.size)  # (the shared arrays are read-only)
    d_offs = torch.from_numpy(o_offs.astype(np.int64)).cuda()
    d_lens = torch.from_numpy(o_lens.astype(np.int32)).cuda()
    d_rows = torch.from_numpy(o_rows.reshape(-1).view(np.int16).copy()).cuda()
    back = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ctx.decode_adaptive(d_cont, o_cont.size, d_offs, d_lens, d_rows, n, ways, chunk, sb, d_out=back[GUARD:GUARD + n], fmt=fmt)
    assert ctx.last_decode_kernel() == D_MODELS[fmt], ctx.last_decode_kernel()
    assert ctx.decode_errors() == 0
    got = back.cpu().numpy()
    wrong = [plan[c] for c in range(nchunks) if not np.array_equal(got[GUARD + c * chunk:GUARD + min(n, (c + 1) * chunk)], h_syms[c * chunk:(c + 1) * chunk])]
    assert not wrong, ("decode_adaptive: chunks decoded wrong", wrong)
    assert np.all(got[:GUARD] == POISON) and np.all(got[GUARD + n:] == POISON), "written outside the output"
    # the batch form
    counts = np.array([m for _, m in plan], dtype=np.uint32)
    sym_offs = GUARD + np.concatenate(([0], np.cumsum(counts.astype(np.int64) + 1)))[:nchunks]
    size = int(sym_offs[-1]) + int(counts[-1]) + GUARD
    want = np.full(size, POISON, dtype=np.uint8)
    for c in range(nchunks):
        want[int(sym_offs[c]):int(sym_offs[c]) + int(counts[c])] = h_syms[c * chunk:c * chunk + int(counts[c])]
    out = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    ctx.decode_batch_adaptive(d_cont, o_cont.size, d_offs, d_lens, d_rows, torch.from_numpy(sym_offs.astype(np.int64)).cuda(),
                              torch.from_numpy(counts.view(np.int32)).cuda(), ways, sb, out, fmt=fmt)
    assert ctx.last_decode_kernel() == D_BATCH[fmt], ctx.last_decode_kernel()
    assert ctx.decode_errors() == 0
    got = out.cpu().numpy()
    wrong = [plan[c] for c in range(nchunks) if not np.array_equal(got[int(sym_offs[c]):int(sym_offs[c]) + int(counts[c])],
                                                                    want[int(sym_offs[c]):int(sym_offs[c]) + int(counts[c])])]
    assert not wrong, ("decode_batch_adaptive: streams decoded wrong", wrong)
    assert np.array_equal(got, want), "decode_batch_adaptive wrote outside its streams"
