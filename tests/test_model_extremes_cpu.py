"""No GPU: the inputs of tests/test_gpu_model_extremes.py reach what that file says they reach, and the plain models of
tests/_model_extremes.py agree with the oracle.

What every class reaches (Oracle.normalize; REACH below asserts it; repairs = symbols squeezed to width 0 that took a slot):

  class          12 bits, 16 384 symbols                                   8 bits (4096 / 8192 / 16 384 symbols)
  dom_first/mid  191 repairs, ONE victim (the dominant symbol: 4032 ->     239 / 247 / 251 repairs, one victim worn down to
                 3841), 255 ones                                            width 1 -- the loop stops there --, all ones
  dom_last       192 repairs (no symbol behind 255 shares its edge), one    240 / 248 / 252, all ones
                 victim, 3841 + 255 ones
  tie_chain      150 repairs over 50 victims: 200, 201, .. 249 in           239 repairs at 16 384, all ones
                 ascending order, each from width 4 down to 1 before the
                 next -- equal widths, lowest index first
  exact_2048     {2048, 2048}, no repair: `small` holds                     {128, 128}
  exact_2049     {2049, 2047}, no repair: `small` does not                  {128, 128}
  exact_4095     {4095, 1}, no repair: one below `always`                   {255, 1}
  constant_x     4096 = M at symbol 0 / 255 (word format: a word leaves     256 = M
                 per symbol, the piece is the worst-case slot)
  all_once       16 each                                                    1 each, no repair
  lane_edges     nine symbols, every one starts on a multiple of M >> 6 behind >= 4 symbols of width 0, the last one is 199
  sparse_16      16 symbols of width M / 16: one every four lanes of the decode-table builder

The bound (need_model's lo against the length of the oracle's stream, both formats, 2 / 64 / 512 ways, every class at 4096,
8192 and 16 384 symbols and at every size of the count-path table it is defined at): where lo is the bound itself the
smallest lo - length is 64 (byte format) and 72 (word format); where lo is the worst-case slot it is 0 for constant word
chunks (the slot IS the stream: 2 n + 4 N bytes) and 56 for a byte chunk of one symbol at 2 ways.
test_the_oracle_stream_fits_lo prints the smallest margin per format and asserts these floors."""
import numpy as np

import _model_extremes as X
from _oracle import FMT_BYTE, FMT_WORD

FORMATS = ((FMT_WORD, 12), (FMT_BYTE, 12), (FMT_BYTE, 8))
CHUNKS = (4096, 8192, 16384)
WAYS = (2, 64, 512)

# (class, nsym, scale_bits) -> (repairs, distinct victims)
REACH = {
    ("dom_first", 16384, 12): (191, 1), ("dom_mid", 16384, 12): (191, 1), ("dom_last", 16384, 12): (192, 1),
    ("tie_chain", 16384, 12): (150, 50),
    ("exact_2048", 4096, 12): (0, 0), ("exact_2049", 4096, 12): (0, 0), ("exact_4095", 4096, 12): (0, 0),
    ("all_once", 4096, 8): (0, 0), ("all_once", 4096, 12): (0, 0),
    ("lane_edges", 4096, 12): (0, 0), ("lane_edges", 4096, 8): (0, 0), ("sparse_16", 4096, 12): (0, 0), ("sparse_16", 4096, 8): (0, 0),
}


def oracle_row(oracle, counts, sb):
    f, _ = oracle.normalize(np.asarray(counts, dtype=np.uint32), 1 << sb)
    return f.astype(np.int64)


def all_sizes(name):
    return [n for n in sorted(set(CHUNKS) | set(X.COUNT_SIZES)) if X.supports(name, n)]


def test_the_histograms_are_exact():
    """Every class, every size it is defined at: the shuffled content has exactly counts_of's histogram, two seeds differ."""
    for name, make in X.HISTOGRAMS.items():
        sizes = all_sizes(name)
        assert sizes, name
        for n in sizes:
            a = make(n, 1)
            assert a.dtype == np.uint8 and a.size == n
            assert np.array_equal(np.bincount(a, minlength=256), X.counts_of(name, n)), (name, n)
            if np.count_nonzero(X.counts_of(name, n)) > 1 and n >= 64:
                assert not np.array_equal(a, make(n, 2)), (name, n)
    for name in ("dom_first", "dom_last", "dom_mid", "constant_0", "constant_255", "all_once"):
        assert all_sizes(name) == sorted(set(CHUNKS) | set(X.COUNT_SIZES)), name  # (what the count-path tests feed: defined everywhere)


def test_normalize_model_is_the_oracles(oracle):
    for name in X.HISTOGRAMS:
        for n in all_sizes(name):
            for sb in (12, 8):
                counts = X.counts_of(name, n)
                width, pairs = X.normalize_model(counts, 1 << sb)
                assert width is not None and int(width.sum()) == 1 << sb, (name, n, sb)
                assert np.array_equal(width, oracle_row(oracle, counts, sb)), (name, n, sb)


def test_every_class_reaches_its_condition(oracle, capsys):
    report = []
    for (name, n, sb), (repairs, victims) in REACH.items():
        counts = X.counts_of(name, n)
        width, pairs = X.normalize_model(counts, 1 << sb)
        assert np.array_equal(width, oracle_row(oracle, counts, sb))
        report.append("%-12s %6d symbols %2d bits: %3d repairs, %2d victims" % (name, n, sb, len(pairs), len({v for _, v in pairs})))
        assert (len(pairs), len({v for _, v in pairs})) == (repairs, victims), (name, n, sb, len(pairs))
    # one victim, worn down: 12 bits -> 3841 and 255 ones
    for name, x in (("dom_first", 0), ("dom_mid", 128), ("dom_last", 255)):
        width, pairs = X.normalize_model(X.counts_of(name, 16384), 4096)
        assert {v for _, v in pairs} == {x} and width[x] == 3841 and np.all(np.delete(width, x) == 1)
        assert [s for s, _ in pairs] == sorted(s for s, _ in pairs)
        for n in CHUNKS:  # 8 bits: the victim ends at width 1 and the loop stops
            width, pairs = X.normalize_model(X.counts_of(name, n), 256)
            assert np.all(width == 1) and 239 <= len(pairs) <= 254 and {v for _, v in pairs} == {x}, (name, n, len(pairs))
            assert np.array_equal(width, oracle_row(oracle, X.counts_of(name, n), 8))
            report.append("%-12s %6d symbols  8 bits: %3d repairs, 1 victim, all ones" % (name, n, len(pairs)))
    # tie order: the victims in ascending index among equal widths, each used up before the next
    width, pairs = X.normalize_model(X.counts_of("tie_chain", 16384), 4096)
    assert [v for _, v in pairs] == [200 + i // 3 for i in range(150)]
    assert np.all(width[200:250] == 1) and np.all(width[250:255] == 4) and np.all(width[:200] == 1)
    width8, pairs8 = X.normalize_model(X.counts_of("tie_chain", 16384), 256)
    assert np.all(width8 == 1) and {v for _, v in pairs8} == {255}
    # the reciprocal classes: width == count at 4096 symbols, and the same widths at every multiple
    for name, want in (("exact_2048", {7: 2048, 250: 2048}), ("exact_2049", {7: 2049, 250: 2047}), ("exact_4095", {0: 4095, 255: 1})):
        for n in CHUNKS:
            row = oracle_row(oracle, X.counts_of(name, n), 12)
            assert {int(s): int(row[s]) for s in np.nonzero(row)[0]} == want, (name, n)
        assert np.array_equal(oracle_row(oracle, X.counts_of(name, 4096), 12), X.counts_of(name, 4096))
    for name, x in (("constant_0", 0), ("constant_255", 255)):
        for sb in (12, 8):
            row = oracle_row(oracle, X.counts_of(name, 4096), sb)
            assert row[x] == 1 << sb and np.count_nonzero(row) == 1
    assert np.all(oracle_row(oracle, X.counts_of("all_once", 4096), 8) == 1)
    with capsys.disabled():
        print("\n" + "\n".join(report))


def test_lane_edges_start_on_lane_boundaries(oracle):
    """From the oracle's row: every occupied symbol of lane_edges (and of sparse_16) starts at lane * (M >> 6) for some lane of
    the decode-table builder; lane_edges: behind a run of at least four symbols of width 0, nothing occupied above 200."""
    for sb in (12, 8):
        per = (1 << sb) >> 6
        for n in CHUNKS + (64, 1024, 5120):
            row = oracle_row(oracle, X.counts_of("lane_edges", n), sb)
            start = np.concatenate(([0], np.cumsum(row)))[:256]
            occ = np.nonzero(row)[0]
            assert [int(s) for s in occ] == [s for s, _ in X.LANE_EDGES] and occ[-1] <= 200
            assert np.all(start[occ] % per == 0), (sb, n)
            assert len({int(x) for x in start[occ] // per}) == len(occ) >= 5  # several, on different lanes
            for s in occ:
                assert s >= 4 and np.all(row[s - 4:s] == 0), (sb, n, int(s))
            assert [int(x) for x in row[occ]] == [w * per for _, w in X.LANE_EDGES]
        row = oracle_row(oracle, X.counts_of("sparse_16", 4096), sb)
        occ = np.nonzero(row)[0]
        assert tuple(int(s) for s in occ) == X.SPARSE_16 and np.all(row[occ] == 4 * per)


def test_the_oracle_stream_fits_lo(oracle, capsys):
    """The condition the GPU tests build on: the oracle's stream of a chunk is never longer than need_model's lo, for the
    uniform and the ragged cap alike.  Margins: 0 where the worst-case slot is used (constant word chunks), 64 and more
    elsewhere."""
    smallest = {}
    for fmt, sb in FORMATS:
        for name, make in X.HISTOGRAMS.items():
            for n in all_sizes(name):
                syms = make(n, 11)
                counts = X.counts_of(name, n)
                row = oracle_row(oracle, counts, sb)
                for ways in WAYS:
                    _, _, lens, rows = oracle.encode_chunked_adaptive(fmt, syms, ways, n, sb, threads=1)
                    assert np.array_equal(rows[0].astype(np.int64), row)
                    for ragged in (False, True):
                        lo, hi = X.need_model(fmt, row, counts, n, ways, sb, ragged)
                        assert lo % 64 == 0 and lo <= hi <= X.worst_slot(n, ways)
                        assert int(lens[0]) <= lo, (fmt, sb, name, n, ways, ragged, int(lens[0]), lo)
                        always = fmt == FMT_WORD and name.startswith("constant")
                        if always:
                            assert lo == hi == X.worst_slot(n, ways) and int(lens[0]) == 2 * n + 4 * ways
                        key = (fmt, sb, "worst-case slot" if lo == X.worst_slot(n, ways) else "bound")
                        m = lo - int(lens[0])
                        if key not in smallest or m < smallest[key][0]:
                            smallest[key] = (m, name, n, ways)
    with capsys.disabled():
        print()
        for (fmt, sb, kind), (m, name, n, ways) in sorted(smallest.items()):
            print("fmt %d, %2d bits, %-15s: smallest lo - oracle length %5d  (%s, %d symbols, %d ways)" % (fmt, sb, kind, m, name, n, ways))
    for (fmt, sb, kind), (m, name, n, ways) in smallest.items():
        assert m >= (0 if kind == "worst-case slot" else 64), (fmt, sb, kind, m, name, n, ways)
    assert smallest[(FMT_WORD, 12, "worst-case slot")][0] == 0


def test_the_factor_is_visible_in_the_plans(capsys):
    """need_floor on the very pieces the GPU tests look at (class_plan: uniform calls; batch_plan: ragged batches): never above
    hi, below lo nowhere, and above lo -- a whole line -- on at least one piece of every ragged batch (FACTOR_SIZES): there a
    kernel without the 1 + 2^-12 factor, which returns lo, is caught."""
    from _kernel_rows import MODEL_ROWS
    calls = [("uniform %d" % chunk, fmt, sb, ways, False, chunk, X.class_plan(chunk)) for fmt, sb in FORMATS for chunk in X.CHUNKS
             for ways in (64, X.OTHER_WAYS[chunk])]
    calls += [("ragged " + r["id"], r["fmt"], r["sb"], r["ways"], True, None, X.batch_plan()) for r in MODEL_ROWS]
    seen = {}
    for what, fmt, sb, ways, is_ragged, chunk, plan in calls:
        for name, n in plan:
            counts = X.counts_of(name, n) if n else np.zeros(256, dtype=np.int64)
            row = X.normalize_model(counts, 1 << sb)[0] if n else counts
            lo, hi = X.need_model(fmt, row, counts, n, ways, sb, is_ragged, chunk_syms=chunk)
            floor = X.need_floor(fmt, row, counts, n, ways, sb, is_ragged, chunk_syms=chunk)
            assert lo <= floor <= hi and hi - lo in (0, 64), (what, name, n, lo, floor, hi)
            k = seen.setdefault(what if is_ragged else "uniform calls", [0, 0])
            k[0] += 1
            k[1] += floor > lo
    with capsys.disabled():
        print()
        for what, (pieces, above) in sorted(seen.items()):
            print("%-22s: need_floor a line above lo on %d of %d pieces" % (what, above, pieces))
    assert all(above >= 1 for what, (_, above) in seen.items() if what != "uniform calls"), seen


def test_need_model_edges():
    """An empty stream of a ragged batch gets the states' lines; the uniform cap is the call's full chunk, not the short last one."""
    z = np.zeros(256)
    assert X.need_model(FMT_WORD, z, z, 0, 64, 12, True) == (256, 256)
    assert X.need_model(FMT_BYTE, z, z, 0, 2, 8, True) == (64, 64)
    counts = X.counts_of("all_once", 1024)
    row, _ = X.normalize_model(counts, 4096)
    for ragged in (False, True):  # 8 bits a symbol, far below either cap
        assert X.need_model(FMT_WORD, row, counts, 1024, 64, 12, ragged, chunk_syms=4096) == (1408, 1408)  # 1024 + 11 + 256 + 64 = 1355
    counts = X.counts_of("constant_0", 1)
    row, _ = X.normalize_model(counts, 256)
    assert X.need_model(FMT_BYTE, row, counts, 1, 2, 8, True) == (64, 64)                     # the stream's own worst case: 2 + 8 bytes
    assert X.need_model(FMT_BYTE, row, counts, 1, 2, 8, False, chunk_syms=4096) == (128, 128)  # 0 + 8 + 64 under the call's cap


def test_the_size_grid_holds_every_count_path():
    """COUNT_TABLE is what the kernel's loop bounds give, for both count passes, and the grid enters every loop: alone, one
    behind the other, once and more than once."""
    assert max(X.COUNT_SIZES) == 16384 + 1024 + 7 and {4096, 4096 + 1024, 4096 - 1, 1024 + 7, 1027, 64, 3, 1} <= set(X.COUNT_SIZES)
    for n in X.COUNT_SIZES:
        for base in X.COUNT_BASES:
            for b in (base, base + 16, base + 8 if base else 32):  # (what counts is the address modulo 16 and modulo 4)
                assert X.count_paths(n, b) == X.table_paths(n, base), (n, b)
            models = X.count_paths(n, base, trip=0)  # k_chunk_models: the trips are rounds of its 1024-loop
            assert models == {X.LOOP if p == X.TRIP else p for p in X.table_paths(n, base)}, (n, base)
    seen = {base: [frozenset(X.table_paths(n, base)) for n in X.COUNT_SIZES] for base in X.COUNT_BASES}
    for combo in ("T", "L", "4", "b", "TL", "T4", "Tb", "Lb", "L4", "4b", "L4b", "TL4b"):
        assert frozenset(X._LETTER[ch] for ch in combo) in seen[0], combo
    assert set(seen[4]) == {frozenset({X.DWORD}), frozenset({X.TAIL}), frozenset({X.DWORD, X.TAIL})}
    assert set(seen[1]) == {frozenset({X.TAIL})}
    # the loops' trip counts: the prefetch branch of the 4096-trip (a next trip exists), two and more rounds of the 1024-loop,
    # a dword loop and a byte tail of more than one round of the wave (256 / 64 symbols), and of less
    assert any(n // 4096 >= 2 for n in X.COUNT_SIZES) and any(n // 4096 == 1 for n in X.COUNT_SIZES)
    assert any(n < 4096 and n // 1024 >= 2 for n in X.COUNT_SIZES) and any((n % 4096) // 1024 == 3 for n in X.COUNT_SIZES)
    assert any(256 < n < 1024 or (n % 1024) & ~3 > 256 for n in X.COUNT_SIZES) and any(0 < (n % 1024) & ~3 < 256 for n in X.COUNT_SIZES)
    assert any(n > 64 for n in X.COUNT_SIZES) and any(n < 64 for n in X.COUNT_SIZES)  # (odd base: the byte loop over the whole chunk)
