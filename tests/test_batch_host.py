"""Ragged batches, the part that needs no GPU: rans_amd_batch_layout and rans_amd_batch_slice against numpy, their argument
errors, and the name test of the batch kernels.

test_no_batch_kernel_without_a_row: every name of the registry's batch family (tests/_kernel_rows.py reads
ryg_rans_amd/csrc/kernel_names.hpp) must be named by a row of BATCH_ROWS, and BATCH_ROWS must name no kernel the registry does
not hold."""
import ctypes as C

import numpy as np
import pytest

import ryg_rans_amd as R
from _batch import edge_counts
from _kernel_rows import BATCH, BATCH_ROWS, registry, row_batch_kernel_names
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

FORMATS = (FMT_BYTE, FMT_WORD, FMT_R64, FMT_ALIAS)
WAYS = (1, 2, 8, 64, 128, 500)
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _up(v, a):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_layout_equals_numpy(fmt):
    counts = edge_counts(3)
    for ways in WAYS:
        bound = np.array([R.chunk_bound(fmt, int(c), ways) for c in counts], dtype=np.uint64)
        for align in (1, 4, 16):
            sym, slot = R.batch_layout(counts, fmt, ways, align)
            assert sym.dtype == np.uint64 and sym.size == counts.size + 1 and slot.size == counts.size + 1
            want_sym = np.concatenate(([0], np.cumsum(_up(counts.astype(np.uint64), align))))
            want_slot = np.concatenate(([0], np.cumsum(_up(bound, 16))))
            assert np.array_equal(sym, want_sym), (ways, align)
            assert np.array_equal(slot, want_slot), (ways, align)
            # every slot holds at least rans_amd_chunk_bound bytes and starts on 16
            assert np.all(np.diff(slot) >= bound) and np.all(slot % 16 == 0)
            # symbol ranges do not overlap and start on the alignment
            assert np.all(sym % align == 0) and np.all(np.diff(sym) >= counts)
    sym, slot = R.batch_layout(np.zeros(0, np.uint32), fmt, 64, 4)
    assert sym.tolist() == [0] and slot.tolist() == [0]


@pytest.mark.parametrize("fmt,sb", [(FMT_BYTE, 16), (FMT_WORD, 12), (FMT_R64, 16), (FMT_ALIAS, 16)])
def test_batch_slots_hold_the_oracles_worst_stream(oracle, fmt, sb):
    """The worst input for a static model: every symbol is the model's rarest one (frequency 1: the most bits a symbol can
    cost).  The oracle's stream of it must fit the slot batch_layout gives a stream of that count."""
    freqs = np.zeros(256, dtype=np.uint32)
    freqs[0] = (1 << sb) - 255
    freqs[1:] = 1
    om = oracle.model(freqs, sb, with_alias=(fmt == FMT_ALIAS))
    counts = np.array([0, 1, 7, 64, 65, 1000, 4099], dtype=np.uint32)
    for ways in (1, 2, 8, 64, 128, 500):
        _, slot = R.batch_layout(counts, fmt, ways, 1)
        for c, room in zip(counts, np.diff(slot)):
            worst = np.full(int(c), 255, dtype=np.uint8)
            assert oracle.encode(fmt, om, worst, ways).size <= int(room), (ways, int(c))


def _slice_numpy(lengths, G):
    lengths = np.asarray(lengths, dtype=np.uint64)
    before = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)  # bytes in front of stream i, i = 0 .. n
    total = int(before[-1])
    targets = np.array([g * total // G for g in range(G)], dtype=np.uint64)
    b = np.searchsorted(before, targets, side="left").astype(np.uint64)
    return np.concatenate((b, [lengths.size])).astype(np.uint64)


def test_batch_slice_equals_searchsorted():
    rng = np.random.default_rng(11)
    cases = [rng.integers(0, 70000, 1000).astype(np.uint32), np.zeros(17, np.uint32), np.array([5], np.uint32),
             np.array([0, 0, 9, 0, 0, 0, 1, 0], np.uint32), np.array([1 << 31] * 5, np.uint32), np.zeros(0, np.uint32),
             np.array([1000000, 1, 1, 1], np.uint32)]
    for lengths in cases:
        for G in (1, 2, 8, lengths.size + 3):
            got = R.batch_slice(lengths, G)
            assert got.size == G + 1 and got[0] == 0 and got[G] == lengths.size
            assert np.all(np.diff(got.astype(np.int64)) >= 0)
            assert np.array_equal(got, _slice_numpy(lengths, G)), (lengths[:8], G)
    # more ranks than streams: some ranks are empty, every stream belongs to exactly one rank
    got = R.batch_slice(np.array([3, 3, 3], np.uint32), 8)
    assert np.count_nonzero(np.diff(got.astype(np.int64)) == 0) >= 5 and int(np.diff(got.astype(np.int64)).sum()) == 3
    # all-zero lengths: everything lands in the last rank
    assert R.batch_slice(np.zeros(6, np.uint32), 4).tolist() == [0, 0, 0, 0, 6]


def test_batch_argument_errors():
    lib = R.lib()
    counts = np.array([5, 6], dtype=np.uint32)
    so, sl = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    cp, sop, slp = counts.ctypes.data_as(u32p), so.ctypes.data_as(u64p), sl.ctypes.data_as(u64p)
    assert lib.rans_amd_batch_layout(cp, 2, FMT_WORD, 64, 1, sop, slp) == R.OK
    assert lib.rans_amd_batch_layout(None, 2, FMT_WORD, 64, 1, sop, slp) == R.E_ARG
    assert lib.rans_amd_batch_layout(cp, 2, FMT_WORD, 64, 1, None, slp) == R.E_ARG
    assert lib.rans_amd_batch_layout(cp, 2, FMT_WORD, 64, 1, sop, None) == R.E_ARG
    assert lib.rans_amd_batch_layout(cp, 2, FMT_WORD, 64, 0, sop, slp) == R.E_ARG
    for fmt, ways in ((FMT_WORD, 0), (FMT_WORD, 513), (7, 64), (-1, 64)):
        assert not R.ways_supported(fmt, ways)
        assert lib.rans_amd_batch_layout(cp, 2, fmt, ways, 1, sop, slp) == R.E_UNSUPPORTED
    with pytest.raises(R.RansAmdError) as e:
        R.batch_layout(counts, FMT_BYTE, 1000)
    assert e.value.status == R.E_UNSUPPORTED
    b = np.zeros(4, np.uint64)
    assert lib.rans_amd_batch_slice(cp, 2, 3, b.ctypes.data_as(u64p)) == R.OK
    assert lib.rans_amd_batch_slice(None, 2, 3, b.ctypes.data_as(u64p)) == R.E_ARG
    assert lib.rans_amd_batch_slice(cp, 2, 3, None) == R.E_ARG
    assert lib.rans_amd_batch_slice(cp, 2, 0, b.ctypes.data_as(u64p)) == R.E_ARG
    # the device entry points refuse NULL handles before they touch a GPU
    assert lib.rans_amd_encode_batch(None, None, None, None, None, 1, 64, None, None, 0, None, None, None) == R.E_ARG
    assert lib.rans_amd_decode_batch(None, None, None, 0, None, None, None, None, 1, 64, None, None, 0, None, None) == R.E_ARG
    assert lib.rans_amd_batch_order(None, None, 1, None, None) == R.E_ARG


# ---- the name test --------------------------------------------------------------------------------------------------


def test_no_batch_kernel_without_a_row():
    """(The scan of the sources this test once read counted its assignment statements to guard its own completeness, and was
    held disjoint from the other families' scans; the launchers now report a KernelId, and registry() asserts that no name
    occurs twice.)"""
    names = registry()[BATCH]
    for must in ("k_decode_batch_word64", "k_decode_batch<word>", "k_decode_batch<byte>", "k_decode_batch<byte, slot records>",
                 "k_decode_batch<r64>", "k_decode_batch<r64 search>", "k_decode_batch<alias>", "k_decode_batch<word, u16 symbols>",
                 "k_encode_batch<word>"):
        assert must in names, must
    assert all(n.startswith(("k_decode_batch", "k_encode_batch")) for n in names), names
    rows = row_batch_kernel_names(BATCH_ROWS)
    assert not names - rows, ("batch kernels no row of BATCH_ROWS expects", sorted(names - rows))
    assert not rows - names, ("BATCH_ROWS names kernels no launcher reports", sorted(rows - names))
    # the check has teeth: without its row a kernel is reported missing
    less = [r for r in BATCH_ROWS if r["decode"] != "k_decode_batch<alias>"]
    assert "k_decode_batch<alias>" in names - row_batch_kernel_names(less)
