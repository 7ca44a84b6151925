"""Ragged batches with one model per stream, the part that needs no GPU: rans_amd_encode_batch_adaptive_bound against numpy
and against the oracle's streams, the argument errors of the three entry points, and the name test of their kernels.

test_no_models_batch_kernel_without_a_row: every name of the registry's batch_models family (tests/_kernel_rows.py reads
ryg_rans_amd/csrc/kernel_names.hpp) must be named by a row of MODEL_ROWS, and MODEL_ROWS must name no kernel the registry does
not hold."""
import ctypes as C

import numpy as np
import pytest

import ryg_rans_amd as R
from _batch import edge_counts
from _kernel_rows import BATCH_MODELS, MODEL_ROWS, registry
from _oracle import FMT_BYTE, FMT_R64, FMT_WORD

WAYS = (1, 2, 8, 64, 128, 500)
u32p = C.POINTER(C.c_uint32)


def _up(v, a):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("fmt", [FMT_BYTE, FMT_WORD])
def test_bound_equals_numpy(fmt):
    counts = edge_counts(3)
    for ways in WAYS:
        # a stream's worst case: two bytes a symbol and the flushed states, in whole 64-byte lines
        want = int(_up(counts.astype(np.uint64) * 2 + ways * 4, 64).sum())
        assert R.encode_batch_adaptive_bound(fmt, counts, ways) == want, ways
        per = [R.encode_batch_adaptive_bound(fmt, counts[c:c + 1], ways) for c in range(counts.size)]
        assert sum(per) == want and all(p % 64 == 0 and p >= R.chunk_bound(fmt, int(c), ways) for p, c in zip(per, counts))
    assert R.encode_batch_adaptive_bound(fmt, np.zeros(0, np.uint32), 64) == 16  # (an empty batch still gets a buffer)


@pytest.mark.parametrize("fmt,sb", [(FMT_BYTE, 8), (FMT_BYTE, 12), (FMT_WORD, 12)])
def test_a_streams_share_of_the_bound_holds_the_oracles_stream(oracle, fmt, sb):
    """All one value (word format: frequency 4096, a word leaves per symbol -- the worst a stream can cost), all 256 values
    once, uniform random: the oracle's stream under the stream's OWN model fits what _bound adds for a stream of that count."""
    rng = np.random.default_rng(5)
    for ways in WAYS:
        for n in (1, ways - 1, ways + 1, 4 * ways + 3, 4099):
            if n == 0:
                continue
            inputs = [np.full(n, 201, dtype=np.uint8), rng.integers(0, 256, n).astype(np.uint8)]
            if n == 4099:
                inputs.append(np.arange(256, dtype=np.uint8))
            for syms in inputs:
                stream = oracle.encode(fmt, oracle.model_for(syms, 256, sb), syms, ways)
                share = R.encode_batch_adaptive_bound(fmt, np.array([syms.size], np.uint32), ways)
                assert stream.size <= share, (ways, syms.size, stream.size, share)
        empty = oracle.encode(fmt, oracle.model_for(np.arange(256, dtype=np.uint8), 256, sb), np.zeros(0, np.uint8), ways)
        assert empty.size == 4 * ways <= R.encode_batch_adaptive_bound(fmt, np.zeros(1, np.uint32), ways)


def test_argument_errors():
    lib = R.lib()
    counts = np.array([5, 6], dtype=np.uint32)
    cp = counts.ctypes.data_as(u32p)
    assert lib.rans_amd_encode_batch_adaptive_bound(FMT_WORD, cp, 2, 64) == 2 * 320
    # _bound: 0 for what the encoder refuses
    assert lib.rans_amd_encode_batch_adaptive_bound(FMT_WORD, None, 2, 64) == 0
    for fmt, ways in ((FMT_WORD, 0), (FMT_WORD, 513), (FMT_R64, 64), (3, 64), (7, 64), (-1, 64)):
        assert lib.rans_amd_encode_batch_adaptive_bound(fmt, cp, 2, ways) == 0, (fmt, ways)
    # the device entry points refuse NULL handles before they touch a GPU
    assert lib.rans_amd_encode_batch_adaptive(None, FMT_WORD, None, 0, None, None, 1, 64, 12, None, 0, None, None, None, None, None) == R.E_ARG
    assert lib.rans_amd_decode_batch_adaptive(None, FMT_WORD, None, 0, None, None, None, None, None, 1, 64, 12, None, None, 0, None,
                                              None) == R.E_ARG
    # ... and check every other argument before they use the context: a block of zeroes stands in for one here (no GPU),
    # with buffers that are never touched because each call is refused
    fake = C.create_string_buffer(4096)
    buf = (C.c_uint64 * 1024)()
    h, b = C.addressof(fake), C.addressof(buf)

    def enc(fmt=FMT_WORD, ways=64, sb=12, out=b, offs=b, lens=b, freqs=b, sym_offs=b, sym_counts=b, syms=b):
        return lib.rans_amd_encode_batch_adaptive(h, fmt, syms, 16, sym_offs, sym_counts, 1, ways, sb, out, 4096, offs, lens, freqs, None, None)

    def dec(fmt=FMT_WORD, ways=64, sb=12, cont=b, offs=b, lens=b, freqs=b, sym_offs=b, sym_counts=b, out=b):
        return lib.rans_amd_decode_batch_adaptive(h, fmt, cont, 4096, offs, lens, freqs, sym_offs, sym_counts, 1, ways, sb, None, out, 16,
                                                  None, None)
    for call in (enc, dec):
        for fmt in (FMT_R64, 3, 7, -1):
            assert call(fmt=fmt) == R.E_UNSUPPORTED, fmt
        assert call(fmt=FMT_WORD, sb=11) == R.E_UNSUPPORTED and call(fmt=FMT_WORD, sb=13) == R.E_UNSUPPORTED
        assert call(fmt=FMT_BYTE, sb=7) == R.E_UNSUPPORTED and call(fmt=FMT_BYTE, sb=13) == R.E_UNSUPPORTED
        assert call(ways=0) == R.E_UNSUPPORTED and call(ways=513) == R.E_UNSUPPORTED
        for name in ("offs", "lens", "freqs", "sym_offs", "sym_counts", "out"):
            assert call(**{name: None}) == R.E_ARG, name
        assert call(freqs=b + 4) == R.E_ARG  # (rows are read and written with 8-byte accesses)
    assert enc(syms=None) == R.E_ARG and dec(cont=None) == R.E_ARG
    assert enc(out=b + 8) == R.E_ARG and dec(cont=b + 8) == R.E_ARG  # 16-byte alignment of the container


def test_no_models_batch_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    names = registry()[BATCH_MODELS]
    assert names == {"k_decode_batch_models<word>", "k_decode_batch_models<byte>", "k_encode_batch_models<word>",
                     "k_encode_batch_models<byte>"}, names
    rows = {r[k] for r in MODEL_ROWS for k in ("decode", "encode")}
    assert not names - rows, ("kernels no row of MODEL_ROWS expects", sorted(names - rows))
    assert not rows - names, ("MODEL_ROWS names kernels no launcher reports", sorted(rows - names))
    # the check has teeth: without its rows a kernel is reported missing
    less = {r[k] for r in MODEL_ROWS if r["fmt"] != FMT_BYTE for k in ("decode", "encode")}
    assert names - less == {"k_decode_batch_models<byte>", "k_encode_batch_models<byte>"}
