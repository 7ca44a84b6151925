"""Ragged batches with thirty-two 2-way byte streams per wave (RANS_AMD_OPT_BATCH_PAIRS), the part that needs no GPU: the name
test of the pair batch kernel, the option's constant, and the proof that the rate inputs of tests/test_gpu_batch_pairs.py
reach the bounds that file claims.

test_no_pair_batch_kernel_without_a_row: every name of the registry's batch_byte_pairs_decode family (tests/_kernel_rows.py
reads ryg_rans_amd/csrc/kernel_names.hpp) must be the decode name of a row of PAIR_ROWS, and PAIR_ROWS must name no decoder
the registry does not hold."""
import numpy as np

import _batch as G
import _kernel_rows as K
import _stream_rate as S
import ryg_rans_amd as R
from _kernel_rows import PAIRS, check_family_rows, check_option_constant
from _oracle import FMT_BYTE


def test_no_pair_batch_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    check_family_rows(PAIRS)


def test_batch_pairs_option_constant():
    check_option_constant("BATCH_PAIRS", 7)


def test_rate_inputs_reach_the_rings_bound():
    """The 16-bit model of 255 frequency-1 symbols and one common symbol (tests/test_gpu_rate_extremes.py b_case's).
      * A state in [2^23, 2^31) that meets a frequency-1 symbol becomes x >> 16 < 2^15 and takes two bytes, in every round: every
        frequency-1-only stream of the GPU file with at least eight rounds has a window of eight rounds that takes 32 bytes,
        what one refill brings -- every window does.
      * A common symbol costs log2(65536 / 65281) = 0.0056 bits: a state takes a byte every 1400 rounds or so.  The common-only
        streams of the 64-stream batch are 384 rounds at the most and take nothing at all -- a cursor that never moves beside
        quad-mates at the bound --, and the 65536-symbol one of the single wave-load has 1000 and more consecutive silent
        rounds.  (No stream of fewer than 1000 rounds can show a thousand silent ones: the thousand rounds are the long
        stream's.)
    The inputs are the GPU file's own generators (tests/_batch.py)."""
    assert K.OPT_BATCH_PAIRS == R.OPT_BATCH_PAIRS and K.OPT_BATCH_GROUPS == R.OPT_BATCH_GROUPS  # (the option these inputs are decoded under)
    assert 16 in G.RATE_BITS and K.PAIR_RATE_ROW[16]["sb"] == 16
    freqs, counts, contents, phases = G.rate_batch(16)
    b_freqs = np.ones(256, dtype=np.uint32)
    b_freqs[S.COMMON] = (1 << 16) - 255
    assert np.array_equal(freqs, b_freqs) and int(freqs.sum()) == 1 << 16
    assert counts.size == G.RATE_STREAMS == 64 and sorted(p % 64 for p in phases) == list(range(64))
    assert set(counts.tolist()) == {128 * b + t for b in (0, 1, 5) for t in (0, 1, 77, 127)}
    kinds = [G.rate_kind(k) for k in range(64)]
    assert all((kinds[k] == "common") == (k % 3 == 2) for k in range(64))
    # every count meets both kinds; in every quad both streams' kinds and counts are on record
    assert {(kinds[k], int(counts[k])) for k in range(64)} == {(kd, c) for kd in ("rare", "common") for c in set(counts.tolist())}
    rare_long = 0
    for k in range(64):
        rb = S.round_bytes(FMT_BYTE, freqs, 16, contents[k], 2)
        n = int(counts[k])
        if kinds[k] == "rare":
            assert np.all(np.isin(contents[k], np.nonzero(freqs == 1)[0]))
            if n // 2 >= 8:
                w = S.windows(rb[:n // 2])
                assert w.size >= 1 and w.max() == 32 and w.min() == 32, (k, n, w.min(), w.max())
                rare_long += 1
        else:
            assert np.all(contents[k] == S.COMMON)
            assert rb.sum() == 0 and S.longest_silence(rb) == (n + 1) // 2, (k, n, int(rb.sum()))
    assert rare_long >= 20, rare_long
    for name in G.RATE_WAVES:
        freqs, counts, contents, phases = G.rate_wave(16, name)
        w_kinds = G.RATE_WAVES[name][1]
        assert counts.size == 32 and len(set(p % 64 for p in phases)) == 32
        for k in range(32):
            rb = S.round_bytes(FMT_BYTE, freqs, 16, contents[k], 2)
            n = int(counts[k])
            if w_kinds[k] == "rare":
                if n // 2 >= 8:
                    w = S.windows(rb[:n // 2])
                    assert w.max() == 32 and w.min() == 32, (name, k, n)
            elif n >= 2000:
                assert S.longest_silence(rb) >= 1000, (name, k, S.longest_silence(rb))
            else:
                assert rb.sum() == 0, (name, k)
    # the stalled cursor really is in the file: a common-only stream of 2000 symbols and more
    assert any(c >= 2000 and kd == "common" for cs, kds in G.RATE_WAVES.values() for c, kd in zip(cs, kds))
