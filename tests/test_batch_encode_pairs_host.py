"""Ragged batches CODED with thirty-two 2-way byte streams per wave (RANS_AMD_OPT_BATCH_ENCODE_PAIRS), the part that needs no
GPU: the name test of the pair batch ENCODER, the option's constant, and the proof that the inputs of
tests/test_gpu_batch_encode_pairs.py reach the bounds that file claims.

test_no_pair_batch_enc_kernel_without_a_row: every name of the registry's batch_byte_pairs_encode family (tests/_kernel_rows.py
reads ryg_rans_amd/csrc/kernel_names.hpp) must be the encode name of a row of ENC_PAIR_ROWS, and ENC_PAIR_ROWS must name no
encoder the registry does not hold."""
import numpy as np

import _batch as G
import _kernel_rows as K
import _stream_rate as S
import ryg_rans_amd as R
from _batch import NO_ZERO_WAVE_LOADS, RATE_WAVES, rate_kind, rate_model
from _kernel_rows import ENC_PAIR_ROWS, ENC_PAIRS, check_family_rows, check_option_constant
from _oracle import FMT_BYTE


def test_no_pair_batch_enc_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    check_family_rows(ENC_PAIRS)
    # the decoder is named where the issue names it, and asked of the default context elsewhere (None)
    assert {(r["sb"], r["decode"]) for r in ENC_PAIR_ROWS} == {(14, "k_decode_batch<byte>"), (16, "k_decode_batch<byte>"), (12, None), (8, None),
                                                              (10, None)}


def test_batch_encode_pairs_option_constant():
    check_option_constant("BATCH_ENCODE_PAIRS", 8)


def _full_windows(rb, n):
    """Sums over every window of eight FULL rounds (an odd count's last round holds state 0 alone)."""
    return S.windows(rb[:n // 2])


def test_rate_inputs_reach_the_rings_bound():
    """1. Under 255 x 1 + one common symbol at 16 bits (_batch.rate_model) a state that meets a frequency-1
    symbol puts two bytes, in every round: the frequency-1-only streams of the GPU file with at least eight rounds hold 32
    bytes in every window of eight full rounds -- a block per check of the pair's ring, its bound --, the common-only ones
    emit nothing (the 65536-symbol one: a thousand and more silent rounds in a row)."""
    assert K.OPT_BATCH_ENCODE_PAIRS == R.OPT_BATCH_ENCODE_PAIRS and K.OPT_BATCH_PAIRS == R.OPT_BATCH_PAIRS
    assert K.E16["sb"] == 16 and K.EMAIN["sb"] == 14
    freqs, counts, contents, _ = G.rate_batch(16)
    assert np.array_equal(freqs, rate_model(16)) and counts.size == 64
    rare_long = 0
    for k in range(64):
        n = int(counts[k])
        rb = S.round_bytes(FMT_BYTE, freqs, 16, contents[k], 2)
        if rate_kind(k) == "rare":
            assert np.all(freqs[contents[k]] == 1)
            if n // 2 >= 8:
                w = _full_windows(rb, n)
                assert w.min() == 32 and w.max() == 32, (k, n, w.min(), w.max())
                rare_long += 1
        else:
            assert np.all(contents[k] == S.COMMON) and rb.sum() == 0, (k, n)
    assert rare_long >= 20, rare_long
    silent = 0
    for name, (w_counts, w_kinds) in RATE_WAVES.items():
        freqs, counts, contents, _ = G.rate_wave(16, name)
        assert counts.size == 32
        for k in range(32):
            n = int(counts[k])
            rb = S.round_bytes(FMT_BYTE, freqs, 16, contents[k], 2)
            if w_kinds[k] == "rare":
                if n // 2 >= 8:
                    w = _full_windows(rb, n)
                    assert w.min() == 32 and w.max() == 32, (name, k, n)
            elif n == 65536:
                assert S.longest_silence(rb) >= 1000, (name, k, S.longest_silence(rb))
                silent += 1
            else:
                assert rb.sum() == 0, (name, k)
    assert silent >= 1


def test_a_dead_pair_is_fed_the_rings_bound():
    """2. The MIRRORED model, f = ones(256), f[255] = 2^16 - 255: byte value 0 -- what a dead pair codes -- is a frequency-1
    symbol.  A stream of zeros holds 32 bytes in every window of eight full rounds (4097 zeros: 30..32, and a window below 32
    holds the odd count's half round); a stream of 255s is silent (4096 of them: 2 bytes in all).
    3. The finish inputs begin with at least 64 frequency-1 symbols other than 0 and never contain 0.
    4. The no-zero model has f[0] == 0, and no content under it holds a 0."""
    f = G.mirrored_model()
    want = np.ones(256, dtype=np.uint32)
    want[255] = (1 << 16) - 255
    assert np.array_equal(f, want) and int(f.sum()) == 1 << 16 and f[0] == 1
    rb = S.round_bytes(FMT_BYTE, f, 16, np.zeros(4096, dtype=np.uint8), 2)
    w = S.windows(rb)
    assert w.min() == 32 and w.max() == 32, (w.min(), w.max())
    rb = S.round_bytes(FMT_BYTE, f, 16, np.zeros(4097, dtype=np.uint8), 2)
    w = S.windows(rb)
    assert rb.size == 2049 and w.min() == 30 and w.max() == 32, (w.min(), w.max())
    assert np.all(_full_windows(rb, 4097) == 32) and np.all(np.nonzero(w < 32)[0] + 8 == rb.size)  # (the window with the half round)
    rb = S.round_bytes(FMT_BYTE, f, 16, np.full(4096, 255, dtype=np.uint8), 2)
    assert rb.sum() == 2 and S.longest_silence(rb) >= 1000, (int(rb.sum()), S.longest_silence(rb))
    # 3.
    freqs, counts, contents = G.finish_batch()
    assert np.array_equal(freqs, f) and counts.tolist() == [128 * (g % 8 + 1) for g in range(32)]
    for g in range(32):
        c = contents[g]
        assert c.size == counts[g] and not np.any(c == 0)
        assert np.all(freqs[c[:64]] == 1) and np.all(c[:64] != 0)
        S.simulate(FMT_BYTE, freqs, 16, c, 2)  # (a valid stream under the model)
    # 4.
    freqs, counts, contents = G.no_zero_batch(*NO_ZERO_WAVE_LOADS)
    assert freqs[0] == 0 and int(freqs.sum()) == 1 << 14 and counts.size == 96 and int(np.count_nonzero(counts == 0)) >= 1
    assert all(contents[k].size == counts[k] and not np.any(contents[k] == 0) for k in range(96))
    assert len({int(c) >> 5 for c in counts[32:64]}) >= 16 and counts[32:64].max() >= 256  # (the pairs die at different pieces)
