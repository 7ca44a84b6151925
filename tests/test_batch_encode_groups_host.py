"""Ragged batches CODED with eight 8-way word streams per wave (RANS_AMD_OPT_BATCH_ENCODE_GROUPS) and the batch encoders'
hand-out order (rans_amd_encode_batch_ordered), the part that needs no GPU: the name test of the group batch ENCODERS, the
option's constant, the entry point, and the proof that the rate inputs of tests/test_gpu_batch_encode_groups.py reach the
bounds that file claims.

test_no_group_batch_enc_kernel_without_a_row: every name of the registry's batch_word_groups_encode family
(tests/_kernel_rows.py reads ryg_rans_amd/csrc/kernel_names.hpp) must be the encode name of a row of ENC_GROUP_ROWS, and
ENC_GROUP_ROWS must name no encoder the registry does not hold."""
import os

import numpy as np

import _stream_rate as S
import ryg_rans_amd as R
from _batch import NO_ZERO_OCTETS, RATE_OCTET_KINDS, finish_octet, no_zero_batch, rate_octet
from _kernel_rows import ENC_GROUPS, ROOT, check_family_rows, check_option_constant
from _oracle import FMT_WORD


def test_no_group_batch_enc_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    check_family_rows(ENC_GROUPS)


def test_batch_encode_groups_option_constant():
    check_option_constant("BATCH_ENCODE_GROUPS", 6)


def test_encode_batch_ordered_refuses_a_null_context():
    assert "rans_amd_encode_batch_ordered" in open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    rc = R.lib().rans_amd_encode_batch_ordered(None, None, None, None, None, 0, 8, None, None, None, 0, None, None, None)
    assert rc == R.E_ARG
    assert b"NULL argument" in R.lib().rans_amd_last_error()


def test_rate_inputs_reach_their_bounds():
    """The rare-only streams of the GPU file's rate octet hold a window of eight rounds with 96 bytes -- a 128-byte block
    per check of the group's ring, the most a valid stream can emit --, its quiet streams have at least 1000 consecutive
    rounds without a byte, and its bursts hold both; the finish octet's streams begin with rare symbols."""
    freqs, counts, contents = rate_octet()
    assert np.array_equal(freqs, S.quiet_model()) and counts.size == 8
    seen = {"rare": 0, "quiet": 0, "bursts": 0}
    for g, kind in enumerate(RATE_OCTET_KINDS):
        assert contents[g].size == counts[g]
        rb = S.round_bytes(FMT_WORD, freqs, 12, contents[g], 8)
        if kind.startswith("rare+"):
            assert np.array_equal(contents[g][:8], S.rare_only(freqs, int(counts[g]), 60 + g)[:8])
            assert S.windows(rb).max() == 96, (g, S.windows(rb).max())
            seen["rare"] += 1
        elif kind == "quiet":
            assert np.all(contents[g] == S.COMMON)
            assert S.longest_silence(rb) >= 1000, (g, S.longest_silence(rb))
            seen["quiet"] += 1
        else:
            w = S.windows(rb)
            assert w.max() == 96 and w.min() == 0, (g, w.min(), w.max())
            seen["bursts"] += 1
    assert min(seen.values()) >= 2, seen
    assert len(set(counts.tolist())) >= 7 and len({int(c) >> 7 for c in counts}) >= 6  # (the groups finish in different iterations)
    freqs, counts, contents = finish_octet()
    rare, common = S.rare_and_common(freqs)
    assert common == 0 and counts.tolist() == [128 * k for k in range(1, 9)]
    for g in range(8):  # whole lines only; the symbols the coder sees last are rare: the state it leaves is large
        assert np.all(np.isin(contents[g][:64], rare)) and S.windows(S.round_bytes(FMT_WORD, freqs, 12, contents[g], 8)).max() == 96
    freqs, counts, contents = no_zero_batch(*NO_ZERO_OCTETS)
    assert freqs[0] == 0 and int(freqs.sum()) == 4096 and counts.size == 24
    assert all(contents[k].size == counts[k] and not np.any(contents[k] == 0) for k in range(24))
    assert len({int(c) >> 7 for c in counts[8:16]}) >= 4 and counts[8:16].max() >= 256
