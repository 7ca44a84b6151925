"""Ragged batches with eight 8-way word streams per wave (RANS_AMD_OPT_BATCH_GROUPS), the part that needs no GPU: the name
test of the group batch kernels and the option's constant.

test_no_group_batch_kernel_without_a_row: every name of the registry's batch_word_groups_decode family (tests/_kernel_rows.py
reads ryg_rans_amd/csrc/kernel_names.hpp) must be the decode name of a row of GROUP_ROWS, and GROUP_ROWS must name no decoder
the registry does not hold."""
import os
import re

import ryg_rans_amd as R
from _kernel_rows import BATCH_WORD_GROUPS_DECODE, GROUP_ROWS, ROOT, registry


def test_no_group_batch_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    names = registry()[BATCH_WORD_GROUPS_DECODE]
    assert "k_decode_batch_word_groups" in names
    rows = {r["decode"] for r in GROUP_ROWS}
    assert names == rows, ("kernels no row of GROUP_ROWS expects", sorted(names - rows), "names no launcher reports", sorted(rows - names))
    # the check has teeth: without its row a kernel is reported missing
    less = {r["decode"] for r in GROUP_ROWS if r["id"] != "word-8-groups"}
    assert "k_decode_batch_word_groups" in names - less


def test_batch_groups_option_constant():
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    m = re.search(r"RANS_AMD_OPT_BATCH_GROUPS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 5
    assert R.OPT_BATCH_GROUPS == 5
    # (a NULL context is refused before the option is looked at; the values 0 and 1 need a context: tests/test_gpu_batch_groups.py)
    assert R.lib().rans_amd_ctx_set_option(None, 5, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()
