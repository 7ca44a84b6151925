"""Ragged batches with eight 8-way word streams per wave (RANS_AMD_OPT_BATCH_GROUPS), the part that needs no GPU: the name
test of the group batch kernels and the option's constant.

test_no_group_batch_kernel_without_a_row: every name of the registry's batch_word_groups_decode family (tests/_kernel_rows.py
reads ryg_rans_amd/csrc/kernel_names.hpp) must be the decode name of a row of GROUP_ROWS, and GROUP_ROWS must name no decoder
the registry does not hold."""
from _kernel_rows import GROUPS, check_family_rows, check_option_constant


def test_no_group_batch_kernel_without_a_row():
    """(No count of assignment statements and no disjointness from other scans any more: the launchers report a KernelId, and
    registry() asserts that no name occurs twice.)"""
    check_family_rows(GROUPS)


def test_batch_groups_option_constant():
    check_option_constant("BATCH_GROUPS", 5)
