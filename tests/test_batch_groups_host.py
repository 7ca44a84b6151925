"""Ragged batches with eight 8-way word streams per wave (RANS_AMD_OPT_BATCH_GROUPS), the part that needs no GPU: the name
test of the group batch kernels and the option's constant.

test_no_group_batch_kernel_without_a_row: the launchers of the kernels that pack several ragged streams into a wave report
their kernel through an out-parameter spelled `*group_batch_kernel = ...;` -- a fourth spelling beside `*name = ...;`
(tests/test_gpu_kernel_matrix.py), `*batch_kernel = ...;` (tests/test_batch_host.py) and `*models_batch_kernel = ...;`
(tests/test_batch_models_host.py), invisible to those three tests.  Every literal of such a statement in
ryg_rans_amd/csrc/*.hip must be the decode name of a row of GROUP_ROWS in tests/test_gpu_batch_groups.py, and GROUP_ROWS must
name no decoder the sources do not contain."""
import glob
import os
import re

import ryg_rans_amd as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ryg_rans_amd", "csrc")
_LITERAL = re.compile(r'"((?:[^"\\]|\\.)*)"')


def source_group_batch_kernel_names(csrc=CSRC):
    """Every string literal of a statement `*group_batch_kernel = ...;` in csrc/*.hip -> (names, number of statements)."""
    names, sites = set(), 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        for m in re.finditer(r"\*group_batch_kernel\s*=\s*([^;]*);", open(path).read()):
            sites += 1
            names.update(_LITERAL.findall(m.group(1)))
    return names, sites


def test_no_group_batch_kernel_without_a_row():
    from test_gpu_batch_groups import GROUP_ROWS
    names, sites = source_group_batch_kernel_names()
    assert sites >= 1, sites
    assert "k_decode_batch_word_groups" in names
    rows = {r["decode"] for r in GROUP_ROWS}
    assert names == rows, ("kernels no row of GROUP_ROWS expects", sorted(names - rows), "names no launcher reports", sorted(rows - names))
    # disjoint from what the three other spellings' scans find
    from test_batch_host import source_batch_kernel_names
    from test_batch_models_host import source_models_batch_kernel_names
    from test_gpu_kernel_matrix import source_kernel_names
    assert not names & source_kernel_names()[0]
    assert not names & source_batch_kernel_names()[0]
    assert not names & source_models_batch_kernel_names()[0]
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
