"""tools/bench_batch_singles.py without a GPU: the committed record of its four rows (profiles/batch_singles.json) recomputes
from its own pass times with tools/bench_batch_families.py's summarise(), the gate holds for every format whose row is in the
library's table, and the rows are held to the library's option, the registry's fourth list and the descriptors of
tests/_batch_singles.py.  Mirrors tests/test_bench_batch_alias_pairs_cpu.py."""
import importlib.util
import json
import os

import pytest

import _batch_singles as N
import ryg_rans_amd as R
from _kernel_rows import ROOT, UNIFORM, registry

spec = importlib.util.spec_from_file_location("bench_batch_singles", os.path.join(ROOT, "tools", "bench_batch_singles.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)  # (it imports tools/bench_batch_families.py from its own directory)
T = B.T
RAW = ("kernel", "pass_ms_mean", "ms_min")  # of a variant: what a run measures; everything else summarise() works out
FORMAT_OF = {"byte": "byte", "rans64": "r64", "word": "word", "alias": "alias"}  # the record's key -> tests/_batch_singles.py's


def committed():
    return json.load(open(os.path.join(ROOT, "profiles", B.OUT)))


@pytest.mark.parametrize("name", list(B.ROWS))
def test_records_recompute(name):
    """Every key of a format's committed record comes out of summarise() with the identical value -- ms_mean, every ratio,
    ordered_gate, accepted and the fastest / slowest passes included -- when it is fed the record's run metadata and, per
    variant, kernel, pass_ms_mean and ms_min alone.  No tolerance: the records were written with round(x, 4)."""
    row = B.ROWS[name]
    rec = committed()["formats"][name]
    variants = T.variant_names(row, True)
    assert variants == ("wave", "wave_ordered", "singles", "singles_ordered", "uniform")
    assert set(variants) == {key for key, val in rec.items() if isinstance(val, dict) and "kernel" in val}
    batch = {key: rec[key] for key in ("symbols", "streams", "mean_stream_syms")}
    batch.update((key, {f: rec[key][f] for f in RAW}) for key in variants)
    assert all(rec[key]["kernel"] == T.expected_kernel(row, key, 1 << 40, 1) for key in variants)
    got = T.summarise(row, {key: rec[key] for key in ("steps", "warmup", "passes", "device")}, {"ragged": batch})
    assert rec["passes"] == row.passes == 3 and rec["n_ways"] == row.ways == 1 and rec["format"] == row.label == name
    assert rec["sym_align"] == row.sym_align == 64 and rec["scale_bits"] == row.scale_bits and rec["uniform_chunk_syms"] == row.chunk == 1024

    def check(want, have, where):
        for key, val in want.items():
            assert key in have, (where, key)
            if isinstance(val, dict):
                check(val, have[key], where + (key,))
            else:
                assert have[key] == val and type(have[key]) is type(val), (where, key, have[key], val)
    check(rec, got, (name,))
    assert set(got) == set(rec)


def test_the_gate_holds_for_every_format_in_one_run():
    """The acceptance condition is the families' own, for all four formats in the same run: the slowest pass of singles_ordered
    is faster than the fastest pass of wave_ordered, on the 181 992-stream log-uniform batch; `accepted` of the file is the
    conjunction (tools/bench_batch_singles.py combine())."""
    rec = committed()
    assert list(rec["formats"]) == list(B.ROWS) == ["byte", "rans64", "word", "alias"]
    assert rec == B.combine(rec["formats"]) and rec["accepted"] is True
    first = rec["formats"]["byte"]
    for name, r in rec["formats"].items():
        assert r["accepted"] is True and r["ordered_gate"] is True, name
        assert r["singles_ordered_slowest_pass_ms"] < r["wave_ordered_fastest_pass_ms"], name
        assert r["streams"] == 181992 and r["symbols"] == first["symbols"] and r["device"] == first["device"], name
        assert (r["steps"], r["warmup"], r["passes"]) == (first["steps"], first["warmup"], first["passes"]), name


def test_rows_against_registry():
    """Every row's option exists in the package and is the descriptors', its family kernel is the format's descriptor's main
    kernel (a name of the registry's fourth list) and its wave kernel the descriptor's, its scale_bits the main row's, its
    uniform kernel a name of the registry's uniform family; and tools/bench_batch_families.py's table is still the six
    families."""
    assert len(T.FAMILIES) == 6
    assert {row.family for row in B.ROWS.values()} == N.fourth_list_names()
    for name, row in B.ROWS.items():
        d = N.SINGLES[FORMAT_OF[name]]
        assert getattr(R, row.option) == d.option == 13
        assert (row.variant, row.side, getattr(R, row.fmt), row.ways, row.scale_bits) == ("singles", d.side, d.fmt, 1, d.main["sb"])
        assert row.family == d.main[d.side] and row.wave == d.wave_kernel
        assert row.uniform == "k_decode_lanes_staged" and row.uniform in registry()[UNIFORM] and row.uniform_below is None
        assert row.batches == ("ragged",) and row.out == B.OUT == "batch_singles.json" and row.sym_align == 64
    assert os.path.exists(os.path.join(ROOT, "profiles", B.OUT))
