"""tools/bench_batch_alias_pairs.py without a GPU: the committed records of its two rows recompute from their own pass times
with tools/bench_batch_families.py's summarise(), and the rows are held to the library's option, the registry's lists and the
descriptor of tests/_batch_alias_pairs.py.  Mirrors tests/test_bench_batch_families_cpu.py."""
import importlib.util
import json
import os

import pytest

import ryg_rans_amd as R
from _batch_alias_pairs import ALIAS_PAIRS, second_list_names
from _kernel_rows import PAIRS, PROW, ROOT, UNIFORM, registry

spec = importlib.util.spec_from_file_location("bench_batch_alias_pairs", os.path.join(ROOT, "tools", "bench_batch_alias_pairs.py"))
A = importlib.util.module_from_spec(spec)
spec.loader.exec_module(A)  # (it imports tools/bench_batch_families.py from its own directory)
T = A.T
RAW = ("kernel", "pass_ms_mean", "ms_min")  # of a variant: what a run measures; everything else summarise() works out


def committed(row):
    return json.load(open(os.path.join(ROOT, "profiles", row.out)))


@pytest.mark.parametrize("name", list(A.ROWS))
def test_records_recompute(name):
    """Every key of the committed record comes out of summarise() with the identical value -- ms_mean, every ratio,
    ordered_gate, accepted and the fastest / slowest passes included -- when it is fed the record's run metadata and, per
    variant, kernel, pass_ms_mean and ms_min alone.  No tolerance: the records were written with round(x, 4)."""
    row = A.ROWS[name]
    rec = committed(row)
    variants = T.variant_names(row, True)
    assert set(variants) == {key for key, val in rec.items() if isinstance(val, dict) and "kernel" in val}
    batch = {key: rec[key] for key in ("symbols", "streams", "mean_stream_syms")}
    batch.update((key, {f: rec[key][f] for f in RAW}) for key in variants)
    assert all(rec[key]["kernel"] == T.expected_kernel(row, key, 1 << 40, 1) for key in variants)
    got = T.summarise(row, {key: rec[key] for key in ("steps", "warmup", "passes", "device")}, {"ragged": batch})
    assert rec["passes"] == row.passes == 3 and rec["n_ways"] == row.ways == 2 and rec["format"] == row.label
    assert rec["sym_align"] == row.sym_align == 4 and rec["scale_bits"] == row.scale_bits == 16 and rec["uniform_chunk_syms"] == row.chunk == 1024

    def check(want, have, where):
        for key, val in want.items():
            assert key in have, (where, key)
            if isinstance(val, dict):
                check(val, have[key], where + (key,))
            else:
                assert have[key] == val and type(have[key]) is type(val), (where, key, have[key], val)
    check(rec, got, (name,))
    assert set(got) == set(rec)


def test_the_gate_and_the_comparison():
    """The acceptance condition is the tool's own: the slowest pass of alias_pairs_ordered is faster than the fastest pass of
    wave_ordered, on the 181 992-stream log-uniform batch -- and the byte pairs' record at 16 bits is a run over the same
    counts (the comparison is reported, not gated on)."""
    rec, byte16 = committed(A.ROWS["alias_pairs"]), committed(A.ROWS["byte_pairs_16bit"])
    assert rec["accepted"] is True and rec["ordered_gate"] is True
    assert rec["alias_pairs_ordered_slowest_pass_ms"] < rec["wave_ordered_fastest_pass_ms"]
    assert rec["streams"] == byte16["streams"] == 181992 and rec["symbols"] == byte16["symbols"]
    assert rec["device"] == byte16["device"] and (rec["steps"], rec["warmup"]) == (byte16["steps"], byte16["warmup"])


def test_rows_against_registry():
    """The alias row's option exists in the package and is the descriptor's, its family kernel is the descriptor's main kernel
    (the one name of the registry's second list) and its wave kernel the descriptor's, its uniform kernel a name of the
    registry's uniform family; the second row is the byte pairs' row of tools/bench_batch_families.py at 16 bits and nothing
    else; and that module's table is still the six families."""
    row, d = A.ROWS["alias_pairs"], ALIAS_PAIRS
    assert list(A.ROWS) == ["alias_pairs", "byte_pairs_16bit"] and len(T.FAMILIES) == 6
    assert getattr(R, row.option) == d.option == 11
    assert (row.variant, row.side, getattr(R, row.fmt), row.ways, row.scale_bits) == ("alias_pairs", d.side, d.fmt, d.ways, d.main["sb"])
    assert row.family == d.main[d.side] and {row.family} == second_list_names(d.family)
    assert row.wave == d.wave_kernel and row.uniform in registry()[UNIFORM] and row.uniform_below is None
    assert row.batches == ("ragged",) and row.out == "batch_alias_pairs.json"
    b16 = A.ROWS["byte_pairs_16bit"]
    assert b16 == T.FAMILIES["pairs"]._replace(scale_bits=16, out=b16.out) and b16.out != T.FAMILIES["pairs"].out
    assert getattr(R, b16.option) == PAIRS.option and b16.family == PROW["byte-2-pairs-16bit"]["decode"] and b16.wave == PAIRS.wave_kernel
    for r in A.ROWS.values():
        assert os.path.exists(os.path.join(ROOT, "profiles", r.out)), r.out
