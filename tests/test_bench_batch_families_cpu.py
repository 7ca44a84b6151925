"""tools/bench_batch_families.py without a GPU: its summarising function recomputes every committed record of the six
streams-per-wave families from the record's own pass times, and its table is held to the library's options, the registry and
the families' descriptors of tests/_kernel_rows.py."""
import importlib.util
import json
import os

import pytest

import ryg_rans_amd as R
from _kernel_rows import ROOT, STREAM_FAMILIES, UNIFORM, registry

spec = importlib.util.spec_from_file_location("bench_batch_families", os.path.join(ROOT, "tools", "bench_batch_families.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)

RAW = ("kernel", "pass_ms_mean", "ms_min")  # of a variant: what a run measures; everything else summarise() works out


def committed(row):
    return json.load(open(os.path.join(ROOT, "profiles", row.out)))


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_records_recompute(family):
    """Every key of the committed record, at both levels, comes out of summarise() with the identical value -- ms_mean, every
    ratio, ordered_gate, accepted and the fastest / slowest passes included -- when it is fed the record's run metadata and, per
    variant, kernel, pass_ms_mean and ms_min alone.  No tolerance: the records were written with round(x, 4)."""
    row = T.FAMILIES[family]
    rec = committed(row)
    nested = {name: rec[name] for name in row.batches} if len(row.batches) > 1 else {"ragged": rec}
    batches = {}
    for name, b in nested.items():
        variants = T.variant_names(row, name == row.batches[-1])
        assert set(variants) == {key for key, val in b.items() if isinstance(val, dict) and "kernel" in val}
        batches[name] = {key: b[key] for key in ("symbols", "streams", "mean_stream_syms")}
        batches[name].update((key, {f: b[key][f] for f in RAW}) for key in variants)
        # the recorded names are the table's (the uniform one at the recorded size: above every threshold)
        assert all(b[key]["kernel"] == T.expected_kernel(row, key, 1 << 40, 1) for key in variants)
    got = T.summarise(row, {key: rec[key] for key in ("steps", "warmup", "passes", "device")}, batches)
    assert rec["passes"] == row.passes and rec["n_ways"] == row.ways and rec["format"] == row.label and rec["sym_align"] == row.sym_align

    def check(want, have, where):
        for key, val in want.items():
            assert key in have, (where, key)
            if isinstance(val, dict):
                check(val, have[key], where + (key,))
            else:
                assert have[key] == val and type(have[key]) is type(val), (where, key, have[key], val)
    check(rec, got, (family,))


def test_table_against_registry():
    """Every row's option exists in the package and is its descriptor's, the row's family kernel is the descriptor's main kernel
    and its wave kernel the descriptor's, its uniform kernels are names of the registry's uniform family, and rows and
    descriptors correspond one to one."""
    by_option = {d.option: d for d in STREAM_FAMILIES}
    assert len(by_option) == len(STREAM_FAMILIES) == len(T.FAMILIES) == 6
    seen = set()
    for name, row in T.FAMILIES.items():
        d = by_option[getattr(R, row.option)]
        seen.add(d.option)
        assert (row.side, getattr(R, row.fmt), row.ways, row.scale_bits) == (d.side, d.fmt, d.ways, d.main["sb"]), name
        assert row.family == d.main[d.side] and row.family in registry()[d.family], name
        assert row.wave == d.wave_kernel, name
        assert row.uniform in registry()[UNIFORM] and (row.uniform_below is None or row.uniform_below[1] in registry()[UNIFORM]), name
        assert name == ("encode_" if row.side == "encode" else "") + row.variant
        assert os.path.exists(os.path.join(ROOT, "profiles", row.out)), name
    assert seen == set(by_option)
