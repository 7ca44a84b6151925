"""tools/bench_batch_encode_alias_pairs.py without a GPU: the committed records of its three rows recompute from their own pass
times with tools/bench_batch_families.py's summarise(), and the rows are held to the library's option, the registry's lists and
the descriptor of tests/_batch_encode_alias_pairs.py.  Mirrors tests/test_bench_batch_alias_pairs_cpu.py."""
import importlib.util
import json
import os

import pytest

import ryg_rans_amd as R
from _batch_encode_alias_pairs import ENC_ALIAS_PAIRS, third_list_names
from _kernel_rows import E16, ENC_PAIRS, ROOT, UNIFORM, registry

spec = importlib.util.spec_from_file_location("bench_batch_encode_alias_pairs", os.path.join(ROOT, "tools", "bench_batch_encode_alias_pairs.py"))
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
    assert rec["sym_align"] == row.sym_align == 4 and rec["scale_bits"] == row.scale_bits and rec["uniform_chunk_syms"] == row.chunk == 1024

    def check(want, have, where):
        for key, val in want.items():
            assert key in have, (where, key)
            if isinstance(val, dict):
                check(val, have[key], where + (key,))
            else:
                assert have[key] == val and type(have[key]) is type(val), (where, key, have[key], val)
    check(rec, got, (name,))
    assert set(got) == set(rec)


def test_the_gate_and_the_comparisons():
    """The acceptance condition is the tool's own, on the 16-bit row: the slowest pass of alias_pairs_ordered is faster than the
    fastest pass of wave_ordered -- k_encode_batch<alias, LDS remap> with the same d_order, in the same run --, on the
    181 992-stream log-uniform batch.  The 12-bit row and the byte pair encoder's at 16 bits are runs over the same counts on
    the same device (the comparisons are reported, not gated on)."""
    rec = committed(A.ROWS["encode_alias_pairs"])
    assert rec["accepted"] is True and rec["ordered_gate"] is True and rec["scale_bits"] == 16
    assert rec["alias_pairs_ordered_slowest_pass_ms"] < rec["wave_ordered_fastest_pass_ms"]
    assert rec["wave_ordered"]["kernel"] == "k_encode_batch<alias, LDS remap>" and rec["alias_pairs_ordered"]["kernel"] == "k_encode_batch_alias_pairs"
    for other in ("encode_alias_pairs_12bit", "encode_byte_pairs_16bit"):
        o = committed(A.ROWS[other])
        assert rec["streams"] == o["streams"] == 181992 and rec["symbols"] == o["symbols"]
        assert rec["device"] == o["device"] and (rec["steps"], rec["warmup"]) == (o["steps"], o["warmup"])


def test_rows_against_registry():
    """The alias rows' option exists in the package and is the descriptor's, their family kernel is the descriptor's main kernel
    (the one name of the registry's third list) and their wave kernel the descriptor's, their uniform kernels names of the
    registry's uniform family; the 12-bit row is the 16-bit row at 12 bits and nothing else; the third row is the byte pair
    encoder's row of tools/bench_batch_families.py at 16 bits and nothing else; and that module's table is still the six
    families."""
    row, d = A.ROWS["encode_alias_pairs"], ENC_ALIAS_PAIRS
    assert list(A.ROWS) == ["encode_alias_pairs", "encode_alias_pairs_12bit", "encode_byte_pairs_16bit"] and len(T.FAMILIES) == 6
    assert getattr(R, row.option) == d.option == 12
    assert (row.variant, row.side, getattr(R, row.fmt), row.ways, row.scale_bits) == ("alias_pairs", d.side, d.fmt, d.ways, d.main["sb"])
    assert row.family == d.main[d.side] and {row.family} == third_list_names(d.family)
    assert row.wave == d.wave_kernel and row.uniform in registry()[UNIFORM] and row.uniform_below[1] in registry()[UNIFORM]
    assert row.batches == ("ragged",) and row.out == "batch_encode_alias_pairs.json"
    r12 = A.ROWS["encode_alias_pairs_12bit"]
    assert r12 == row._replace(scale_bits=12, out=r12.out) and r12.out != row.out
    b16 = A.ROWS["encode_byte_pairs_16bit"]
    assert b16 == T.FAMILIES["encode_pairs"]._replace(scale_bits=16, out=b16.out) and b16.out != T.FAMILIES["encode_pairs"].out
    assert getattr(R, b16.option) == ENC_PAIRS.option and b16.family == E16["encode"] and E16["sb"] == 16 and b16.wave == ENC_PAIRS.wave_kernel
    for r in A.ROWS.values():
        assert os.path.exists(os.path.join(ROOT, "profiles", r.out)), r.out
