"""tools/bench_batch_families.py on the GPU, one small run per family: --symbols 4194304 (about 700 ragged streams with a partial
last wave-load, 8192 equal ones: above every family's threshold of 8, 32 or 64 streams), two launches behind one warm-up launch,
one pass, in this process through the tool's entry function.  The tool verifies every variant and asserts the kernel it
reports before it times anything; the test asserts that this happened for every variant, and that the record it wrote holds
every key of the committed one at both levels.  No timing is asserted.

Wall time on an MI355X: 4.6 s for the six cases -- 1.6 s the first one (it loads the kernels), 0.8 s each of the two lane families
(two batches), 0.5 s each of the others."""
import importlib.util
import json
import os

import pytest

from _kernel_rows import ROOT

spec = importlib.util.spec_from_file_location("bench_batch_families", os.path.join(ROOT, "tools", "bench_batch_families.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def missing(want, have, where=()):
    """The keys of `want`, nested ones included, that `have` lacks."""
    out = []
    for k, v in want.items():
        if k not in have:
            out.append(where + (k,))
        elif isinstance(v, dict):
            out += missing(v, have[k], where + (k,))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_small_run(family, tmp_path, capsys):
    row, out = T.FAMILIES[family], tmp_path / "record.json"
    assert __debug__, "the tool's checks are assert statements"
    T.main(["--family", family, "--symbols", "4194304", "--steps", "2", "--warmup", "1", "--passes", "1", "--out", str(out)])
    err = capsys.readouterr().err.splitlines()
    rec = json.load(open(out))
    nested = {name: rec[name] for name in row.batches} if len(row.batches) > 1 else {"ragged": rec}
    for name, b in nested.items():
        # enough for every family's kernel, and the ragged batch's last wave-load is partial at 8, 32 and 64 streams per wave
        assert b["streams"] >= 64 and (name == "equal" or all(b["streams"] % per_wave for per_wave in (8, 32, 64))), (name, b["streams"])
        for key in T.variant_names(row, name == row.batches[-1]):
            assert "%s: %s verified, %s" % (name, key, b[key]["kernel"]) in err, (name, key)
            assert len(b[key]["pass_ms_mean"]) == 1
            if key != "uniform":
                assert b[key]["kernel"] == T.expected_kernel(row, key)
    assert missing(json.load(open(os.path.join(ROOT, "profiles", row.out))), rec) == []
