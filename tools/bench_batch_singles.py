#!/usr/bin/env python3
"""Ragged batch DECODE of the non-interleaved (1-way) layout of all four formats: one stream per wave against sixty-four
streams per wave (RANS_AMD_OPT_BATCH_SINGLES), one run on one GPU.

    python tools/bench_batch_singles.py [--format byte|rans64|word|alias|all]

The method is tools/bench_batch_families.py's run_batch -- workload (181 992 log-uniform streams, about 1 GiB of symbols, laid
out at sym_align 64), verification of every variant and of the kernel it reports, alternating passes over wave, wave_ordered,
singles, singles_ordered and uniform (the n_ways = 1 uniform decode of the same symbols in 1024-symbol chunks on
k_decode_lanes_staged: the floor) -- and its summarise() with the families' own gate per format: the slowest pass of
singles_ordered beats the fastest pass of wave_ordered.  This file adds the rows only (that module's FAMILIES is the six
families of tests/_kernel_rows.py) and puts the four records into one file, profiles/batch_singles.json:

    {"formats": {"byte": <record>, "rans64": <record>, "word": <record>, "alias": <record>}, "accepted": every format's gate}

  byte     FMT_BYTE at 14 bits (main.cpp)          k_decode_batch<byte>   against k_decode_batch_singles<byte>
  rans64   FMT_R64 at 14 bits (main64.cpp)         k_decode_batch<r64>    against k_decode_batch_singles<r64>
  word     FMT_WORD at 12 bits (main_simd.cpp)     k_decode_batch<word>   against k_decode_batch_singles<word>
  alias    FMT_ALIAS at 16 bits (main_alias.cpp)   k_decode_batch<alias>  against k_decode_batch_singles<alias>"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_batch_families as T  # noqa: E402  (puts the repository root on sys.path)

OUT = "batch_singles.json"


def _row(fmt, label, short, sb):
    return T.Family("singles", "decode", fmt, label, 1, sb, 64, 1024, ("ragged",), 3, "OPT_BATCH_SINGLES", "k_decode_batch<%s>" % short,
                    "k_decode_batch_singles<%s>" % short, "k_decode_lanes_staged", None, OUT)


ROWS = {
    "byte": _row("FMT_BYTE", "byte", "byte", 14),
    "rans64": _row("FMT_R64", "rans64", "r64", 14),
    "word": _row("FMT_WORD", "word", "word", 12),
    "alias": _row("FMT_ALIAS", "alias", "alias", 16),
}


def combine(records):
    """{format: summarise()'s record} -> the file's content.  Pure (tests/test_bench_batch_singles_cpu.py)."""
    return {"formats": records, "accepted": all(r["accepted"] for r in records.values())}


def draw_counts(symbols, seed):
    """run_family's ragged draw: log-uniform in [0, 64 Ki], as many streams as hold `symbols` symbols."""
    import numpy as np
    rng = np.random.default_rng(seed)
    mean = (T.MAX_LEN + 1) / np.log(T.MAX_LEN + 1.0)
    counts = (np.exp(rng.random(int(symbols / mean * 1.05) + 16) * np.log(T.MAX_LEN + 1.0)) - 1.0).astype(np.uint32)
    return counts[:int(np.searchsorted(np.cumsum(counts.astype(np.int64)), symbols)) + 1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--format", default="all", choices=list(ROWS) + ["all"])
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="default: profiles/" + OUT)
    args = ap.parse_args(argv)

    import torch
    assert torch.cuda.is_available(), "bench_batch_singles.py needs a GPU"
    counts = draw_counts(args.symbols, args.seed)
    run = {"steps": args.steps, "warmup": args.warmup, "passes": args.passes, "device": torch.cuda.get_device_name(0)}
    records = {}
    for name in (ROWS if args.format == "all" else [args.format]):
        row = ROWS[name]
        records[name] = T.summarise(row, run, {"ragged": T.run_batch(row, args, "ragged", counts, True)})
        torch.cuda.empty_cache()
        print("%s: %s" % (name, json.dumps(records[name])), file=sys.stderr, flush=True)
    result = combine(records)
    out = args.out or os.path.join(T.ROOT, "profiles", OUT)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
