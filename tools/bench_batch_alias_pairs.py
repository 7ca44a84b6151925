#!/usr/bin/env python3
"""Ragged batch DECODE of the reference's 2-way alias layout (main_alias.cpp, 16 bits): one stream per wave against thirty-two
streams per wave (RANS_AMD_OPT_BATCH_ALIAS_PAIRS), one run on one GPU.

    python tools/bench_batch_alias_pairs.py [--row alias_pairs|byte_pairs_16bit]

The method is tools/bench_batch_families.py's run_family -- workload (181 992 log-uniform streams, about 1 GiB of symbols),
verification of every variant and of the kernel it reports, alternating passes, summarise() and its `accepted` gate: the slowest
pass of <variant>_ordered beats the fastest pass of wave_ordered.  This file adds the rows only (that module's FAMILIES is the
six families of tests/_kernel_rows.py):

  alias_pairs        FMT_ALIAS at 16 bits: k_decode_batch<alias> against k_decode_batch_alias_pairs, the uniform decode of the
                     same symbols in 1024-symbol chunks on k_decode_lanes_staged -> profiles/batch_alias_pairs.json
  byte_pairs_16bit   the byte pairs' row at 16 bits instead of its 14 (64 KiB of cum2sym: one block per CU), for the comparison
                     that is the reason the alias layout exists: small tables at 16 bits
                     -> profiles/batch_alias_pairs_byte16.json"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_batch_families as T  # noqa: E402  (puts the repository root on sys.path)

ROWS = {
    "alias_pairs": T.Family("alias_pairs", "decode", "FMT_ALIAS", "alias", 2, 16, 4, 1024, ("ragged",), 3, "OPT_BATCH_ALIAS_PAIRS",
                            "k_decode_batch<alias>", "k_decode_batch_alias_pairs", "k_decode_lanes_staged", None, "batch_alias_pairs.json"),
    "byte_pairs_16bit": T.FAMILIES["pairs"]._replace(scale_bits=16, out="batch_alias_pairs_byte16.json"),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--row", default="alias_pairs", choices=list(ROWS))
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, help="default: the row's (3)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="default: the row's file under profiles/")
    args = ap.parse_args(argv)

    import torch
    assert torch.cuda.is_available(), "bench_batch_alias_pairs.py needs a GPU"
    row = ROWS[args.row]
    args.passes = args.passes or row.passes
    return T.run_family(row, args, args.out or os.path.join(T.ROOT, "profiles", row.out))


if __name__ == "__main__":
    main()
