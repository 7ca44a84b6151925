#!/usr/bin/env python3
"""Ragged batch ENCODE of the reference's 2-way alias layout (main_alias.cpp, 16 bits): one stream per wave against thirty-two
streams per wave (RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS), one run on one GPU.

    python tools/bench_batch_encode_alias_pairs.py [--row encode_alias_pairs|encode_alias_pairs_12bit|encode_byte_pairs_16bit]

The method is tools/bench_batch_families.py's run_family -- workload (181 992 log-uniform streams, about 1 GiB of symbols),
verification of every variant and of the kernel it reports, alternating passes, summarise() and its `accepted` gate: the slowest
pass of <variant>_ordered beats the fastest pass of wave_ordered, in the same run.  This file adds the rows only (that module's
FAMILIES is the six families of tests/_kernel_rows.py):

  encode_alias_pairs        FMT_ALIAS at 16 bits, the reference's prob_bits: k_encode_batch<alias, LDS remap> against
                            k_encode_batch_alias_pairs (128 KiB of remap16 in LDS: one block of 13 waves per CU), the uniform
                            encode of the same symbols in 1024-symbol chunks beside them -> profiles/batch_encode_alias_pairs.json
  encode_alias_pairs_12bit  the same at 12 bits, where two blocks of 16 waves share a CU: what the 16-bit occupancy costs
                            -> profiles/batch_encode_alias_pairs_12bit.json
  encode_byte_pairs_16bit   the byte pair ENCODER's row at 16 bits instead of its 14, on the same counts: what the put's extra
                            gather and the block shape cost together -> profiles/batch_encode_alias_pairs_byte16.json"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bench_batch_families as T  # noqa: E402  (puts the repository root on sys.path)

_ALIAS = T.Family("alias_pairs", "encode", "FMT_ALIAS", "alias", 2, 16, 4, 1024, ("ragged",), 3, "OPT_BATCH_ENCODE_ALIAS_PAIRS",
                  "k_encode_batch<alias, LDS remap>", "k_encode_batch_alias_pairs", "k_encode_lanes_staged", (6, "k_encode_lanes16"),
                  "batch_encode_alias_pairs.json")
ROWS = {
    "encode_alias_pairs": _ALIAS,
    "encode_alias_pairs_12bit": _ALIAS._replace(scale_bits=12, out="batch_encode_alias_pairs_12bit.json"),
    "encode_byte_pairs_16bit": T.FAMILIES["encode_pairs"]._replace(scale_bits=16, out="batch_encode_alias_pairs_byte16.json"),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--row", default="encode_alias_pairs", choices=list(ROWS))
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, help="default: the row's (3)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="default: the row's file under profiles/")
    args = ap.parse_args(argv)

    import torch
    assert torch.cuda.is_available(), "bench_batch_encode_alias_pairs.py needs a GPU"
    row = ROWS[args.row]
    args.passes = args.passes or row.passes
    return T.run_family(row, args, args.out or os.path.join(T.ROOT, "profiles", row.out))


if __name__ == "__main__":
    main()
