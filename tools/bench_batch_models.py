#!/usr/bin/env python3
"""Ragged batches with one model per stream against the uniform per-chunk-model calls on the same symbols, one run on one GPU.

Word format, 64-way, about 1 GiB of symbols (bench.gen_zipf, seed 1) cut into streams whose lengths are drawn log-uniform
from [0, 64 Ki] with a fixed seed, sym_align = 4.  Timed with bench.py's own loop (bench.timed_launches: settle, `--steps`
back-to-back launches between HIP events):

  encode_ragged           Context.encode_batch_adaptive
  encode_uniform          Context.encode_adaptive_sized in chunks of the batch's mean length rounded to a multiple of 64 (no
                          register-resident size: the two-pass form, the one a ragged stream takes)
  decode_ragged           Context.decode_batch_adaptive, streams claimed in index order
  decode_ragged_ordered   ... with the order of Context.batch_order (longest bucket first)
  decode_uniform          Context.decode_adaptive of the uniform container

and written with the ratios uniform / ragged to profiles/batch_models.json (or --out).  No ratio is demanded anywhere: the
file is the record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_models.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    assert torch.cuda.is_available(), "bench_batch_models.py needs a GPU"
    ways, max_len, sb, fmt = 64, 65536, 12, R.FMT_WORD
    rng = np.random.default_rng(args.seed)
    mean = (max_len + 1) / np.log(max_len + 1.0)  # of the log-uniform draw below
    counts = (np.exp(rng.random(int(args.symbols / mean * 1.05) + 16) * np.log(max_len + 1.0)) - 1.0).astype(np.uint32)
    keep = int(np.searchsorted(np.cumsum(counts.astype(np.int64)), args.symbols)) + 1
    counts = counts[:keep]
    sym_offs, _ = R.batch_layout(counts, fmt, ways, 4)
    n_streams, n = counts.size, int(sym_offs[-1])

    ctx = R.Context(0)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
    covered = torch.zeros(n + 1, dtype=torch.int32, device="cuda")  # (the padding between streams is never written)
    covered.index_add_(0, d_sym[:-1], torch.ones(n_streams, dtype=torch.int32, device="cuda"))
    covered.index_add_(0, d_sym[:-1] + d_counts.to(torch.int64), torch.full((n_streams,), -1, dtype=torch.int32, device="cuda"))
    mask = torch.cumsum(covered[:n], 0) > 0
    del covered
    res = {}

    def record(key, fn, kernel, **more):
        ms, ms_min = bench.timed_launches(torch, fn, args.steps, args.warmup)
        res[key] = {"kernel": kernel(), "ms_mean": round(ms, 4), "ms_min": round(ms_min, 4), **more}

    # ---- ragged
    cont, offs, lens, rows, total = ctx.encode_batch_adaptive(d_syms, d_sym, d_counts, ways, sb, fmt=fmt)
    record("encode_ragged",
           lambda: ctx.encode_batch_adaptive(d_syms, d_sym, d_counts, ways, sb, fmt=fmt, d_out=cont, sync=False, d_offsets=offs,
                                             d_lengths=lens, d_freqs=rows),
           lambda: ctx.last_encode_kernel()[0], container_bytes=total)
    ctx.encode_status()
    d_order = ctx.batch_order(d_counts)
    out = torch.empty_like(d_syms)
    for key, order in (("decode_ragged", None), ("decode_ragged_ordered", d_order)):
        def fn(order=order):
            return ctx.decode_batch_adaptive(cont, total, offs, lens, rows, d_sym, d_counts, ways, sb, out, fmt=fmt, d_order=order,
                                             sync=False)
        out.zero_()
        fn()
        assert ctx.decode_errors() == 0 and torch.equal(out[mask], d_syms[mask]), key
        record(key, fn, ctx.last_decode_kernel)
    del cont, mask

    # ---- uniform, at the batch's mean length
    chunk = max(64, int(round(counts.mean() / 64.0)) * 64)
    assert chunk not in (4096, 8192, 16384)
    u_cont, u_offs, u_lens, u_rows, u_total = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt)
    record("encode_uniform",
           lambda: ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt, d_out=u_cont, sync=False, d_offsets=u_offs,
                                             d_lengths=u_lens, d_freqs=u_rows),
           lambda: ctx.last_encode_kernel()[0], container_bytes=u_total, chunk_syms=chunk)
    ctx.encode_status()
    out.zero_()
    ctx.decode_adaptive(u_cont, u_total, u_offs, u_lens, u_rows, n, ways, chunk, sb, d_out=out, fmt=fmt)
    assert torch.equal(out, d_syms)
    record("decode_uniform",
           lambda: ctx.decode_adaptive(u_cont, u_total, u_offs, u_lens, u_rows, n, ways, chunk, sb, d_out=out, sync=False, fmt=fmt),
           ctx.last_decode_kernel, chunk_syms=chunk)
    assert ctx.decode_errors() == 0

    def ratio(a, b):
        return round(res[a]["ms_mean"] / res[b]["ms_mean"], 4)
    result = {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), "n_ways": ways, "format": "word",
              "scale_bits": sb, "sym_align": 4, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), **res,
              "encode_uniform_over_ragged": ratio("encode_uniform", "encode_ragged"),
              "decode_uniform_over_ragged": ratio("decode_uniform", "decode_ragged"),
              "decode_uniform_over_ragged_ordered": ratio("decode_uniform", "decode_ragged_ordered")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
