#!/usr/bin/env python3
"""Ragged batch decode against uniform decode of the same symbols, one run on one GPU.

Word format, 64-way, about 1 GiB of symbols (bench.gen_zipf, seed 1) cut into streams whose lengths are drawn log-uniform
from [0, 64 Ki] with a fixed seed.  Three decodes of those symbols are timed with bench.py's own loop (bench.timed_launches:
settle, `--steps` back-to-back launches between HIP events):

  ragged           Context.decode_batch, streams claimed in index order
  ragged_ordered   Context.decode_batch with the order of Context.batch_order (longest bucket first)
  uniform          Context.decode of the same symbols in chunks of the batch's mean length rounded to a multiple of 64

and written with the two ratios uniform / ragged to profiles/batch_ragged.json (or --out)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_ragged.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    assert torch.cuda.is_available(), "bench_batch.py needs a GPU"
    ways, max_len = 64, 65536
    rng = np.random.default_rng(args.seed)
    mean = (max_len + 1) / np.log(max_len + 1.0)  # of the log-uniform draw below
    counts = (np.exp(rng.random(int(args.symbols / mean * 1.05) + 16) * np.log(max_len + 1.0)) - 1.0).astype(np.uint32)
    keep = int(np.searchsorted(np.cumsum(counts.astype(np.int64)), args.symbols)) + 1
    counts = counts[:keep]
    sym_offs, slot_offs = R.batch_layout(counts, R.FMT_WORD, ways, 4)
    n_streams, n = counts.size, int(sym_offs[-1])

    ctx = R.Context(0)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx.count_freqs_device(d_syms, 256), 4096)
    gm = ctx.model(R.FMT_WORD, freqs, 12)
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
    d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
    cont, offs, lens = ctx.encode_batch(gm, d_syms, d_sym, d_counts, ways, d_slot)
    ctx.encode_status()
    # (the batch decodes from a compact container, like the uniform run)
    c_cont, c_offs, c_total = ctx.compact(cont, int(slot_offs[-1]), offs, lens, n_streams)
    del cont
    d_order = ctx.batch_order(d_counts)
    out = torch.empty_like(d_syms)

    def ragged(order):
        return lambda: ctx.decode_batch(gm, c_cont, c_total, c_offs, lens, d_sym, d_counts, ways, out, d_order=order, sync=False)

    res = {}
    for key, fn in (("ragged", ragged(None)), ("ragged_ordered", ragged(d_order))):
        out.zero_()
        fn()
        # (the padding between streams is never written: compare stream symbols only)
        covered = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        covered.index_add_(0, d_sym[:-1], torch.ones(n_streams, dtype=torch.int32, device="cuda"))
        covered.index_add_(0, d_sym[:-1] + d_counts.to(torch.int64), torch.full((n_streams,), -1, dtype=torch.int32, device="cuda"))
        mask = torch.cumsum(covered[:n], 0) > 0
        assert ctx.decode_errors() == 0 and torch.equal(out[mask], d_syms[mask]), key
        ms, ms_min = bench.timed_launches(torch, fn, args.steps, args.warmup)
        res[key] = {"kernel": ctx.last_decode_kernel(), "ms_mean": round(ms, 4), "ms_min": round(ms_min, 4)}
    del c_cont

    chunk = max(64, int(round(counts.mean() / 64.0)) * 64)
    u_cont, u_offs, u_lens, u_total = ctx.encode(gm, d_syms, ways, chunk)
    out.zero_()
    ctx.decode(gm, u_cont, u_total, u_offs, u_lens, n, ways, chunk, d_out=out)
    assert torch.equal(out, d_syms)
    ms, ms_min = bench.timed_launches(
        torch, lambda: ctx.decode(gm, u_cont, u_total, u_offs, u_lens, n, ways, chunk, d_out=out, sync=False), args.steps, args.warmup)
    res["uniform"] = {"kernel": ctx.last_decode_kernel(), "ms_mean": round(ms, 4), "ms_min": round(ms_min, 4), "chunk_syms": chunk}
    assert ctx.decode_errors() == 0

    result = {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), "n_ways": ways, "format": "word",
              "sym_align": 4, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), **res,
              "uniform_over_ragged": round(res["uniform"]["ms_mean"] / res["ragged"]["ms_mean"], 4),
              "uniform_over_ragged_ordered": round(res["uniform"]["ms_mean"] / res["ragged_ordered"]["ms_mean"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
