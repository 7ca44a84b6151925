#!/usr/bin/env python3
"""Ragged batch decode of the reference's 2-way rans64 layout: one stream per wave against sixty-four streams per wave
(RANS_AMD_OPT_BATCH_LANES), one run on one GPU.  The method is tools/bench_batch_pairs.py's.

rans64 format, 2-way, a 14-bit model, about 1 GiB of symbols (bench.gen_zipf, seed 1), laid out with sym_align = 64, in two
batches:

  ragged   streams whose lengths are drawn log-uniform from [0, 64 Ki] with a fixed seed (181 992 streams: the batch of
           tools/bench_batch_groups.py and tools/bench_batch_pairs.py)
  equal    streams of 512 symbols each (BASELINE config 2's shape)

Per batch, all in this one process:

  wave             Context.decode_batch, option off (k_decode_batch<r64>), streams claimed in index order
  wave_ordered     ... with the order of Context.batch_order (longest bucket first): the yardstick
  lanes            Context.decode_batch on a context with the option on (k_decode_batch_r64_lanes), index order
  lanes_ordered    ... with the order of Context.batch_order: streams of one length bucket share a wave
  uniform          (equal batch only) Context.decode of the same symbols as 512-symbol chunks (k_decode_lanes_r64x2, or its
                   packed-slot form): for information

Every variant is first checked for equality of the decoded symbols, then they are timed with bench.py's own loop
(bench.timed_launches: settle, `--steps` back-to-back launches between HIP events), ALTERNATING: `--passes` passes over
the variants, one timed_launches call per variant and pass.  A variant's ms_mean is the mean over its passes, ms_min the
smallest launch of any pass.  `ordered_gate` says whether the slowest pass of lanes_ordered beats the fastest pass of
wave_ordered.  Written to profiles/batch_r64_lanes.json (or --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_batch(args, torch, np, bench, R, name, counts):
    ways, sb, chunk = 2, 14, 512
    sym_offs, slot_offs = R.batch_layout(counts, R.FMT_R64, ways, 64)
    n_streams, n = counts.size, int(sym_offs[-1])
    ctx_off, ctx_on = R.Context(0), R.Context(0)
    ctx_on.set_option(R.OPT_BATCH_LANES, 1)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx_off.count_freqs_device(d_syms, 256), 1 << sb)
    gm = {ctx_off: ctx_off.model(R.FMT_R64, freqs, sb), ctx_on: ctx_on.model(R.FMT_R64, freqs, sb)}
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
    d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
    cont, offs, lens = ctx_off.encode_batch(gm[ctx_off], d_syms, d_sym, d_counts, ways, d_slot)
    ctx_off.encode_status()
    # (the batch decodes from a compact container, like the uniform run)
    c_cont, c_offs, c_total = ctx_off.compact(cont, int(slot_offs[-1]), offs, lens, n_streams)
    del cont
    d_order = ctx_off.batch_order(d_counts)
    out = torch.empty_like(d_syms)
    # (the padding between streams is never written by a batch decode: compare stream symbols only)
    covered = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    covered.index_add_(0, d_sym[:-1], torch.ones(n_streams, dtype=torch.int32, device="cuda"))
    covered.index_add_(0, d_sym[:-1] + d_counts.to(torch.int64), torch.full((n_streams,), -1, dtype=torch.int32, device="cuda"))
    mask = torch.cumsum(covered[:n], 0) > 0
    del covered

    def ragged(ctx, order):
        return ctx, lambda: ctx.decode_batch(gm[ctx], c_cont, c_total, c_offs, lens, d_sym, d_counts, ways, out, d_order=order, sync=False)

    variants = {
        "wave": ragged(ctx_off, None),
        "wave_ordered": ragged(ctx_off, d_order),
        "lanes": ragged(ctx_on, None),
        "lanes_ordered": ragged(ctx_on, d_order),
    }
    if name == "equal":
        assert n == n_streams * chunk
        u_cont, u_offs, u_lens, u_total = ctx_off.encode(gm[ctx_off], d_syms, ways, chunk)
        variants["uniform"] = (ctx_off, lambda: ctx_off.decode(gm[ctx_off], u_cont, u_total, u_offs, u_lens, n, ways, chunk, d_out=out, sync=False))
    res = {}
    for key, (ctx, fn) in variants.items():
        out.zero_()
        fn()
        torch.cuda.synchronize()
        assert ctx.decode_errors() == 0, key
        assert torch.equal(out, d_syms) if key == "uniform" else torch.equal(out[mask], d_syms[mask]), key
        res[key] = {"kernel": ctx.last_decode_kernel(), "pass_ms_mean": [], "ms_min": None}
        if key == "uniform":
            assert res[key]["kernel"].startswith("k_decode_lanes_r64x2"), res[key]["kernel"]
        else:  # (a time under a name is the time of that kernel)
            assert res[key]["kernel"] == ("k_decode_batch_r64_lanes" if key.startswith("lanes") else "k_decode_batch<r64>"), (key, res[key]["kernel"])
    for _ in range(args.passes):
        for key, (ctx, fn) in variants.items():
            ms, ms_min = bench.timed_launches(torch, fn, args.steps, args.warmup)
            r = res[key]
            r["pass_ms_mean"].append(round(ms, 4))
            r["ms_min"] = round(ms_min if r["ms_min"] is None else min(r["ms_min"], ms_min), 4)
            assert ctx.decode_errors() == 0, key
    for r in res.values():
        r["ms_mean"] = round(sum(r["pass_ms_mean"]) / len(r["pass_ms_mean"]), 4)

    def ratio(a, b):
        return round(res[a]["ms_mean"] / res[b]["ms_mean"], 4)

    result = {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), **res,
              "wave_over_lanes": ratio("wave", "lanes"),
              "wave_ordered_over_lanes_ordered": ratio("wave_ordered", "lanes_ordered"),
              "lanes_over_lanes_ordered": ratio("lanes", "lanes_ordered"),
              "ordered_gate": max(res["lanes_ordered"]["pass_ms_mean"]) < min(res["wave_ordered"]["pass_ms_mean"])}
    if "uniform" in res:
        result["uniform_chunk_syms"] = chunk
        result["lanes_ordered_over_uniform"] = ratio("lanes_ordered", "uniform")
        result["lanes_over_uniform"] = ratio("lanes", "uniform")
    for c in (ctx_on, ctx_off):
        c.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_r64_lanes.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    assert torch.cuda.is_available(), "bench_batch_lanes.py needs a GPU"
    max_len = 65536
    rng = np.random.default_rng(args.seed)
    mean = (max_len + 1) / np.log(max_len + 1.0)  # of the log-uniform draw below
    counts = (np.exp(rng.random(int(args.symbols / mean * 1.05) + 16) * np.log(max_len + 1.0)) - 1.0).astype(np.uint32)
    keep = int(np.searchsorted(np.cumsum(counts.astype(np.int64)), args.symbols)) + 1
    batches = {"ragged": counts[:keep], "equal": np.full(max(64, args.symbols // 512), 512, dtype=np.uint32)}
    result = {"n_ways": 2, "format": "rans64", "scale_bits": 14, "sym_align": 64, "steps": args.steps, "warmup": args.warmup,
              "passes": args.passes, "device": torch.cuda.get_device_name(0)}
    for name, c in batches.items():
        result[name] = run_batch(args, torch, np, bench, R, name, c)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
