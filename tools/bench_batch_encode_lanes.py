#!/usr/bin/env python3
"""Ragged batch ENCODE of the reference's 2-way rans64 layout: one stream per wave against sixty-four streams per wave
(RANS_AMD_OPT_BATCH_ENCODE_LANES), one run on one GPU.  The workloads are tools/bench_batch_lanes.py's, the method
tools/bench_batch_encode_pairs.py's.

rans64 format, 2-way, a 14-bit model, about 1 GiB of symbols (bench.gen_zipf, seed 1), laid out with sym_align = 64, in two
batches:

  ragged   streams whose lengths are drawn log-uniform from [0, 64 Ki] with a fixed seed (181 992 streams)
  equal    streams of 512 symbols each (2 Mi streams: BASELINE config 2's shape)

Per batch, all in this one process, into one container and one index:

  wave             Context.encode_batch, option off (k_encode_batch<r64>), streams claimed in index order
  wave_ordered     ... with the order of Context.batch_order (longest bucket first): the yardstick
  lanes            Context.encode_batch on a context with the option on (k_encode_batch_r64_lanes), index order
  lanes_ordered    ... with the same order: streams of one length bucket share a wave
  uniform          (equal batch only) Context.encode_slots of the same symbols as 512-symbol chunks (k_encode_lanes_r64x2): for
                   information

Every ragged variant is first checked for equality with `wave` (offsets, lengths, every stream byte; each stream ends at its
slot's end) and the uniform one is decoded back, then they are timed with bench.py's own loop (bench.timed_launches: settle,
`--steps` back-to-back launches between HIP events), ALTERNATING: `--passes` passes over the variants, one timed_launches
call per variant and pass, so that no variant has a stretch of the run to itself.  A variant's ms_mean is the mean over its
passes, ms_min the smallest launch of any pass.  `ordered_gate` says whether the slowest pass of lanes_ordered beats the
fastest pass of wave_ordered; the top-level `accepted` is the gate of both batches.  Written to
profiles/batch_encode_r64_lanes.json (or --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_batch(args, torch, np, bench, R, name, counts):
    ways, sb, chunk = 2, 14, 512
    sym_offs, slot_offs = R.batch_layout(counts, R.FMT_R64, ways, 64)
    n_streams, n, cap = counts.size, int(sym_offs[-1]), int(slot_offs[-1])
    ctx_off, ctx_on = R.Context(0), R.Context(0)
    ctx_on.set_option(R.OPT_BATCH_ENCODE_LANES, 1)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx_off.count_freqs_device(d_syms, 256), 1 << sb)
    gm = {ctx_off: ctx_off.model(R.FMT_R64, freqs, sb), ctx_on: ctx_on.model(R.FMT_R64, freqs, sb)}
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
    d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
    d_order = ctx_off.batch_order(d_counts)
    # one container, one index for every ragged variant (each launch writes all of it)
    cont = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
    lens = torch.zeros(n_streams, dtype=torch.int32, device="cuda")

    def ragged(ctx, order):
        return ctx, lambda: ctx.encode_batch(gm[ctx], d_syms, d_sym, d_counts, ways, d_slot, d_out=cont, d_offsets=offs, d_lengths=lens,
                                             out_cap=cap, d_order=order)

    variants = {
        "wave": ragged(ctx_off, None),
        "wave_ordered": ragged(ctx_off, d_order),
        "lanes": ragged(ctx_on, None),
        "lanes_ordered": ragged(ctx_on, d_order),
    }
    if name == "equal":
        assert n == n_streams * chunk
        u_chunks = R.num_chunks(n, chunk)
        u_total = R.encode_slots_bound(R.FMT_R64, n, ways, chunk)
        u_cont = torch.empty(u_total, dtype=torch.uint8, device="cuda")
        u_offs = torch.zeros(u_chunks + 1, dtype=torch.int64, device="cuda")
        u_lens = torch.zeros(u_chunks, dtype=torch.int32, device="cuda")
        variants["uniform"] = (ctx_off, lambda: ctx_off.encode_slots(gm[ctx_off], d_syms, ways, chunk, d_out=u_cont, sync=False,
                                                                     d_offsets=u_offs, d_lengths=u_lens))
    res = {}
    want = gaps = None
    for key, (ctx, fn) in variants.items():
        if key != "uniform":
            cont.zero_(); offs.zero_(); lens.zero_()
        fn()
        torch.cuda.synchronize()
        ctx.encode_status()
        if key == "wave":  # the bytes of the streams: what lies between them is whatever a 16-byte flush left there
            d = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")
            d.index_add_(0, offs, torch.ones(n_streams, dtype=torch.int32, device="cuda"))
            d.index_add_(0, offs + lens.to(torch.int64), torch.full((n_streams,), -1, dtype=torch.int32, device="cuda"))
            gaps = torch.cumsum(d[:cap], 0) <= 0
            del d
            want = (cont.masked_fill(gaps, 0), offs.clone(), lens.clone())
            assert torch.equal(offs + lens.to(torch.int64), d_slot[1:]), "a stream does not end at its slot's end"
        elif key == "uniform":
            back = ctx_off.decode(gm[ctx_off], u_cont, u_total, u_offs, u_lens, n, ways, chunk)
            assert ctx_off.decode_errors() == 0 and torch.equal(back, d_syms), key
            del back
        else:
            assert torch.equal(offs, want[1]) and torch.equal(lens, want[2]) and torch.equal(cont.masked_fill(gaps, 0), want[0]), key
        res[key] = {"kernel": ctx.last_encode_kernel()[0], "pass_ms_mean": [], "ms_min": None}
        if key == "uniform":
            assert res[key]["kernel"] == "k_encode_lanes_r64x2", res[key]["kernel"]
        else:  # (a time under a name is the time of that kernel)
            assert res[key]["kernel"] == ("k_encode_batch_r64_lanes" if key.startswith("lanes") else "k_encode_batch<r64>"), (key, res[key]["kernel"])
    del want, gaps
    for k in range(args.passes):
        print("%s: pass %d of %d" % (name, k + 1, args.passes), file=sys.stderr, flush=True)
        for key, (ctx, fn) in variants.items():
            ms, ms_min = bench.timed_launches(torch, fn, args.steps, args.warmup)
            r = res[key]
            r["pass_ms_mean"].append(round(ms, 4))
            r["ms_min"] = round(ms_min if r["ms_min"] is None else min(r["ms_min"], ms_min), 4)
            ctx.encode_status()
    for r in res.values():
        r["ms_mean"] = round(sum(r["pass_ms_mean"]) / len(r["pass_ms_mean"]), 4)

    def ratio(a, b):
        return round(res[a]["ms_mean"] / res[b]["ms_mean"], 4)

    result = {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), **res,
              "wave_over_lanes": ratio("wave", "lanes"),
              "wave_ordered_over_lanes_ordered": ratio("wave_ordered", "lanes_ordered"),
              "lanes_over_lanes_ordered": ratio("lanes", "lanes_ordered"),
              # the condition: the wave kernel's fastest pass with d_order is still slower than the lane kernel's slowest
              "wave_ordered_fastest_pass_ms": min(res["wave_ordered"]["pass_ms_mean"]),
              "lanes_ordered_slowest_pass_ms": max(res["lanes_ordered"]["pass_ms_mean"]),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_encode_r64_lanes.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    assert torch.cuda.is_available(), "bench_batch_encode_lanes.py needs a GPU"
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
    result["accepted"] = all(result[name]["ordered_gate"] for name in batches)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
