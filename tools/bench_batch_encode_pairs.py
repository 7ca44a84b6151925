#!/usr/bin/env python3
"""Ragged batch ENCODE of the reference's 2-way byte layout: one stream per wave against thirty-two streams per wave
(RANS_AMD_OPT_BATCH_ENCODE_PAIRS), with and without a hand-out order, one run on one GPU.  The method is
tools/bench_batch_encode_groups.py's, the workload tools/bench_batch_pairs.py's.

Byte format, 2-way, a 14-bit model, about 1 GiB of symbols (bench.gen_zipf, seed 1) cut into streams whose lengths are drawn
log-uniform from [0, 64 Ki] with a fixed seed, laid out with sym_align = 4.  Five encodes of those symbols, all in this one
process:

  wave             Context.encode_batch, option off (k_encode_batch<byte>), streams claimed in index order
  wave_ordered     ... with the order of Context.batch_order (longest bucket first): the yardstick
  pairs            Context.encode_batch on a context with the option on (k_encode_batch_byte_pairs), index order
  pairs_ordered    ... with the order of Context.batch_order: streams of one length bucket share a wave
  uniform          Context.encode_slots of the same symbols in 1024-symbol chunks

Every ragged variant is first checked for equality with `wave` (offsets, lengths, every stream byte) and the uniform one is
decoded back, then they are timed with bench.py's own loop (bench.timed_launches: settle, `--steps` back-to-back launches
between HIP events), ALTERNATING: `--passes` passes over the five variants, one timed_launches call per variant and pass, so
that no variant has a stretch of the run to itself.  A variant's ms_mean is the mean over its passes, ms_min the smallest
launch of any pass.  Written with the ratios wave / pairs (above 1: the pair kernel is faster) and the acceptance test --
the wave kernel's fastest pass with d_order against the pair kernel's slowest -- to profiles/batch_encode_pairs.json (or
--out)."""
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
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_encode_pairs.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    assert torch.cuda.is_available(), "bench_batch_encode_pairs.py needs a GPU"
    ways, max_len, chunk, sb = 2, 65536, 1024, 14
    rng = np.random.default_rng(args.seed)
    mean = (max_len + 1) / np.log(max_len + 1.0)  # of the log-uniform draw below
    counts = (np.exp(rng.random(int(args.symbols / mean * 1.05) + 16) * np.log(max_len + 1.0)) - 1.0).astype(np.uint32)
    keep = int(np.searchsorted(np.cumsum(counts.astype(np.int64)), args.symbols)) + 1
    counts = counts[:keep]
    sym_offs, slot_offs = R.batch_layout(counts, R.FMT_BYTE, ways, 4)
    n_streams, n, cap = counts.size, int(sym_offs[-1]), int(slot_offs[-1])

    ctx_off, ctx_on = R.Context(0), R.Context(0)
    ctx_on.set_option(R.OPT_BATCH_ENCODE_PAIRS, 1)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx_off.count_freqs_device(d_syms, 256), 1 << sb)
    gm = {ctx_off: ctx_off.model(R.FMT_BYTE, freqs, sb), ctx_on: ctx_on.model(R.FMT_BYTE, freqs, sb)}
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

    u_chunks = R.num_chunks(n, chunk)
    u_total = R.encode_slots_bound(R.FMT_BYTE, n, ways, chunk)
    u_cont = torch.empty(u_total, dtype=torch.uint8, device="cuda")
    u_offs = torch.zeros(u_chunks + 1, dtype=torch.int64, device="cuda")
    u_lens = torch.zeros(u_chunks, dtype=torch.int32, device="cuda")

    def uniform():
        ctx_off.encode_slots(gm[ctx_off], d_syms, ways, chunk, d_out=u_cont, sync=False, d_offsets=u_offs, d_lengths=u_lens)

    variants = {
        "wave": ragged(ctx_off, None),
        "wave_ordered": ragged(ctx_off, d_order),
        "pairs": ragged(ctx_on, None),
        "pairs_ordered": ragged(ctx_on, d_order),
        "uniform": (ctx_off, uniform),
    }
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
        if key != "uniform":  # (a time under a name is the time of that kernel)
            assert res[key]["kernel"] == ("k_encode_batch_byte_pairs" if key.startswith("pairs") else "k_encode_batch<byte>"), (key, res[key]["kernel"])
    del want, gaps
    for _ in range(args.passes):
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

    result = {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), "n_ways": ways, "format": "byte", "scale_bits": sb,
              "sym_align": 4, "steps": args.steps, "warmup": args.warmup, "passes": args.passes, "uniform_chunk_syms": chunk,
              "device": torch.cuda.get_device_name(0), **res,
              "wave_over_pairs": ratio("wave", "pairs"),
              "wave_ordered_over_pairs_ordered": ratio("wave_ordered", "pairs_ordered"),
              "wave_over_wave_ordered": ratio("wave", "wave_ordered"),
              "pairs_over_pairs_ordered": ratio("pairs", "pairs_ordered"),
              "pairs_ordered_over_uniform": ratio("pairs_ordered", "uniform"),
              # accepted: the wave kernel's fastest pass with d_order is still slower than the pair kernel's slowest
              "wave_ordered_fastest_pass_ms": min(res["wave_ordered"]["pass_ms_mean"]),
              "pairs_ordered_slowest_pass_ms": max(res["pairs_ordered"]["pass_ms_mean"]),
              "accepted": min(res["wave_ordered"]["pass_ms_mean"]) > max(res["pairs_ordered"]["pass_ms_mean"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
