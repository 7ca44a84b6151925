#!/usr/bin/env python3
"""Ragged batches: one stream per wave against the streams-per-wave kernel of a family, one run on one GPU.

    python tools/bench_batch_families.py --family groups|encode_groups|pairs|encode_pairs|lanes|encode_lanes|all

One row of FAMILIES per family (the kBatchFamilies of ryg_rans_amd/csrc/launchers.hpp, the descriptors of tests/_kernel_rows.py):
what the six runs differ in.  Everything else is one method.

The workload: about 1 GiB of symbols (bench.gen_zipf, seed 1) under a model of the row's scale_bits, laid out with the row's
sym_align, in the row's batches:

  ragged   streams whose lengths are drawn log-uniform from [0, 64 Ki] with a fixed seed (181 992 streams)
  equal    streams of one uniform chunk each (the lane families: 2 Mi streams of 512 symbols, BASELINE config 2's shape)

Per batch, all in this one process (<v> is the row's variant: groups, pairs or lanes):

  wave           Context.decode_batch / encode_batch, option off (the wave kernel), streams claimed in index order
  wave_ordered   ... with the order of Context.batch_order (longest bucket first): the yardstick
  <v>            the same call on a context with the row's option on (the family's kernel), index order
  <v>_ordered    ... with the order of Context.batch_order: streams of one length bucket share a wave
  uniform        (the row's last batch only) Context.decode / encode_slots of the same symbols in uniform chunks: the floor

Every variant is first verified -- a decoder: the decoded symbols of every stream and decode_errors() == 0; an encoder:
offsets, lengths and every stream byte equal to `wave`, each stream ending at its slot's end, the uniform one decoded back --
and must report the kernel the row names (a time under a name is the time of that kernel).  Then they are timed with bench.py's
own loop (bench.timed_launches: settle, `--steps` back-to-back launches between HIP events), ALTERNATING: `--passes` passes
over the variants, one timed_launches call per variant and pass, so that no variant has a stretch of the run to itself.
summarise() turns the passes into the record: a variant's ms_mean is the mean over its passes, ms_min the smallest launch of any
pass; the ratios a_over_b are ms_mean(a) / ms_mean(b) (wave over <v> above 1: the family's kernel is faster); `ordered_gate`
says whether the slowest pass of <v>_ordered beats the fastest pass of wave_ordered, `accepted` is the gate of every batch.
Written to the row's file under profiles/ (or --out; with --family all, --out names a directory)."""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# fmt / option: attributes of ryg_rans_amd; label: the record's "format"; chunk: the uniform chunk size (and the equal batch's
# stream length); wave / family / uniform: the kernels the variants must report; uniform_below: (batches of 64 chunks per CU,
# kernel) -- with fewer batches the library's uniform encoder is that one (encode_lanes.hip: the staged lane encoders start at
# six batches per CU, the 2-way rans64 one at one WHOLE batch per CU); out: the default file under profiles/
Family = collections.namedtuple("Family", "variant side fmt label ways scale_bits sym_align chunk batches passes option wave family uniform "
                                "uniform_below out")
FAMILIES = {
    "groups": Family("groups", "decode", "FMT_WORD", "word", 8, 12, 4, 1024, ("ragged",), 3, "OPT_BATCH_GROUPS",
                     "k_decode_batch<word>", "k_decode_batch_word_groups", "k_decode_word_groups", None, "batch_groups.json"),
    "encode_groups": Family("groups", "encode", "FMT_WORD", "word", 8, 12, 4, 1024, ("ragged",), 3, "OPT_BATCH_ENCODE_GROUPS",
                            "k_encode_batch<word>", "k_encode_batch_word_groups", "k_encode_word_groups", None, "batch_encode_groups.json"),
    "pairs": Family("pairs", "decode", "FMT_BYTE", "byte", 2, 14, 4, 1024, ("ragged",), 3, "OPT_BATCH_PAIRS",
                    "k_decode_batch<byte>", "k_decode_batch_byte_pairs", "k_decode_byte_pairs", None, "batch_pairs.json"),
    "encode_pairs": Family("pairs", "encode", "FMT_BYTE", "byte", 2, 14, 4, 1024, ("ragged",), 3, "OPT_BATCH_ENCODE_PAIRS",
                           "k_encode_batch<byte>", "k_encode_batch_byte_pairs", "k_encode_lanes_staged", (6, "k_encode_lanes16"),
                           "batch_encode_pairs.json"),
    "lanes": Family("lanes", "decode", "FMT_R64", "rans64", 2, 14, 64, 512, ("ragged", "equal"), 5, "OPT_BATCH_LANES",
                    "k_decode_batch<r64>", "k_decode_batch_r64_lanes", "k_decode_lanes_r64x2<packed slots>", None, "batch_r64_lanes.json"),
    "encode_lanes": Family("lanes", "encode", "FMT_R64", "rans64", 2, 14, 64, 512, ("ragged", "equal"), 5, "OPT_BATCH_ENCODE_LANES",
                           "k_encode_batch<r64>", "k_encode_batch_r64_lanes", "k_encode_lanes_r64x2", (1, "k_encode_lanes16"),
                           "batch_encode_r64_lanes.json"),
}
MAX_LEN = 65536


def variant_names(row, with_uniform):
    v = row.variant
    return ("wave", "wave_ordered", v, v + "_ordered") + (("uniform",) if with_uniform else ())


def expected_kernel(row, key, chunks=0, num_cus=0):
    """The kernel variant `key` must report; the uniform one for `chunks` uniform chunks on `num_cus` CUs."""
    if key != "uniform":
        return row.family if key.startswith(row.variant) else row.wave
    if row.uniform_below:
        batches = chunks // 64 if row.fmt == "FMT_R64" else (chunks + 63) // 64
        if batches < row.uniform_below[0] * num_cus:
            return row.uniform_below[1]
    return row.uniform


def summarise(row, run, batches):
    """The record of one run.  run: steps, warmup, passes, device.  batches: {name: {symbols, streams, mean_stream_syms, and per
    variant {kernel, pass_ms_mean, ms_min}}}, the row's batches in order.  A row with the ragged batch alone gives a flat
    record, the others one dict per batch.  Pure: no torch, no GPU (tests/test_bench_batch_families_cpu.py recomputes the
    committed records with it)."""
    v = row.variant
    out = {"n_ways": row.ways, "format": row.label, "scale_bits": row.scale_bits, "sym_align": row.sym_align, "steps": run["steps"],
           "warmup": run["warmup"], "passes": run["passes"], "device": run["device"]}
    done = {}
    for name, b in batches.items():
        keys = variant_names(row, "uniform" in b)
        res = {k: dict(b[k], ms_mean=round(sum(b[k]["pass_ms_mean"]) / len(b[k]["pass_ms_mean"]), 4)) for k in keys}

        def ratio(a, c):
            return round(res[a]["ms_mean"] / res[c]["ms_mean"], 4)

        r = {"symbols": b["symbols"], "streams": b["streams"], "mean_stream_syms": b["mean_stream_syms"], **res,
             "wave_over_" + v: ratio("wave", v),
             "wave_ordered_over_%s_ordered" % v: ratio("wave_ordered", v + "_ordered"),
             "wave_over_wave_ordered": ratio("wave", "wave_ordered"),
             "%s_over_%s_ordered" % (v, v): ratio(v, v + "_ordered"),
             # the condition: the wave kernel's fastest pass with d_order is still slower than the family's slowest
             "wave_ordered_fastest_pass_ms": min(res["wave_ordered"]["pass_ms_mean"]),
             v + "_ordered_slowest_pass_ms": max(res[v + "_ordered"]["pass_ms_mean"])}
        r["ordered_gate"] = r[v + "_ordered_slowest_pass_ms"] < r["wave_ordered_fastest_pass_ms"]
        if "uniform" in res:
            r["uniform_chunk_syms"] = row.chunk
            r[v + "_ordered_over_uniform"] = ratio(v + "_ordered", "uniform")
            r[v + "_over_uniform"] = ratio(v, "uniform")
        done[name] = r
    out.update(done["ragged"] if tuple(batches) == ("ragged",) else done)
    out["accepted"] = all(r["ordered_gate"] for r in done.values())
    return out


def run_batch(row, args, name, counts, with_uniform):
    """Verify, then time, every variant of one batch -> the batch's entry for summarise()."""
    import numpy as np
    import torch

    import bench
    import ryg_rans_amd as R

    fmt, ways, sb, chunk, decode = getattr(R, row.fmt), row.ways, row.scale_bits, row.chunk, row.side == "decode"
    sym_offs, slot_offs = R.batch_layout(counts, fmt, ways, row.sym_align)
    n_streams, n, cap = counts.size, int(sym_offs[-1]), int(slot_offs[-1])
    ctx_off, ctx_on = R.Context(0), R.Context(0)
    ctx_on.set_option(getattr(R, row.option), 1)
    d_syms = bench.gen_zipf(torch, n, 256, 1.0, 1, "cuda")
    freqs, _ = R.normalize_freqs(ctx_off.count_freqs_device(d_syms, 256), 1 << sb)
    gm = {ctx_off: ctx_off.model(fmt, freqs, sb), ctx_on: ctx_on.model(fmt, freqs, sb)}
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_sym = torch.from_numpy(sym_offs.astype(np.int64)).cuda()
    d_slot = torch.from_numpy(slot_offs.astype(np.int64)).cuda()
    d_order = ctx_off.batch_order(d_counts)
    assert not with_uniform or name == "ragged" or n == n_streams * chunk

    def covered(starts, lengths, size):
        """size booleans: the bytes inside [start, start + length) of any stream"""
        d = torch.zeros(size + 1, dtype=torch.int32, device="cuda")
        d.index_add_(0, starts, torch.ones(n_streams, dtype=torch.int32, device="cuda"))
        d.index_add_(0, starts + lengths.to(torch.int64), torch.full((n_streams,), -1, dtype=torch.int32, device="cuda"))
        return torch.cumsum(d[:size], 0) > 0

    want = {}  # an encoder's yardstick: what `wave` wrote
    if decode:
        cont, offs, lens = ctx_off.encode_batch(gm[ctx_off], d_syms, d_sym, d_counts, ways, d_slot)
        ctx_off.encode_status()
        # (the batch decodes from a compact container, like the uniform run)
        c_cont, c_offs, c_total = ctx_off.compact(cont, cap, offs, lens, n_streams)
        del cont
        out = torch.empty_like(d_syms)
        # (the padding between streams is never written by a batch decode: compare stream symbols only)
        mask = covered(d_sym[:-1], d_counts, n)
        if with_uniform:
            u_cont, u_offs, u_lens, u_total = ctx_off.encode(gm[ctx_off], d_syms, ways, chunk)

        def ragged(ctx, order):
            return ctx, lambda: ctx.decode_batch(gm[ctx], c_cont, c_total, c_offs, lens, d_sym, d_counts, ways, out, d_order=order, sync=False)

        def uniform():
            ctx_off.decode(gm[ctx_off], u_cont, u_total, u_offs, u_lens, n, ways, chunk, d_out=out, sync=False)

        def verify(key, ctx, fn):
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert ctx.decode_errors() == 0, key
            assert torch.equal(out, d_syms) if key == "uniform" else torch.equal(out[mask], d_syms[mask]), key
            return ctx.last_decode_kernel()

        def status(ctx, key):
            assert ctx.decode_errors() == 0, key
    else:
        # one container, one index for every ragged variant (each launch writes all of it)
        cont = torch.empty(cap, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
        if with_uniform:
            u_chunks, u_total = R.num_chunks(n, chunk), R.encode_slots_bound(fmt, n, ways, chunk)
            u_cont = torch.empty(u_total, dtype=torch.uint8, device="cuda")
            u_offs = torch.zeros(u_chunks + 1, dtype=torch.int64, device="cuda")
            u_lens = torch.zeros(u_chunks, dtype=torch.int32, device="cuda")

        def ragged(ctx, order):
            return ctx, lambda: ctx.encode_batch(gm[ctx], d_syms, d_sym, d_counts, ways, d_slot, d_out=cont, d_offsets=offs, d_lengths=lens,
                                                 out_cap=cap, d_order=order)

        def uniform():
            ctx_off.encode_slots(gm[ctx_off], d_syms, ways, chunk, d_out=u_cont, sync=False, d_offsets=u_offs, d_lengths=u_lens)

        def verify(key, ctx, fn):
            if key != "uniform":
                cont.zero_(); offs.zero_(); lens.zero_()
            fn()
            torch.cuda.synchronize()
            ctx.encode_status()
            if key == "wave":  # the bytes of the streams: what lies between them is whatever a 16-byte flush left there
                want["gaps"] = ~covered(offs, lens, cap)
                want.update(cont=cont.masked_fill(want["gaps"], 0), offs=offs.clone(), lens=lens.clone())
                assert torch.equal(offs + lens.to(torch.int64), d_slot[1:]), "a stream does not end at its slot's end"
            elif key == "uniform":
                back = ctx_off.decode(gm[ctx_off], u_cont, u_total, u_offs, u_lens, n, ways, chunk)
                assert ctx_off.decode_errors() == 0 and torch.equal(back, d_syms), key
            else:
                assert torch.equal(offs, want["offs"]) and torch.equal(lens, want["lens"]), key
                assert torch.equal(cont.masked_fill(want["gaps"], 0), want["cont"]), key
            return ctx.last_encode_kernel()[0]

        def status(ctx, key):
            ctx.encode_status()

    v = row.variant
    variants = {"wave": ragged(ctx_off, None), "wave_ordered": ragged(ctx_off, d_order), v: ragged(ctx_on, None),
                v + "_ordered": ragged(ctx_on, d_order)}
    if with_uniform:
        variants["uniform"] = (ctx_off, uniform)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for key, (ctx, fn) in variants.items():
        kernel = verify(key, ctx, fn)
        assert kernel == expected_kernel(row, key, R.num_chunks(n, chunk), num_cus), (key, kernel)
        print("%s: %s verified, %s" % (name, key, kernel), file=sys.stderr, flush=True)
        res[key] = {"kernel": kernel, "pass_ms_mean": [], "ms_min": None}
    want.clear()
    for k in range(args.passes):
        print("%s: pass %d of %d" % (name, k + 1, args.passes), file=sys.stderr, flush=True)
        for key, (ctx, fn) in variants.items():
            ms, ms_min = bench.timed_launches(torch, fn, args.steps, args.warmup)
            r = res[key]
            r["pass_ms_mean"].append(round(ms, 4))
            r["ms_min"] = round(ms_min if r["ms_min"] is None else min(r["ms_min"], ms_min), 4)
            status(ctx, key)
    for c in (ctx_on, ctx_off):
        c.close()
    return {"symbols": n, "streams": n_streams, "mean_stream_syms": round(float(counts.mean()), 1), **res}


def run_family(row, args, out):
    import numpy as np
    import torch

    rng = np.random.default_rng(args.seed)
    mean = (MAX_LEN + 1) / np.log(MAX_LEN + 1.0)  # of the log-uniform draw below
    counts = (np.exp(rng.random(int(args.symbols / mean * 1.05) + 16) * np.log(MAX_LEN + 1.0)) - 1.0).astype(np.uint32)
    keep = int(np.searchsorted(np.cumsum(counts.astype(np.int64)), args.symbols)) + 1
    draws = {"ragged": counts[:keep], "equal": np.full(max(64, args.symbols // row.chunk), row.chunk, dtype=np.uint32)}
    batches = {}
    for name in row.batches:
        batches[name] = run_batch(row, args, name, draws[name], name == row.batches[-1])
        torch.cuda.empty_cache()
    run = {"steps": args.steps, "warmup": args.warmup, "passes": args.passes, "device": torch.cuda.get_device_name(0)}
    result = summarise(row, run, batches)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--family", required=True, choices=list(FAMILIES) + ["all"])
    ap.add_argument("--symbols", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)  # (bench.py's defaults)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, help="default: the family's (3; the lane families 5)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="default: the family's file under profiles/; with --family all, a directory")
    args = ap.parse_args(argv)

    import torch
    assert torch.cuda.is_available(), "bench_batch_families.py needs a GPU"
    passes, results = args.passes, {}
    for name in (FAMILIES if args.family == "all" else [args.family]):
        row = FAMILIES[name]
        args.passes = passes or row.passes
        if args.family == "all":
            out = os.path.join(args.out or os.path.join(ROOT, "profiles"), row.out)
        else:
            out = args.out or os.path.join(ROOT, "profiles", row.out)
        results[name] = run_family(row, args, out)
    return results


if __name__ == "__main__":
    main()
