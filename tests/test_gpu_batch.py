"""Ragged batches on the GPU: many independent streams, each with its own symbol count, every stream against the oracle.

BATCH_ROWS (tests/_kernel_rows.py): one row per shape, naming the batch kernels the library must report for it
(tests/test_batch_host.py holds the rows to the names the launchers can report); the harness is tests/_batch.py.  Every row
runs in the regimes of tests/test_gpu_kernel_matrix.py --

  U  one stream per launch (each of the mandatory lengths in turn)
  H  about half as many streams as there are resident waves
  R  at least 4 x (CUs x 2 blocks x 16 waves) streams: several rounds of the persistent grid

-- with lengths drawn log-uniform from [0, 64 Ki] (fixed seed) that always include 0, 1, N-1, N, N+1, 4N+3 and 65536, once
with sym_align = 1 (odd output addresses: element stores) and once with sym_align = 4 (dword stores).  Input is
bench.gen_zipf with seed 1; the checker is the CPU oracle (Oracle.encode per stream, threaded over the host cores), never
the library itself.  Output buffers are filled with a poison value first: the padding between streams and a guard region
behind the last one must come back untouched."""
import numpy as np
import pytest

from _around_coders import ref_order_keys
from _batch import POISON, Batch, draw_lengths, graph_decode_script, mandatory_lengths, resident_waves, run_graph_script, run_row
from _kernel_rows import BATCH_ROWS, ROW


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def _cases():
    for r in BATCH_ROWS:
        for regime in ("U", "H", "R"):
            yield pytest.param(r, regime, id="%s-%s" % (r["id"], regime), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,regime", list(_cases()))
def test_batch_row_every_stream_equals_oracle(gpu, oracle, row, regime):
    R, ctx, torch = gpu
    resident = resident_waves(torch)
    if regime == "U":
        batches = [np.array([ln], dtype=np.uint32) for ln in mandatory_lengths(row["ways"])]
    else:
        n_streams = resident // 2 if regime == "H" else 4 * resident
        assert (0 < n_streams < resident) if regime == "H" else n_streams >= 4 * resident
        batches = [draw_lengths(n_streams, row["ways"], 7)]
        assert set(mandatory_lengths(row["ways"])) <= set(batches[0].tolist())
    for counts in batches:
        b = Batch(R, ctx, torch, oracle, row, counts)
        for align in (1, 4):
            run_row(b, align)
        assert ctx.decode_errors() == 0


LARGE = [("word-64", 20000), ("word-8", 20000), ("byte-2", 20000), ("r64-2", 20000)]


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", LARGE)
def test_batch_large_reference_layouts(gpu, oracle, rid, n_streams):
    """2 x 10^4 streams of a reference layout (word 64-way, word 8-way, byte 2-way, rans64 2-way), every stream against the
    oracle (threaded over the host cores).  Wall time on an MI355X with 16 host threads: 2.1 s (byte 2-way), 1.7 s (word
    8-way), less than that for word 64-way and rans64 2-way; this whole file takes 56 s."""
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW[rid], draw_lengths(n_streams, ROW[rid]["ways"], 13))
    run_row(b, 4)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_batch_damage_is_counted_and_contained(gpu, oracle):
    """One flipped byte in k streams, one length shortened by a unit, one sym_offset past out_syms: h_bad_streams is exactly
    the number damaged, every other stream decodes right, nothing outside the streams' ranges is written."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = Batch(R, ctx, torch, oracle, row, draw_lengths(600, 64, 21))
    for align in (1, 4):
        d_buf, sym_offs, slot_offs = b.laid_out(align)
        d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
        cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 64, d_slot)
        ctx.encode_status()
        h_offs, h_lens = offs.cpu().numpy()[:b.n], lens.cpu().numpy()[:b.n]
        rng = np.random.default_rng(3)
        # (a flipped byte is only certain to be noticed where symbols depend on it: streams of at least 4 N + 3 symbols)
        long_ones = np.nonzero(b.counts >= 4 * 64 + 3)[0]
        picked = rng.choice(long_ones, 7, replace=False)
        flipped, short, far = picked[:5], picked[5], picked[6]
        bad_cont = cont.clone()
        for c in flipped:  # inside the flushed states: a final state can no longer be L... or the cursor misses its end
            bad_cont[int(h_offs[c]) + 1] ^= 0x40
        bad_lens = lens.clone()
        bad_lens[int(short)] -= 2
        bad_sym = d_sym.clone()
        bad_sym[int(far)] = d_buf.numel() - int(b.counts[far]) + 1  # one symbol past the end
        out = torch.full_like(d_buf, b.poison())
        with pytest.raises(R.RansAmdError) as e:
            ctx.decode_batch(b.gm, bad_cont, int(slot_offs[-1]), offs, bad_lens, bad_sym, b.d_counts, 64, out)
        assert e.value.status == R.E_CORRUPT
        assert e.value.bad_streams == 7, "h_bad_streams as the call wrote it"
        assert ctx.decode_errors() == 0  # (reported and reset by that call)
        got, want = out.cpu().numpy(), d_buf.cpu().numpy()
        damaged = set(int(c) for c in picked)
        keep = np.ones(want.size, dtype=bool)
        for c in damaged:
            keep[int(sym_offs[c]):int(sym_offs[c]) + int(b.counts[c])] = False
        assert np.array_equal(got[keep], want[keep]), "an undamaged stream, the padding or the guard differs"
        assert np.all(got[int(sym_offs[far]):int(sym_offs[far]) + int(b.counts[far])] == POISON), "the stream with the bad sym_offset was written"
        assert np.all(got[int(sym_offs[-1]):] == POISON)


@pytest.mark.gpu
def test_batch_encode_rejects_bad_slots(gpu, oracle):
    """The slot index is data.  A slot that starts or ends off 16 bytes, is smaller than rans_amd_chunk_bound of its count,
    ends before it starts or ends beyond out_cap is not written: d_lengths[c] = 0, encode_status() reports E_SPACE, every
    other stream is the oracle's, and the poison in the rejected slots, between the slots and behind out_cap is intact."""
    R, ctx, torch = gpu
    for rid in ("word-64", "byte-2"):
        row = ROW[rid]
        ways = row["ways"]
        counts = draw_lengths(400, ways, 71)
        b = Batch(R, ctx, torch, oracle, row, counts)
        d_buf, sym_offs, _ = b.laid_out(4)
        bound = np.array([R.chunk_bound(row["fmt"], int(c), ways) for c in counts], dtype=np.int64)
        # every slot is 32 bytes larger than rans_amd_chunk_bound of its count: a stream ends at its slot's end, so the
        # head of every slot must stay poison
        sizes = bound + 32
        idx = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        cap = int(idx[-1])
        big = np.nonzero(counts >= 1000)[0]
        off16, past = int(big[0]), 399
        small = int(big[(big > off16 + 2) & (big < past - 1)][0])
        bad_idx = idx.copy()
        bad_idx[off16 + 1] += 8          # slot off16 ends off 16 bytes, and slot off16 + 1 starts there
        bad_idx[small] = bad_idx[small + 1] - (bound[small] - 16)  # slot `small` one granule too small (and slot small - 1 larger)
        rejected = {off16, off16 + 1, small}
        out_cap = cap - 16               # the last slot ends beyond out_cap
        rejected.add(past)
        assert len(rejected) == 4
        d_out = torch.full((cap + 4096,), POISON, dtype=torch.uint8, device="cuda")
        cont, offs, lens = ctx.encode_batch(b.gm, d_buf, b.dev(sym_offs, np.int64), b.d_counts, ways, b.dev(bad_idx, np.int64), d_out=d_out,
                                            out_cap=out_cap)
        with pytest.raises(R.RansAmdError) as e:
            ctx.encode_status()
        assert e.value.status == R.E_SPACE
        h, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy().view(np.uint32)
        for c in range(b.n):
            lo, hi = int(bad_idx[c]), int(bad_idx[c + 1])
            if c in rejected:
                assert h_lens[c] == 0, (rid, c)
                if hi > lo:
                    assert np.all(h[lo:hi] == POISON), (rid, "a rejected slot was written", c)
            else:
                ln = int(h_lens[c])
                assert ln == b.lens[c] and int(h_offs[c]) == hi - ln, (rid, c)
                assert np.array_equal(h[hi - ln:hi], b.streams[c]), (rid, "stream", c)
                # (below the stream only what a 16-byte flush may touch: the slack of the slot's first 16 bytes stays poison)
                assert np.all(h[lo:lo + 16] == POISON), (rid, "the head of a slot was written", c)
        assert np.all(h[cap:] == POISON), "written behind the container"


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [1, 33, 100000])
def test_batch_order(gpu, oracle, n_streams):
    R, ctx, torch = gpu
    counts = draw_lengths(n_streams, 64, 31)
    if n_streams == 33:
        counts = np.array([(1 << k) - 1 for k in range(33)], dtype=np.uint64).clip(0, 0xffffffff).astype(np.uint32)  # one per bucket
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    order = ctx.batch_order(d_counts).cpu().numpy().view(np.uint32)
    assert np.array_equal(np.sort(order), np.arange(n_streams, dtype=np.uint32)), "not a permutation"
    keys = ref_order_keys(counts[order])  # (in integers: no float log2 next to a power of two)
    assert np.all(np.diff(keys) <= 0), "bucket keys increase"
    if n_streams == 33:
        assert keys.tolist() == list(range(32, -1, -1))
        return
    # decode_batch with the order gives what it gives without
    small = counts.copy()
    if n_streams > 1000:
        small = np.minimum(counts, 2048)  # (10^5 streams: short ones, the order is what is under test)
    b = Batch(R, ctx, torch, oracle, ROW["word-64"], small)
    d_order = ctx.batch_order(b.d_counts)
    d_buf, sym_offs, slot_offs = b.laid_out(4)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 64, d_slot)
    ctx.encode_status()
    outs = []
    for o in (None, d_order):
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, cont, int(slot_offs[-1]), offs, lens, d_sym, b.d_counts, 64, out, d_order=o)
        outs.append(out)
    assert torch.equal(outs[0], d_buf) and torch.equal(outs[1], outs[0])


@pytest.mark.gpu
def test_batch_slice_ranges_decode_like_one_shot(gpu, oracle):
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW["byte-2"], draw_lengths(3000, 2, 41))
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 4, with_oracle_container=False)
    h_cont, h_offs, h_lens = cont.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n]
    bounds = R.batch_slice(h_lens, 8)
    out = torch.full_like(d_buf, b.poison())
    for g in range(8):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        if lo == hi:
            continue
        bb, be, rebased = R.container_slice(h_offs, h_lens, lo, hi)
        piece = torch.zeros(be - bb + 16, dtype=torch.uint8, device="cuda")
        piece[:be - bb] = torch.from_numpy(h_cont[bb:be]).cuda()
        ctx.decode_batch(b.gm, piece, be - bb, b.dev(rebased[:hi - lo], np.int64), lens[lo:hi], d_sym[lo:hi], b.d_counts[lo:hi], 2, out,
                         n_streams=hi - lo)
    assert torch.equal(out, d_buf)
    sizes = [int(h_lens[int(bounds[g]):int(bounds[g + 1])].sum()) for g in range(8)]
    assert max(sizes) <= sum(sizes) / 8 + int(h_lens.max())


@pytest.mark.gpu
def test_batch_container_compact_then_decode(gpu, oracle):
    R, ctx, torch = gpu
    b = Batch(R, ctx, torch, oracle, ROW["r64-2"], draw_lengths(2000, 2, 51))
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 1, with_oracle_container=False)
    c_cont, c_offs, c_total = ctx.compact(cont, int(slot_offs[-1]), offs, lens, b.n)
    assert c_total < int(slot_offs[-1])
    b.check_streams(c_cont.cpu().numpy(), c_offs.cpu().numpy()[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n], "compacted batch")
    out = torch.full_like(d_buf, b.poison())
    ctx.decode_batch(b.gm, c_cont, c_total, c_offs, lens, d_sym, b.d_counts, 2, out)
    assert torch.equal(out, d_buf)


@pytest.mark.gpu
def test_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch, replayed three times, in a child process under a time limit of its own.  Graph replay
    needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    run_graph_script(tmp_path, "graph_batch.py", graph_decode_script("k_decode_batch_word64"))
