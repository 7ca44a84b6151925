"""k_decode_word64 around its chunk hand-out: word format, 64-way, 12 bits throughout.

Written with the pacing experiment of profiles/word64_pacing.md (the waves of a block watching each other's progress on a
board in LDS, the fast ones giving up issue slots; chunks handed out from more counters, by a static stride, or without a
claim for a wave's first chunk).  Pacing lost and is not in the tree; the cases stay, because whatever changes how this
kernel's waves come by their chunks has to pass them: it may not change a byte, hang a launch in which almost nobody has
work, or leave a counter dirty for the next launch.  Every case feeds the decoder a container the ORACLE made (threaded host
encode), compares the output with the input, and asserts decode_errors() == 0 and last_decode_kernel() ==
"k_decode_word64".  W = 32 x the device's CU count = the waves of a full launch (2 blocks of 16 waves per CU).

One input (bench.gen_zipf, seed 1, W x 32768 + 65 symbols) and one model serve every case; the oracle's container of a
(chunk size, length) pair is made once and kept."""
import time

import numpy as np
import pytest

from _oracle import FMT_WORD

pytestmark = pytest.mark.gpu
KERNEL = "k_decode_word64"
LAUNCH_DEADLINE_S = 30.0  # a launch of this file takes well under a millisecond


class Shared:
    def __init__(self, R, ctx, torch, oracle):
        import bench
        self.R, self.ctx, self.torch, self.oracle = R, ctx, torch, oracle
        self.W = 32 * torch.cuda.get_device_properties(0).multi_processor_count
        self.d_all = bench.gen_zipf(torch, self.W * 32768 + 65, 256, 1.0, 1, "cuda")
        self.h_all = self.d_all.cpu().numpy()
        # (the model of a fixed 1 Mi-symbol prefix: every byte value occurs in it)
        self.freqs, _ = R.normalize_freqs(ctx.count_freqs_device(self.d_all[:1 << 20], 256), 4096)
        self.gm = ctx.model(R.FMT_WORD, self.freqs, 12)
        self.om = oracle.model(self.freqs, 12)
        self.made = {}

    def container(self, chunk, n):
        """The oracle's container of the first n symbols in chunks of `chunk`, on the device: (cont, bytes, offs, lens)."""
        key = (chunk, n)
        if key not in self.made:
            torch = self.torch
            cont, offs, lens = self.oracle.encode_chunked_mt(FMT_WORD, self.om, self.h_all[:n], 64, chunk, align=16)
            d_cont = torch.zeros(cont.size + 64, dtype=torch.uint8, device="cuda")
            d_cont[:cont.size] = torch.from_numpy(cont).cuda()
            self.made[key] = (d_cont, cont.size, torch.from_numpy(offs.astype(np.int64)).cuda(),
                              torch.from_numpy(lens.astype(np.int32)).cuda())
        return self.made[key]

    def launch(self, cont, nbytes, offs, lens, n, chunk, out):
        """One decode that must END: issued without a wait, then polled against a deadline of its own."""
        torch = self.torch
        self.ctx.decode(self.gm, cont, nbytes, offs, lens, n, 64, chunk, d_out=out, sync=False)
        done = torch.cuda.Event()
        done.record()
        t0 = time.perf_counter()
        while not done.query():
            assert time.perf_counter() - t0 < LAUNCH_DEADLINE_S, "the launch did not end (chunk %d, n %d)" % (chunk, n)
        assert self.ctx.last_decode_kernel() == KERNEL, self.ctx.last_decode_kernel()

    def roundtrip(self, chunk, n):
        torch = self.torch
        cont, nbytes, offs, lens = self.container(chunk, n)
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")  # (a guard behind the last symbol)
        self.launch(cont, nbytes, offs, lens, n, chunk, out[:n])
        assert self.ctx.decode_errors() == 0, (chunk, n)
        assert torch.equal(out[:n], self.d_all[:n]), "decoded symbols differ from the input (chunk %d, n %d)" % (chunk, n)
        assert bool((out[n:] == 0xA5).all()), "symbols were written behind the output (chunk %d, n %d)" % (chunk, n)


@pytest.fixture(scope="module")
def shared(oracle):
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield Shared(R, ctx, torch, oracle)
    ctx.close()


def test_more_than_one_grid_round_uneven_split(shared):
    """1024-symbol chunks, 2 W + 3 of them: every wave takes two or three chunks, three are left over for a third round."""
    shared.roundtrip(1024, (2 * shared.W + 3) * 1024)


@pytest.mark.parametrize("chunk,extra", [(260, 5), (4096, 5)])
def test_chunks_shorter_than_one_pacing_interval(shared, chunk, extra):
    """Chunks of 1 and 16 groups of four rounds (the experiment's pacing interval was 32; the hand-over of the next chunk starts
    10 groups before a chunk's end): W + 5 of them, so some waves take a second one."""
    shared.roundtrip(chunk, (shared.W + extra) * chunk)


def test_one_full_chunk_per_wave(shared):
    """32768-symbol chunks, exactly W: the whole grid, one chunk per wave, every wave in phase with every other."""
    shared.roundtrip(32768, shared.W * 32768)


@pytest.mark.parametrize("nchunks", [1, 2, 15, 17, 33])
def test_almost_nobody_has_work(shared, nchunks):
    """A block in which one wave, two, all but one, or (in the second block) one wave has a 32768-symbol chunk: waves that
    watch their block-mates must not wait for, or measure themselves against, waves that never move.  The launch must end."""
    shared.roundtrip(32768, nchunks * 32768)


@pytest.mark.parametrize("last", [1, 63, 64, 65])
def test_ragged_last_chunk(shared, last):
    """n is no multiple of the chunk: 19 chunks of 32768 symbols and a last one of less than a round, a round less one symbol,
    one round, a round and a symbol."""
    shared.roundtrip(32768, 19 * 32768 + last)


def test_one_damaged_chunk_in_the_middle(shared):
    """2 W chunks of 16384 symbols, the middle one's length cut by one unit: exactly one chunk is counted, every other chunk
    decodes to the input."""
    torch, W, chunk = shared.torch, shared.W, 16384
    n = 2 * W * chunk
    cont, nbytes, offs, lens = shared.container(chunk, n)
    bad_lens = lens.clone()
    mid = W
    bad_lens[mid] -= 2
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    shared.launch(cont, nbytes, offs, bad_lens, n, chunk, out)
    assert shared.ctx.decode_errors() == 1
    assert torch.equal(out[:mid * chunk], shared.d_all[:mid * chunk]), "a chunk in front of the damaged one differs"
    assert torch.equal(out[(mid + 1) * chunk:], shared.d_all[(mid + 1) * chunk:n]), "a chunk behind the damaged one differs"


@pytest.mark.parametrize("nchunks", [40, 48])
def test_graph_replays_start_clean(shared, nchunks):
    """Three replays under torch.cuda.graph with an eager launch in between (40 chunks: three blocks with waves to spare; 48:
    a whole multiple of the launch's waves): whatever hands the chunks out starts clean every time."""
    torch, ctx, chunk = shared.torch, shared.ctx, 32768
    n = nchunks * chunk
    cont, nbytes, offs, lens = shared.container(chunk, n)
    want = shared.d_all[:n]
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    shared.launch(cont, nbytes, offs, lens, n, chunk, out)  # (once outside the capture: the workspaces exist afterwards)
    assert torch.equal(out, want)
    out_g = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.decode(shared.gm, cont, nbytes, offs, lens, n, 64, chunk, d_out=out_g, sync=False)
    assert not bool(out_g.any())  # capturing ran nothing
    for rep in range(3):
        out_g.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert ctx.decode_errors() == 0 and ctx.last_decode_kernel() == KERNEL
        assert torch.equal(out_g, want), ("replay", rep)
        out.zero_()
        shared.launch(cont, nbytes, offs, lens, n, chunk, out)
        assert ctx.decode_errors() == 0
        assert torch.equal(out, want), ("eager launch behind replay", rep)
    del g


def test_ragged_batch_unchanged(shared, oracle):
    """k_decode_batch_word64 (the same source, its ragged instantiation: untouched by anything done to the uniform one) on 2000
    streams with log-uniform lengths in [0, 64 Ki], from a container the oracle made, at odd and at dword-aligned output
    offsets."""
    from _batch import Batch, draw_lengths
    from _kernel_rows import ROW
    R, ctx, torch = shared.R, shared.ctx, shared.torch
    b = Batch(R, ctx, torch, oracle, ROW["word-64"], draw_lengths(2000, 64, 31))
    o_cont, o_starts, o_bytes = b.oracle_container()
    d_cont, d_starts, d_lens = b.dev(o_cont, np.uint8), b.dev(o_starts, np.int64), b.dev(b.lens, np.int32)
    for align in (1, 4):
        d_buf, sym_offs, _ = b.laid_out(align)
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, d_cont, o_bytes, d_starts, d_lens, b.dev(sym_offs, np.int64), b.d_counts, 64, out)
        assert ctx.last_decode_kernel() == "k_decode_batch_word64", ctx.last_decode_kernel()
        assert ctx.decode_errors() == 0
        assert torch.equal(out, d_buf), "a stream of the batch differs (align %d)" % align
