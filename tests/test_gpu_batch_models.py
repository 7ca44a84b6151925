"""Ragged batches with one model per stream on the GPU (rans_amd_encode_batch_adaptive / rans_amd_decode_batch_adaptive):
every stream's frequency row and bytes against the oracle, which builds the model of each stream from that stream alone
(Oracle.count_freqs + normalize + encode per stream, threaded over the host cores; the library never checks itself).

MODEL_ROWS (tests/_kernel_rows.py): one row per shape, naming the kernels the library must report for it
(tests/test_batch_models_host.py holds the rows to the names the launchers can report).  Regimes U, H and R, the lengths, the
poison rules and ModelBatch are tests/_batch.py's.  Input is bench.gen_zipf with seed 1, stream c's symbols rotated by (37 c) mod 256, so that the
rows differ from stream to stream; four more streams are always in: 4096 and 16384 symbols exactly (the sizes the uniform
encoder keeps register-resident: here they take the two-pass form), one value repeated 4 N + 3 times (word format: frequency
4096, a word leaves per symbol) and all 256 values once (at 8 bits every frequency is 1)."""
import numpy as np
import pytest

from _batch import POISON, ModelBatch, draw_lengths, graph_decode_script, mandatory_lengths, resident_waves, run_graph_script
from _batch import run_model_row as run_row
from _kernel_rows import MODEL_ROW as ROW
from _kernel_rows import MODEL_ROWS
from _oracle import FMT_BYTE, FMT_WORD

ONE_VALUE = 201


def special_streams(ways):
    """(count, content) of the four streams every batch carries behind the drawn ones; content None = the rotated zipf symbols."""
    return [(4096, None), (16384, None), (4 * ways + 3, np.full(4 * ways + 3, ONE_VALUE, dtype=np.uint8)),
            (256, np.arange(256, dtype=np.uint8))]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    yield R, ctx, torch
    ctx.close()


def with_specials(counts, ways):
    sp = special_streams(ways)
    all_counts = np.concatenate((counts, np.array([s[0] for s in sp], dtype=np.uint32)))
    return all_counts, {counts.size + i: s[1] for i, s in enumerate(sp) if s[1] is not None}


def _cases():
    for r in MODEL_ROWS:
        for regime in ("U", "H", "R"):
            yield pytest.param(r, regime, id="%s-%s" % (r["id"], regime), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,regime", list(_cases()))
def test_models_row_every_stream_equals_oracle(gpu, oracle, row, regime):
    R, ctx, torch = gpu
    resident = resident_waves(torch)
    ways = row["ways"]
    if regime == "U":  # one stream per launch
        batches = [(np.array([ln], dtype=np.uint32), None) for ln in mandatory_lengths(ways)]
        batches += [(np.array([s[0]], dtype=np.uint32), None if s[1] is None else {0: s[1]}) for s in special_streams(ways)]
    else:
        n_streams = resident // 2 if regime == "H" else 4 * resident
        drawn = draw_lengths(n_streams - 4, ways, 7)
        assert set(mandatory_lengths(ways)) <= set(drawn.tolist())
        batches = [with_specials(drawn, ways)]
        assert (0 < batches[0][0].size < resident) if regime == "H" else batches[0][0].size >= 4 * resident
    for counts, contents in batches:
        b = ModelBatch(R, ctx, torch, oracle, row, counts, contents)
        if b.n > 1:  # (a shared-model shortcut cannot pass)
            nonempty = b.rows[b.counts > 0]
            assert np.unique(nonempty, axis=0).shape[0] >= 2, "the streams' rows do not differ"
        for align in (1, 4):
            run_row(b, align)
        assert ctx.decode_errors() == 0


def test_the_oracle_takes_the_required_shapes(oracle):
    """No GPU: the checker itself on the shapes the batches must hold -- a one-symbol stream (word 8-way: 32 bytes of states
    and one word), one value repeated, all 256 values once, N - 1 symbols, an empty stream -- encode and decode again."""
    for fmt, sb in ((FMT_WORD, 12), (FMT_BYTE, 12), (FMT_BYTE, 8)):
        for ways in (2, 8, 64, 128):
            shapes = [np.array([7], np.uint8), np.full(ways + 1, 9, np.uint8), np.full(4 * ways + 3, 9, np.uint8),
                      np.arange(256, dtype=np.uint8), (np.arange(ways - 1) * 37 % 256).astype(np.uint8)]
            for syms in shapes:
                om = oracle.model_for(syms, 256, sb)
                stream = oracle.encode(fmt, om, syms, ways)
                assert np.array_equal(oracle.decode(fmt, om, stream, syms.size, ways), syms)
                if fmt == FMT_WORD and syms.size == 1:
                    assert stream.size == 4 * ways + 2
            assert oracle.encode(fmt, om, np.zeros(0, np.uint8), ways).size == 4 * ways


@pytest.mark.gpu
def test_models_large_word8(gpu, oracle):
    """2 x 10^4 streams of the reference's 8-way word layout, sym_align = 4, every stream against the oracle."""
    R, ctx, torch = gpu
    row = ROW["word-8"]
    counts, contents = with_specials(draw_lengths(20000, 8, 13), 8)
    b = ModelBatch(R, ctx, torch, oracle, row, counts, contents)
    run_row(b, 4)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_models_damage_is_counted_and_contained(gpu, oracle):
    """A flipped byte in the flushed states of five streams, one row whose sum is off by one, one sym_offset past out_syms:
    E_CORRUPT with bad_streams exactly seven; every other stream, the padding and the guard are intact; a stream of 0
    symbols whose row is garbage still decodes (its row is neither read nor validated)."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(600, 64, 21))
    for align in (1, 4):
        d_buf, sym_offs = b.laid_out(align)
        d_sym = b.dev(sym_offs, np.int64)
        h, (cont, offs, lens, rows, total) = b.encode(d_buf, d_sym)
        rng = np.random.default_rng(3)
        # (a flipped byte is only certain to be noticed where symbols depend on it: streams of at least 4 N + 3 symbols)
        long_ones = np.nonzero(b.counts >= 4 * 64 + 3)[0]
        picked = rng.choice(long_ones, 7, replace=False)
        flipped, bad_row, far = picked[:5], int(picked[5]), int(picked[6])
        empty = np.nonzero(b.counts == 0)[0]
        assert empty.size >= 1
        bad_cont = cont.clone()
        for c in flipped:
            bad_cont[int(h[1][c]) + 1] ^= 0x40
        bad_rows = h[3].copy()
        bad_rows[bad_row, int(np.argmax(bad_rows[bad_row]))] += 1  # the sum is 4097
        bad_rows[int(empty[0])] = 0xA5A5                           # garbage where nothing is read
        bad_sym = d_sym.clone()
        bad_sym[far] = d_buf.numel() - int(b.counts[far]) + 1      # one symbol past the end
        out = torch.full_like(d_buf, POISON)
        with pytest.raises(R.RansAmdError) as e:
            b.decode(bad_cont, total, offs, lens, b.d_rows(bad_rows), bad_sym, out)
        assert e.value.status == R.E_CORRUPT
        assert e.value.bad_streams == 7, "h_bad_streams as the call wrote it"
        assert ctx.decode_errors() == 0  # (reported and reset by that call)
        got, want = out.cpu().numpy(), d_buf.cpu().numpy()
        keep = np.ones(want.size, dtype=bool)
        for c in picked:
            keep[int(sym_offs[c]):int(sym_offs[c]) + int(b.counts[c])] = False
        assert np.array_equal(got[keep], want[keep]), "an undamaged stream, the padding or the guard differs"
        assert np.all(got[int(sym_offs[far]):int(sym_offs[far]) + int(b.counts[far])] == POISON), "the stream with the bad sym_offset was written"
        assert np.all(got[int(sym_offs[bad_row]):int(sym_offs[bad_row]) + int(b.counts[bad_row])] == POISON), "the stream with the bad row was written"
        assert np.all(got[int(sym_offs[-1]):] == POISON)
        # the garbage row alone is no damage
        ok_rows = h[3].copy()
        ok_rows[int(empty[0])] = 0xA5A5
        out = torch.full_like(d_buf, POISON)
        b.decode(cont, total, offs, lens, b.d_rows(ok_rows), d_sym, out)
        assert torch.equal(out, d_buf)


@pytest.mark.gpu
def test_models_encode_without_room(gpu, oracle):
    """out_cap one line short of what the batch uses: E_SPACE, the streams that fit are the oracle's, the lengths of the
    others are 0, nothing at or behind out_cap is written.  And a symbol range outside [0, in_syms) is not read: E_ARG."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(300, 64, 71))
    d_buf, sym_offs = b.laid_out(4)
    d_sym = b.dev(sym_offs, np.int64)
    h, _ = b.encode(d_buf, d_sym)
    used = h[4]
    cap = used - 64
    d_out = torch.full((b.bound + 4096,), POISON, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda")
    d_lens = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    d_freqs = torch.zeros(b.n * 256, dtype=torch.int16, device="cuda")
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_batch_adaptive(d_buf, d_sym, b.d_counts, 64, 12, fmt=FMT_WORD, d_out=d_out, cap=cap, d_offsets=d_offs,
                                  d_lengths=d_lens, d_freqs=d_freqs)
    assert e.value.status == R.E_SPACE
    cont, offs, lens = d_out.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32)
    ends = h[1][:b.n] + h[2]  # (the layout does not depend on the capacity)
    fits = ends <= cap
    assert 0 < np.count_nonzero(~fits) < b.n
    for c in range(b.n):
        if fits[c]:
            assert lens[c] == b.lens[c] and offs[c] == h[1][c], c
            assert np.array_equal(cont[int(offs[c]):int(offs[c]) + int(lens[c])], b.streams[c]), c
        else:
            assert lens[c] == 0, c
    assert np.all(cont[cap:] == POISON), "written at or behind out_cap"
    # the symbol index is data: the last stream pushed one symbol past in_syms
    bad_sym = d_sym.clone()
    last = int(np.nonzero(b.counts > 0)[0][-1])
    bad_sym[last] = d_buf.numel() - int(b.counts[last]) + 1
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_batch_adaptive(d_buf, bad_sym, b.d_counts, 64, 12, fmt=FMT_WORD)
    assert e.value.status == R.E_ARG


@pytest.mark.gpu
def test_models_decode_order(gpu, oracle):
    """decode_batch_adaptive with rans_amd_batch_order's permutation gives what it gives without: the row index is the stream
    index after the order."""
    R, ctx, torch = gpu
    row = ROW["word-64"]
    b = ModelBatch(R, ctx, torch, oracle, row, draw_lengths(3000, 64, 31))
    d_buf, sym_offs = b.laid_out(4)
    d_sym = b.dev(sym_offs, np.int64)
    _, (cont, offs, lens, rows, total) = b.encode(d_buf, d_sym)
    d_order = ctx.batch_order(b.d_counts)
    assert not np.array_equal(d_order.cpu().numpy(), np.arange(b.n))
    outs = []
    for o in (None, d_order):
        out = torch.full_like(d_buf, POISON)
        b.decode(cont, total, offs, lens, rows, d_sym, out, d_order=o)
        outs.append(out)
    assert torch.equal(outs[0], d_buf) and torch.equal(outs[1], outs[0])


@pytest.mark.gpu
def test_models_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch_adaptive, replayed three times, in a child process under a time limit of its own.  Graph
    replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply."""
    run_graph_script(tmp_path, "graph_batch_models.py", graph_decode_script("k_decode_batch_models<word>", per_stream_models=True))
