"""Ragged batches of the reference's 8-way word layout with EIGHT streams per wave: k_decode_batch_word_groups, the kernel
rans_amd_decode_batch launches on a context with RANS_AMD_OPT_BATCH_GROUPS = 1.

GROUP_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_groups_host.py holds the rows
to the names the launchers can report).  The helpers are tests/_batch.py's: every decode is checked against the symbols
the oracle's streams were made from, from the GPU's own container and from one the oracle made (shuffled, unit-aligned
offsets, gaps), into a poison-filled buffer whose padding and guard must come back untouched.

A wave's eight groups hold eight streams with eight different symbol counts: the wave runs the 16-round sequence
max(count >> 7) times, a group that has run out of 128-byte lines is parked (its bits of the ballot zeroed, its state put
back behind every block, its line not stored), and what count & 127 leaves goes one round at a time.  The shapes below
are the smallest at which that can go wrong."""
import numpy as np
import pytest

from _batch import (GUARD, POISON, Batch, Coded, draw_lengths, draw_log_uniform, graph_decode_script, mandatory_lengths, resident_waves,
                    run_graph_script, run_row)
from _kernel_rows import GROW, OPT_BATCH_GROUPS, ROW
from _oracle import FMT_WORD


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    ctx.set_option(OPT_BATCH_GROUPS, 1)
    off = R.Context(0)  # the option at its default: the wave-per-stream kernels
    yield R, ctx, torch, off
    off.close()
    ctx.close()


OCTETS = {
    "one-line-each": [128] * 8,
    "boundaries": [0, 1, 7, 8, 9, 127, 128, 129],
    "seven-parked-512-blocks": [65536, 0, 0, 0, 0, 0, 0, 1],
    "every-group-parks-elsewhere": [128 * (g + 1) + 5 * g for g in range(8)],
    "all-empty": [0] * 8,
    "second-octet-of-one": [300] * 9,
    "mandatory-and-200s": mandatory_lengths(8) + [200] * 7,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OCTETS))
def test_single_octets(gpu, oracle, name):
    """One or two octets: one line each and no tail; every block and tail boundary in one wave; seven groups parked for 512
    blocks while one refills its ring throughout; every group parking at another block with another tail; eight empty
    streams; a second octet of one stream and seven empty groups; the mandatory lengths.  Each at sym_align 1 (all
    symbols a round at a time, byte stores) and 4.  Wall time on an MI355X: 0.6 s for the first case (it loads the
    kernels), 0.01 s for each of the others; this whole file takes 12 s."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, GROW, np.array(OCTETS[name], dtype=np.uint32))
    for align in (1, 4):
        run_row(b, align)
    assert ctx.decode_errors() == 0
    assert ctx.launch_spans(1)[0] > 0.0, "the launch recorded no span"


@pytest.mark.gpu
def test_order(gpu, oracle):
    """17 streams: the reversed identity, the result of batch_order, and an order with one entry replaced by n_streams --
    that position is one failed stream, every stream still named decodes right, the stream that lost its position is not
    written.  0.03 s."""
    R, ctx, torch, _ = gpu
    n = 17
    b = Batch(R, ctx, torch, oracle, GROW, draw_lengths(n, 8, 23))
    for align in (1, 4):
        c = Coded(b, align)
        c.decode_all(None, "no order")
        c.decode_all(b.dev(np.arange(n)[::-1], np.int32), "reversed identity")
        d_order = ctx.batch_order(b.d_counts)
        assert sorted(d_order.cpu().tolist()) == list(range(n))
        c.decode_all(d_order, "batch_order")
        lost = int(np.argmax(b.counts))  # (a stream with symbols: its range would show a write)
        order = np.arange(n)
        order[lost] = n
        want = c.d_buf.cpu().numpy().copy()
        lo = int(c.sym_offs[lost])
        want[lo:lo + int(b.counts[lost])] = POISON
        for name, cont, nbytes, offs, lens in c.containers():
            out = torch.full_like(c.d_buf, b.poison())
            with pytest.raises(R.RansAmdError) as e:
                ctx.decode_batch(b.gm, cont, nbytes, offs, lens, c.d_sym, b.d_counts, 8, out, d_order=b.dev(order, np.int32))
            assert e.value.status == R.E_CORRUPT and e.value.bad_streams == 1, (name, e.value.bad_streams)
            assert ctx.last_decode_kernel() == GROW["decode"]
            assert np.array_equal(out.cpu().numpy(), want), (name, "a named stream differs, or the stream without a position was written")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer octets than the launch has resident waves, lengths log-uniform up to 64 Ki with the mandatory ones.
    several: at least 1.25 x as many octets as resident waves, so that waves come back for further claims; lengths
    log-uniform up to 1024 (the oracle's side stays in seconds).  The last octet of each is partial; each with and
    without d_order at sym_align = 4.  Wall time on an MI355X: 0.7 s (half), 5.6 s (several: 81 925 calls
    of the oracle)."""
    R, ctx, torch, _ = gpu
    resident = resident_waves(torch)
    if regime == "half":
        octets = resident // 8
        counts = draw_lengths(octets * 8 - 3, 8, 7)
        assert 0 < octets < resident and set(mandatory_lengths(8)) <= set(counts.tolist())
    else:
        octets = resident + resident // 4 + 1
        counts = draw_log_uniform(octets * 8 - 3, 1024, 9)
        assert 4 * octets >= 5 * resident
    b = Batch(R, ctx, torch, oracle, GROW, counts)
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 4)
    out = torch.full_like(d_buf, b.poison())
    ctx.decode_batch(b.gm, cont, int(slot_offs[-1]), offs, lens, d_sym, b.d_counts, 8, out, d_order=ctx.batch_order(b.d_counts))
    assert ctx.last_decode_kernel() == GROW["decode"]
    assert torch.equal(out, d_buf), "decode under batch_order's order"
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_damage_is_counted_and_contained_inside_one_octet(gpu, oracle):
    """16 streams of 300..5000 symbols; four streams of the FIRST octet are damaged: a byte flipped in the flushed states,
    a length shortened by 2, an odd offset, a sym_offset one symbol past out_syms.  bad_streams is 4, as the
    wave-per-stream kernel reports for the same damaged batch; the other twelve streams, the padding and the guard are
    exact; the streams with the bad sym_offset and the odd offset are not written.  0.01 s."""
    R, ctx, torch, off = gpu
    counts = np.random.default_rng(17).integers(300, 5001, 16).astype(np.uint32)
    b = Batch(R, ctx, torch, oracle, GROW, counts)
    gm_off = off.model(FMT_WORD, b.freqs, 12)
    flipped, short, odd, far = 1, 3, 4, 6
    damaged = (flipped, short, odd, far)
    for align in (1, 4):
        c = Coded(b, align)
        for name, cont, nbytes, offs, lens in c.containers():
            h_offs = offs.cpu().numpy()
            bad_cont = cont.clone()
            bad_cont[int(h_offs[flipped]) + 1] ^= 0x40  # inside the flushed states
            bad_lens = lens.clone()
            bad_lens[short] -= 2
            bad_offs = offs.clone()
            bad_offs[odd] += 1
            bad_sym = c.d_sym.clone()
            bad_sym[far] = c.d_buf.numel() - int(counts[far]) + 1  # one symbol past the end
            reported = []
            for cx, gm, kernel in ((ctx, b.gm, GROW["decode"]), (off, gm_off, "k_decode_batch<word>")):
                out = torch.full_like(c.d_buf, b.poison())
                with pytest.raises(R.RansAmdError) as e:
                    cx.decode_batch(gm, bad_cont, nbytes, bad_offs, bad_lens, bad_sym, b.d_counts, 8, out)
                assert e.value.status == R.E_CORRUPT and cx.last_decode_kernel() == kernel, (name, cx.last_decode_kernel())
                assert cx.decode_errors() == 0  # (reported and reset by that call)
                reported.append(e.value.bad_streams)
                got, want = out.cpu().numpy(), c.d_buf.cpu().numpy()
                keep = np.ones(want.size, dtype=bool)
                for s in damaged:
                    keep[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] = False
                assert np.array_equal(got[keep], want[keep]), (name, kernel, "an undamaged stream, the padding or the guard differs")
                for s in (far, odd):
                    assert np.all(got[int(c.sym_offs[s]):int(c.sym_offs[s]) + int(counts[s])] == POISON), (name, kernel, "stream", s, "was written")
                assert np.all(got[int(c.sym_offs[-1]):] == POISON) and got.size == int(c.sym_offs[-1]) + GUARD
            assert reported == [4, 4], (name, align, reported)


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("word-64", 20), ("word-u16-64", 20), ("word-8", 7), ("byte-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """64-way, u16 symbols, fewer than eight 8-way streams and the byte format take the wave-per-stream kernels on the
    context with the option on, and decode right.  0.03 s per case."""
    R, ctx, torch, _ = gpu
    row = ROW[rid]
    assert row["decode"] != GROW["decode"]
    b = Batch(R, ctx, torch, oracle, row, draw_lengths(n_streams, row["ways"], 29))
    run_row(b, 4)  # (asserts the row's kernel names)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the group kernel."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, GROW, np.array([300] * 9, dtype=np.uint32))
    for bad in (2, -1):
        with pytest.raises(R.RansAmdError) as e:
            ctx.set_option(OPT_BATCH_GROUPS, bad)
        assert e.value.status == R.E_ARG
    run_row(b, 4)
    ctx.set_option(OPT_BATCH_GROUPS, 0)
    try:
        run_row(Batch(R, ctx, torch, oracle, ROW["word-8"], b.counts), 4)
    finally:
        ctx.set_option(OPT_BATCH_GROUPS, 1)
    run_row(b, 4)


@pytest.mark.gpu
def test_group_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 8-way streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply.  2.5 s."""
    run_graph_script(tmp_path, "graph_batch_groups.py",
                     graph_decode_script(GROW["decode"], ways=8, option="OPT_BATCH_GROUPS"))
