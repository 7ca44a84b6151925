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

from _batch import (Batch, check_damage_inside_one_wave_load, check_decode_order, check_option_takes_zero_or_one,
                    check_other_shape_keeps_its_kernels, draw_lengths, draw_log_uniform, mandatory_lengths, option_contexts, resident_waves,
                    run_family_graph, run_row)
from _kernel_rows import GROUPS, GROW, OPT_BATCH_GROUPS


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_GROUPS)


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
    check_decode_order(gpu, oracle, GROUPS, 17, (1, 4))


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
    check_damage_inside_one_wave_load(gpu, oracle, GROUPS, 16, (1, 3, 4, 6), 2, lambda off, ln, nbytes: off + 1, (4,))


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("word-64", 20), ("word-u16-64", 20), ("word-8", 7), ("byte-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """64-way, u16 symbols, fewer than eight 8-way streams and the byte format take the wave-per-stream kernels on the
    context with the option on, and decode right.  0.03 s per case."""
    check_other_shape_keeps_its_kernels(gpu, oracle, GROUPS, rid, n_streams)


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the group kernel."""
    check_option_takes_zero_or_one(gpu, oracle, GROUPS)


@pytest.mark.gpu
def test_group_batch_decode_in_a_captured_graph(tmp_path):
    """One captured decode_batch of 3000 8-way streams with the option on: one eager call first, then three replays, each
    equal to the eager result, in a child process under a time limit of its own.  Graph replay needs the process's default
    of four hardware queues: with GPU_MAX_HW_QUEUES set below that the test does not apply.  2.5 s."""
    run_family_graph(tmp_path, GROUPS, "graph_batch_groups.py")
