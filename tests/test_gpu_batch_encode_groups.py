"""Ragged batches of the reference's 8-way word layout CODED with eight streams per wave: k_encode_batch_word_groups, the
kernel rans_amd_encode_batch[_ordered] launches on a context with RANS_AMD_OPT_BATCH_ENCODE_GROUPS = 1, and the hand-out
order of the batch encoders (d_order).

ENC_GROUP_ROWS (tests/_kernel_rows.py) names the kernel the library must report (tests/test_batch_encode_groups_host.py holds
the rows to the names the launchers can report).  The helpers are tests/_batch.py's: run_row checks the reported kernel,
every stream byte for byte against the oracle's, each ending at its slot's end, and decodes the result.

The coder works from a stream's last symbol to its first, so a wave's eight groups start together and finish at different
times: a group is finalised (states, last blocks, index entry) right behind its last round and is dead from then on, while
the wave's sixteen-round sequence -- full exec, LDS writes under the whole wave's ballot -- runs on for the others.  The
shapes below are the smallest at which that can go wrong.

Containers of two encodes are compared over the bytes of their streams: the 16-byte piece that holds a stream's first byte
is stored whole, and what it holds below the stream is whatever the group's ring held (as with the wave kernels' flushes).
Wall time on an MI355X: 12.7 s for the 21 cases of this file -- 6.0 s of it the `several` regime (81 925 calls of the oracle),
2.7 s the captured graph's child process, 1.7 s the first case's setup and 0.6 s its call (they load the kernels), 0.7 s the
`half` regime, 0.2 s the order test, 0.04 s and less for each of the others."""
import numpy as np
import pytest

from _batch import (NO_ZERO_OCTETS, Batch, check_bad_slots, check_encode_order, check_no_false_e_model, check_option_takes_zero_or_one,
                    check_other_shape_keeps_its_kernels, check_true_e_model, draw_lengths, draw_log_uniform, finish_octet, mandatory_lengths,
                    option_contexts, rate_octet, resident_waves, run_family_graph, run_row, same_result)
from _kernel_rows import ENC_GROUPS, EROW, OPT_BATCH_ENCODE_GROUPS, OPT_BATCH_GROUPS, ROW
from _oracle import FMT_WORD

WAVE = ENC_GROUPS.wave_kernel


@pytest.fixture(scope="module")
def gpu():
    yield from option_contexts(OPT_BATCH_ENCODE_GROUPS)


OCTETS = {
    "one-line-each": [128] * 8,
    "boundaries": [0, 1, 7, 8, 9, 127, 128, 129],
    "seven-dead-512-lines": [65536, 0, 0, 0, 0, 0, 0, 1],
    "every-group-finishes-elsewhere": [128 * (g + 1) + 5 * g for g in range(8)],
    "all-empty": [0] * 8,
    "second-octet-of-one": [300] * 9,
    "mandatory-and-200s": mandatory_lengths(8) + [200] * 7,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OCTETS))
def test_single_octets(gpu, oracle, name):
    """One or two octets: one line each and no tail; every line and tail boundary in one wave; seven groups dead for 512
    lines while one keeps flushing; every group finishing in another iteration with another tail; eight empty streams
    (32 bytes of flushed initial states each); a second octet of one stream; the mandatory lengths.  Each at sym_align 1
    (every symbol a round at a time, byte loads) and 4."""
    R, ctx, torch, _ = gpu
    b = Batch(R, ctx, torch, oracle, EROW, np.array(OCTETS[name], dtype=np.uint32))
    for align in (1, 4):
        run_row(b, align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_finish_hazard(gpu, oracle):
    """Every group finishes at a line boundary while others run on, and its free-running state emits (finish_octet): the
    write lands where the stream's last word went.  Every stream equals the oracle's -- in particular its last bytes written,
    the flushed states and the word below them (the stream's first 34 bytes)."""
    R, ctx, torch, _ = gpu
    freqs, counts, contents = finish_octet()
    b = Batch(R, ctx, torch, oracle, EROW, counts, contents=contents, freqs=freqs)
    cont, offs, lens = run_row(b, 4)[:3]
    h, h_offs = cont.cpu().numpy(), offs.cpu().numpy()
    for g in range(8):
        a = int(h_offs[g])
        assert b.lens[g] >= 34 and np.array_equal(h[a:a + 34], b.streams[g][:34]), ("states and last word of group", g)


@pytest.mark.gpu
def test_rate_extremes_in_one_wave(gpu, oracle):
    """rate_octet: 96 bytes per eight rounds beside streams that flush no block for a thousand rounds, and bursts, at
    different lengths, at sym_align 4 and 1."""
    R, ctx, torch, _ = gpu
    freqs, counts, contents = rate_octet()
    b = Batch(R, ctx, torch, oracle, EROW, counts, contents=contents, freqs=freqs)
    for align in (4, 1):
        run_row(b, align)
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_no_false_e_model_from_parked_groups(gpu, oracle):
    """A model without byte value 0, contents that never use it, uneven lengths: dead groups are fed zeros and read the
    record of byte value 0, which must not reach the flags.  encode_status() is OK (run_row asks) and every stream is the
    oracle's."""
    check_no_false_e_model(gpu, oracle, ENC_GROUPS, NO_ZERO_OCTETS)


@pytest.mark.gpu
def test_true_e_model_is_reported_and_contained(gpu, oracle):
    """The same batch with one symbol of one stream overwritten by 0 on the device: E_MODEL, as the default context reports
    for the same batch; every stream of the other octets is the oracle's; nothing is written outside the container."""
    check_true_e_model(gpu, oracle, ENC_GROUPS, NO_ZERO_OCTETS)


@pytest.mark.gpu
def test_order(gpu, oracle):
    """17 streams.  No order, the reversed identity and batch_order's result give the same streams, offsets and lengths; an
    order with one entry replaced by n_streams reports E_ARG, every stream still named is exact, and the stream that lost
    its position keeps its slot's poison and its pre-filled index entries.  The same on the default context and on a
    64-way batch, which report the wave kernel."""
    _, ctx, _, off = gpu
    counts = draw_lengths(17, 8, 23)
    for cx, row in ((ctx, EROW), (off, ROW["word-8"]), (ctx, ROW["word-64"])):
        check_encode_order(gpu, oracle, cx, row, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["half", "several"])
def test_half_and_several(gpu, oracle, regime):
    """half: fewer octets than the launch has resident waves, lengths log-uniform up to 64 Ki with the mandatory ones.
    several: at least 1.25 x as many octets as resident waves, so that waves come back for further claims and must reset
    x, c, fb and their rings; lengths log-uniform up to 1024 (the oracle's side stays in seconds).  The last octet of each
    is partial; sym_align = 4; then the same batch under batch_order's order: the same result."""
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
    b = Batch(R, ctx, torch, oracle, EROW, counts)
    cont, offs, lens, d_buf, d_sym, d_slot, sym_offs, slot_offs = run_row(b, 4, with_oracle_container=False)
    ordered = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, 8, d_slot, d_order=ctx.batch_order(b.d_counts))
    assert ctx.last_encode_kernel()[0] == EROW["encode"]
    ctx.encode_status()
    same_result(torch, (cont, offs, lens), ordered, b.n, "under batch_order")
    assert ctx.decode_errors() == 0


@pytest.mark.gpu
def test_bad_slots(gpu, oracle):
    """test_batch_encode_rejects_bad_slots' construction on the 8-way shape with the option on: every slot 32 bytes larger
    than its bound; a slot off 16 bytes on both sides (two streams), one a granule too small, one beyond out_cap -- each in
    an octet with valid streams.  E_SPACE, the rejected slots keep their poison and get lengths 0, every other stream is
    exact, the first 16 bytes of every accepted slot are still poison, nothing is written behind the container."""
    check_bad_slots(gpu, oracle, ENC_GROUPS)


@pytest.mark.gpu
@pytest.mark.parametrize("rid,n_streams", [("word-64", 20), ("word-u16-64", 20), ("word-8", 7), ("byte-2", 40)])
def test_other_shapes_keep_their_kernels_with_the_option_on(gpu, oracle, rid, n_streams):
    """64-way, u16 symbols, fewer than eight 8-way streams and the byte format take the wave-per-stream kernels on the
    context with the option on, and code right."""
    check_other_shape_keeps_its_kernels(gpu, oracle, ENC_GROUPS, rid, n_streams)


@pytest.mark.gpu
def test_option_takes_zero_or_one(gpu, oracle):
    """Any other value is E_ARG and changes nothing; 0 restores the wave-per-stream kernel, 1 the group kernel; the
    decoder's option alone leaves the encoder where it was."""
    off = gpu[3]
    b = check_option_takes_zero_or_one(gpu, oracle, ENC_GROUPS)
    off.set_option(OPT_BATCH_GROUPS, 1)
    try:
        d_buf, sym_offs, slot_offs = b.laid_out(4)
        off.encode_batch(off.model(FMT_WORD, b.freqs, 12), d_buf, b.dev(sym_offs, np.int64), b.d_counts, 8, b.dev(slot_offs, np.int64))
        assert off.last_encode_kernel()[0] == WAVE, off.last_encode_kernel()
        off.encode_status()
    finally:
        off.set_option(OPT_BATCH_GROUPS, 0)


@pytest.mark.gpu
def test_group_batch_encode_in_a_captured_graph(tmp_path):
    """One captured encode_batch of 3000 8-way streams with the option on: one eager call first, then three replays into a
    poison-refilled container, each equal to the eager result (stream bytes, offsets, lengths), in a child process under a
    time limit of its own.  Graph replay needs the process's default of four hardware queues: with GPU_MAX_HW_QUEUES set
    below that the test does not apply."""
    run_family_graph(tmp_path, ENC_GROUPS, "graph_batch_encode_groups.py")
