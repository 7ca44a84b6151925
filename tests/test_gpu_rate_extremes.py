"""The ragged-batch and ring decoders at the ends of the formats' stream rates: streams that take the most a valid stream
can (96 bytes per eight rounds of an 8-way word stream, 32 per eight rounds of a 2-way byte stream), streams that take
nothing for a thousand rounds, and bursts of both -- at every stream start phase, beside one another in one wave, and
under every model class the encoders' division-free update distinguishes.

tests/_stream_rate.py holds the models, the contents and a numpy model of the bytes every round takes;
tests/test_stream_rate_cpu.py proves without a GPU that the inputs built here reach the bounds named below, and that
RATE_CASES names every batch kernel.  Every check is against Oracle.encode or the input symbols, never the library
itself; output buffers are poison-filled with padding and a guard that must come back untouched (the helpers are
tests/test_gpu_batch.py's and tests/test_gpu_batch_groups.py's).

Two things differ from what one might expect:
  * the symbols that move a rare-only stream's lock-step pattern against the round numbers are its LAST 8 p symbols (the
    first the coder sees); in front of the stream they could not move anything (tests/_stream_rate.py says why);
  * under 3841 + 255 x 1 (here 3826 + 16 + 254 x 1) no input is silent for 1024 rounds -- a common symbol costs 0.093 bits
    (0.098), every state takes a word every 172 (162) rounds --, so every case of section a runs under a second model as
    well, 4065 + 16 + 15 x 1, whose common-only streams take nothing for 1400 rounds and more.

Wall time on an MI355X: 3.9 s for the 80 cases of this file -- 1.9 s of it the first case's setup and 0.7 s its call (they
load the kernels), 0.01 to 0.04 s for each of the others."""
import numpy as np
import pytest

import _stream_rate as S
from _batch import GUARD, POISON, Batch, mandatory_lengths, run_row
from _kernel_rows import BATCH_ROWS, GROUP_ROWS, GROW, OPT_BATCH_GROUPS
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

# ---- section a: k_decode_batch_word_groups, rate x phase x parking --------------------------------------------------
A_MODELS = {"3826-16-254x1": S.rate_model_16, "4065-16-15x1": S.quiet_model}
A_KINDS = ("rare+0", "rare+1", "rare+2", "rare+3", "common", "bursts", "zipf")
A_COUNTS = tuple(128 * b + t for b in (0, 1, 5) for t in (0, 1, 77, 127))
A_STREAMS = 64
A_BATCHES = len(A_KINDS)  # stream k of batch j holds kind (k + j) mod 7: every kind at every phase


def a_phase(k):
    return (2 * k) % 128


def a_kind(j, k):
    return A_KINDS[(k + j) % len(A_KINDS)]


def a_count(j, k):
    return A_COUNTS[(5 * k + j + k // 12) % len(A_COUNTS)]


def a_content(freqs, kind, n, seed):
    if kind.startswith("rare+"):
        return S.rare_only(freqs, n, seed, shift=int(kind[5:]))
    if kind == "common":
        return S.common_only(freqs, n)
    if kind == "bursts":
        return S.bursts(freqs, n, seed, lead=8 * (seed % 8))  # (the runs start at every round modulo 8)
    return S.zipf_under(freqs, n, seed)


def a_batch(model, j):
    """-> (freqs, counts, {stream: symbols}, phases) of batch j of section a."""
    freqs = A_MODELS[model]()
    counts = np.array([a_count(j, k) for k in range(A_STREAMS)], dtype=np.uint32)
    contents = {k: a_content(freqs, a_kind(j, k), int(counts[k]), 100 * j + k) for k in range(A_STREAMS)}
    return freqs, counts, contents, [a_phase(k) for k in range(A_STREAMS)]


# one wave each: a fast group beside parked ones, and a stalled cursor beside draining ones
A_WAVES = {
    "fast-beside-parked": ([65536, 0, 0, 0, 0, 0, 0, 1], ["rare+0"] * 8),
    "stalled-beside-draining": ([65536] + [128 * (g + 1) for g in range(7)], ["common"] + ["rare+%d" % (g % 4) for g in range(7)]),
}


def a_wave(model, name):
    freqs = A_MODELS[model]()
    counts, kinds = A_WAVES[name]
    contents = {k: a_content(freqs, kinds[k], counts[k], 900 + k) for k in range(8)}
    return freqs, np.array(counts, dtype=np.uint32), contents, [(34 * k + 6) % 128 for k in range(8)]


# ---- section b: the uniform ring decoders at every phase and the rate bound -------------------------------------------
B_CHUNKS = 64
B_CASES = {
    # id: (fmt, scale_bits, interleave, chunk, content, phase modulus, decoder, compact encoder)
    "word-groups-rare": (FMT_WORD, 12, 8, 1024 + 36, "rare", 128, "k_decode_word_groups", "k_encode_word_groups"),
    "word-groups-bursts": (FMT_WORD, 12, 8, 1024 + 36, "bursts", 128, "k_decode_word_groups", "k_encode_word_groups"),
    "word-groups-common": (FMT_WORD, 12, 8, 1024 + 36, "common", 128, "k_decode_word_groups", "k_encode_word_groups"),
    "byte-pairs-16bit-mod32": (FMT_BYTE, 16, 2, 256 + 4, "rare", 32, "k_decode_byte_pairs", "k_encode_lanes16"),
    "byte-pairs-16bit-mod64": (FMT_BYTE, 16, 2, 256 + 4, "rare", 64, "k_decode_byte_pairs", "k_encode_lanes16"),
    "byte-pairs-14bit-mod32": (FMT_BYTE, 14, 2, 256 + 4, "rare", 32, "k_decode_byte_pairs", "k_encode_lanes16"),
    "byte-pairs-14bit-mod64": (FMT_BYTE, 14, 2, 256 + 4, "rare", 64, "k_decode_byte_pairs", "k_encode_lanes16"),
    "byte-pairs-16bit-common": (FMT_BYTE, 16, 2, 256 + 4, "common", 32, "k_decode_byte_pairs", "k_encode_lanes16"),
}


def b_case(bid):
    """-> (freqs, [the symbols of chunk c], phases).  Word format: chunk c is rare-only with c mod 4 shifting symbols per state
    behind it, or bursts whose runs start at round c mod 8, at offset == 2 c (mod 128).  Byte format: frequency-1 symbols
    only, chunk c at offset == c (mod 32 / 64)."""
    fmt, sb, ways, chunk, content, modulus = B_CASES[bid][:6]
    if fmt == FMT_WORD:
        freqs = S.rate_model_16()
        if content == "rare":
            data = [S.rare_only(freqs, chunk, 300 + c, shift=c % 4) for c in range(B_CHUNKS)]
        elif content == "bursts":
            data = [S.bursts(freqs, chunk, 400 + c, lead=8 * (c % 8)) for c in range(B_CHUNKS)]
        else:
            data = [S.common_only(freqs, chunk) for c in range(B_CHUNKS)]
        return freqs, data, [(2 * c) % modulus for c in range(B_CHUNKS)]
    freqs = np.ones(256, dtype=np.uint32)
    freqs[S.COMMON] = (1 << sb) - 255
    if content == "rare":
        data = [S.rare_only(freqs, chunk, 500 + c) for c in range(B_CHUNKS)]
    else:
        data = [S.common_only(freqs, chunk) for c in range(B_CHUNKS)]
    return freqs, data, [c % modulus for c in range(B_CHUNKS)]


# ---- section c: every batch row under the model classes ---------------------------------------------------------------
C_ROWS = list(BATCH_ROWS) + list(GROUP_ROWS)
C_STREAMS = 40
C_KINDS = ("rare", "common", "bursts", "drawn")


def c_one_symbol(row):
    """A one-symbol model (frequency 2^scale_bits) is inside the working range of the byte and rans64 coders and of the alias
    coder below 16 bits; the word format's threshold wraps."""
    return row["fmt"] in (FMT_BYTE, FMT_R64) or (row["fmt"] == FMT_ALIAS and row["sb"] < 16)


def c_classes(row):
    return S.class_models(row["sb"], row["K"], c_one_symbol(row))


def c_counts(ways):
    must = [4 * ways * 16 + 3 if v == 65536 else v for v in mandatory_lengths(ways)]
    return np.array([must[k % len(must)] for k in range(C_STREAMS)], dtype=np.uint32)


def c_content(freqs, kind, n, seed):
    if kind == "rare":
        return S.rare_only(freqs, n, seed)
    if kind == "common":
        return S.common_only(freqs, n)
    if kind == "bursts":
        return S.bursts(freqs, n, seed)
    return S.drawn(freqs, n, seed)


def c_batch(row, freqs):
    counts = c_counts(row["ways"])
    return counts, {k: c_content(freqs, C_KINDS[k % len(C_KINDS)], int(counts[k]), 700 + k) for k in range(C_STREAMS)}


# ---- the case table: which kernel names this file asserts under a rare-only and under a common-only stream --------------
def _rate_cases():
    cases = [{"section": "a", "id": "groups-" + m, "kernels": (GROW["decode"], GROW["encode"], "k_decode_batch<word>"),
              "contents": ("rare", "common", "bursts", "zipf")} for m in A_MODELS]
    for bid, c in B_CASES.items():
        cases.append({"section": "b", "id": bid, "kernels": (c[6], c[7]), "contents": (c[4],)})
    for row in C_ROWS:
        cases.append({"section": "c", "id": row["id"], "kernels": (row["decode"], row["encode"]), "contents": C_KINDS})
    return cases


RATE_CASES = _rate_cases()


def kernels_under(content):
    return {k for c in RATE_CASES if content in c["contents"] for k in c["kernels"]}


# ---- the GPU part -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    # (tests/test_gpu_batch_groups.py's fixture; a fixture of another test module cannot be imported without running that
    #  module's contexts beside these)
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    on = R.Context(0)
    on.set_option(OPT_BATCH_GROUPS, 1)
    off = R.Context(0)  # the option at its default: the wave-per-stream kernels
    yield R, on, torch, off
    off.close()
    on.close()


def decode_everywhere(b, off, align, phases):
    """One encode_batch (every stream == the oracle's, at its slot's end), then decode_batch of the GPU's container, of the
    oracle's shuffled one and of the oracle's streams packed at `phases` (mod 128), each with and without batch_order's
    order, on the context with the group option and on the one without: the laid-out input every time, poison included."""
    R, ctx, torch, row = b.R, b.ctx, b.torch, b.row
    ways = row["ways"]
    d_buf, sym_offs, slot_offs = b.laid_out(align)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, ways, d_slot)
    assert ctx.last_encode_kernel()[0] == row["encode"] and ctx.last_encode_placement() == 2, ctx.last_encode_kernel()
    ctx.encode_status()
    h_offs, h_lens = offs.cpu().numpy().astype(np.uint64)[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n]
    assert np.array_equal(h_offs + h_lens, slot_offs[1:]), "a stream does not end at its slot's end"
    b.check_streams(cont.cpu().numpy(), h_offs, h_lens, "encode_batch align %d" % align)
    o_cont, o_starts, o_bytes = b.oracle_container()
    p_cont, p_starts, p_bytes = S.pack_at_phases(b.streams, phases, 128, order=np.random.default_rng(11).permutation(b.n))
    d_lens = b.dev(b.lens, np.int32)
    containers = (("gpu", cont, int(slot_offs[-1]), offs, lens),
                  ("oracle", b.dev(o_cont, np.uint8), o_bytes, b.dev(o_starts, np.int64), d_lens),
                  ("phases", b.dev(p_cont, np.uint8), p_bytes, b.dev(p_starts, np.int64), d_lens))
    gm_off = off.model(row["fmt"], b.freqs, row["sb"])
    d_order = ctx.batch_order(b.d_counts)
    for cx, gm, kernel in ((ctx, b.gm, row["decode"]), (off, gm_off, "k_decode_batch<word>")):
        for name, c, nbytes, o, ln in containers:
            for order in (None, d_order):
                out = torch.full_like(d_buf, b.poison())
                cx.decode_batch(gm, c, nbytes, o, ln, d_sym, b.d_counts, ways, out, d_order=order)
                assert cx.last_decode_kernel() == kernel, (cx.last_decode_kernel(), name)
                assert torch.equal(out, d_buf), (kernel, name, "align", align, "order" if order is not None else "no order")
                assert cx.decode_errors() == 0, (kernel, name)
    assert d_buf.numel() == int(sym_offs[-1]) + GUARD


def _a_cases():
    for model in A_MODELS:
        for j in range(A_BATCHES):
            yield pytest.param(model, j, id="%s-batch%d" % (model, j), marks=pytest.mark.gpu)
        for name in A_WAVES:
            yield pytest.param(model, name, id="%s-%s" % (model, name), marks=pytest.mark.gpu)


@pytest.mark.parametrize("model,which", list(_a_cases()))
def test_group_batch_decoder_rate_phase_parking(gpu, oracle, model, which):
    """k_decode_batch_word_groups.  Batches 0..6: 64 streams, stream k of the phase-packed container at offset == 2 k (mod 128)
    -- all 64 even phases, the eight states straddling the first 128-byte block from phase 98 on --, its content kind
    (k + j) mod 7 of rare-only with 0..3 shifting symbols per state, common-only, bursts, Zipf, its count one of 128 b + t,
    b in {0, 1, 5}, t in {0, 1, 77, 127}: over the seven batches every kind meets every phase and every count.  Rare-only
    streams take 96 bytes in every window of eight rounds, the refill's bound; the groups of one wave differ in kind and
    count.  The two single waves: 65536 rare-only symbols beside six empty streams and one symbol, and 65536 common-only
    symbols (a cursor that stands still for hundreds of rounds) beside seven rare-only streams of 128 (g + 1) symbols that
    park one after the other.  Each at sym_align 4 and 1, with and without batch_order, from three containers; the context
    without the option decodes the same bytes through k_decode_batch<word>."""
    R, ctx, torch, off = gpu
    freqs, counts, contents, phases = a_batch(model, which) if isinstance(which, int) else a_wave(model, which)
    b = Batch(R, ctx, torch, oracle, GROW, counts, contents=contents, freqs=freqs)
    for align in (4, 1):
        decode_everywhere(b, off, align, phases)


@pytest.mark.gpu
@pytest.mark.parametrize("bid", list(B_CASES))
def test_uniform_ring_decoders_rate_times_phase(gpu, oracle, bid):
    """k_decode_word_groups: 64 chunks of 1024 + 36 symbols, chunk c at offset == 2 c (mod 128) of a container packed by hand;
    rare-only (96 bytes per eight rounds) with c mod 4 shifting symbols per state, then bursts.  k_decode_byte_pairs: 64
    chunks of 256 + 4 frequency-1 symbols, chunk c at offset == c (mod 32) and (mod 64); at scale_bits = 16 every state
    takes two bytes in every round, 32 bytes per eight rounds, the ring's bound sustained (the library takes this model
    for the pair decoder); at 14 bits the window maximum is 28.  Then the GPU's own compact encode of the same symbols:
    every chunk == the oracle's stream, and its decode."""
    R, _, torch, ctx = gpu
    fmt, sb, ways, chunk, _, modulus, dec_kernel, enc_kernel = B_CASES[bid]
    freqs, data, phases = b_case(bid)
    om, gm = oracle.model(freqs, sb), ctx.model(fmt, freqs, sb)
    streams = [oracle.encode(fmt, om, d, ways) for d in data]
    cont, starts, nbytes = S.pack_at_phases(streams, phases, modulus)
    whole = np.concatenate(data)
    lens = np.array([s.size for s in streams], dtype=np.int32)
    back = torch.full((whole.size + 256,), POISON, dtype=torch.uint8, device="cuda")
    out = back[128:128 + whole.size]
    d_offs = torch.from_numpy(np.concatenate((starts, [nbytes])).astype(np.int64)).cuda()
    ctx.decode(gm, torch.from_numpy(cont).cuda(), nbytes, d_offs, torch.from_numpy(lens).cuda(), whole.size, ways, chunk, d_out=out)
    assert ctx.last_decode_kernel() == dec_kernel, ctx.last_decode_kernel()
    assert ctx.decode_errors() == 0
    host = back.cpu().numpy()
    assert np.array_equal(host[128:128 + whole.size], whole), "decode of the container packed by hand"
    assert (host[:128] == POISON).all() and (host[128 + whole.size:] == POISON).all(), "written outside the output"
    # the GPU's own compact container
    g_cont, g_offs, g_lens, total = ctx.encode(gm, torch.from_numpy(whole).cuda(), ways, chunk)
    assert ctx.last_encode_kernel()[0] == enc_kernel, ctx.last_encode_kernel()
    ctx.encode_status()
    h, h_offs, h_lens = g_cont[:total].cpu().numpy(), g_offs.cpu().numpy(), g_lens.cpu().numpy()
    assert np.array_equal(h_lens[:B_CHUNKS].astype(np.int64), lens.astype(np.int64)), "lengths differ from the oracle's"
    for c in range(B_CHUNKS):
        assert np.array_equal(h[int(h_offs[c]):int(h_offs[c]) + int(lens[c])], streams[c]), ("chunk", c)
    back.fill_(POISON)
    ctx.decode(gm, g_cont, total, g_offs, g_lens, whole.size, ways, chunk, d_out=out)
    assert ctx.last_decode_kernel() == dec_kernel, ctx.last_decode_kernel()
    assert ctx.decode_errors() == 0
    host = back.cpu().numpy()
    assert np.array_equal(host[128:128 + whole.size], whole), "decode of the GPU's own container"
    assert (host[:128] == POISON).all() and (host[128 + whole.size:] == POISON).all(), "written outside the output"


def _c_cases():
    for row in C_ROWS:
        for name, _ in c_classes(row):
            yield pytest.param(row, name, id="%s-%s" % (row["id"], name), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,cls", list(_c_cases()))
def test_batch_rows_under_the_model_classes(gpu, oracle, row, cls):
    """Every row of BATCH_ROWS and GROUP_ROWS under a model that is all-but-one frequency 1, powers of two, M/2 + 1 and M/2 - 1,
    3 / 5 / 7 / ..., and (byte, rans64) one symbol: 40 streams of the mandatory lengths (65536 replaced by 64 N + 3), contents
    rare-only / common-only / bursts / drawn from the model in turn.  encode_batch: every stream == Oracle.encode, at its
    slot's end; decode_batch of the GPU's and the oracle's container; sym_align 1 and 4 (run_row; every decode_batch in it
    is a synchronous call, which raises by itself when a stream fails and resets the count decode_errors() reads).  Every
    class that has symbols without a record -- all but the first: such a symbol in one stream is E_MODEL, and the next call
    on the context succeeds."""
    R, on, torch, off = gpu
    ctx = on if row["decode"] == GROW["decode"] else off
    freqs = dict(c_classes(row))[cls]
    counts, contents = c_batch(row, freqs)
    b = Batch(R, ctx, torch, oracle, row, counts, contents=contents, freqs=freqs)
    for align in (1, 4):
        run_row(b, align)
        assert ctx.decode_errors() == 0
    if not np.any(freqs == 0):
        return
    d_buf, sym_offs, slot_offs = b.laid_out(4)
    d_sym, d_slot = b.dev(sym_offs, np.int64), b.dev(slot_offs, np.int64)
    victim = int(np.argmax(counts))
    stray = int(np.nonzero(freqs == 0)[0][0])
    bad = d_buf.clone()
    bad[int(sym_offs[victim]) + int(counts[victim]) // 2] = stray
    ctx.encode_batch(b.gm, bad, d_sym, b.d_counts, row["ways"], d_slot)
    with pytest.raises(R.RansAmdError) as e:
        ctx.encode_status()
    assert e.value.status == R.E_MODEL
    cont, offs, lens = ctx.encode_batch(b.gm, d_buf, d_sym, b.d_counts, row["ways"], d_slot)
    assert ctx.last_encode_kernel()[0] == row["encode"], ctx.last_encode_kernel()
    ctx.encode_status()
    b.check_streams(cont.cpu().numpy(), offs.cpu().numpy().astype(np.uint64)[:b.n], lens.cpu().numpy().view(np.uint32)[:b.n], "after E_MODEL")
