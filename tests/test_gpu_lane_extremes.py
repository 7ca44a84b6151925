"""The lane-per-chunk kernels at the ends of the formats' stream rates, lane beside lane: one chunk per lane, 64 chunks per
wave, and in one wave lanes that take the most a valid stream can (frequency-1 symbols only: 2 scale_bits bytes per
16-symbol group), lanes that take nothing for the whole chunk, bursts of both and symbols drawn from the model.

The lane kernels have no ragged form, so the batch work of tests/test_gpu_rate_extremes.py never reached them; their input
so far was Zipf under its own model (about a byte per symbol in every lane) and one rare-only input in which all 64 lanes
hold the same kind of chunk.  Their correctness rests on per-lane invariants at a 16-symbol group boundary -- the staged
decoder's "at least 64 bytes ahead", k_decode_lanes_r64x2's ">= 48 B ahead" with its side path for the whole wave when any
lane is short and the pieces parked per fetch instruction under lane masks, the staged encoders' "a line that has filled
up" per lane, k_encode_lanes_r64x2's bytes derived from the ring position -- and on hand-written arithmetic that had seen
three normalised histograms.

tests/_stream_rate.py holds the models, the contents of a grid of chunks (vectorised) and the numpy model of the bytes
every round takes; tests/test_lane_rate_cpu.py proves without a GPU that the inputs built here sit where this file says
and that LANE_CASES names every lane kernel.  Every comparison is against Oracle.encode / bench.oracle_check_chunks / the
input symbols, never the library; every decode of this file goes into a poison-filled buffer with a guard in front and
behind; after every call the kernel the library reports is asserted, and decode_errors() == 0 after every healthy decode.

What a wave holds: S.lane_patterns(), 35 waves -- rotating (lane l holds kind (l + r) mod 5), quad-mates-differ ([rare,
common, bursts, drawn] x 16 and its rotations: the four lanes that fetch one another's lines and park one another's
pieces), one rare lane among 63 common ones (lane 0..3 of a first, a middle and the last quad), one common lane among 63
rare ones, all rare, all common.  Batch b of every input holds pattern b mod 35, so ONE launch runs all of them; the last
batch has 37 chunks and the last chunk is ragged: lanes without a chunk sit beside the extremes.

  section a  LANE_ROWS x chunk sizes, 35 batches and a part: the decoder from three containers (the GPU's own compact one,
             the oracle's, the oracle's streams packed with every lane at its own offset modulo 128), k_encode_lanes16 in
             the compact, slot and sized layouts
  section b  LANE_ROWS at six batches per CU (one for k_encode_lanes_r64x2): the staged encoders in every layout and under
             OPT_LANE_FUSED_PLACEMENT, the decoders on what they made
  section c  LANE_ROWS under the model classes of the encoders' division-free update, both directions, both sizes; a symbol
             without a record is E_MODEL -- for k_encode_lanes_r64x2 at each of the four tracked record registers
  section d  thresholds: a largest frequency of 4095 / 4096 (packed slot records), scale_bits 7 and 16 in both r64x2 kernels,
             a one-symbol model (frequency 2^16) through k_encode_lanes_r64x2, k_decode_lanes on chunks of 2^19 + 2 symbols

What the cases are tight against (mutated builds of the library, one at a time, never committed): the format's own
maximum of 32 bytes per group, not the kernels' looser figures.  The staged decoder's refill threshold lowered from 64
to 32 bytes ahead and k_decode_lanes_r64x2's side-path threshold lowered from 48 to 40 decode every valid stream -- no
stream takes more than 32 bytes per group, and the r64x2 window reads 8 ahead --, and every case here passes on them; at 31
and at 36, one unit below what a valid stream needs, the rare-only lanes of the 16-bit rows fail (byte-1-16bit, alias256-8
and byte-2-16bit-261 in sections a and c; r64-2-16bit in sections a and c: the phase-packed container, where lanes start
at every offset).  E64_FRONT's v_cmpx_gt made ge fails the one-symbol cases (a record with cmpl = 0); packed records
built for a frequency of 4096 fail test_packed_slot_records_at_4095_and_4096[13-4096] and [14-4096].

Wall time on an MI355X: 36.6 s for the 132 cases of this file (tests/test_gpu_rate_extremes.py in the same session: 3.3 s for
its 80) -- 1.5 s of it the first case's setup; the slowest case is test_per_lane_register_window_decoder[all-rare] at 1.0 s
(32 Mi symbols through one wave of k_decode_lanes), the cases at six batches per CU take 0.3 to 0.5 s, those of section a
0.1 to 0.2 s."""
import numpy as np
import pytest

import _stream_rate as S
from _batch import GUARD, POISON
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

OPT_LANE_FUSED_PLACEMENT = 1  # (ryg_rans_amd.OPT_LANE_FUSED_PLACEMENT; the number is the ABI's, tests/test_abi.py)

D_ST, D_RX, D_RXP, D_L, D_BP = ("k_decode_lanes_staged", "k_decode_lanes_r64x2", "k_decode_lanes_r64x2<packed slots>", "k_decode_lanes",
                                "k_decode_byte_pairs")
E_ST, E_L16, E_RX = "k_encode_lanes_staged", "k_encode_lanes16", "k_encode_lanes_r64x2"
W_WORD, W_BYTE, W_R64, W_ALIAS = "k_encode<word>", "k_encode<byte>", "k_encode<r64>", "k_encode<alias, LDS remap>"

PART = 37  # chunks of the last batch
SMALL_BATCHES = len(S.lane_patterns())  # section a: every pattern once


def _lane(rid, fmt, sb, ways, model, decode, big, wave, lanes_decoder=True):
    """decode: the decoder of chunks of a multiple of 64 symbols; big: the encoder from `per_cu` batches per CU on; wave: the
    wave encoder sized slots fall to below that (k_encode_lanes16 cannot tell that a chunk does not fit)."""
    return {"id": rid, "fmt": fmt, "sb": sb, "ways": ways, "K": 256, "model": model, "decode": decode, "big": big, "wave": wave,
            "per_cu": 1 if big == E_RX else 6, "lanes_decoder": lanes_decoder}


LANE_ROWS = [
    _lane("word-4-rate", FMT_WORD, 12, 4, S.rate_model_16, D_ST, E_ST, W_WORD),
    _lane("word-4-quiet", FMT_WORD, 12, 4, S.quiet_model, D_ST, E_ST, W_WORD),
    _lane("byte-1-14bit", FMT_BYTE, 14, 1, lambda: S.lane_model(14), D_ST, E_ST, W_BYTE),
    _lane("byte-1-16bit", FMT_BYTE, 16, 1, lambda: S.lane_model(16), D_ST, E_ST, W_BYTE),
    _lane("alias256-8", FMT_ALIAS, 16, 8, lambda: S.lane_model(16), D_ST, E_ST, W_ALIAS),
    _lane("r64-1", FMT_R64, 14, 1, lambda: S.lane_model(14), D_ST, E_ST, W_R64),
    # (encoder rows: the decoder of this layout is k_decode_byte_pairs, covered by tests/test_gpu_rate_extremes.py -- but for
    #  chunks that are no multiple of 4 symbols, which the staged lane decoder takes)
    _lane("byte-2-14bit", FMT_BYTE, 14, 2, lambda: S.lane_model(14), D_BP, E_ST, W_BYTE, lanes_decoder=False),
    _lane("byte-2-16bit", FMT_BYTE, 16, 2, lambda: S.lane_model(16), D_BP, E_ST, W_BYTE, lanes_decoder=False),
    _lane("r64-2-12bit-packed", FMT_R64, 12, 2, lambda: S.lane_model(12), D_RXP, E_RX, W_R64),
    _lane("r64-2-14bit-packed", FMT_R64, 14, 2, S.packed_model_14, D_RXP, E_RX, W_R64),
    _lane("r64-2-14bit", FMT_R64, 14, 2, lambda: S.lane_model(14), D_RX, E_RX, W_R64),  # (a frequency above 4095: no packed records)
    _lane("r64-2-16bit", FMT_R64, 16, 2, lambda: S.lane_model(16), D_RX, E_RX, W_R64),
]
ROW = {r["id"]: r for r in LANE_ROWS}


def is_r64x2(row):
    return row["big"] == E_RX


def small_sizes(row):
    """64, 192 (three trips: a pair and a single one in the r64x2 decoder's paired stores) and 256 for every row; 272 (a
    multiple of 16, not of 64) and 256 + 5 (the staged decoder's element-wise tail; k_encode_lanes16 at any count) for the
    rows whose kernels take them -- the r64x2 kernels take multiples of 64 alone."""
    return (64, 192, 256) if is_r64x2(row) else (64, 192, 256, 272, 261)


def wrap_chunk(row):
    """The smallest multiple of 64 symbols whose rare-only stream -- 2 scale_bits bytes per 16 symbols and the flushed states
    -- is longer than the 128-byte ring."""
    states = row["ways"] * S.STATE_BYTES[row["fmt"]]
    chunk = 64
    while chunk // 16 * 2 * row["sb"] + states <= 128:
        chunk += 64
    return chunk


def big_sizes(row):
    return (wrap_chunk(row),) if is_r64x2(row) else (wrap_chunk(row), 272)


def decoder_of(row, chunk):
    if is_r64x2(row) or row["lanes_decoder"]:
        return row["decode"]
    return D_BP if chunk % 4 == 0 else D_ST


def expect_small(row, chunk):
    """Fewer batches than the staged encoders want: k_encode_lanes16; sized slots: the wave encoder."""
    return {"decode": decoder_of(row, chunk), "encode": (E_L16, 0), "slots": (E_L16, 2), "sized": (row["wave"], 2)}


def expect_big(row, chunk):
    return {"decode": decoder_of(row, chunk), "encode": (row["big"], 0), "slots": (row["big"], 2), "sized": (row["big"], 2)}


def geometry(full_batches, chunk):
    """-> (chunks, symbols): `full_batches` whole batches, a last batch of PART chunks, the last chunk ragged."""
    nchunks = 64 * full_batches + PART
    return nchunks, (nchunks - 1) * chunk + chunk // 3 + 1


def lane_input(freqs, kinds_of, full_batches, chunk, seed):
    """-> (symbols, kind per chunk)"""
    nchunks, n = geometry(full_batches, chunk)
    kinds = kinds_of(nchunks)
    return S.chunk_grid(freqs, kinds, chunk, seed).reshape(-1)[:n], kinds


def one_symbol_ok(row):
    """(tests/test_gpu_rate_extremes.py c_one_symbol)"""
    return row["fmt"] in (FMT_BYTE, FMT_R64) or (row["fmt"] == FMT_ALIAS and row["sb"] < 16)


def classes_of(row):
    return S.class_models(row["sb"], row["K"], one_symbol_ok(row))


def class_rows():
    """The rows that differ in more than their model (section c brings its own)."""
    seen, out = set(), []
    for row in LANE_ROWS:
        key = (row["fmt"], row["sb"], row["ways"])
        if key not in seen:
            seen.add(key)
            out.append(row)
    return out


def class_row(row, freqs):
    """The row under another model: the 2-way rans64 decoder reads packed slot records where the model has them -- scale_bits
    <= 14 and no frequency above 4095 (model.h)."""
    if not is_r64x2(row):
        return row
    return dict(row, decode=D_RXP if row["sb"] <= 14 and int(np.max(freqs)) <= 4095 else D_RX)


# ---- section d's inputs -------------------------------------------------------------------------------------------------
R64X2 = {"fmt": FMT_R64, "ways": 2, "big": E_RX, "wave": W_R64, "per_cu": 1, "lanes_decoder": True}
D_TOP = [(sb, top) for sb in (13, 14) for top in (4095, 4096)]
D_BITS = [(sb, cls) for sb in (7, 16) for cls in ("all-but-one-1", "above-and-below-half")]
HUGE_CHUNK = (1 << 19) + 2
HUGE_PATTERNS = ("quad-mates-differ-0", "all-rare", "all-common")


def top_row(sb, top):
    return dict(R64X2, id="r64-2-%dbit-top-%d" % (sb, top), sb=sb, K=256, decode=D_RXP if top <= 4095 else D_RX,
                model=lambda: S.top_frequency_model(sb, top))


def bits_row(sb, cls):
    return dict(R64X2, id="r64-2-%dbit-%s" % (sb, cls), sb=sb, K=64, decode=D_RXP if sb <= 14 else D_RX,
                model=lambda: dict(S.class_models(sb, 64, False))[cls])


def one_symbol_row():
    return dict(R64X2, id="r64-2-16bit-one-symbol", sb=16, K=256, decode=D_RX, model=lambda: dict(S.class_models(16, 256, True))["one-symbol"])


def rare_and_drawn(nchunks):
    return S.turn_kinds(nchunks, (S.RARE, S.DRAWN))


def rare_and_common(nchunks):
    return S.turn_kinds(nchunks, (S.RARE, S.COMMON_K))


# ---- the case table: which kernel names this file asserts, under which inputs -------------------------------------------
ALL_INPUTS = ("rare", "common", "mixed")  # S.pattern_kinds: all-rare, all-common and 33 mixed waves in every launch


def _lane_cases():
    cases = []
    for row in LANE_ROWS:
        for chunk in small_sizes(row):
            cases.append({"section": "a", "id": "%s-%d" % (row["id"], chunk), "kernels": (decoder_of(row, chunk), E_L16), "inputs": ALL_INPUTS})
        for chunk in big_sizes(row):
            cases.append({"section": "b", "id": "%s-%d" % (row["id"], chunk), "kernels": (decoder_of(row, chunk), row["big"]),
                          "inputs": ALL_INPUTS})
    for row in class_rows():
        for name, freqs in classes_of(row):
            cases.append({"section": "c", "id": "%s-%s" % (row["id"], name), "kernels": (decoder_of(class_row(row, freqs), 64), row["big"], E_L16),
                          "inputs": ("mixed",)})
    for sb, top in D_TOP:
        cases.append({"section": "d", "id": top_row(sb, top)["id"], "kernels": (top_row(sb, top)["decode"], E_L16), "inputs": ("mixed",)})
    for sb, cls in D_BITS:
        cases.append({"section": "d", "id": bits_row(sb, cls)["id"], "kernels": (bits_row(sb, cls)["decode"], E_RX), "inputs": ("mixed",)})
    cases.append({"section": "d", "id": one_symbol_row()["id"], "kernels": (D_RX, E_RX), "inputs": ("common",)})
    for pat in HUGE_PATTERNS:
        cases.append({"section": "d", "id": "byte-2-huge-chunks-" + pat, "kernels": (D_L, E_L16),
                      "inputs": ({"all-rare": "rare", "all-common": "common"}.get(pat, "mixed"),)})
    return cases


LANE_CASES = _lane_cases()


def kernels_under(inp, cases=None):
    return {k for c in (LANE_CASES if cases is None else cases) if inp in c["inputs"] for k in c["kernels"]}


# ---- the GPU part -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    fused = R.Context(0)  # (its own context: options must not leak)
    fused.set_option(OPT_LANE_FUSED_PLACEMENT, 1)
    yield R, ctx, torch, fused
    fused.close()
    ctx.close()


def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def guarded_decode(ctx, torch, gm, row, chunk, h_syms, what, d_cont, nbytes, d_offs, d_lens, kernel):
    """One decode into a poison-filled buffer with GUARD symbols in front and behind -> the output == the input, the guards
    untouched, the kernel the one expected, no chunk flagged."""
    n = h_syms.size
    back = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ctx.decode(gm, d_cont, nbytes, d_offs, d_lens, n, row["ways"], chunk, d_out=back[GUARD:GUARD + n])
    assert ctx.last_decode_kernel() == kernel, (what, ctx.last_decode_kernel(), "expected", kernel)
    assert ctx.decode_errors() == 0, what
    host = back.cpu().numpy()
    got = host[GUARD:GUARD + n]
    if not np.array_equal(got, h_syms):
        first = int(np.nonzero(got != h_syms)[0][0])
        raise AssertionError((row["id"], what, "first wrong symbol", first, "chunk", first // chunk, "lane", (first // chunk) % 64,
                              "batch", first // chunk // 64, "symbol of the chunk", first % chunk))
    assert (host[:GUARD] == POISON).all() and (host[GUARD + n:] == POISON).all(), (what, "written outside the output")


def run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, kernels, phases=True, fused_batches_ok=False):
    """Every layout of the encoder the shape gets (tests/_every_chunk.py: every chunk == the oracle's stream, the index follows
    the layout's rule, every container decodes, the decoder also on the oracle's container), then the decoder into guarded
    buffers from the GPU's compact container, the oracle's, and the oracle's streams packed at S.lane_phases; under
    OPT_LANE_FUSED_PLACEMENT the compact layout once more, placed by the coder itself where the launcher fuses."""
    import bench
    from _every_chunk import check_every_chunk
    R, ctx, torch, fused = gpu
    fmt, sb, ways, K = row["fmt"], row["sb"], row["ways"], row["K"]
    n = h_syms.size
    nchunks = (n + chunk - 1) // chunk
    d_syms = torch.from_numpy(h_syms).cuda()
    gm = ctx.model(fmt, freqs, sb)
    # sized slots where a tight slot is smaller than the worst-case one (_every_chunk.py asserts as much)
    sized = ctx.tight_slot_bytes(gm, ways, chunk) < R.slot_bytes(fmt, n, ways, chunk)
    art = check_every_chunk(R, ctx, torch, fmt, sb, K, ways, chunk, n, kernels=kernels, damaged=False, sized=sized, sized_ratio=None,
                            all_overflow_at_half=False, d_syms=d_syms, freqs=freqs)
    assert ctx.decode_errors() == 0
    dec = kernels["decode"]
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the GPU's compact container", art["cont"], art["total"], art["offs"], art["lens"], dec)
    om = oracle.model(freqs, sb, with_alias=(fmt == FMT_ALIAS))
    o_cont, o_offs, o_lens = oracle.encode_chunked_mt(fmt, om, h_syms, ways, chunk, align=16)
    d_lens = torch.from_numpy(o_lens.astype(np.int32)).cuda()
    d_cont = torch.from_numpy(np.concatenate((o_cont, np.zeros(64, np.uint8)))).cuda()
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the oracle's container", d_cont, o_cont.size,
                   torch.from_numpy(o_offs.astype(np.int64)).cuda(), d_lens, dec)
    if phases:
        streams = [o_cont[int(o_offs[c]):int(o_offs[c]) + int(o_lens[c])] for c in range(nchunks)]
        p_cont, p_starts, p_bytes = S.pack_at_phases(streams, S.lane_phases(nchunks, S.UNIT[fmt]), 128)
        guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the oracle's streams at every phase", torch.from_numpy(p_cont).cuda(), p_bytes,
                       torch.from_numpy(np.concatenate((p_starts, [p_bytes])).astype(np.int64)).cuda(), d_lens, dec)
    # the compact layout under OPT_LANE_FUSED_PLACEMENT: placement 1 where the staged kernels take the shape with six batches per CU
    gm_f = fused.model(fmt, freqs, sb)
    f_cont, f_offs, f_lens, f_total = fused.encode(gm_f, d_syms, ways, chunk)
    name, placement = kernels["encode"]
    assert (fused.last_encode_kernel()[0], fused.last_encode_placement()) == (name, 1 if fused_batches_ok else placement), \
        (fused.last_encode_kernel(), fused.last_encode_placement())
    assert bench.oracle_check_chunks(dict(art, cont=f_cont, offs=f_offs, lens=f_lens, total=f_total)) == nchunks
    guarded_decode(fused, torch, gm_f, row, chunk, h_syms, "the fused placement's container", f_cont, f_total, f_offs, f_lens, dec)
    return d_syms, gm


def _a_cases():
    for row in LANE_ROWS:
        for chunk in small_sizes(row):
            yield pytest.param(row, chunk, id="%s-%d" % (row["id"], chunk), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,chunk", list(_a_cases()))
def test_lane_decoders_and_the_per_lane_encoder(gpu, oracle, row, chunk):
    """Section a.  35 batches -- one per pattern of S.lane_patterns() -- and a last one of 37 chunks, the last chunk ragged: the
    decoder of the row from three containers, and k_encode_lanes16 (the encoder below six batches per CU) in the compact,
    slot and sized layouts, every chunk against the oracle's stream."""
    freqs = row["model"]()
    h_syms, _ = lane_input(freqs, S.pattern_kinds, SMALL_BATCHES, chunk, 1000 + chunk)
    run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, expect_small(row, chunk))


def _b_cases():
    for row in LANE_ROWS:
        for chunk in big_sizes(row):
            yield pytest.param(row, chunk, id="%s-%d" % (row["id"], chunk), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,chunk", list(_b_cases()))
def test_staged_lane_encoders(gpu, oracle, row, chunk):
    """Section b.  Six batches of 64 chunks per CU (one for k_encode_lanes_r64x2) and a part: k_encode_lanes_staged /
    k_encode_lanes_r64x2 in the compact, slot and sized layouts and under OPT_LANE_FUSED_PLACEMENT (six batches per CU for
    both: the fused placement has no smaller threshold), batch b holding pattern b mod 35; chunks of the smallest size that
    wraps the 128-byte ring, and of 272 symbols."""
    _, _, torch, _ = gpu
    freqs = row["model"]()
    kernels = expect_big(row, chunk)
    if is_r64x2(row):  # the dispatch threshold itself: one batch per CU, no fused placement there
        h_syms, _ = lane_input(freqs, S.pattern_kinds, cus(torch), chunk, 2000 + chunk)
        run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, kernels, phases=False)
    h_syms, _ = lane_input(freqs, S.pattern_kinds, 6 * cus(torch), chunk, 3000 + chunk)
    run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, kernels, phases=False, fused_batches_ok=True)


def _c_cases():
    for row in class_rows():
        for name, _ in classes_of(row):
            yield pytest.param(row, name, id="%s-%s" % (row["id"], name), marks=pytest.mark.gpu)


def stray_positions(row, chunk):
    """(chunk, symbol of the chunk) of the stray symbols, one per call.  k_encode_lanes_r64x2 finds a stray by v_max3 over the
    cmpl words of four record registers -- symbol i of a group lands in the one of i mod 4 --: one stray each, inside a
    full group, in four different lanes."""
    if is_r64x2(row):
        return [(64 * 3 + 5 + 17 * j, 16 + 4 * j + j) for j in range(4)]
    return [(64 * 2 + 41, chunk // 2)]


@pytest.mark.parametrize("row,cls", list(_c_cases()))
def test_lane_rows_under_the_model_classes(gpu, oracle, row, cls):
    """Section c.  Every row under a model that is all-but-one frequency 1, powers of two, M/2 + 1 and M/2 - 1, 3 / 5 / 7 / ...,
    and (byte, rans64) one symbol; chunks of 64 symbols, rare-only / common-only / bursts / drawn in turn by chunk.  At the
    staged encoders' size (k_encode_lanes_r64x2 does its renormalisation test and mulhi64 in its own asm) and at section a's
    (k_encode_lanes16), every layout, both directions.  Every class that has symbols without a record: one such symbol in
    one lane's chunk is E_MODEL, and the next call on the context succeeds."""
    import bench
    R, ctx, torch, _ = gpu
    chunk = 64
    freqs = dict(classes_of(row))[cls]
    row = class_row(row, freqs)
    h_syms, _ = lane_input(freqs, S.turn_kinds, SMALL_BATCHES, chunk, 4000)
    run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, expect_small(row, chunk))
    h_syms, _ = lane_input(freqs, S.turn_kinds, row["per_cu"] * cus(torch), chunk, 5000)
    d_syms, gm = run_lane_case(gpu, oracle, row, freqs, h_syms, chunk, expect_big(row, chunk), phases=False,
                               fused_batches_ok=not is_r64x2(row))
    if not np.any(freqs == 0):
        return
    stray = int(np.nonzero(freqs == 0)[0][0])
    for c, i in stray_positions(row, chunk):
        bad = d_syms.clone()
        bad[c * chunk + i] = stray
        with pytest.raises(R.RansAmdError) as e:
            ctx.encode(gm, bad, row["ways"], chunk)
        assert e.value.status == R.E_MODEL, (c, i)
        assert ctx.last_encode_kernel()[0] == row["big"], ctx.last_encode_kernel()
    cont, offs, lens, total = ctx.encode(gm, d_syms, row["ways"], chunk)
    assert ctx.last_encode_kernel()[0] == row["big"], ctx.last_encode_kernel()
    art = {"fmt": row["fmt"], "sb": row["sb"], "K": row["K"], "ways": row["ways"], "chunk": chunk, "n": h_syms.size, "freqs": freqs,
           "d_syms": d_syms, "cont": cont, "offs": offs, "lens": lens, "total": total}
    assert bench.oracle_check_chunks(art) == (h_syms.size + chunk - 1) // chunk, "after E_MODEL"


@pytest.mark.gpu
@pytest.mark.parametrize("sb,top", D_TOP)
def test_packed_slot_records_at_4095_and_4096(gpu, oracle, sb, top):
    """Section d.  The packed slot records hold "no frequency above 4095" at scale_bits <= 14: a 2-way rans64 model whose
    largest frequency is exactly 4095 decodes through k_decode_lanes_r64x2<packed slots>, one with exactly 4096 through
    k_decode_lanes_r64x2 -- rare-only and drawn chunks in turn (the drawn ones hit the largest frequency), chunks of 192."""
    row = top_row(sb, top)
    freqs = row["model"]()
    h_syms, _ = lane_input(freqs, rare_and_drawn, SMALL_BATCHES, 192, 6000 + top)
    run_lane_case(gpu, oracle, row, freqs, h_syms, 192, expect_small(row, 192))


@pytest.mark.gpu
@pytest.mark.parametrize("sb,cls", D_BITS)
def test_r64x2_kernels_at_scale_bits_7_and_16(gpu, oracle, sb, cls):
    """Section d.  Both r64x2 kernels multiply by v_mul_u32_u24 / v_mad_u32_u24 ("freq <= 2^16, q >> 32 < 2^24"): tight at
    scale_bits 7, the lowest the launchers admit, where a state reaches 2^56.  64 symbols (K must not exceed 2^7), all but
    one of frequency 1 and M/2 + 1 beside M/2 - 1, rare-only and common-only chunks in turn, one batch per CU."""
    _, _, torch, _ = gpu
    row = bits_row(sb, cls)
    freqs = row["model"]()
    h_syms, _ = lane_input(freqs, rare_and_common, cus(torch), 64, 7000 + sb)
    run_lane_case(gpu, oracle, row, freqs, h_syms, 64, expect_big(row, 64), phases=False)


@pytest.mark.gpu
def test_one_symbol_model_at_16_bits_through_the_r64x2_encoder(gpu, oracle):
    """Section d.  A frequency of 2^16 -- a one-symbol model at scale_bits 16 -- at the size that reaches k_encode_lanes_r64x2
    (tests/test_gpu_parity.py test_single_symbol_models stays below one batch per CU).  Its record is cmpl = 0, rcp = 2^63,
    rcp_shift = 15: the renormalisation test x.hi + (0 << 15) >= 2^31 never fires, as rans64.h:83's x >= 2^63 never does,
    and x + bias + q * 0 leaves the state where it is.  Every chunk is the two flushed states, as the oracle's."""
    _, _, torch, _ = gpu
    row = one_symbol_row()
    freqs = row["model"]()
    h_syms, _ = lane_input(freqs, lambda nchunks: np.full(nchunks, S.COMMON_K, dtype=np.uint8), cus(torch), 64, 8000)
    assert np.all(h_syms == 256 - 56)
    run_lane_case(gpu, oracle, row, freqs, h_syms, 64, expect_big(row, 64), phases=False)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", HUGE_PATTERNS)
def test_per_lane_register_window_decoder(gpu, oracle, pattern):
    """Section d.  k_decode_lanes, the fallback for chunks of 512 Ki symbols and more: 64 chunks of 2^19 + 2 symbols and a ragged
    one, 2-way byte format at 14 bits -- one wave whose quad-mates differ, one of rare-only lanes (28 bytes per 16 symbols
    through the per-lane 16-byte window for half a million symbols) and one of common-only lanes.  From the oracle's
    container and from the GPU's own (k_encode_lanes16), into guarded buffers."""
    import bench
    R, ctx, torch, _ = gpu
    row = dict(ROW["byte-2-14bit"], id="byte-2-huge-chunks")
    freqs = row["model"]()
    chunk, nchunks = HUGE_CHUNK, 65
    n = 64 * chunk + 1000
    kinds = S.pattern_kinds(nchunks, names=(pattern,))
    h_syms = S.chunk_grid(freqs, kinds, chunk, 9000).reshape(-1)[:n]
    d_syms = torch.from_numpy(h_syms).cuda()
    gm = ctx.model(row["fmt"], freqs, row["sb"])
    cont, offs, lens, total = ctx.encode(gm, d_syms, 2, chunk)
    assert ctx.last_encode_kernel()[0] == E_L16, ctx.last_encode_kernel()
    art = {"fmt": row["fmt"], "sb": row["sb"], "K": 256, "ways": 2, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms,
           "cont": cont, "offs": offs, "lens": lens, "total": total}
    assert bench.oracle_check_chunks(art) == nchunks
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the GPU's compact container", cont, total, offs, lens, D_L)
    om = oracle.model(freqs, row["sb"])
    o_cont, o_offs, o_lens = oracle.encode_chunked_mt(row["fmt"], om, h_syms, 2, chunk, align=16)
    d_lens = torch.from_numpy(o_lens.astype(np.int32)).cuda()
    streams = [o_cont[int(o_offs[c]):int(o_offs[c]) + int(o_lens[c])] for c in range(nchunks)]
    p_cont, p_starts, p_bytes = S.pack_at_phases(streams, S.lane_phases(nchunks, 1), 128)
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the oracle's streams at every phase", torch.from_numpy(p_cont).cuda(), p_bytes,
                   torch.from_numpy(np.concatenate((p_starts, [p_bytes])).astype(np.int64)).cuda(), d_lens, D_L)
