"""The wave-per-chunk kernels (decode_wave.hip, decode_dual.hip, encode_wave.hip) at the ends of the formats' stream rates, at
every start phase: chunks that take the most a valid stream can between two checkpoints of the decoders' stream window
(interval_bound: 512 bytes -- kMaxAdvance itself -- for every row of 128 states and more per checkpoint interval and for the
64-way byte and alias formats at 16 bits, 384 for the 64-way word format), chunks that take nothing, bursts of both and
symbols drawn from the model, neighbouring chunks differing in kind and start phase.

What these kernels rest on and the suite had not pinned: kMaxAdvance (a valid stream reaches it exactly, and the window
then refills at every second checkpoint), where the cursor stands at a checkpoint (exactly on the mark: refill; one unit
below: no refill, and up to 512 - unit bytes past the mark into the mirror), the hand-over of k_decode_word64 (the next
chunk's claim, index entry, states and first two blocks requested kClaimAhead = 10 and kDataAhead = 5 groups before the
end: chunks of 0, 1, 2, 5, 6, 10 and 11 groups take different paths), the two windows of k_decode_dual<alias>, and the
wave encoders outside the 64-way word and byte formats.

tests/_stream_rate.py holds the models, the contents, the numpy model of the bytes every round takes and a plain model of
the window (window_walk); tests/test_wave_rate_cpu.py proves without a GPU that the inputs built here sit where this file
says and that WAVE_ROWS names every wave kernel.  Every comparison is against Oracle.encode / bench.oracle_check_chunks /
the input symbols, never the library; every decode goes into a poison-filled buffer with a guard in front and behind;
after every call the kernel the library reports is asserted, and decode_errors() == 0 after every healthy decode.

Chunk sizes (N: the interleave).  The fast stores of every wave decoder need a chunk size that is a multiple of 4 bytes
(wave_shape.hpp decode_out_aligned), so "twelve groups, three full rounds through the element-store tail and a partial
round" comes twice: 51 N + 5 symbols (odd: the any-N kernels with element stores and a checkpoint in front of every
sub-step; the library reports k_decode<word> for the 64-way word format and k_decode<alias> for the dual rows) and 51 N + 4
(the group loops of the kernels the rows name, then the tail); and 4 N, one group without a tail.  k_decode_dual<alias>
runs its paired loop on chunks of a multiple of 256 symbols alone (decode_dual.hip shape_ok), so its rows also get 48 N.
Twelve groups of a rare-only 64-way chunk at 16 bits are 6 KiB of stream: three laps of the 2 KiB ring.

  section a  WAVE_ROWS x chunk sizes, 64 chunks and a ragged one: the kinds in turn by chunk (rare, common, bursts of 64 and
             of 16, drawn), all rare, all common; the encoder's compact container against the oracle, the decoder from four
             containers (the GPU's, the oracle's, the oracle's streams at offset unit x (c mod 16 / unit) modulo 16 and at
             S.lane_phases modulo 128 -- byte streams: twice, the second time 64 further), container_bytes exact and poison
             behind the last byte; the two per-chunk-model rows on constant chunks mixed with uniform and Zipf ones
  section b  steered chunks -- the cursor one unit below the mark and exactly on it, each followed by a maximal interval, every
             overshoot modulo 16 -- for every row whose interval_bound is 512 and the 64-way word row, at every start residue
  section c  the hand-over ladder of k_decode_word64: chunks of 256 g + t symbols, at one unit of work and over several rounds
             of the grid, and all lengths in one launch of k_decode_batch_word64
  section d  every row's encoder in the compact, slot and sized layouts (tests/_every_chunk.py), OPT_FUSED_PLACEMENT = 0 for
             the 64-way word and byte rows, and sized slots at tight_slot_bytes: who overflows, exact room, E_SPACE
  section e  every row under the model classes of the encoders' division-free update; a symbol without a record is E_MODEL,
             deep in the group part of a chunk and in its element-store tail

Rows whose kernel differs from the issue's table: none by name; by size, the odd chunk size moves word-64-* to k_decode<word> and
the dual rows to k_decode<alias> (`unaligned` of the row), which is why the aligned twin of that size exists.

What the cases are tight against (two mutated builds of the library, each run once, never committed; both change nothing
but which bytes of a wave's own LDS window are read):
  * the mirror copy in StreamWindow::put shortened from 768 to 256 bytes (stale LDS beyond 2048 + 256): 60 of the 201 cases run
    fail, every one with a chunk flagged or a wrong symbol -- all eleven steered cases of section b; in section a the aligned
    51 N + 4 size of every word row, of byte-64-14bit and byte-64-12bit and the quiet row's long size; the ladder from g = 6 on
    and its batch form; the same rows in sections d and e.  byte-64-16bit, the alias rows and rans64 pass sections a, d and e
    on it and fail section b alone: their rare-only chunks renormalise in lock-step, 128 bytes a round, so from any start the
    cursor passes the ring's end by less than 16 bytes -- only the steered chunks make it run deep into the mirror.  The odd
    size (a checkpoint in front of every sub-step) and 4 N pass, as they must: they never read past 2048 + 256.
  * `cur > mark` in place of `>=` in StreamWindow::checkpoint: all 201 cases pass, and from the code they have to.  A cursor
    exactly on the mark that is not refilled is the cursor one unit below it, moved by a unit: it runs at most kMaxAdvance
    past the mark and reads one sub-step further, 2048 + 512 + 256 = the mirror's end (the static_assert behind kMaxAdvance),
    and the next checkpoint refills.  The two comparisons decode every valid stream alike; no test can tell them apart.

Wall time on an MI355X: 9 to 11 s for the 202 cases of this file -- 1.7 s of it the first case's setup (it loads the kernels);
the slowest case is test_word64_hand_over_ladder_in_one_batch at 0.45 s, then the quiet row's chunks of 1030 rounds at
0.25 s; every other case takes 0.02 to 0.2 s.  With tests/test_gpu_lane_extremes.py, tests/test_gpu_rate_extremes.py and
tests/test_gpu_kernel_matrix.py in one run (before the ladder's g = 7 was added): 505 cases in 86 s."""
import numpy as np
import pytest

import _stream_rate as S
from _batch import GUARD, POISON
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

OPT_FUSED_PLACEMENT, OPT_DUAL_DECODE = 2, 3  # (ryg_rans_amd.OPT_*; the numbers are the ABI's, tests/test_abi.py)

D_W64, D_W, D_W16 = "k_decode_word64", "k_decode<word>", "k_decode<word, u16 symbols>"
D_B, D_BF, D_R, D_RS = "k_decode<byte>", "k_decode<byte, slot records>", "k_decode<r64>", "k_decode<r64 search>"
D_A, D_DUAL = "k_decode<alias>", "k_decode_dual<alias>"
D_WA, D_BA = "k_decode<word, per-chunk models>", "k_decode<byte, per-chunk models>"
E_W, E_B, E_R, E_RF, E_A = "k_encode<word>", "k_encode<byte>", "k_encode<r64>", "k_encode<r64 full-width>", "k_encode<alias, LDS remap>"
E_WA, E_BA = "k_encode<word, per-chunk models>", "k_encode<byte, per-chunk models>"
E_WAD, E_BAD = "k_encode_adaptive<word>", "k_encode_adaptive<byte>"

NCHUNKS = 64  # full chunks per launch; a ragged one follows


def _wave(rid, fmt, sb, K, ways, model, decode, encode, cadence, bound, unaligned=None, opts=(), shift=False, group_syms=None):
    """cadence: sub-steps (renormalisations of 64 states) between two window checkpoints on the path the row names, taken from
    the issue's table, not measured; bound: (states, rounds) of such an interval -- S.interval_bound turns it into bytes;
    unaligned: the decoder of a chunk size that is no multiple of 4 bytes, where it has another name; shift: the model has the
    frequency-16 symbol S.SHIFT; group_syms: the fast loop runs on chunks of a multiple of that many symbols alone."""
    return {"id": rid, "fmt": fmt, "sb": sb, "K": K, "ways": ways, "model": model, "decode": decode, "encode": encode, "cadence": cadence,
            "bound": S.interval_bound(fmt, sb, *bound), "interval": bound, "unaligned": unaligned or decode, "opts": tuple(opts),
            "shift": shift, "group_syms": group_syms, "sym_bytes": 1 if K <= 256 else 2}


WAVE_ROWS = [
    # ---- k_decode_word64: a checkpoint in front of every group of four rounds
    _wave("word-64-rate", FMT_WORD, 12, 256, 64, S.rate_model_16, D_W64, E_W, 4, (64, 4), unaligned=D_W, shift=True),
    _wave("word-64-quiet", FMT_WORD, 12, 256, 64, S.quiet_model, D_W64, E_W, 4, (64, 4), unaligned=D_W, shift=True),
    # ---- k_decode<word>, 2 / 4 / 8 states per lane: a checkpoint every four sub-steps -- two rounds, one round, half a round
    _wave("word-128", FMT_WORD, 12, 256, 128, S.rate_model_16, D_W, E_W, 4, (128, 2), shift=True),
    _wave("word-256", FMT_WORD, 12, 256, 256, S.rate_model_16, D_W, E_W, 4, (256, 1), shift=True),
    _wave("word-512", FMT_WORD, 12, 256, 512, S.rate_model_16, D_W, E_W, 4, (256, 1), shift=True),
    # (idle tail lanes: the any-N path, a checkpoint in front of every sub-step)
    _wave("word-100", FMT_WORD, 12, 256, 100, S.rate_model_16, D_W, E_W, 1, (64, 1), shift=True),
    # ---- u16 symbols: one state per lane checks once per pair of rounds, two states per lane every four sub-steps
    _wave("word-u16-64", FMT_WORD, 12, 1024, 64, lambda: S.model_rare(12, 1024), D_W16, E_W, 2, (64, 2)),
    _wave("word-u16-128", FMT_WORD, 12, 1024, 128, lambda: S.model_rare(12, 1024), D_W16, E_W, 4, (128, 2)),
    # ---- the byte format
    _wave("byte-64-16bit", FMT_BYTE, 16, 256, 64, lambda: S.lane_model(16), D_B, E_B, 4, (64, 4)),
    _wave("byte-64-14bit", FMT_BYTE, 14, 256, 64, lambda: S.lane_model(14), D_B, E_B, 4, (64, 4)),
    _wave("byte-128-16bit", FMT_BYTE, 16, 256, 128, lambda: S.lane_model(16), D_B, E_B, 4, (128, 2)),
    _wave("byte-64-12bit", FMT_BYTE, 12, 256, 64, lambda: S.lane_model(12), D_BF, E_B, 4, (64, 4)),
    # ---- rans64: a checkpoint every two sub-steps; the search decoder (17 bits and more) has element stores alone and
    #      checks in front of every sub-step
    _wave("r64-64-16bit", FMT_R64, 16, 256, 64, lambda: S.lane_model(16), D_R, E_R, 2, (64, 2)),
    _wave("r64-64-14bit", FMT_R64, 14, 256, 64, lambda: S.lane_model(14), D_R, E_R, 2, (64, 2)),
    _wave("r64-128-16bit", FMT_R64, 16, 256, 128, lambda: S.lane_model(16), D_R, E_R, 2, (128, 1)),
    _wave("r64-search-64-17bit", FMT_R64, 17, 256, 64, lambda: S.lane_model(17), D_RS, E_RF, 1, (64, 1)),
    _wave("r64-search-64-31bit", FMT_R64, 31, 256, 64, lambda: S.lane_model(31), D_RS, E_RF, 1, (64, 1)),
    # ---- the alias format; two chunks per wave where the option asks for it and for the 4096-symbol model
    _wave("alias256-64", FMT_ALIAS, 16, 256, 64, lambda: S.lane_model(16), D_A, E_A, 4, (64, 4)),
    _wave("alias256-64-dual", FMT_ALIAS, 16, 256, 64, lambda: S.lane_model(16), D_DUAL, E_A, 4, (64, 4), unaligned=D_A,
          opts=((OPT_DUAL_DECODE, 2),), group_syms=256),
    _wave("alias4096-64", FMT_ALIAS, 16, 4096, 64, lambda: S.model_rare(16, 4096), D_DUAL, E_A, 4, (64, 4), unaligned=D_A, group_syms=256),
]
ROW = {r["id"]: r for r in WAVE_ROWS}

# one model per chunk: the extremes are CONSTANT chunks.  Word format: the chunk's own model has frequency 4096, the 32-bit
# threshold ((L >> 12) << 16) * 4096 wraps to 0 and every symbol pushes a word out: 2 n + 256 bytes, 128 in every round, 512 per
# group of four -- the only 64-way word path that reaches kMaxAdvance (S.simulate does not model the wrap; the proof is the
# oracle's stream size).  Byte format: a constant chunk is the flushed states alone.
ADAPTIVE_ROWS = [
    {"id": "word-64-per-chunk", "fmt": FMT_WORD, "sb": 12, "K": 256, "ways": 64, "decode": D_WA, "encode": E_WA, "sized": E_WAD, "bound": 512},
    {"id": "byte-64-per-chunk", "fmt": FMT_BYTE, "sb": 12, "K": 256, "ways": 64, "decode": D_BA, "encode": E_BA, "sized": E_BAD, "bound": 0},
]


def aligned(row, chunk):
    """wave_shape.hpp decode_out_aligned: a chunk size of a multiple of 4 bytes (the output pointer is the allocator's)."""
    return (chunk * row["sym_bytes"]) % 4 == 0


def decoder_of(row, chunk):
    return row["decode"] if aligned(row, chunk) else row["unaligned"]


def odd_size(N):
    return 12 * 4 * N + 3 * N + 5


def tail_size(N):
    return 12 * 4 * N + 3 * N + 4


LONG_ROUNDS = 1030  # (the quiet row: a common-only chunk that takes nothing for more than 1024 rounds)


def sizes(row):
    N = row["ways"]
    out = [odd_size(N), tail_size(N), 4 * N]
    if row["group_syms"]:
        out.append(12 * 4 * N)
    if row["id"] == "word-64-quiet":
        out.append(LONG_ROUNDS * N + 4)
    return out


def fast_layout(row, chunk):
    """-> (cadence, first sub-step of the element-store tail) of the path a full chunk of this size takes: the row's group loop
    over whole groups of four rounds (pairs of rounds: u16 symbols) and element stores behind it, or element stores for all."""
    N = row["ways"]
    K = (N + 63) // 64
    rounds = chunk // N
    fast = aligned(row, chunk) and N == 64 * K and row["cadence"] != 1
    if row["group_syms"] and chunk % row["group_syms"]:
        fast = False
    if not fast:
        return 1, 0
    per = 2 if row["sym_bytes"] == 2 and not row["group_syms"] else 4
    return row["cadence"], (rounds // per) * per * K


KINDS5 = (S.RARE, S.COMMON_K, S.BURSTS64, S.BURSTS16, S.DRAWN)
SETS = ("turn", "all-rare", "all-common")


def set_kinds(which, nchunks):
    if which == "turn":
        return S.turn_kinds(nchunks, KINDS5)
    return np.full(nchunks, S.RARE if which == "all-rare" else S.COMMON_K, dtype=np.uint8)


def chunk_content(row, freqs, kind, n, c, seed):
    """Chunk c of a kind: rare-only (word rows whose model has it: c mod 4 shifting symbols per state behind the rare ones),
    common-only, runs of 64 / 16 rare and common symbols in turn (S.burst_lead(c) cut off the first run), drawn from the model."""
    if kind == S.RARE:
        return S.rare_only(freqs, n, seed + c, shift=c % 4 if row["shift"] else 0, n_ways=row["ways"])
    if kind == S.COMMON_K:
        return S.common_only(freqs, n)
    if kind in (S.BURSTS64, S.BURSTS16):
        return S.bursts(freqs, n, seed + c, lead=int(S.burst_lead(c)), run=64 if kind == S.BURSTS64 else 16)
    return S.drawn(freqs, n, seed + c)


def ragged(chunk):
    return chunk // 3 + 1


def wave_input(row, freqs, chunk, which, seed=100, nchunks=NCHUNKS):
    """-> (symbols of nchunks full chunks and a ragged last one, kind per chunk)."""
    kinds = set_kinds(which, nchunks + 1)
    parts = [chunk_content(row, freqs, int(kinds[c]), chunk if c < nchunks else ragged(chunk), c, seed) for c in range(nchunks + 1)]
    return np.concatenate(parts), kinds


def phases16(nchunks, unit):
    """Chunk c at offset unit x (c mod (16 / unit)) modulo 16."""
    return unit * (np.arange(nchunks) % (16 // unit))


def phases128(nchunks, unit):
    """The packings modulo 128: S.lane_phases -- 64 different offsets over 64 chunks, every multiple of a 2- or 4-byte unit --
    and, for the byte streams, the same moved on by 64: every offset."""
    ph = S.lane_phases(nchunks, unit)
    return [ph] if unit > 1 else [ph, (ph + 64) % 128]


# ---- section b: steered chunks ------------------------------------------------------------------------------------------
B_LANES = (0, 1, 3, 7, 21, 40, 63)
B_LEADS = (4, 5, 8, 12)
B_ROWS = [r["id"] for r in WAVE_ROWS if r["bound"] == 512 and r["cadence"] != 1] + ["word-64-rate"]


def b_size(row):
    """Twelve groups and the tail; the paired loop of the dual decoder: twelve groups.  rans64 at 16 bits: a state takes a dword
    every second round, and the states of a partial last round -- the first the coder sees -- would run a round ahead of the
    others for the whole chunk (124 of 128 states in step: 496 bytes, not 512); hence whole rounds there."""
    N = row["ways"]
    return 12 * 4 * N if row["group_syms"] else 51 * N if row["fmt"] == FMT_R64 else tail_size(N)


def b_chunks(row, freqs):
    """64 steered chunks: chunk c leads with B_LEADS[c mod 4] rounds in which B_LANES[(c div 4) mod 7] states out of every 64
    hold rare symbols, rare-only rounds follow to the chunk's size."""
    N = row["ways"]
    n = b_size(row)
    rounds = (n + N - 1) // N
    out = []
    for c in range(NCHUNKS):
        lead, lanes = B_LEADS[c % 4], B_LANES[(c // 4) % 7] * N // 64
        out.append(S.steered(freqs, lanes, lead, rounds - lead, 700 + c, N)[:n])
    return out


# ---- section c: the hand-over ladder ------------------------------------------------------------------------------------
LADDER_G = (0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12)  # (7: the first chunk whose data step falls inside the group loop)
LADDER_T = (0, 1, 63, 64 + 5)
LADDER_T4 = (4, 60, 64 + 4)  # the aligned neighbours of 1, 63 and 69: a uniform call reaches k_decode_word64 with these alone
LADDER_CHUNKS = 40


def ladder_sizes(g):
    return [256 * g + t for t in LADDER_T + LADDER_T4 if 256 * g + t > 0]


def ladder_batch_counts():
    """The lengths of the batch form: an Euler circuit through the complete directed graph (loops included) over LADDER_G --
    every ordered pair of path lengths is a pair of neighbours --, the tails in turn."""
    n = len(LADDER_G)
    nxt = [0] * n
    walk, stack = [], [0]
    while stack:  # Hierholzer; vertex v's unused edges are v -> nxt[v] .. n - 1
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    ts = LADDER_T + LADDER_T4
    return np.array([256 * LADDER_G[v] + ts[(3 * i) % len(ts)] for i, v in enumerate(walk)], dtype=np.uint32), [LADDER_G[v] for v in walk]


# ---- section e ----------------------------------------------------------------------------------------------------------
def one_symbol_ok(row):
    """(tests/test_gpu_rate_extremes.py c_one_symbol)"""
    return row["fmt"] in (FMT_BYTE, FMT_R64) or (row["fmt"] == FMT_ALIAS and row["sb"] < 16)


def classes_of(row):
    return S.class_models(row["sb"], row["K"], one_symbol_ok(row))


def class_rows():
    """The rows that differ in more than their model."""
    seen, out = set(), []
    for row in WAVE_ROWS:
        key = (row["fmt"], row["sb"], row["K"], row["ways"], row["opts"])
        if key not in seen:
            seen.add(key)
            out.append(row)
    return out


# ---- the case table: which kernel names this file asserts, under which inputs -------------------------------------------
def _wave_cases():
    cases = []
    for row in WAVE_ROWS:
        for chunk in sizes(row):
            cases.append({"section": "a", "id": "%s-%d" % (row["id"], chunk), "kernels": (decoder_of(row, chunk), row["encode"]),
                          "inputs": ("rare", "common", "mixed")})
    for row in ADAPTIVE_ROWS:
        cases.append({"section": "a", "id": row["id"], "kernels": (row["decode"], row["encode"], row["sized"]), "inputs": ("rare", "common", "mixed")})
    return cases


WAVE_CASES = _wave_cases()


def kernels_under(inp, cases=None):
    return {k for c in (WAVE_CASES if cases is None else cases) if inp in c["inputs"] for k in c["kernels"]}


# ---- the GPU part -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import ryg_rans_amd as R
    ctx = R.Context(0)
    dual = R.Context(0)  # (contexts of their own: options must not leak)
    dual.set_option(OPT_DUAL_DECODE, 2)
    unfused = R.Context(0)
    unfused.set_option(OPT_FUSED_PLACEMENT, 0)
    yield R, ctx, torch, {(): ctx, ((OPT_DUAL_DECODE, 2),): dual, "unfused": unfused}
    unfused.close()
    dual.close()
    ctx.close()


def context_of(gpu, row):
    return gpu[3][row["opts"]]


def to_device(torch, h):
    """(torch has no u16: such symbols travel as int16, as the library's own tensors do)"""
    return torch.from_numpy(h.view(np.int16) if h.dtype == np.uint16 else h).cuda()


def poison_of(h):
    return POISON if h.dtype == np.uint8 else -23131  # 0xA5A5 as int16


def exact_container(torch, h_cont, nbytes):
    """The container's bytes in an allocation whose every other byte is poison: container_bytes is passed exactly, and what lies
    behind the last chunk's last byte is not zeros."""
    d = torch.full((((nbytes + 15) & ~15) + 256,), POISON, dtype=torch.uint8, device="cuda")
    d[:nbytes] = torch.from_numpy(np.ascontiguousarray(h_cont[:nbytes])).cuda()
    return d


def guarded_decode(ctx, torch, gm, row, chunk, h_syms, what, d_cont, nbytes, d_offs, d_lens, kernel):
    """One decode into a poison-filled buffer with GUARD symbols in front and behind -> the output == the input, the guards
    untouched, the kernel the one expected, no chunk flagged."""
    n = h_syms.size
    h_in = h_syms.view(np.int16) if h_syms.dtype == np.uint16 else h_syms
    back = torch.full((n + 2 * GUARD,), poison_of(h_syms), dtype=torch.uint8 if h_syms.dtype == np.uint8 else torch.int16, device="cuda")
    ctx.decode(gm, d_cont, nbytes, d_offs, d_lens, n, row["ways"], chunk, d_out=back[GUARD:GUARD + n])
    assert ctx.last_decode_kernel() == kernel, (row["id"], chunk, what, ctx.last_decode_kernel(), "expected", kernel)
    assert ctx.decode_errors() == 0, (row["id"], chunk, what)
    host = back.cpu().numpy()
    got = host[GUARD:GUARD + n]
    if not np.array_equal(got, h_in):
        first = int(np.nonzero(got != h_in)[0][0])
        raise AssertionError((row["id"], what, "first wrong symbol", first, "chunk", first // chunk, "symbol of the chunk", first % chunk,
                              "round", (first % chunk) // row["ways"]))
    assert (host[:GUARD] == poison_of(h_syms)).all() and (host[GUARD + n:] == poison_of(h_syms)).all(), (what, "written outside the output")


def oracle_streams(oracle, row, freqs, h_syms, chunk):
    """-> (the oracle's container, offsets, lengths, its chunks' streams)"""
    om = oracle.model(freqs, row["sb"], with_alias=(row["fmt"] == FMT_ALIAS))
    o_cont, o_offs, o_lens = oracle.encode_chunked_mt(row["fmt"], om, h_syms, row["ways"], chunk, align=16)
    streams = [o_cont[int(o_offs[c]):int(o_offs[c]) + int(o_lens[c])] for c in range(o_lens.size)]
    return o_cont, o_offs, o_lens, streams


def decode_packed(ctx, torch, gm, row, chunk, h_syms, streams, phases, modulus, what, kernel):
    p_cont, p_starts, p_bytes = S.pack_at_phases(streams, phases, modulus)
    assert p_bytes == int(p_starts[-1]) + streams[-1].size  # the last chunk ends on the container's last byte
    lens = np.array([s.size for s in streams], dtype=np.int32)
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, what, exact_container(torch, p_cont, p_bytes), p_bytes,
                   torch.from_numpy(np.concatenate((p_starts, [p_bytes])).astype(np.int64)).cuda(), torch.from_numpy(lens).cuda(), kernel)


def run_wave_case(gpu, oracle, row, freqs, h_syms, chunk, encoder=True):
    """The compact encode (every chunk == the oracle's stream, kernel and placement asserted), then the decoder into guarded
    buffers from the GPU's container, the oracle's, and the oracle's streams packed at both sets of phases."""
    import bench
    R, _, torch, _ = gpu
    ctx = context_of(gpu, row)
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    n = h_syms.size
    nchunks = (n + chunk - 1) // chunk
    dec = decoder_of(row, chunk)
    gm = ctx.model(fmt, freqs, sb)
    if encoder:
        d_syms = to_device(torch, h_syms)
        cont, offs, lens, total = ctx.encode(gm, d_syms, ways, chunk)
        assert (ctx.last_encode_kernel()[0], ctx.last_encode_placement()) == (row["encode"], 1), (row["id"], ctx.last_encode_kernel(),
                                                                                                  ctx.last_encode_placement())
        art = {"fmt": fmt, "sb": sb, "K": row["K"], "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms, "cont": cont,
               "offs": offs, "lens": lens, "total": total}
        assert bench.oracle_check_chunks(art) == nchunks
        guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the GPU's compact container", exact_container(torch, cont[:total].cpu().numpy(), total),
                       total, offs, lens, dec)
    o_cont, o_offs, o_lens, streams = oracle_streams(oracle, row, freqs, h_syms, chunk)
    d_lens = torch.from_numpy(o_lens.astype(np.int32)).cuda()
    guarded_decode(ctx, torch, gm, row, chunk, h_syms, "the oracle's container", exact_container(torch, o_cont, o_cont.size), o_cont.size,
                   torch.from_numpy(o_offs.astype(np.int64)).cuda(), d_lens, dec)
    unit = S.UNIT[fmt]
    decode_packed(ctx, torch, gm, row, chunk, h_syms, streams, phases16(nchunks, unit), 16, "every phase modulo 16", dec)
    for ph in phases128(nchunks, unit):
        decode_packed(ctx, torch, gm, row, chunk, h_syms, streams, ph, 128, "every phase modulo 128", dec)
    return streams


def _a_cases():
    for row in WAVE_ROWS:
        for chunk in sizes(row):
            yield pytest.param(row, chunk, id="%s-%d" % (row["id"], chunk), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,chunk", list(_a_cases()))
def test_wave_kernels_rate_times_phase(gpu, oracle, row, chunk):
    """Section a.  64 chunks and a ragged one, three sets: the five kinds in turn by chunk (neighbouring chunks differ, and
    the dual decoder's pairs hold every adjacent combination), all rare (both windows of a pair at the maximum together),
    all common."""
    freqs = row["model"]()
    for which in SETS:
        h_syms, _ = wave_input(row, freqs, chunk, which)
        run_wave_case(gpu, oracle, row, freqs, h_syms, chunk)


def adaptive_input(chunk, nchunks=NCHUNKS):
    """Constant chunks (one symbol each, another symbol every time) mixed with uniform-random and Zipf chunks, chunk by chunk,
    a constant pair and a random pair among them; the ragged last chunk is constant."""
    rng = np.random.default_rng(31)
    kinds = ["constant", "uniform", "constant", "zipf", "constant", "constant", "uniform", "uniform"]
    parts = []
    for c in range(nchunks + 1):
        n = chunk if c < nchunks else ragged(chunk)
        kind = kinds[c % len(kinds)] if c < nchunks else "constant"
        if kind == "constant":
            parts.append(np.full(n, (37 * c + 5) % 256, dtype=np.uint8))
        elif kind == "uniform":
            parts.append(rng.integers(0, 256, n, dtype=np.uint8))
        else:
            parts.append(S.zipf_under(np.ones(256), n, 40 + c).astype(np.uint8))
    return np.concatenate(parts), [kinds[c % len(kinds)] for c in range(nchunks)] + ["constant"]


def _adaptive_cases():
    for row in ADAPTIVE_ROWS:
        for chunk in (odd_size(64), tail_size(64), 4 * 64):
            yield pytest.param(row, chunk, id="%s-%d" % (row["id"], chunk), marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,chunk", list(_adaptive_cases()))
def test_per_chunk_models_on_constant_chunks(gpu, oracle, row, chunk):
    """Section a, the per-chunk-model rows.  Both encoders (the three-launch path and the one-kernel one): every chunk's row and
    stream == the oracle's; the decoder on both containers, on the oracle's, and on the oracle's streams at every phase, into
    guarded buffers."""
    R, ctx, torch, _ = gpu
    fmt, sb, ways = row["fmt"], row["sb"], row["ways"]
    h_syms, _ = adaptive_input(chunk)
    n = h_syms.size
    nchunks = (n + chunk - 1) // chunk
    d_syms = torch.from_numpy(h_syms).cuda()

    def decode(what, d_cont, nbytes, d_offs, d_lens, d_rows):
        back = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
        ctx.decode_adaptive(d_cont, nbytes, d_offs, d_lens, d_rows, n, ways, chunk, sb, d_out=back[GUARD:GUARD + n], fmt=fmt)
        assert ctx.last_decode_kernel() == row["decode"], (what, ctx.last_decode_kernel())
        assert ctx.decode_errors() == 0, what
        host = back.cpu().numpy()
        assert np.array_equal(host[GUARD:GUARD + n], h_syms), what
        assert (host[:GUARD] == POISON).all() and (host[GUARD + n:] == POISON).all(), (what, "written outside the output")

    cont, offs, lens, rows, total = ctx.encode_adaptive_sized(d_syms, ways, chunk, sb, fmt=fmt)
    assert ctx.last_encode_kernel()[0] == row["sized"], ctx.last_encode_kernel()
    h_lens = lens.cpu().numpy().astype(np.uint32)
    h_rows = rows.cpu().numpy()
    count, bad = oracle.compare_container_adaptive(fmt, h_syms, ways, chunk, sb, cont[:total].cpu().numpy(), offs.cpu().numpy().astype(np.uint64),
                                                   h_lens, h_rows)
    assert count == nchunks and bad == -1, bad
    decode("the one-kernel encoder's container", cont, total, offs, lens, rows)
    c0, o0, l0, r0, t0 = ctx.encode_adaptive(d_syms, ways, chunk, sb, fmt=fmt)
    assert ctx.last_encode_kernel()[0] == row["encode"], ctx.last_encode_kernel()
    count, bad = oracle.compare_container_adaptive(fmt, h_syms, ways, chunk, sb, c0[:t0].cpu().numpy(), o0.cpu().numpy().astype(np.uint64), h_lens,
                                                   h_rows)
    assert count == nchunks and bad == -1, bad
    decode("the three-launch encoder's container", exact_container(torch, c0[:t0].cpu().numpy(), t0), t0, o0, l0, r0)
    o_cont, o_offs, o_lens, o_rows = oracle.encode_chunked_adaptive(fmt, h_syms, ways, chunk, sb)
    assert np.array_equal(o_lens, h_lens) and np.array_equal(o_rows.reshape(-1), h_rows.view(np.uint16))
    d_rows = torch.from_numpy(o_rows.reshape(-1).view(np.int16)).cuda()
    d_lens = torch.from_numpy(o_lens.astype(np.int32)).cuda()
    decode("the oracle's container", exact_container(torch, o_cont, o_cont.size), o_cont.size, torch.from_numpy(o_offs.astype(np.int64)).cuda(),
           d_lens, d_rows)
    streams = [o_cont[int(o_offs[c]):int(o_offs[c]) + int(o_lens[c])] for c in range(nchunks)]
    unit = S.UNIT[fmt]
    for phases, modulus in [(phases16(nchunks, unit), 16)] + [(ph, 128) for ph in phases128(nchunks, unit)]:
        p_cont, p_starts, p_bytes = S.pack_at_phases(streams, phases, modulus)
        decode("every phase modulo %d" % modulus, exact_container(torch, p_cont, p_bytes), p_bytes,
               torch.from_numpy(np.concatenate((p_starts, [p_bytes])).astype(np.int64)).cuda(), d_lens, d_rows)


# ---- section b ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rid", B_ROWS)
def test_steered_cursor_at_the_mark(gpu, oracle, rid):
    """Section b.  64 steered chunks -- tests/test_wave_rate_cpu.py proves that they put the cursor one unit below the mark
    without a refill and exactly on it with one, each in front of a maximal interval, and that the overshoot at a refill
    takes every multiple of the unit modulo 16 -- decoded from the phase-packed container at every rotation of the start
    residues: chunk c at offset unit x ((c + rot) mod (16 / unit)) modulo 16.  The decoder alone."""
    R, _, torch, _ = gpu
    row = ROW[rid]
    ctx = context_of(gpu, row)
    freqs = row["model"]()
    fmt, unit = row["fmt"], S.UNIT[row["fmt"]]
    chunk = b_size(row)
    om = oracle.model(freqs, row["sb"], with_alias=(fmt == FMT_ALIAS))
    data = b_chunks(row, freqs)
    streams = [oracle.encode(fmt, om, d, row["ways"]) for d in data]
    h_syms = np.concatenate(data)
    gm = ctx.model(fmt, freqs, row["sb"])
    for rot in range(16 // unit):
        decode_packed(ctx, torch, gm, row, chunk, h_syms, streams, unit * ((np.arange(NCHUNKS) + rot) % (16 // unit)), 16,
                      "steered, rotation %d" % rot, decoder_of(row, chunk))


# ---- section c ----------------------------------------------------------------------------------------------------------
def resident_waves(torch):
    from _batch import resident_waves as rw
    return rw(torch)


@pytest.mark.gpu
@pytest.mark.parametrize("g", LADDER_G)
def test_word64_hand_over_ladder(gpu, oracle, g):
    """Section c.  Chunks of 256 g + t symbols, 40 per launch and a ragged one, kinds in turn, from the four containers of section
    a.  By g, the groups of a chunk, the next chunk's two steps fall: both behind the group loop, which has no pass (g = 0, 1);
    the claim in the loop's first pass and the data step behind the loop (2 .. 6: the data step's pass, five groups on, does
    not exist); the claim in the first pass and the data step five passes later (7, 9, 10); the claim kClaimAhead groups before
    the end and the data step kDataAhead before it (11, 12).  t = 1, 63 and 69 make a chunk size that is no multiple of 4 -- the library
    sends it to k_decode<word> --, so their aligned neighbours 4, 60 and 68 run as well: the tail behind the hand-over in
    k_decode_word64.  Then every size over several rounds of the grid: 4 x resident_waves chunks, the index of the 40 repeated
    (the decoders take any offset for any chunk), the output compared with the symbols repeated."""
    R, ctx, torch, _ = gpu
    row = ROW["word-64-rate"]
    freqs = row["model"]()
    gm = ctx.model(FMT_WORD, freqs, 12)
    many = 4 * resident_waves(torch)
    for chunk in ladder_sizes(g):
        dec = decoder_of(row, chunk)
        assert (dec == D_W64) == (chunk % 4 == 0)
        h_syms, _ = wave_input(row, freqs, chunk, "turn", seed=300 + chunk, nchunks=LADDER_CHUNKS)
        streams = run_wave_case(gpu, oracle, row, freqs, h_syms, chunk, encoder=False)
        # several rounds of the grid
        full = streams[:LADDER_CHUNKS]
        p_cont, p_starts, p_bytes = S.pack_at_phases(full, phases16(LADDER_CHUNKS, 2), 16)
        reps = (many + LADDER_CHUNKS - 1) // LADDER_CHUNKS
        d_offs = torch.from_numpy(np.concatenate((np.tile(p_starts, reps), [p_bytes])).astype(np.int64)).cuda()
        d_lens = torch.from_numpy(np.tile(np.array([s.size for s in full], dtype=np.int32), reps)).cuda()
        d_one = torch.from_numpy(h_syms[:LADDER_CHUNKS * chunk]).cuda()
        n = reps * LADDER_CHUNKS * chunk
        back = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
        ctx.decode(gm, exact_container(torch, p_cont, p_bytes), p_bytes, d_offs, d_lens, n, 64, chunk, d_out=back[GUARD:GUARD + n])
        assert ctx.last_decode_kernel() == dec, (chunk, ctx.last_decode_kernel())
        assert ctx.decode_errors() == 0, chunk
        assert reps * LADDER_CHUNKS >= many
        assert torch.equal(back[GUARD:GUARD + n].view(reps, -1), d_one.expand(reps, -1)), (chunk, "several rounds of the grid")
        assert bool((back[:GUARD] == POISON).all()) and bool((back[GUARD + n:] == POISON).all()), (chunk, "written outside the output")


@pytest.mark.gpu
def test_word64_hand_over_ladder_in_one_batch(gpu, oracle):
    """Section c, the batch form (k_decode_batch_word64): the streams' lengths walk an Euler circuit over the ladder's path
    lengths, so one launch hands over between every ordered pair of them; kinds in turn by stream.  tests/_batch.py's
    run_row (encode_batch against the oracle, decode_batch of the GPU's and of the oracle's shuffled container, laid-out
    input with poison between the streams and a guard) at sym_align 4 and 1, then the phase-packed container."""
    from _batch import Batch, run_row
    from _kernel_rows import ROW as BATCH_ROW
    R, ctx, torch, _ = gpu
    row = ROW["word-64-rate"]
    brow = BATCH_ROW["word-64"]
    freqs = row["model"]()
    counts, _ = ladder_batch_counts()
    kinds = S.turn_kinds(counts.size, KINDS5)
    contents = {k: chunk_content(row, freqs, int(kinds[k]), int(counts[k]), k, 500) for k in range(counts.size)}
    b = Batch(R, ctx, torch, oracle, brow, counts, contents=contents, freqs=freqs)
    for align in (4, 1):
        _, _, _, d_buf, d_sym, _, _, _ = run_row(b, align)
        assert ctx.decode_errors() == 0
        p_cont, p_starts, p_bytes = S.pack_at_phases(b.streams, phases16(b.n, 2), 16)
        out = torch.full_like(d_buf, b.poison())
        ctx.decode_batch(b.gm, exact_container(torch, p_cont, p_bytes), p_bytes, b.dev(p_starts, np.int64), b.dev(b.lens, np.int32), d_sym,
                         b.d_counts, 64, out)
        assert ctx.last_decode_kernel() == brow["decode"], ctx.last_decode_kernel()
        assert torch.equal(out, d_buf), ("every phase modulo 16", align)
        assert ctx.decode_errors() == 0


# ---- section d ----------------------------------------------------------------------------------------------------------
def _d_cases():
    for row in WAVE_ROWS:
        yield pytest.param(row, False, id=row["id"], marks=pytest.mark.gpu)
    for row in WAVE_ROWS:  # the 64-way word and byte rows once more, the coder followed by the layout and compaction kernels
        if row["ways"] == 64 and row["fmt"] in (FMT_WORD, FMT_BYTE) and row["K"] == 256:
            yield pytest.param(row, True, id=row["id"] + "-unfused", marks=pytest.mark.gpu)


@pytest.mark.parametrize("row,unfused", list(_d_cases()))
def test_wave_encoders_in_every_layout(gpu, oracle, row, unfused):
    """Section d.  Section a's input (kinds in turn; chunks of 51 N + 4 and of 4 N symbols) through encode, encode_slots and
    encode_sized (tests/_every_chunk.py: every chunk == the oracle's stream in every layout, the index follows the layout's
    rule, kernel and placement flag asserted, every container decodes).  Then sized slots at tight_slot_bytes(model) by hand:
    every chunk whose oracle stream is longer than the slot lies in the overflow region -- all rare-only chunks do --, no
    common-only chunk does (its stream is the states and a few units); exact room for the overflow succeeds, one chunk fewer
    is E_SPACE, and a healthy call right behind starts clean."""
    import bench
    from _every_chunk import check_every_chunk
    R, _, torch, ctxs = gpu
    ctx = ctxs["unfused"] if unfused else context_of(gpu, row)
    fmt, sb, K, ways = row["fmt"], row["sb"], row["K"], row["ways"]
    freqs = row["model"]()
    E = row["encode"]
    for chunk in (tail_size(ways), 4 * ways):
        h_syms, kinds = wave_input(row, freqs, chunk, "turn")
        n, nchunks = h_syms.size, NCHUNKS + 1
        d_syms = to_device(torch, h_syms)
        kernels = {"decode": decoder_of(row, chunk), "encode": (E, 0 if unfused else 1), "slots": (E, 2), "sized": (E, 2)}
        gm = ctx.model(fmt, freqs, sb)
        sized = ctx.tight_slot_bytes(gm, ways, chunk) < R.slot_bytes(fmt, n, ways, chunk)
        check_every_chunk(R, ctx, torch, fmt, sb, K, ways, chunk, n, kernels=kernels, damaged=False, sized=sized, sized_ratio=None,
                          all_overflow_at_half=False, d_syms=d_syms, freqs=freqs)
        assert ctx.decode_errors() == 0
        if chunk != tail_size(ways):
            continue
        assert sized, "no tight slot below the worst case"
        slot = ctx.tight_slot_bytes(gm, ways, chunk)
        worst = R.slot_bytes(fmt, n, ways, chunk)
        _, _, o_lens, _ = oracle_streams(oracle, row, freqs, h_syms, chunk)
        over = o_lens.astype(np.int64) > slot
        assert over[:NCHUNKS][kinds[:NCHUNKS] == S.RARE].all(), "a rare-only chunk that fits a tight slot"
        assert not over[kinds == S.COMMON_K].any(), "a common-only chunk longer than a tight slot"
        # (the coder gives a chunk up once less than two rounds' worst case is left of its slot: a chunk a little shorter than
        #  the slot may overflow as well -- how many do, the library says; which must and which must not, the oracle's lengths)
        t_cont, t_offs, t_lens, t_total, t_slot = ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, overflow_chunks=nchunks)
        outside = t_offs.cpu().numpy()[:nchunks].astype(np.int64) >= nchunks * slot
        assert outside[over].all(), "a chunk longer than its slot that is not in the overflow region"
        assert not outside[kinds == S.COMMON_K].any(), "a common-only chunk in the overflow region"
        room = int(outside.sum())
        assert NCHUNKS // len(KINDS5) <= room < nchunks
        t_cont, t_offs, t_lens, t_total, t_slot = ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, overflow_chunks=room)
        assert (ctx.last_encode_kernel()[0], ctx.last_encode_placement()) == (E, 2), ctx.last_encode_kernel()
        assert t_slot == slot and np.array_equal(t_lens.cpu().numpy().astype(np.int64), o_lens.astype(np.int64))
        assert np.array_equal(t_offs.cpu().numpy()[:nchunks].astype(np.int64) >= nchunks * slot, outside)
        art = {"fmt": fmt, "sb": sb, "K": K, "ways": ways, "chunk": chunk, "n": n, "freqs": freqs, "d_syms": d_syms, "cont": t_cont,
               "offs": t_offs, "lens": t_lens, "total": t_total, "slot": slot, "worst": worst}
        assert bench.oracle_check_chunks(art) == nchunks
        guarded_decode(ctx, torch, gm, row, chunk, h_syms, "sized slots, exact room", t_cont, t_total, t_offs, t_lens, decoder_of(row, chunk))
        with pytest.raises(R.RansAmdError) as e:
            ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, overflow_chunks=room - 1)
        assert e.value.status == R.E_SPACE
        t_cont, t_offs, t_lens, t_total, _ = ctx.encode_sized(gm, d_syms, ways, chunk, slot=slot, overflow_chunks=room)
        assert bench.oracle_check_chunks(dict(art, cont=t_cont, offs=t_offs, lens=t_lens, total=t_total)) == nchunks, "after E_SPACE"


# ---- section e ----------------------------------------------------------------------------------------------------------
def _e_cases():
    for row in class_rows():
        for name, _ in classes_of(row):
            yield pytest.param(row, name, id="%s-%s" % (row["id"], name), marks=pytest.mark.gpu)


def stray_positions(row, chunk):
    """(chunk, symbol of the chunk): deep in the group part of a chunk, and in the element-store tail (the last full round)."""
    N = row["ways"]
    return [(17, 7 * 4 * N + 2 * N + 5), (42, 12 * 4 * N + 2 * N + N // 2)]


@pytest.mark.parametrize("row,cls", list(_e_cases()))
def test_wave_rows_under_the_model_classes(gpu, oracle, row, cls):
    """Section e.  Every row under a model that is all-but-one frequency 1, powers of two, M/2 + 1 and M/2 - 1, 3 / 5 / 7 / ...,
    and (byte, rans64) one symbol; chunks of 51 N + 4 symbols, kinds in turn; both directions, four containers.  Every class
    that has symbols without a record: one such symbol is E_MODEL, deep in the group part of a chunk and in its element-store
    tail, and the next call on the context succeeds."""
    import bench
    R, _, torch, _ = gpu
    ctx = context_of(gpu, row)
    freqs = dict(classes_of(row))[cls]
    row = dict(row, shift=False)  # (the classes have no shifting symbol)
    chunk = tail_size(row["ways"])
    h_syms, _ = wave_input(row, freqs, chunk, "turn", seed=900)
    run_wave_case(gpu, oracle, row, freqs, h_syms, chunk)
    if not np.any(freqs == 0):
        return
    stray = int(np.nonzero(freqs == 0)[0][0])
    gm = ctx.model(row["fmt"], freqs, row["sb"])
    d_syms = to_device(torch, h_syms)
    for c, i in stray_positions(row, chunk):
        bad = d_syms.clone()
        bad[c * chunk + i] = stray
        with pytest.raises(R.RansAmdError) as e:
            ctx.encode(gm, bad, row["ways"], chunk)
        assert e.value.status == R.E_MODEL, (c, i)
        assert ctx.last_encode_kernel()[0] == row["encode"], ctx.last_encode_kernel()
    cont, offs, lens, total = ctx.encode(gm, d_syms, row["ways"], chunk)
    art = {"fmt": row["fmt"], "sb": row["sb"], "K": row["K"], "ways": row["ways"], "chunk": chunk, "n": h_syms.size, "freqs": freqs,
           "d_syms": d_syms, "cont": cont, "offs": offs, "lens": lens, "total": total}
    assert bench.oracle_check_chunks(art) == NCHUNKS + 1, "after E_MODEL"
