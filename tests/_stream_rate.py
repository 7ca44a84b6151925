"""How many stream bytes every decode round takes: a plain numpy model of the four stream formats, written from the format
definitions in include/ryg_rans_amd/compat/*.h (rans_byte.h:62-128 and :291-318, rans_word_compat.h, rans64.h:77-121 and
:286-316, rans_alias_compat.h) -- not from the kernels, not from the oracle.  TEST INFRASTRUCTURE ONLY.

round_bytes() is what the rate-extreme tests (tests/test_stream_rate_cpu.py, tests/test_gpu_rate_extremes.py) rest on: the
first proves on the CPU that the inputs below reach the bounds the GPU tests claim, the second decodes those inputs.
tests/test_lane_rate_cpu.py and tests/test_gpu_lane_extremes.py are the same pair for the lane-per-chunk kernels: group_bytes()
turns round_bytes() into bytes per 16-symbol group of one lane's chunk, chunk_grid() builds the chunks of a whole launch.
tests/test_wave_rate_cpu.py and tests/test_gpu_wave_extremes.py are the pair for the wave-per-chunk kernels: interval_bound() is
the most a valid stream takes between two checkpoints of the decoders' stream window, window_walk() a plain model of that
window, steered() the input that puts the cursor of a rare-only stream where one wants it.

Two facts about the formats that shape the inputs:

  * the bytes round r takes depend on the symbols of the rounds >= r alone (a decoder's state in round r is the coder's
    state before it coded round r, and the coder works last to first).  So nothing put in FRONT of a run of symbols can move
    the run's byte pattern against the round numbers; only what follows the run can.  The symbols that shift the lock-step
    pattern of a rare-only stream are therefore its LAST 8 p symbols (p per state) -- the first p symbols the coder sees.
  * a symbol of frequency 1 in a 12-bit word model makes the state a shift register: x' = x >> 12, a word whenever that is
    below 2^16.  The bit length b of a state then walks 29 -> 17 -> 21 -> 25 -> 29: three rounds of four take a word, and
    every window of eight rounds takes exactly six words per state, 96 bytes per eight states -- whatever the phase.  A
    symbol of frequency 16 removes exactly 8 bits, two steps of that walk in one round: p of them behind the rare symbols put
    the round without a word at the four residues modulo 4."""
import numpy as np

from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

STATE_BYTES = {FMT_BYTE: 4, FMT_WORD: 4, FMT_ALIAS: 4, FMT_R64: 8}
UNIT = {FMT_BYTE: 1, FMT_ALIAS: 1, FMT_WORD: 2, FMT_R64: 4}
_LOW = {FMT_BYTE: 1 << 23, FMT_ALIAS: 1 << 23, FMT_WORD: 1 << 16, FMT_R64: 1 << 31}  # RANS_BYTE_L, RANS_WORD_L, RANS64_L
_UNIT_BITS = {FMT_BYTE: 8, FMT_ALIAS: 8, FMT_WORD: 16, FMT_R64: 32}
_MAX_UNITS = {FMT_BYTE: 2, FMT_ALIAS: 2, FMT_WORD: 1, FMT_R64: 1}  # `while` in the byte formats, `if` in the other two


def simulate(fmt, freqs, scale_bits, syms, n_ways, remap=None, per_state=False):
    """-> (bytes per round, the flushed states); with per_state also the units every state takes in every round, [rounds,
    n_ways].  Symbol i is state i mod n_ways's; a round is one symbol of every state.

    The coder's pass (last symbol first) yields the renormalisation units of every round and the final states; the
    decoder's pass then starts from those states and runs x = f (x >> sb) + (x & mask) - start and the format's
    renormalisation, counting what it takes.  It must find the symbols again, take exactly the units the coder left for
    the round, and end with every state at the format's lower bound.  `remap` (alias format): the model's permutation of
    the 2^sb slots, cumulative position -> slot (the identity in the other formats)."""
    f = np.asarray(freqs, dtype=np.uint64)
    cum = np.concatenate(([0], np.cumsum(f))).astype(np.uint64)
    sb = np.uint64(scale_bits)
    total = 1 << scale_bits
    assert int(cum[-1]) == total, "the frequencies do not sum to 2^scale_bits"
    low, ubits, max_units = np.uint64(_LOW[fmt]), np.uint64(_UNIT_BITS[fmt]), _MAX_UNITS[fmt]
    umask = np.uint64((1 << _UNIT_BITS[fmt]) - 1)
    mask = np.uint64(total - 1)
    if remap is None:
        fwd = inv = None
    else:
        fwd = np.asarray(remap, dtype=np.uint64)
        inv = np.zeros(total, dtype=np.uint64)
        inv[fwd] = np.arange(total, dtype=np.uint64)
    s_all = np.asarray(syms).astype(np.int64)
    n, N = s_all.size, int(n_ways)
    rounds = (n + N - 1) // N
    assert n == 0 or int(f[s_all].min()) > 0, "a symbol without a record"
    x = np.full(N, low, dtype=np.uint64)
    taken = np.zeros((rounds, N), dtype=np.uint8)  # units per state
    bits = np.zeros((rounds, N), dtype=np.uint64)  # ... and their bits, the unit put last on top
    # ---- the coder: renormalise to below ((L >> sb) << unit) * freq, then x = ((x / f) << sb) + x % f + start
    for r in range(rounds - 1, -1, -1):
        s = s_all[r * N:(r + 1) * N]
        k = s.size
        fr, st = f[s], cum[s]
        x_max = ((low >> sb) << ubits) * fr
        xs = x[:k].copy()
        for u in range(max_units):
            m = xs >= x_max
            bits[r, :k] |= np.where(m, (xs & umask) << np.uint64(u * int(ubits)), np.uint64(0))
            taken[r, :k] += m
            xs = np.where(m, xs >> ubits, xs)
        assert np.all(xs < x_max), "a state the format's renormalisation cannot bring down"
        pos = xs % fr + st
        x[:k] = ((xs // fr) << sb) + (pos if fwd is None else fwd[pos])
    states = x.copy()
    # ---- the decoder
    per_round = np.zeros(rounds, dtype=np.int64)
    for r in range(rounds):
        s = s_all[r * N:(r + 1) * N]
        k = s.size
        xs = x[:k]
        slot = xs & mask
        pos = slot if inv is None else inv[slot]
        found = np.searchsorted(cum, pos, side="right") - 1
        assert np.array_equal(found, s), ("round", r, "decodes other symbols")
        xs = f[found] * (xs >> sb) + pos - cum[found]
        got = np.zeros(k, dtype=np.uint8)
        rest = bits[r, :k].copy()
        for u in range(max_units):
            m = xs < low
            sh = np.where(taken[r, :k] > got, (taken[r, :k] - got - 1).astype(np.uint64) * ubits, np.uint64(0))
            xs = np.where(m, (xs << ubits) | ((rest >> sh) & umask), xs)
            got += m
        assert np.array_equal(got, taken[r, :k]), ("round", r, "takes other units than the coder left")
        assert np.all(xs >= low), ("round", r, "a state below the format's lower bound")
        x[:k] = xs
        per_round[r] = int(got.sum()) * UNIT[fmt]
    assert np.all(x == low), "the states do not end at the format's lower bound"
    if per_state:
        return per_round, states, taken
    return per_round, states


def round_bytes(fmt, freqs, scale_bits, syms, n_ways, remap=None):
    """Per round, the bytes the n_ways states take together."""
    return simulate(fmt, freqs, scale_bits, syms, n_ways, remap)[0]


def stream_states(fmt, stream, n_ways):
    """The flushed states at the head of a stream: state 0 first, 4 bytes each (8 in rans64), little-endian."""
    head = np.ascontiguousarray(stream[:n_ways * STATE_BYTES[fmt]])
    return head.view(np.uint64 if fmt == FMT_R64 else np.uint32).astype(np.uint64)


def windows(per_round, w=8):
    """Sums over every window of w consecutive rounds (empty where there are fewer than w rounds)."""
    c = np.concatenate(([0], np.cumsum(per_round)))
    return c[w:] - c[:-w]


def group_bytes(per_round, n_ways, group=16):
    """Bytes per `group`-symbol group of one lane's chunk: the sums over every window of group / n_ways rounds (the lane
    kernels refill, flush and check their invariants once per 16 symbols, wherever the group boundary falls)."""
    assert group % n_ways == 0
    return windows(per_round, group // n_ways)


def rare_group_bytes(fmt, scale_bits, n_ways, group=16):
    """(least, most) bytes a window of group / n_ways rounds of frequency-1 symbols takes -- from the formats alone.  A symbol
    of frequency 1 makes the decoder's step x = x >> scale_bits (its slot is its start): exactly scale_bits bits leave the
    state.  A state's bit length is in [b, b + u) before and after the window (u: the unit's bits), so the k units that
    come in satisfy T - u < k u < T + u for the T = (group / n_ways) scale_bits bits that left: k = T / u where u divides T,
    floor or ceil otherwise -- whatever the state was when the window began."""
    lost, u = (group // n_ways) * scale_bits, _UNIT_BITS[fmt]
    return n_ways * (lost // u) * UNIT[fmt], n_ways * ((lost + u - 1) // u) * UNIT[fmt]


def interval_bound(fmt, scale_bits, states, rounds):
    """The most bytes a valid stream can take in an interval of `rounds` rounds of `states` states -- from the format alone,
    as rare_group_bytes: a round removes at most scale_bits bits from a state (a frequency-1 symbol: x = x >> scale_bits),
    a state's bit length lies in a range one unit wide before and after the interval, so at most ceil(rounds scale_bits /
    unit bits) units come in; and no more than the format's renormalisation can bring in in `rounds` rounds (two units per
    round in the byte formats, one in the other two)."""
    units = (rounds * scale_bits + _UNIT_BITS[fmt] - 1) // _UNIT_BITS[fmt]
    return states * min(units, rounds * _MAX_UNITS[fmt]) * UNIT[fmt]


def substep_bytes(taken, fmt, n_ways):
    """The bytes of every sub-step, in the decoders' order: a sub-step is the renormalisation of 64 states (one per lane of a
    wave) -- round r of an N-way stream is ceil(N / 64) of them, states 0..63 first.  `taken`: simulate(per_state=True)."""
    taken = np.asarray(taken, dtype=np.int64)
    k = (int(n_ways) + 63) // 64
    padded = np.zeros((taken.shape[0], 64 * k), dtype=np.int64)
    padded[:, :taken.shape[1]] = taken
    return (padded.reshape(taken.shape[0], k, 64).sum(axis=2) * UNIT[fmt]).reshape(-1)


RING_BLOCK, RING_BYTES, RING_MIRROR = 1024, 2048, 768  # (the comment at the top of decode_common.hpp; wave_shape.hpp)


def window_walk(substeps, first, cadence, every_from=None):
    """A plain model of the decoders' stream window, written from the comment at the top of decode_common.hpp: a 2 KiB ring
    filled in aligned 1 KiB blocks, the cursor starting at `first` mod 16 (the window opens at the 16-byte granule of the
    first unit), the mark at 1024.  A checkpoint falls in front of sub-step 0, cadence, 2 cadence ... (from sub-step
    `every_from` on: in front of every sub-step -- the element-store tail).  At a checkpoint with cursor >= mark: while the
    mark is 1024 the first half is refilled and the mark goes to 2048; otherwise the cursor drops by 2048, the second half is
    refilled and the mark returns to 1024.  Between checkpoints the cursor only moves up.
    -> ([(cursor - mark, refilled, bytes of the interval that follows)] per checkpoint, the largest ring offset reached)."""
    b = np.asarray(substeps, dtype=np.int64)
    n = b.size
    at = [i for i in range(n) if (every_from is not None and i >= every_from) or i % cadence == 0]
    cur, mark, top = int(first) & 15, RING_BLOCK, 0
    out = []
    for j, i in enumerate(at):
        rel = cur - mark
        refilled = cur >= mark
        if refilled:
            if mark == RING_BLOCK:
                mark = RING_BYTES
            else:
                cur -= RING_BYTES
                mark = RING_BLOCK
        nxt = at[j + 1] if j + 1 < len(at) else n
        took = int(b[i:nxt].sum())
        out.append((rel, refilled, took))
        cur += took
        top = max(top, cur)
    return out, top


def longest_silence(per_round):
    """The longest run of consecutive rounds that take no byte."""
    best = run = 0
    for v in per_round:
        run = run + 1 if v == 0 else 0
        best = max(best, run)
    return best


# ---- models -----------------------------------------------------------------------------------------------------------
COMMON, SHIFT = 0, 1  # the common symbol; the frequency-16 symbol behind the rare ones (rate_model, quiet_model)


def rate_model():
    """3841 + 255 x 1 over 256 symbols."""
    f = np.ones(256, dtype=np.uint32)
    f[COMMON] = 4096 - 255
    return f


def rate_model_16():
    """... one of the rare symbols widened to frequency 16 (the common one gives the 15 up): 3826, 16, 254 x 1."""
    f = np.ones(256, dtype=np.uint32)
    f[SHIFT] = 16
    f[COMMON] = 4096 - 16 - 254
    return f


def quiet_model():
    """4065, 16, 15 x 1, and 239 symbols without a record.  A state loses log2(4096 / 4065) = 0.011 bits per common symbol:
    16 bits last 1450 rounds.  (Under 3841 + 255 x 1 a state loses 0.093 bits per common symbol and takes a word every 172
    or 173 rounds -- every state in the same round, as all of them hold the same value: no window of 1024 silent rounds
    exists under that model, whatever the input.)"""
    f = np.zeros(256, dtype=np.uint32)
    f[COMMON], f[SHIFT] = 4096 - 16 - 15, 16
    f[2:17] = 1
    return f


def lane_model(sb):
    """255 x 1 and one common symbol at 2^sb."""
    f = np.ones(256, dtype=np.uint32)
    f[COMMON] = (1 << sb) - 255
    return f


def model_rare(sb, K):
    """K - 1 symbols of frequency 1 and one common symbol at 2^sb, for alphabets above 256 as well (u16 symbols)."""
    f = np.ones(K, dtype=np.uint32)
    f[COMMON] = (1 << sb) - (K - 1)
    return f


def packed_model_14():
    """252 x 1 and four symbols of 4033 at 2^14: frequency-1 symbols under a model whose largest frequency fits the 12-bit
    field of the rans64 packed slot records.  (No silent extreme: the commonest symbol still costs two bits.)"""
    f = np.ones(256, dtype=np.uint32)
    f[:4] = 4033
    assert int(f.sum()) == 1 << 14
    return f


def top_frequency_model(sb, top):
    """Largest frequency exactly `top` (4095 / 4096) at 2^sb, 13 or 14 bits: `top`, three (one) further common symbols of at
    most 4094, frequency 1 for the rest."""
    f = np.ones(256, dtype=np.uint32)
    k = 2 if sb == 13 else 4
    rest = (1 << sb) - (256 - k) - top
    f[0] = top
    share = [rest // (k - 1) + (1 if i < rest % (k - 1) else 0) for i in range(k - 1)]
    f[1:k] = share
    assert int(f.sum()) == 1 << sb and int(f.max()) == top and int(np.count_nonzero(f == top)) == 1
    return f


def class_models(sb, K, one_symbol):
    """The model classes of the encoders' division-free update at 2^sb over K symbols -> [(name, freqs)]."""
    M = 1 << sb
    out = []
    f = np.ones(K, dtype=np.uint32)
    f[3 % K] = M - (K - 1)
    out.append(("all-but-one-1", f))
    f = np.zeros(K, dtype=np.uint32)
    f[:sb] = [M >> (k + 1) for k in range(sb)]  # M/2 ... 1
    f[sb] = 1
    out.append(("powers-of-two", f))
    f = np.zeros(K, dtype=np.uint32)
    f[10], f[11] = M // 2 + 1, M // 2 - 1
    out.append(("above-and-below-half", f))
    f = np.zeros(K, dtype=np.uint32)
    third = ((M - 15) // 3) | 1
    f[:5] = [3, 5, 7, M - 15 - third, third]
    out.append(("odd", f))
    if one_symbol:
        f = np.zeros(K, dtype=np.uint32)
        f[K - 56] = M
        out.append(("one-symbol", f))
    for _, f in out:
        assert int(f.sum()) == M
    return out


# ---- contents ---------------------------------------------------------------------------------------------------------
def rare_and_common(freqs):
    """(the symbols of the smallest frequency on record, the symbol of the largest)."""
    f = np.asarray(freqs)
    return np.nonzero(f == f[f > 0].min())[0], int(np.argmax(f))


def _dtype(freqs):
    return np.uint8 if len(freqs) <= 256 else np.uint16


def rare_only(freqs, n, seed, shift=0, n_ways=8):
    """n symbols of the smallest frequency (drawn with a fixed seed); the last shift * n_ways of them -- `shift` per state, the
    first the coder sees -- are the frequency-16 symbol SHIFT."""
    rare, _ = rare_and_common(freqs)
    out = rare[np.random.default_rng(seed).integers(0, rare.size, n)].astype(_dtype(freqs))
    if shift:
        assert freqs[SHIFT] == 16
        out[max(0, n - shift * n_ways):] = SHIFT
    return out


def common_only(freqs, n):
    return np.full(n, rare_and_common(freqs)[1], dtype=_dtype(freqs))


def bursts(freqs, n, seed, lead=0, run=64):
    """Runs of `run` rare and `run` common symbols in turn; `lead` symbols of the first (rare) run are cut off, which moves the
    runs against the round numbers."""
    out = rare_only(freqs, n, seed)
    out[((np.arange(n) + lead) // run) % 2 == 1] = rare_and_common(freqs)[1]
    return out


def steered(freqs, lanes_rare, lead_rounds, rare_rounds, seed, n_ways):
    """(lead_rounds + rare_rounds) n_ways symbols: in the first lead_rounds rounds states 0 .. lanes_rare - 1 hold rare
    symbols and the others the common one, rare-only rounds follow.  The bytes of a round depend on the rounds from it on
    alone, so the rare-only part renormalises in lock-step whatever leads it, and the lead moves the decoder's cursor by
    whatever multiple of the unit its rare states take: the cursor of a rare-only stream can be put anywhere."""
    n = (lead_rounds + rare_rounds) * n_ways
    out = rare_only(freqs, n, seed).reshape(lead_rounds + rare_rounds, n_ways)
    out[:lead_rounds, lanes_rare:] = rare_and_common(freqs)[1]
    return out.reshape(-1)


def drawn(freqs, n, seed):
    f = np.asarray(freqs, dtype=np.float64)
    return np.random.default_rng(seed).choice(f.size, n, p=f / f.sum()).astype(_dtype(freqs))


# ---- contents of a grid of chunks, one chunk per lane of a wave ---------------------------------------------------------
LANE_KINDS = ("rare", "common", "bursts64", "bursts16", "drawn")
RARE, COMMON_K, BURSTS64, BURSTS16, DRAWN = range(5)
QUADS = (0, 7, 15)  # a first, a middle and the last quad of a wave


def lane_patterns():
    """What the 64 lanes of a wave hold -> [(name, kind of lane 0..63)], 35 waves:
      rotating-r          lane l holds LANE_KINDS[(l + r) mod 5]: over the five every lane position meets every kind
      quad-mates-differ-r [rare, common, bursts, drawn] x 16 rotated by r (runs of 64 in the even quads, of 16 in the odd ones)
      one-rare-qQ-lL      one rare lane -- lane L of quad Q -- among 63 common ones
      one-common-qQ-lL    the inverse: a lane that asks for nothing beside 63 that take the most
      all-rare, all-common"""
    out = []
    lanes = np.arange(64)
    for r in range(5):
        out.append(("rotating-%d" % r, (lanes + r) % 5))
    quad = np.array([RARE, COMMON_K, BURSTS64, DRAWN])
    for r in range(4):
        k = quad[(lanes + r) % 4]
        k[(k == BURSTS64) & ((lanes // 4) % 2 == 1)] = BURSTS16
        out.append(("quad-mates-differ-%d" % r, k))
    for name, one, rest in (("one-rare", RARE, COMMON_K), ("one-common", COMMON_K, RARE)):
        for q in QUADS:
            for l in range(4):
                k = np.full(64, rest)
                k[4 * q + l] = one
                out.append(("%s-q%d-l%d" % (name, q, l), k))
    out.append(("all-rare", np.full(64, RARE)))
    out.append(("all-common", np.full(64, COMMON_K)))
    return [(n, k.astype(np.uint8)) for n, k in out]


def pattern_kinds(nchunks, names=None):
    """Kind of every chunk: batch b (64 chunks, one wave) holds pattern b mod len(patterns) of lane_patterns() (`names`: of
    those alone)."""
    pats = [k for n, k in lane_patterns() if names is None or n in names]
    table = np.stack(pats)
    c = np.arange(nchunks)
    return table[(c // 64) % len(pats), c % 64]


def turn_kinds(nchunks, kinds=(RARE, COMMON_K, BURSTS64, DRAWN)):
    """The kinds in turn by chunk."""
    return np.asarray(kinds, dtype=np.uint8)[np.arange(nchunks) % len(kinds)]


def burst_lead(c):
    """Symbols cut off the first (rare) run of chunk c's bursts: a multiple of 8 -- of every interleave --, 0 .. 120, spread by
    a multiplicative hash so that it does not follow the lane or the batch."""
    return 8 * (((np.asarray(c, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(9)) % np.uint64(16)).astype(np.int64)


def chunk_grid(freqs, kinds, chunk, seed, first_chunk=0):
    """-> symbols [len(kinds), chunk]: chunk c of kind kinds[c] (an index into LANE_KINDS), vectorised over the grid.  rare:
    symbols of the smallest frequency on record; common: the commonest symbol; bursts64 / bursts16: runs of 64 / 16 rare and
    as many common symbols in turn, burst_lead(first_chunk + c) symbols of the first run cut off; drawn: from the model."""
    f = np.asarray(freqs, dtype=np.int64)
    kinds = np.asarray(kinds)
    rare, common = rare_and_common(freqs)
    rng = np.random.default_rng(seed)
    n = kinds.size
    out = rare.astype(_dtype(freqs))[rng.integers(0, 256, (n, chunk), dtype=np.uint8) % rare.size]
    out[kinds == COMMON_K] = common
    pos = np.arange(chunk)
    for kind, run in ((BURSTS64, 64), (BURSTS16, 16)):
        rows = np.nonzero(kinds == kind)[0]
        if rows.size:
            sub = out[rows]
            sub[((pos[None, :] + burst_lead(rows + first_chunk)[:, None]) // run) % 2 == 1] = common
            out[rows] = sub
    rows = np.nonzero(kinds == DRAWN)[0]
    if rows.size:
        cum = np.cumsum(f)
        out[rows] = np.searchsorted(cum, rng.integers(0, int(cum[-1]), (rows.size, chunk)), side="right").astype(out.dtype)
    return out


def lane_phases(nchunks, unit):
    """Start offsets modulo 128 for pack_at_phases: lane l of batch b at unit * ((l + 7 b) mod (128 / unit)).  Units of 1 and 2
    bytes: the 64 lanes of a wave at 64 different offsets; over 19 (10, 5) batches every multiple of the unit is met."""
    c = np.arange(nchunks)
    return unit * ((c % 64 + 7 * (c // 64)) % (128 // unit))


_ORACLE = []


def zipf_under(freqs, n, seed):
    """The control: the suite's existing generator (Oracle.gen_zipf, bit-identical to bench.gen_zipf, s = 1) over as many
    ranks as the model has symbols on record, rank r mapped onto the r-th most frequent of them.  Under 3826 + 16 + 254 x 1
    every symbol has a record and that mapping is the identity: the symbols are the generator's own.  The quiet model has
    239 symbols without a record, which the generator's 256 ranks would hit; hence the mapping."""
    if not _ORACLE:
        from _oracle import Oracle
        _ORACLE.append(Oracle())
    f = np.asarray(freqs)
    order = np.argsort(-f.astype(np.int64), kind="stable")[:int(np.count_nonzero(f))]
    return order[_ORACLE[0].gen_zipf(n, K=order.size, s=1.0, seed=seed).astype(np.int64)].astype(_dtype(freqs))


# ---- containers packed by hand ----------------------------------------------------------------------------------------
def pack_at_phases(streams, phases, modulus, order=None):
    """The streams back to back (in `order`), each moved up to the next offset == its phase (mod modulus) ->
    (container with 16 bytes of zeros behind it, starts, bytes in use)."""
    starts = np.zeros(len(streams), dtype=np.int64)
    at = 0
    for c in (range(len(streams)) if order is None else order):
        at += (int(phases[c]) - at) % modulus
        starts[c] = at
        at += int(streams[c].size)
    cont = np.zeros(at + 16, dtype=np.uint8)
    for c, s in enumerate(streams):
        cont[starts[c]:starts[c] + s.size] = s
    assert all(int(starts[c]) % modulus == int(phases[c]) % modulus for c in range(len(streams)))
    return cont, starts, at
