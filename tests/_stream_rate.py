"""How many stream bytes every decode round takes: a plain numpy model of the four stream formats, written from the format
definitions in include/ryg_rans_amd/compat/*.h (rans_byte.h:62-128 and :291-318, rans_word_compat.h, rans64.h:77-121 and
:286-316, rans_alias_compat.h) -- not from the kernels, not from the oracle.  TEST INFRASTRUCTURE ONLY.

round_bytes() is what the rate-extreme tests (tests/test_stream_rate_cpu.py, tests/test_gpu_rate_extremes.py) rest on: the
first proves on the CPU that the inputs below reach the bounds the GPU tests claim, the second decodes those inputs.

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


def simulate(fmt, freqs, scale_bits, syms, n_ways, remap=None):
    """-> (bytes per round, the flushed states).  Symbol i is state i mod n_ways's; a round is one symbol of every state.

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


def drawn(freqs, n, seed):
    f = np.asarray(freqs, dtype=np.float64)
    return np.random.default_rng(seed).choice(f.size, n, p=f / f.sum()).astype(_dtype(freqs))


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
