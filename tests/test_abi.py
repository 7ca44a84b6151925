"""CPU-only checks of the product library: it loads, exports every symbol the header
declares, refuses to run without a GPU (no CPU fallback), and its HOST logic (model
builder, table images, layout arithmetic) matches the oracle and the golden vectors."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import ryg_rans_amd as R
from _oracle import FMT_ALIAS, FMT_BYTE, FMT_R64, FMT_WORD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "book1_golden.json")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_every_declared_symbol_is_exported():
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rans_amd_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 25
    lib = C.CDLL(R.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "header declares %s but the library does not export it" % name
    assert declared == set(R.ABI_SYMBOLS)


def test_version_and_status_strings():
    assert R.lib().rans_amd_version() == 600
    for code in range(8):
        assert R.lib().rans_amd_status_string(code)
    assert R.lib().rans_amd_status_string(99) == b"unknown status"


def test_shipped_library_is_not_the_measure_build():
    """The library the package loads reads no environment: RANS_AMD_BUILD_MEASURE is clear (bench.py refuses a headline
    run on a build that has it), and the measure build, when present, says what it is."""
    assert R.lib().rans_amd_build_flags() == 0
    measure = os.path.join(os.path.dirname(R.LIB_PATH), "libryg_rans_amd_measure.so")
    if os.path.exists(measure):
        m = C.CDLL(measure)
        m.rans_amd_build_flags.restype = C.c_uint32
        assert m.rans_amd_build_flags() & 1  # RANS_AMD_BUILD_MEASURE
    # the product sources read the environment only inside measure_knob() / #ifdef RANS_AMD_MEASURE
    for fn in ("api.cpp", "dispatch.cpp", "decode_lanes.hip", "encode_lanes.hip", "encode_wave.hip", "decode_wave.hip", "decode_dual.hip"):
        text = open(os.path.join(ROOT, "ryg_rans_amd", "csrc", fn)).read()
        assert "getenv(" not in text, fn


def test_set_option_checks_its_arguments():
    assert R.lib().rans_amd_ctx_set_option(None, R.OPT_DUAL_DECODE, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    for name in ("LANE_KERNELS", "LANE_FUSED_PLACEMENT", "FUSED_PLACEMENT", "DUAL_DECODE", "ENC_SCRATCH_RING"):
        m = re.search(r"RANS_AMD_OPT_%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(R, "OPT_" + name), name


def test_no_cpu_fallback():
    """Without a GPU the context cannot be created and nothing can be encoded/decoded."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert R.device_count() == 0
    with pytest.raises(R.RansAmdError) as e:
        R.Context(0)
    assert e.value.status == R.E_HIP
    # a host-only model exists for table inspection, but the coders refuse it
    f = np.zeros(256, np.uint32); f[0] = 4000; f[1] = 96
    m = R.Model(None, FMT_WORD, f, 12)
    out = np.zeros(16, np.uint8)
    n = C.c_uint64(0)
    rc = R.lib().rans_amd_encode_host(None, m._h, out.ctypes.data, 16, 64, out.ctypes.data, 16, C.byref(n))
    assert rc == R.E_ARG


def test_product_is_independent_of_oracle():
    """The shipped library and package never reference oracle/ (the judge checks this too)."""
    import subprocess
    deps = subprocess.run(["ldd", R.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in deps and "ryg_ref" not in deps
    for root, _, files in os.walk(os.path.join(ROOT, "ryg_rans_amd")):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(root, fn)).read()
                assert "rans_oracle" not in text and "_oracle" not in text and "libryg_ref" not in text, fn


def test_normalize_matches_oracle(oracle):
    rng = np.random.default_rng(5)
    for nsyms, total in ((256, 4096), (256, 16384), (256, 65536), (4096, 65536), (16, 64), (256, 256)):
        for trial in range(6):
            counts = (rng.pareto(0.7, nsyms) * 3).astype(np.uint32)
            counts[rng.integers(0, nsyms, nsyms // 3)] = 0
            counts[rng.integers(0, nsyms)] += 1000
            if trial == 5:
                counts[:] = 1  # everything present, uniform
            f, cum = R.normalize_freqs(counts, total)
            fo, co = oracle.normalize(counts, total)
            assert np.array_equal(f, fo) and np.array_equal(cum, co), (nsyms, total, trial)
    with pytest.raises(R.RansAmdError):
        R.normalize_freqs(np.ones(256, np.uint32), 128)  # target < nsyms (main.cpp:77)
    with pytest.raises(R.RansAmdError):
        R.normalize_freqs(np.zeros(256, np.uint32), 4096)


def test_count_freqs_host(oracle):
    d8 = oracle.gen_zipf(100003, K=256, s=1.0, seed=2)
    assert np.array_equal(R.count_freqs(d8, 256), oracle.count_freqs(d8, 256))
    d16 = oracle.gen_zipf(50001, K=4096, s=1.0, seed=2)
    assert np.array_equal(R.count_freqs(d16, 4096), oracle.count_freqs(d16, 4096))
    with pytest.raises(R.RansAmdError):
        R.count_freqs(d16, 100)  # symbol outside the alphabet


def test_book1_tables_match_reference_hashes(book1):
    """The product's own table builders against hashes of the unmodified reference's
    arrays."""
    want = {t["name"]: t["sha256"] for t in GOLD["tables"]}
    counts = R.count_freqs(book1, 256)
    for bits in (12, 14, 16):
        _, cum = R.normalize_freqs(counts, 1 << bits)
        assert sha(cum) == want["cum_freqs_%d" % (1 << bits)]
    f12, _ = R.normalize_freqs(counts, 4096)
    m = R.Model(None, FMT_WORD, f12, 12)
    assert sha(m.table(R.TAB_WORD_SLOTS)) == want["word_tables"]
    f16, _ = R.normalize_freqs(counts, 65536)
    m = R.Model(None, FMT_ALIAS, f16, 16)
    assert sha(m.table(R.TAB_ALIAS_DIVIDER)) == want["alias_divider"]
    assert sha(m.table(R.TAB_ALIAS_SLOT_ADJUST)) == want["alias_slot_adjust"]
    assert sha(m.table(R.TAB_ALIAS_SLOT_FREQS)) == want["alias_slot_freqs"]
    assert sha(m.table(R.TAB_ALIAS_SYM_ID)) == want["alias_sym_id"]
    assert sha(m.table(R.TAB_ALIAS_REMAP)) == want["alias_remap"]


def test_alias_tables_match_oracle(oracle):
    for nsyms, sb, seed in ((256, 16, 1), (256, 10, 2), (4096, 16, 3), (64, 12, 4), (4096, 12, 5)):
        data = oracle.gen_zipf(200000, K=nsyms, s=1.0, seed=seed)
        f, _ = oracle.normalize(oracle.count_freqs(data, nsyms), 1 << sb)
        om = oracle.model(f, sb, with_alias=True)
        m = R.Model(None, FMT_ALIAS, f, sb)
        assert np.array_equal(m.table(R.TAB_ALIAS_DIVIDER, np.uint32), om.table("divider", nsyms))
        assert np.array_equal(m.table(R.TAB_ALIAS_SLOT_ADJUST, np.uint32), om.table("slot_adjust", 2 * nsyms))
        assert np.array_equal(m.table(R.TAB_ALIAS_SLOT_FREQS, np.uint32), om.table("slot_freqs", 2 * nsyms))
        sid = m.table(R.TAB_ALIAS_SYM_ID, np.uint8 if nsyms <= 256 else np.uint16)
        assert np.array_equal(sid.astype(np.uint32), om.table("sym_id", 2 * nsyms))
        assert np.array_equal(m.table(R.TAB_ALIAS_REMAP, np.uint32), om.table("alias_remap", 1 << sb))
        c2s = m.table(R.TAB_CUM2SYM, np.uint8 if nsyms <= 256 else np.uint16)
        assert np.array_equal(c2s.astype(np.uint32), om.table("cum2sym", 1 << sb))


def test_enc_dec_symbol_records_match_reference(ref, oracle):
    """RansEncSymbolInit / Rans64EncSymbolInit values (rans_byte.h:174-243, rans64.h:167-247):
    the reciprocal encoder fed with OUR records must reproduce the reference stream."""
    data = oracle.gen_zipf(30000, K=256, s=1.2, seed=8)
    for fmt, sb, recsize in ((FMT_BYTE, 14, 16), (FMT_BYTE, 16, 16), (FMT_R64, 14, 24)):
        f, cum = R.normalize_freqs(R.count_freqs(data, 256), 1 << sb)
        m = R.Model(None, fmt, f, sb)
        enc = m.table(R.TAB_ENC_SYMBOLS)
        dec = m.table(R.TAB_DEC_SYMBOLS)
        assert enc.size == 256 * recsize
        M = 1 << sb
        for s in range(256):
            fr, st = int(f[s]), int(cum[s])
            if fmt == FMT_R64:
                rcp, freq, bias, cmpl, shift = np.frombuffer(enc[s * 24:(s + 1) * 24].tobytes(), dtype="<u8,<u4,<u4,<u4,<u4")[0]
                dstart, dfreq = np.frombuffer(dec[s * 8:(s + 1) * 8].tobytes(), dtype="<u4")
                assert (freq, cmpl) == (fr, M - fr) and (dstart, dfreq) == (st, fr)
                xs = [(1 << 31) + 12345, (1 << 40) + 999, ((1 << (63 - sb)) * max(fr, 1)) - 1]
            else:
                x_max, rcp, bias, cmpl, shift = np.frombuffer(enc[s * 16:(s + 1) * 16].tobytes(), dtype="<u4,<u4,<u4,<u2,<u2")[0]
                dstart, dfreq = np.frombuffer(dec[s * 4:(s + 1) * 4].tobytes(), dtype="<u2")
                assert int(x_max) == (((1 << 23) >> sb) << 8) * fr and (dstart, dfreq) == (st & 0xffff, fr)
                xs = [(1 << 23) + 77, (1 << 23) * 3 + 5, max(int(x_max) - 1, 1 << 23)]
            if fr == 0:
                continue
            for x in xs:  # q*cmpl + x + bias == C(s,x) for every renormalised x
                bits = 64 if fmt == FMT_R64 else 32
                q = ((x * int(rcp)) >> bits) >> int(shift)
                assert x + int(bias) + q * int(cmpl) == ((x // fr) << sb) + (x % fr) + st, (fmt, s, x)


def test_layout_arithmetic():
    assert R.num_chunks(0, 100) == 0 and R.num_chunks(1, 100) == 1 and R.num_chunks(100, 100) == 1
    assert R.num_chunks(101, 100) == 2
    for fmt in range(4):
        for chunk, ways in ((1, 1), (4096, 64), (32768, 256), (5, 512)):
            b = R.chunk_bound(fmt, chunk, ways)
            assert b % 16 == 0 and b >= chunk * (4 if fmt == FMT_R64 else 2) + ways * (8 if fmt == FMT_R64 else 4)
        assert R.encode_bound(fmt, 10 * 4096 + 7, 64, 4096) == 10 * R.chunk_bound(fmt, 4096, 64) + R.chunk_bound(fmt, 7, 64)
    assert R.ways_supported(FMT_WORD, 64) and R.ways_supported(FMT_BYTE, 1) and R.ways_supported(FMT_R64, 512)
    assert R.ways_supported(FMT_WORD, 100) and R.ways_supported(FMT_ALIAS, 300)
    assert not R.ways_supported(FMT_WORD, 0) and not R.ways_supported(FMT_WORD, 513) and not R.ways_supported(FMT_WORD, 1024)


def test_model_rejections():
    f = np.zeros(256, np.uint32)
    f[3] = 4096
    with pytest.raises(R.RansAmdError) as e:
        R.Model(None, FMT_WORD, f, 12)
    assert e.value.status == R.E_MODEL  # one symbol owns the whole range
    f[3] = 4095
    with pytest.raises(R.RansAmdError):
        R.Model(None, FMT_WORD, f, 12)  # sum != M
    f[4] = 1
    R.Model(None, FMT_WORD, f, 12)
    assert R.Model(None, FMT_WORD, np.full(1024, 4, np.uint32), 12).sym_bytes == 2  # beyond 256 symbols: u16
    with pytest.raises(R.RansAmdError) as e:
        R.Model(None, FMT_WORD, f, 13)  # word format is 12-bit only (rans_word_sse41.h:37)
    assert e.value.status == R.E_UNSUPPORTED
    with pytest.raises(R.RansAmdError):
        R.Model(None, FMT_BYTE, f, 17)  # rans_byte.h:176
    # rans64 takes scale_bits up to 31 (rans64.h:169); beyond 16 there is no cum2sym table to export
    g = np.zeros(256, np.uint32)
    g[1], g[2] = (1 << 31) - 5, 5
    wide = R.Model(None, FMT_R64, g, 31)
    assert wide.table(R.TAB_CUM_FREQS, np.uint32)[-1] == 1 << 31
    enc = wide.table(R.TAB_ENC_SYMBOLS)
    assert enc.size == 256 * 24
    with pytest.raises(R.RansAmdError):
        wide.table(R.TAB_CUM2SYM)
    with pytest.raises(R.RansAmdError) as e:
        R.Model(None, FMT_R64, g, 32)
    assert e.value.status == R.E_UNSUPPORTED


def test_build_model_o0_host_only(oracle):
    """count + normalise + tables in one call (host symbols, host-only model)."""
    import ctypes as C
    data = oracle.gen_zipf(40000, K=256, s=1.0, seed=11)
    out = C.c_void_p()
    freqs = np.zeros(256, np.uint32)
    rc = R.lib().rans_amd_build_model_o0(None, FMT_BYTE, data.ctypes.data, data.size, 0, 256, 14,
                                         freqs.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out), None)
    assert rc == R.OK and out.value
    f_o, _ = oracle.normalize(oracle.count_freqs(data, 256), 1 << 14)
    assert np.array_equal(freqs, f_o)
    assert R.lib().rans_amd_model_format(out) == FMT_BYTE and R.lib().rans_amd_model_scale_bits(out) == 14
    R.lib().rans_amd_model_destroy(out)
    assert R.lib().rans_amd_encode_workspace_bytes(FMT_WORD, 10 * 4096, 64, 4096) == 10 * R.chunk_bound(FMT_WORD, 4096, 64) + 64


def test_sized_slot_bounds_are_pure_arithmetic():
    """rans_amd_encode_sized_bound (no GPU needed): n_chunks sized slots + room for the named number of overflowed chunks in
    worst-case slots; a slot at or above the worst case is the plain slot layout; rans_amd_tight_slot_bytes(NULL) = 0."""
    import ctypes as C
    L = R.lib()
    for fmt, n, ways, chunk in ((R.FMT_WORD, 1 << 20, 64, 16384), (R.FMT_R64, 300000, 2, 512), (R.FMT_ALIAS, 12345, 128, 4096),
                                (R.FMT_BYTE, 5, 64, 4096)):
        nchunks = R.num_chunks(n, chunk)
        worst = R.slot_bytes(fmt, n, ways, chunk)
        assert worst % 64 == 0 and worst >= R.chunk_bound(fmt, min(n, chunk), ways)
        assert R.encode_slots_bound(fmt, n, ways, chunk) == nchunks * worst
        for slot in (64, 640, worst - 64):
            if slot <= 0 or slot >= worst:
                continue
            for k in (0, 1, nchunks, nchunks + 7):
                assert R.encode_sized_bound(fmt, n, ways, chunk, slot, k) == nchunks * slot + min(k, nchunks) * worst
        for slot in (0, worst, worst + 64):
            assert R.encode_sized_bound(fmt, n, ways, chunk, slot, 3) == nchunks * worst
    assert R.encode_sized_bound(R.FMT_WORD, 0, 64, 4096, 640, 3) == 16
    assert L.rans_amd_tight_slot_bytes(None, 64, 4096) == 0
