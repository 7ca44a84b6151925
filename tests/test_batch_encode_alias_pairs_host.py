"""Ragged batches CODED with thirty-two 2-way alias streams per wave (RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS), the part that needs
no GPU: the option's constant in the header's THIRD enum, the registry's third list held to ENC_ALIAS_PAIR_ROWS with the first
two lists left as they were, a plain-integer model of the kernel's put step held to the reference's formula on the oracle's
tables, the proof that the rate inputs of tests/test_gpu_batch_encode_alias_pairs.py reach the ring's bound as ALIAS streams, and
the launcher's LDS plan as plain arithmetic."""
import os
import re
import subprocess

import numpy as np

import _batch as G
import _batch_alias_pairs as A
import _batch_encode_alias_pairs as E
import _stream_rate as S
import ryg_rans_amd as R
from _kernel_rows import CSRC, OPTIONS, PAIR_SHAPES, ROOT, registry
from _oracle import FMT_ALIAS


def test_batch_encode_alias_pairs_option_constant():
    """RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS is 12 in the header's THIRD enum, which stands behind the declaration of
    rans_amd_ctx_set_option, and in the package; the first enum still holds its eleven options and the second exactly
    BATCH_ALIAS_PAIRS = 11, directly in front of the declaration; the version has not moved (additions only); and a NULL context
    is refused before the option is looked at."""
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    assert E.OPT_BATCH_ENCODE_ALIAS_PAIRS == R.OPT_BATCH_ENCODE_ALIAS_PAIRS == 12 == len(OPTIONS) + len(A.OPTIONS_MORE)
    assert E.OPTIONS_THIRD == ("BATCH_ENCODE_ALIAS_PAIRS",)
    first = re.search(r"enum rans_amd_option \{(.*?)\n\};", header, re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", first, re.M)] == list(zip(OPTIONS, range(11)))
    more = re.search(r"\};\n[^\n]*\nenum rans_amd_option_more \{(.*?)\n\};\nint rans_amd_ctx_set_option\(", header, re.S)
    assert more and re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", more.group(1), re.M) == [("BATCH_ALIAS_PAIRS", "11")]
    third = re.search(r"\nint rans_amd_ctx_set_option\([^\n]*\);\n[^\n]*\nenum rans_amd_option_third \{(.*?)\n\};", header, re.S)
    assert third, "the third enum does not stand behind the declaration of rans_amd_ctx_set_option"
    assert re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", third.group(1), re.M) == [("BATCH_ENCODE_ALIAS_PAIRS", "12")]
    assert "k_encode_batch_alias_pairs" in third.group(1)
    assert len(re.findall(r"^enum rans_amd_option", header, re.M)) == 3
    for v, n in enumerate(OPTIONS + A.OPTIONS_MORE + E.OPTIONS_THIRD):
        assert getattr(R, "OPT_" + n) == v, n
    assert re.search(r"#define\s+RANS_AMD_VERSION\s+600\b", header)
    assert R.lib().rans_amd_ctx_set_option(None, 12, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()


def test_no_alias_pair_batch_enc_kernel_without_a_row():
    """The third list is exactly one line; its family's names are the encode names of ENC_ALIAS_PAIR_ROWS, in both directions
    (the driver itself fails unless the id is kKernelEntryCount + kAliasPairKernelEntryCount + 1 and leads back to its row, and
    on a name or family of the first two lists); the rows are the pair shapes with the wave decoder; and the check has teeth:
    without the main row the name is reported missing.  The first two lists are as they were."""
    assert E.third_list() == [("batch_alias_pairs_encode", "k_encode_batch_alias_pairs")]
    assert A.second_list() == [("batch_alias_pairs_decode", "k_decode_batch_alias_pairs")]
    d = E.ENC_ALIAS_PAIRS
    E.check_third_list_rows(d)
    assert d.option == 12 and d.side == "encode" and d.fmt == FMT_ALIAS and d.ways == 2 and d.streams == 32
    assert d.main is E.EAMAIN and d.main["sb"] == 16 and d.wave_kernel == "k_encode_batch<alias, LDS remap>" and d.shapes == PAIR_SHAPES
    assert d.graph == ("FMT_ALIAS", 16, "OPT_BATCH_ENCODE_ALIAS_PAIRS")
    assert [(r["sb"], r["K"]) for r in E.ENC_ALIAS_PAIR_ROWS] == [(16, 256), (14, 256), (12, 256), (8, 256), (10, 64)]
    assert all(r["encode"] == E.KERNEL and r["decode"] == "k_decode_batch<alias>" for r in E.ENC_ALIAS_PAIR_ROWS)
    try:
        E.check_third_list_rows(d, rows=[])
    except AssertionError as e:
        assert "k_encode_batch_alias_pairs" in str(e) and "kernels no row expects" in str(e)
    else:
        raise AssertionError("a name without a row went unnoticed")
    try:  # (dropping the main row alone: the other rows still name the kernel, the shapes say what is missing)
        E.check_third_list_rows(d, rows=[r for r in d.rows if r is not d.main])
    except AssertionError:
        pass
    else:
        raise AssertionError("the missing main row went unnoticed")
    src = open(os.path.join(CSRC, "kernel_names.hpp")).read()
    assert src.count('"k_encode_batch_alias_pairs"') == 1 and src.count('"k_decode_batch_alias_pairs"') == 1
    registry()
    exe = os.path.join(ROOT, "build", "kernel_names", "kernel_names_driver")
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 53 and not [ln for ln in lines if "alias_pairs" in ln]
    assert lines[-1] == "batch_r64_lanes_encode\tk_encode_batch_r64_lanes"


def test_the_id_follows_the_second_list(tmp_path):
    """The third list's one id is 53 + 1 + 1 = 55, ids of all three lists lead to their rows, and an identifier in no list does
    not compile."""
    src = tmp_path / "id.cpp"
    src.write_text('#include "kernel_names.hpp"\nusing namespace rans_amd;\n'
                   'static_assert((int)KernelId::encode_batch_alias_pairs == 55 && kKernelEntryCount == 53 && kAliasPairKernelEntryCount == 1, "id");\n'
                   'static_assert(kAliasPairEncodeKernelEntryCount == 1, "one entry");\n'
                   'static_assert(kernel_entry(KernelId::encode_batch_alias_pairs).family == KernelFamily::batch_alias_pairs_encode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_batch_alias_pairs).family == KernelFamily::batch_alias_pairs_decode, "row");\n'
                   'static_assert(kernel_entry(KernelId::encode_batch_r64_lanes).family == KernelFamily::batch_r64_lanes_encode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_word64).family == KernelFamily::uniform, "row");\n'
                   'int main() { return 0; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)]).returncode == 0
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::encode_batch_alias_pairs_no_such; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "encode_batch_alias_pairs_no_such" in r.stderr


def _row_models(oracle, row):
    """The models a row's batches use: the zipf model of the GPU file's batches, the rate model (255 x 1 and one common symbol:
    at 16 bits the frequency 2^16 - 255) and, for 256 symbols, the mirrored and the no-zero model."""
    sb, K = row["sb"], row["K"]
    zipf = oracle.gen_zipf(1 << 20, K=K, s=1.0, seed=1)
    models = [oracle.normalize(oracle.count_freqs(zipf, K), 1 << sb)[0]]
    if K == 256 and sb > 8:
        models += [G.rate_model(sb), G.no_zero_model(sb)]
    if K == 256 and sb == 16:
        models.append(G.mirrored_model())
    return models


def test_put_step_model_is_the_reference_formula(oracle):
    """The kernel's put as plain integers (tests/_batch_encode_alias_pairs.py kernel_put: RANS_AE_ROUND's instructions in order
    on the records the prologue builds) equals ((x / freq) << scale_bits) + alias_remap[(x % freq) + start]
    (main_alias.cpp:249) on the oracle's tables: for every row and each of its models, EVERY (symbol, rem) pair -- all
    2^scale_bits of them -- under the smallest and the largest quotient of the range a state is in behind its
    renormalisation, [freq << (23 - scale_bits), freq << (31 - scale_bits)), and under drawn ones.  That covers frequency 1 (the
    8-bit row holds nothing else), frequency 2^16 - 255, and the 64-symbol row.  The gather's index is (x % freq) + start."""
    seen = set()
    for row in E.ENC_ALIAS_PAIR_ROWS:
        sb, K = row["sb"], row["K"]
        for freqs in _row_models(oracle, row):
            om = oracle.model(freqs, sb, with_alias=True)
            tables = E.device_records(om, sb)
            f = np.asarray(freqs, dtype=np.uint64)
            cum = om.table("cum", K + 1).astype(np.uint64)
            sym = np.repeat(np.arange(K), f.astype(np.int64))  # slot -> its symbol: every (symbol, rem) pair once
            rem = np.arange(1 << sb, dtype=np.uint64) - cum[sym]
            assert sym.size == 1 << sb and np.all(rem < f[sym])
            seen |= set(int(v) for v in np.unique(f))
            q_lo, q_hi = 1 << (23 - sb), (1 << (31 - sb)) - 1
            rng = np.random.default_rng(sb * 1000 + K)
            quotients = [np.full(sym.size, q_lo, dtype=np.uint64), np.full(sym.size, q_hi, dtype=np.uint64), np.full(sym.size, q_lo + 1, dtype=np.uint64),
                         np.full(sym.size, q_hi - 1, dtype=np.uint64)] + [rng.integers(q_lo, q_hi + 1, sym.size, dtype=np.uint64) for _ in range(3)]
            for q in quotients:
                x = q * f[sym] + rem
                assert int(x.min()) >= (int(f[f > 0].min()) << (23 - sb)) and int(x.max()) < (1 << 31)
                x_k, at = E.kernel_put(tables, sb, sym, x)
                assert np.array_equal(x_k, E.reference_put(om, sb, sym, x)), (row["id"], int(q[0]))
                assert np.array_equal(at, rem + cum[sym]), (row["id"], "the gather's index")
    assert 1 in seen and (1 << 16) - 255 in seen


def test_put_step_gathers_inside_the_table_whatever_the_lane_holds(oracle):
    """Dead pairs, pairs without a stream and byte values without a record run the sequence under full exec: for ANY byte value
    -- the 64-symbol row's 64..255 and the no-zero model's 0 have the no-record form -- and ANY 32-bit state, 0 and 0xffffffff
    among them, the model's gather index stays inside remap16 (numpy would raise on an index outside it).  A no-record value's
    record is {0, ~0, 0, ~0}: x_max = 0xffffffff, so its two compares pass for no state a stream can hold."""
    for row in E.ENC_ALIAS_PAIR_ROWS:
        sb, K = row["sb"], row["K"]
        for freqs in _row_models(oracle, row):
            tables = E.device_records(oracle.model(freqs, sb, with_alias=True), sb)
            rng = np.random.default_rng(7)
            x = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
            x[:6] = (0, 0xffffffff, 0x80000000, (1 << sb) - 1, 1 << 23, (1 << 31) - 1)
            sym = rng.integers(0, 256, x.size)
            sym[:6] = (255, 255, 0, 0, K - 1, K % 256)
            _, at = E.kernel_put(tables, sb, sym, x)
            assert int(at.max()) < (1 << sb) == tables[1].size
            none = np.nonzero(np.asarray([k >= K or freqs[k] == 0 for k in range(256)]))[0]
            assert none.size == (256 - K) + int(np.count_nonzero(np.asarray(freqs) == 0))
            for k in none:
                assert [int(tables[0][j][k]) for j in range(4)] == [0, 0xffffffff, 0, 0xffffffff]
            if none.size:
                _, at = E.kernel_put(tables, sb, np.resize(none, x.size), x)
                assert int(at.max()) < (1 << sb)


def test_rate_inputs_reach_the_rings_bound_as_alias_streams(oracle):
    """255 x 1 + one common symbol (tests/_batch.py rate_model), coded on the CPU with the kernel's records and put step
    (encode_rounds): every stream IS the oracle's 2-way alias stream of that input, byte for byte, and
      * at 16 bits a frequency-1-only stream emits two bytes per state in EVERY round -- 32 bytes in every window of eight
        full rounds, a block per check of the pair's ring, its bound; at 14 bits 28;
      * at 16 bits a common-only stream of the batch emits nothing, and the 65536-symbol one of the single wave-load nothing for
        a thousand rounds and more.
    The inputs are the GPU file's own generators."""
    for sb in G.RATE_BITS:
        assert E.ENC_ALIAS_PAIR_RATE_ROW[sb]["sb"] == sb and E.ENC_ALIAS_PAIR_RATE_ROW[sb]["fmt"] == FMT_ALIAS
        freqs, counts, contents, _ = G.rate_batch(sb)
        assert np.array_equal(freqs, G.rate_model(sb))
        om = oracle.model(freqs, sb, with_alias=True)
        tables = E.device_records(om, sb)
        rare_long = silent = 0
        for k in range(G.RATE_STREAMS):
            n = int(counts[k])
            stream, rb = E.encode_rounds(tables, sb, contents[k])
            assert np.array_equal(stream, oracle.encode(FMT_ALIAS, om, contents[k], 2)), (sb, k)
            if G.rate_kind(k) == "rare":
                assert np.all(freqs[contents[k]] == 1)
                if n // 2 >= 8:
                    w = S.windows(rb[:n // 2])
                    want = 32 if sb == 16 else 28
                    assert w.min() == want and w.max() == want, (sb, k, n, w.min(), w.max())
                    rare_long += 1
            else:
                assert np.all(contents[k] == S.COMMON)
                if sb == 16:
                    assert rb.sum() == 0 and S.longest_silence(rb) == (n + 1) // 2, (sb, k)
                    silent += n > 0
        assert rare_long >= 20 and silent >= (12 if sb == 16 else 0), (sb, rare_long, silent)
    om = oracle.model(G.rate_model(16), 16, with_alias=True)
    tables = E.device_records(om, 16)
    long_silent = 0
    for name, (w_counts, w_kinds) in G.RATE_WAVES.items():
        freqs, counts, contents, _ = G.rate_wave(16, name)
        for k in (0, 1, 17):  # the 65536-symbol stream and two of its wave-mates
            n = int(counts[k])
            stream, rb = E.encode_rounds(tables, 16, contents[k])
            assert np.array_equal(stream, oracle.encode(FMT_ALIAS, om, contents[k], 2)), (name, k)
            if w_kinds[k] == "rare":
                if n // 2 >= 8:
                    w = S.windows(rb[:n // 2])
                    assert w.min() == 32 and w.max() == 32, (name, k, n)
            elif n >= 2000:
                assert S.longest_silence(rb) >= 1000, (name, k, S.longest_silence(rb))
                long_silent += 1
            else:
                assert rb.sum() == 0, (name, k)
    assert long_silent >= 1
    # the dead pair's diet (finish_batch): byte value 0 under the mirrored model is a frequency-1 symbol, 32 bytes per window
    om = oracle.model(G.mirrored_model(), 16, with_alias=True)
    zeros = np.zeros(4096, dtype=np.uint8)
    stream, rb = E.encode_rounds(E.device_records(om, 16), 16, zeros)
    assert np.array_equal(stream, oracle.encode(FMT_ALIAS, om, zeros, 2))
    w = S.windows(rb)
    assert w.min() == 32 and w.max() == 32


def test_lds_plan():
    """pairs_plan.hpp's enc_alias_pairs_plan as plain arithmetic (a g++ driver prints it): 4 KiB of records + remap16 (2 <<
    scale_bits bytes) + 2176 bytes of rows per wave stay inside the CU's 160 KiB for scale_bits 8..16 (the records are padded to
    256 whatever the alphabet: both alphabets take the same plan); sixteen waves twice per CU up to 14 bits, once at 15; at 16
    bits 13 waves, once.  A block is never more than 1024 threads and never empty; past 16 bits there is no plan."""
    plan = E.lds_plan()
    cap, rows = 160 * 1024, 2176
    want = {8: (16, 2), 9: (16, 2), 10: (16, 2), 11: (16, 2), 12: (16, 2), 13: (16, 2), 14: (16, 2), 15: (16, 1), 16: (13, 1)}
    for sb in range(8, 17):
        tables, waves, lds, per_cu = plan[sb]
        assert tables == 4096 + (2 << sb) and lds == tables + waves * rows <= cap, sb
        assert (waves, per_cu) == want[sb] and per_cu * lds <= cap, (sb, waves, per_cu)
        assert waves == min(16, (cap - tables) // rows) and 1 <= waves <= 16
        assert per_cu == (2 if waves == 16 and 2 * lds <= cap else 1)
    assert plan[14][2] == 71680 and plan[15][2] == 104448 and plan[16][2] == 4096 + 131072 + 13 * rows == 163456
    assert plan[17] == (0, 0, 0, 0)
    for sb in range(0, 8):  # (not launched -- the launcher takes 8..16 --, but the arithmetic holds)
        assert plan[sb][1] == 16 and plan[sb][3] == 2
