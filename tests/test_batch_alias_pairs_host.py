"""Ragged batches with thirty-two 2-way alias streams per wave (RANS_AMD_OPT_BATCH_ALIAS_PAIRS), the part that needs no GPU:
the option's constant in the header's second enum, the registry's second list held to ALIAS_PAIR_ROWS with the first list left
as it was, the proof that the rate inputs of tests/test_gpu_batch_alias_pairs.py reach the ring's bound as ALIAS streams, and a
plain-integer model of the kernel's symbol step held to the reference's formula on the oracle's tables."""
import os
import re
import subprocess

import numpy as np

import _batch as G
import _batch_alias_pairs as A
import _stream_rate as S
import ryg_rans_amd as R
from _kernel_rows import CSRC, OPTIONS, PAIR_SHAPES, ROOT, registry
from _oracle import FMT_ALIAS, FMT_BYTE


def test_batch_alias_pairs_option_constant():
    """RANS_AMD_OPT_BATCH_ALIAS_PAIRS is 11 in the header's SECOND enum and in the package; the first enum still holds its
    eleven options where they were (tests/_kernel_rows.py's check_option_constant counts exactly those); the version has not
    moved (additions only); and a NULL context is refused before the option is looked at."""
    header = open(os.path.join(ROOT, "include", "ryg_rans_amd.h")).read()
    assert A.OPT_BATCH_ALIAS_PAIRS == R.OPT_BATCH_ALIAS_PAIRS == 11 == len(OPTIONS) and A.OPTIONS_MORE == ("BATCH_ALIAS_PAIRS",)
    first = re.search(r"enum rans_amd_option \{(.*?)\n\};", header, re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", first, re.M)] == list(zip(OPTIONS, range(11)))
    more = re.search(r"\};\n[^\n]*\nenum rans_amd_option_more \{(.*?)\n\};\nint rans_amd_ctx_set_option", header, re.S)
    assert more, "the second enum does not stand directly behind the first, in front of rans_amd_ctx_set_option"
    assert re.findall(r"^    RANS_AMD_OPT_(\w+)\s*=\s*(\d+)", more.group(1), re.M) == [("BATCH_ALIAS_PAIRS", "11")]
    for v, n in enumerate(OPTIONS + A.OPTIONS_MORE):
        assert getattr(R, "OPT_" + n) == v, n
    assert re.search(r"#define\s+RANS_AMD_VERSION\s+600\b", header)
    assert R.lib().rans_amd_ctx_set_option(None, 11, 1) == R.E_ARG
    assert b"ctx is NULL" in R.lib().rans_amd_last_error()


def test_no_alias_pair_batch_kernel_without_a_row():
    """The second list prints exactly one line; its family's names are the decode names of ALIAS_PAIR_ROWS, in both directions
    (the driver itself fails unless the id is kKernelEntryCount + 1 and leads back to its row, and on a name or family of the
    first list); the rows are the pair shapes with the wave encoder; and the check has teeth: without the main row the name is
    reported missing."""
    assert A.second_list() == [("batch_alias_pairs_decode", "k_decode_batch_alias_pairs")]
    d = A.ALIAS_PAIRS
    A.check_second_list_rows(d)
    assert d.option == 11 and d.side == "decode" and d.fmt == FMT_ALIAS and d.ways == 2 and d.streams == 32
    assert d.main is A.AMAIN and d.main["sb"] == 16 and d.wave_kernel == "k_decode_batch<alias>" and d.shapes == PAIR_SHAPES
    assert d.graph == ("FMT_ALIAS", 16, "OPT_BATCH_ALIAS_PAIRS")
    assert [(r["id"], r["sb"], r["K"]) for r in A.ALIAS_PAIR_ROWS] == [
        ("alias-2-pairs", 16, 256), ("alias-2-pairs-14bit", 14, 256), ("alias-2-pairs-12bit", 12, 256), ("alias-2-pairs-8bit", 8, 256),
        ("alias-2-pairs-64sym-10bit", 10, 64)]
    assert all(r["decode"] == A.KERNEL and r["encode"] == "k_encode_batch<alias, LDS remap>" for r in A.ALIAS_PAIR_ROWS)
    try:
        A.check_second_list_rows(d, rows=[r for r in d.rows if not r["id"].startswith(d.main["id"])])
    except AssertionError as e:
        assert "k_decode_batch_alias_pairs" in str(e) and "kernels no row expects" in str(e)
    else:
        raise AssertionError("a name without a row went unnoticed")
    src = open(os.path.join(CSRC, "kernel_names.hpp")).read()
    assert src.count('"k_decode_batch_alias_pairs"') == 1


def test_the_id_follows_the_first_list(tmp_path):
    """The second list's one id is kKernelEntryCount + 1 = 54, ids of both lists lead to their rows, and an identifier in
    neither list does not compile."""
    src = tmp_path / "id.cpp"
    src.write_text('#include "kernel_names.hpp"\nusing namespace rans_amd;\n'
                   'static_assert((int)KernelId::decode_batch_alias_pairs == kKernelEntryCount + 1 && kKernelEntryCount == 53, "id");\n'
                   'static_assert(kAliasPairKernelEntryCount == 1, "one entry");\n'
                   'static_assert(kernel_entry(KernelId::decode_batch_alias_pairs).family == KernelFamily::batch_alias_pairs_decode, "row");\n'
                   'static_assert(kernel_entry(KernelId::encode_batch_r64_lanes).family == KernelFamily::batch_r64_lanes_encode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_word64).family == KernelFamily::uniform, "row");\n'
                   'int main() { return 0; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)]).returncode == 0
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::decode_batch_alias_pairs_no_such; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "decode_batch_alias_pairs_no_such" in r.stderr


def test_the_first_list_prints_what_it_printed():
    """The first list's 53 lines, family and name, are the ones it printed before this family: the uniform kernels, the batch
    kernels, the per-stream-model kernels and the six streams-per-wave families in their order, the lane encoder last -- and the
    new name and family are not among them."""
    registry()
    exe = os.path.join(ROOT, "build", "kernel_names", "kernel_names_driver")
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 53 and not [ln for ln in lines if "alias_pairs" in ln]
    families = [ln.split("\t")[0] for ln in lines]
    assert families == ["uniform"] * 30 + ["batch"] * 13 + ["batch_models"] * 4 + [
        "batch_word_groups_decode", "batch_word_groups_encode", "batch_byte_pairs_decode", "batch_byte_pairs_encode", "batch_r64_lanes_decode",
        "batch_r64_lanes_encode"]
    assert lines[0] == "uniform\tk_decode_word64" and lines[37] == "batch\tk_decode_batch<alias>"
    assert lines[47:] == ["batch_word_groups_decode\tk_decode_batch_word_groups", "batch_word_groups_encode\tk_encode_batch_word_groups",
                          "batch_byte_pairs_decode\tk_decode_batch_byte_pairs", "batch_byte_pairs_encode\tk_encode_batch_byte_pairs",
                          "batch_r64_lanes_decode\tk_decode_batch_r64_lanes", "batch_r64_lanes_encode\tk_encode_batch_r64_lanes"]
    assert all(A.KERNEL not in names for names in registry().values())


def _alias_rounds(oracle, freqs, sb, syms):
    """The oracle's 2-way alias stream of `syms`, decoded by the plain-integer model -> bytes per round."""
    om = oracle.model(freqs, sb, with_alias=True)
    out, per_round = A.decode_rounds(om, sb, oracle.encode(FMT_ALIAS, om, syms, 2), syms.size)
    assert np.array_equal(out, syms)
    return per_round


def test_rate_inputs_reach_the_rings_bound_as_alias_streams(oracle):
    """255 x 1 + one common symbol (tests/_batch.py rate_model), the ORACLE's 2-way alias streams, decoded on the CPU with the
    kernel's symbol step and the byte format's renormalisation, counting the bytes of every round.
      * An alias stream renormalises as a byte stream does, and a frequency-1 symbol leaves x >> scale_bits whatever its slot:
        at 16 bits a state in [2^23, 2^31) falls below 2^15 and takes two bytes in EVERY round -- 4 bytes per round and pair,
        32 in every window of eight rounds wherever it starts: what one refill of the ring brings.
      * At 14 bits the same streams take what tests/_stream_rate.py predicts for the BYTE format round for round (the encoder's
        threshold for a frequency-1 symbol, 2^17, is a multiple of 2^14: the low bits, where the alias remap differs, decide
        nothing): 28 bytes in every window, 8 rounds x 2 states x 14 bits.
      * At 16 bits a common-only stream of the batch takes nothing at all, and the 65536-symbol one of the single wave-load
        nothing for more than a thousand rounds.
    The inputs are the GPU file's own generators."""
    for sb in G.RATE_BITS:
        assert A.ALIAS_PAIR_RATE_ROW[sb]["sb"] == sb and A.ALIAS_PAIR_RATE_ROW[sb]["fmt"] == FMT_ALIAS
        freqs, counts, contents, _ = G.rate_batch(sb)
        assert np.array_equal(freqs, G.rate_model(sb))
        rare_long = silent = 0
        for k in range(G.RATE_STREAMS):
            n = int(counts[k])
            rb = _alias_rounds(oracle, freqs, sb, contents[k])
            if G.rate_kind(k) == "rare":
                assert np.all(freqs[contents[k]] == 1)
                assert np.array_equal(rb, S.round_bytes(FMT_BYTE, freqs, sb, contents[k], 2)), (sb, k)
                if n // 2 >= 8:
                    w = S.windows(rb[:n // 2])
                    if sb == 16:
                        assert np.all(rb[:n // 2] == 4) and w.min() == 32 and w.max() == 32, (k, n, w.min(), w.max())
                    else:
                        assert w.min() == 28 and w.max() == 28, (k, n, w.min(), w.max())
                    rare_long += 1
            else:
                assert np.all(contents[k] == S.COMMON)
                if sb == 16:  # (at 14 bits a common symbol costs 0.023 bits: a byte every 350 rounds or so)
                    assert rb.sum() == 0 and S.longest_silence(rb) == (n + 1) // 2, (sb, k)
                    silent += n > 0
        assert rare_long >= 20 and silent >= (12 if sb == 16 else 0), (sb, rare_long, silent)
    for name, (w_counts, w_kinds) in G.RATE_WAVES.items():
        freqs, counts, contents, _ = G.rate_wave(16, name)
        for k in (0, 1, 17):  # the 65536-symbol stream and two of its wave-mates
            n = int(counts[k])
            rb = _alias_rounds(oracle, freqs, 16, contents[k])
            if w_kinds[k] == "rare":
                if n // 2 >= 8:
                    w = S.windows(rb[:n // 2])
                    assert w.min() == 32 and w.max() == 32, (name, k, n)
            elif n >= 2000:
                assert S.longest_silence(rb) >= 1000, (name, k, S.longest_silence(rb))
            else:
                assert rb.sum() == 0, (name, k)
    assert any(c >= 2000 and kd == "common" for cs, kds in G.RATE_WAVES.values() for c, kd in zip(cs, kds))


def test_symbol_step_model_is_the_reference_formula(oracle):
    """The kernel's symbol step as plain integers (tests/_batch_alias_pairs.py kernel_step: RANS_A_ROUND's instructions in
    order, on the tables the library builds from the oracle's) returns the symbol and the next state of RansDecGetAlias
    (main_alias.cpp:252-267) on the oracle's tables: for each row's model -- the zipf model the GPU file's batches use and the
    rate model -- over EVERY slot value x & mask under high parts across the working range [2^23, 2^31): three of them at 16
    bits, nine otherwise.  And for ANY 32-bit state the two gathers stay inside the tables."""
    for row in A.ALIAS_PAIR_ROWS:
        sb, K = row["sb"], row["K"]
        log2n = K.bit_length() - 1
        zipf = oracle.gen_zipf(1 << 20, K=K, s=1.0, seed=1)
        models = [oracle.normalize(oracle.count_freqs(zipf, K), 1 << sb)[0]]
        if K == 256 and sb > 8:
            models.append(G.rate_model(sb))
        for freqs in models:
            om = oracle.model(freqs, sb, with_alias=True)
            tables = A.device_tables(om)
            low = np.arange(1 << sb, dtype=np.uint64)
            top = (1 << (31 - sb)) - 1
            highs = [1 << (23 - sb), top, (1 << (27 - sb)) + 12345 % (1 << (23 - sb))]
            if sb < 16:
                highs += [(1 << (23 - sb)) + 1, top - 1, 3 << (24 - sb), 5 << (25 - sb), (1 << (29 - sb)) + 77, (1 << (30 - sb)) + 1]
            for hi in highs:
                assert (1 << 23) <= (hi << sb) < (1 << 31)
                x = (np.uint64(hi) << np.uint64(sb)) | low
                s_k, x_k = A.kernel_step(tables, sb, log2n, x)
                s_r, x_r = A.reference_step(om, sb, log2n, x)
                assert np.array_equal(s_k, s_r) and np.array_equal(x_k, x_r), (row["id"], hi)
                # every slot decodes to a symbol that owns it: freq * q + (position inside the symbol's range)
                f = np.asarray(freqs, dtype=np.uint64)[s_k.astype(np.int64)]
                assert np.all(f > 0) and np.all(x_k - f * np.uint64(hi) < f), (row["id"], hi)
            # free-running pairs: any 32-bit state indexes inside both tables (numpy would raise on an index outside them)
            wild = np.random.default_rng(5).integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
            wild[:4] = (0, 0xffffffff, 0x80000000, (1 << sb) - 1)
            s_w, _ = A.kernel_step(tables, sb, log2n, wild)
            assert tables[0].size == K and tables[1].size == tables[2].size == 2 * K and int(s_w.max()) < K
