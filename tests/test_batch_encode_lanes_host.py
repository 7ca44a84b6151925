"""Ragged batches CODED with sixty-four 2-way rans64 streams per wave (RANS_AMD_OPT_BATCH_ENCODE_LANES), the part that needs no
GPU: the option's constant, the registry's family held to ENC_LANE_ROWS, the family's id at the end of the one list, the proof
that the rate inputs of tests/test_gpu_batch_encode_lanes.py reach the bounds that file claims, and every stream of that file's
wave-loads inside its slot under the oracle."""
import os
import subprocess

import numpy as np

import _batch_encode_lanes as E
import _batch_lanes as L
import _stream_rate as S
import ryg_rans_amd as R
from _batch import no_zero_batch
from _kernel_rows import (BATCH_R64_LANES_ENCODE, CSRC, ENC_LANE_ROWS, ENC_LANES, LANE_SHAPES, check_family_rows, check_option_constant,
                          registry)
from _oracle import FMT_R64


def test_batch_encode_lanes_option_constant():
    check_option_constant("BATCH_ENCODE_LANES", 10)


def test_no_lane_batch_enc_kernel_without_a_row():
    """The family holds exactly one name; the family's names are the encode names of ENC_LANE_ROWS, in both directions; the rows
    are LANE_SHAPES with the wave decoder; and the check has teeth: without its rows the name is reported missing
    (check_family_rows)."""
    d = ENC_LANES
    check_family_rows(d)
    assert registry()[BATCH_R64_LANES_ENCODE] == {"k_encode_batch_r64_lanes"}
    assert d.option == 10 and d.side == "encode" and d.fmt == FMT_R64 and d.ways == 2 and d.streams == 64
    assert d.main["sb"] == 14 and d.wave_kernel == "k_encode_batch<r64>" and d.shapes == LANE_SHAPES
    assert d.graph == ("FMT_R64", 14, "OPT_BATCH_ENCODE_LANES")
    assert all(r["decode"] == "k_decode_batch<r64>" and r["encode"] == "k_encode_batch_r64_lanes" for r in ENC_LANE_ROWS)
    src = open(os.path.join(CSRC, "kernel_names.hpp")).read()
    assert src.count('"k_encode_batch_r64_lanes"') == 1


def test_the_id_follows_the_first_list(tmp_path):
    """The lane encoder's id is the one list's last, 53 as it was behind a list of 52; both lane ids lead to their own
    families; and an identifier that is in no list does not compile."""
    src = tmp_path / "id.cpp"
    src.write_text('#include "kernel_names.hpp"\nusing namespace rans_amd;\n'
                   'static_assert((int)KernelId::encode_batch_r64_lanes == 53 && kKernelEntryCount == 53, "id");\n'
                   'static_assert(kernel_entry(KernelId::encode_batch_r64_lanes).family == KernelFamily::batch_r64_lanes_encode, "row");\n'
                   'static_assert(kernel_entry(KernelId::decode_batch_r64_lanes).family == KernelFamily::batch_r64_lanes_decode, "row");\n'
                   'int main() { return 0; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)]).returncode == 0
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::encode_batch_r64_lanes_no_such; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "encode_batch_r64_lanes_no_such" in r.stderr


def test_rate_inputs_reach_the_rings_bound():
    """255 x 1 and one common symbol at 2^16, 2-way rans64, coder's view (rans64.h:83-94).
      * Rans64EncPut with freq 1 at 16 bits: x_max = 2^47; a state in [2^31, 2^47) emits nothing and becomes x << 16 + start, in
        [2^47, 2^63); from there it emits one dword (x >>= 32: [2^15, 2^31)) and is back in [2^31, 2^47).  So a state emits
        exactly one dword every SECOND symbol, from Rans64EncInit's 2^31 on: four dwords per state and 16-symbol group, 32
        bytes for both states, in EVERY group -- half the 64 bytes a group can emit at the most and a line every second
        group, the rate at which the ring's 128 bytes and the flush behind every group are exercised hardest by valid input
        (S.group_bytes over every window of eight rounds, wherever the group boundary falls);
      * a common symbol costs 0.0056 bits: the common-only streams of the batch take nothing at all, and the 65536-symbol one
        is silent for more than a thousand rounds in a row -- its lane asks for no line while its quad-mates flush;
      * the burst streams (runs of 16 rare and 16 common symbols) have groups at 32 bytes and silent rounds in one stream.
    The inputs are the GPU file's own generators (L.rate_batch, E.rate_wave)."""
    assert S.rare_group_bytes(FMT_R64, 16, 2) == (32, 32)
    freqs, counts, contents, _ = L.rate_batch(16)
    assert np.array_equal(freqs, S.lane_model(16)) and counts.size == 64
    kinds = [L.rate_kind(k) for k in range(64)]
    at_bound = silent = burst_both = 0
    for k in range(64):
        n = int(counts[k])
        rb = S.round_bytes(FMT_R64, freqs, 16, contents[k], 2)
        full = rb[:n // 2]  # rounds with both states
        if kinds[k] == "rare":
            assert np.all(freqs[contents[k]] == 1)
            if n >= 16:
                w = S.group_bytes(full, 2)
                assert w.size >= 1 and w.min() == 32 and w.max() == 32, (k, n, w.min(), w.max())
                at_bound += 1
        elif kinds[k] == "common":
            assert np.all(contents[k] == S.COMMON) and rb.sum() == 0, (k, n)
            silent += n > 0
        elif n >= 64:
            w = S.group_bytes(full, 2)
            assert w.max() == 32 and S.longest_silence(rb) >= 7, (k, n, w.max(), S.longest_silence(rb))
            burst_both += 1
    assert at_bound >= 12 and silent >= 12 and burst_both >= 8, (at_bound, silent, burst_both)
    # one dword every second symbol per state: the units of every state in every round of a rare-only stream alternate 0, 1
    k = next(k for k in range(64) if kinds[k] == "rare" and counts[k] >= 320)
    per_state = np.asarray(S.simulate(FMT_R64, freqs, 16, contents[k][:320], 2, per_state=True)[2])
    assert per_state.shape == (160, 2) and set(np.unique(per_state).tolist()) == {0, 1}
    assert np.all(per_state[:-1] + per_state[1:] == 1), "a state emits in two rounds running, or in neither"
    # the 14-bit batch is the same input under 255 x 1 + 16129: 24 to 32 bytes per group
    freqs14, _, contents14, _ = L.rate_batch(14)
    assert S.rare_group_bytes(FMT_R64, 14, 2) == (24, 32)
    w = S.group_bytes(S.round_bytes(FMT_R64, freqs14, 14, contents14[k], 2)[:int(counts[k]) // 2], 2)
    assert w.min() >= 24 and w.max() == 32
    # the two waves: a rare-only stream of 65536 beside common-only ones, and the inverse
    for name, (w_counts, w_kinds) in E.RATE_WAVES.items():
        freqs, counts, contents = E.rate_wave(16, name)
        assert counts.size == 64 and counts[0] == 65536 and len(w_kinds) == 64
        for k in range(64):
            n = int(counts[k])
            rb = S.round_bytes(FMT_R64, freqs, 16, contents[k], 2)
            if w_kinds[k] == "rare":
                assert np.all(freqs[contents[k]] == 1)
                w = S.group_bytes(rb[:n // 2], 2)
                assert w.size >= 1 and w.min() == 32 and w.max() == 32, (name, k, n)
            elif n == 65536:
                assert S.longest_silence(rb) >= 1000, (name, k, S.longest_silence(rb))
            else:
                assert rb.sum() == 0, (name, k)
        if name == "stalled-beside-draining":  # the rare streams drain one after another: sixteen different block counts
            assert len({int(c) >> 6 for c in counts[1:]}) == 16
    # the no-zero batch of the model-flag tests: byte value 0 has no record and no content holds it; three wave-loads whose
    # lanes finish at different blocks, some dead from the start
    freqs, counts, contents = no_zero_batch(*E.NO_ZERO_LANE_LOADS)
    assert freqs[0] == 0 and int(freqs.sum()) == 1 << 14 and counts.size == 192 and int(np.count_nonzero(counts == 0)) >= 1
    assert all(contents[k].size == counts[k] and not np.any(contents[k] == 0) for k in range(192))
    assert len({int(c) >> 6 for c in counts[64:128]}) >= 12 and counts[64:128].max() >= 256


def test_every_wave_load_stays_inside_its_slots(oracle):
    """Every stream of the GPU file's wave-loads and rate inputs, coded by the oracle, is no longer than
    rans_amd_chunk_bound(R64, count, 2) = align16(4 count + 16) -- a dword per symbol at the most and the two flushed
    states --, which is the size of its slot in rans_amd_batch_layout at every alignment the GPU file uses."""
    def check(freqs, sb, counts, contents, what):
        om = oracle.model(np.ascontiguousarray(freqs, dtype=np.uint32), sb)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        slots = None
        for align in E.ALIGNS:
            sym_offs, slot_offs = R.batch_layout(counts, FMT_R64, 2, align)
            assert np.all(sym_offs[:-1] % align == 0) and np.all(slot_offs % 16 == 0)
            assert slots is None or np.array_equal(slots, slot_offs)
            slots = slot_offs
        sizes = np.diff(slots.astype(np.int64))
        for c in range(counts.size):
            n = int(counts[c])
            assert sizes[c] == R.chunk_bound(FMT_R64, n, 2) == (4 * n + 16 + 15) // 16 * 16, (what, c)
            ln = oracle.encode(FMT_R64, om, contents(c, n), 2).size
            assert 16 <= ln <= sizes[c] and ln % 4 == 0, (what, c, n, ln, int(sizes[c]))

    zipf = oracle.gen_zipf(1 << 20, K=256, s=1.0, seed=1)
    f14, _ = oracle.normalize(oracle.count_freqs(zipf, 256), 1 << 14)
    for name, counts in E.WAVE_LOADS.items():
        assert len(counts) >= 64
        check(f14, 14, counts, lambda c, n: zipf[1000 * c:1000 * c + n], name)
    for sb in (16, 14):
        freqs, counts, contents, _ = L.rate_batch(sb)
        check(freqs, sb, counts, lambda c, n: contents[c], "rate_batch %d" % sb)
    for name in E.RATE_WAVES:
        freqs, counts, contents = E.rate_wave(16, name)
        check(freqs, 16, counts, lambda c, n: contents[c], name)
    # the worst case itself: rare-only at 16 bits takes exactly a dword every second symbol per state -- half the bound
    freqs, counts, contents = E.rate_wave(16, "fast-beside-dead")
    ln = oracle.encode(FMT_R64, oracle.model(freqs, 16), contents[0], 2).size
    assert ln == 2 * 65536 + 16, ln
