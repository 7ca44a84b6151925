"""Ragged batches with sixty-four 2-way rans64 streams per wave (RANS_AMD_OPT_BATCH_LANES), the part that needs no GPU: the
option's constant, the registry's family held to LANE_ROWS, a pin of the registry's one list, the proof that the rate inputs of
tests/test_gpu_batch_lanes.py reach the bounds that file claims, and the verdict of every case of its damage catalogue, worked
out by the plain reference decoder of tests/_verdict.py."""
import os
import subprocess

import numpy as np
import pytest

import _batch_lanes as L
import _stream_rate as S
from _kernel_rows import BATCH_R64_LANES_DECODE, CSRC, LANES, ROOT, check_family_rows, check_option_constant, registry
from _oracle import FMT_R64


def test_batch_lanes_option_constant():
    check_option_constant("BATCH_LANES", 9)


def test_no_lane_batch_kernel_without_a_row():
    """The family holds exactly one name; the family's names are the decode names of LANE_ROWS, in both directions; and the
    check has teeth: without its rows the name is reported missing."""
    check_family_rows(LANES)
    assert registry()[BATCH_R64_LANES_DECODE] == {"k_decode_batch_r64_lanes"}


def test_the_one_list_is_what_it_is():
    """tests/kernel_names_driver.cpp prints the registry's 53 lines: the 52 it printed before the lane encoder's family joined
    the list, in their order, and that family's one behind them (every id stays what it was)."""
    registry()
    exe = os.path.join(ROOT, "build", "kernel_names", "kernel_names_driver")
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 53 and lines[0] == "uniform\tk_decode_word64"
    assert lines[50] == "batch_byte_pairs_encode\tk_encode_batch_byte_pairs" and lines[51] == "batch_r64_lanes_decode\tk_decode_batch_r64_lanes"
    assert lines[52] == "batch_r64_lanes_encode\tk_encode_batch_r64_lanes"
    assert [ln for ln in lines if "r64_lanes" in ln] == lines[51:]


def test_a_name_not_in_the_list_does_not_compile(tmp_path):
    src = tmp_path / "no_such_kernel.cpp"
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::decode_batch_r64_lanes_no_such; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "decode_batch_r64_lanes_no_such" in r.stderr
    src.write_text('#include "kernel_names.hpp"\nint main() { return (int)rans_amd::KernelId::decode_batch_r64_lanes; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-I", CSRC, "-fsyntax-only", str(src)]).returncode == 0


def test_rate_inputs_reach_the_rings_bound():
    """255 x 1 and one common symbol at 2^16, 2-way rans64.
      * a frequency-1 symbol makes the step x = x >> 16: a state loses 8 x 16 bits per 16-symbol group and takes exactly four
        dwords -- 32 bytes per group for both states, in EVERY window of eight rounds (S.rare_group_bytes: the unit divides
        the bits lost), what the ring's invariant (>= 48 bytes ahead, of which the window reads 8 ahead) must cover;
      * a common symbol costs 0.0056 bits: the common-only streams (383 symbols at the most) take nothing at all, a cursor
        that stands still beside quad-mates at the bound;
      * the burst streams (runs of 16 rare and 16 common symbols) have groups at 32 bytes and silent rounds in one stream.
    The inputs are the GPU file's own generators (L.rate_batch)."""
    assert S.rare_group_bytes(FMT_R64, 16, 2) == (32, 32)
    freqs, counts, contents, phases = L.rate_batch(16)
    assert np.array_equal(freqs, S.lane_model(16)) and int(freqs.sum()) == 1 << 16
    assert counts.size == 64 and sorted(set(p % 64 for p in phases)) == list(range(0, 64, 4))
    assert set(counts.tolist()) == {64 * b + t for b in (0, 1, 5) for t in (0, 1, 31, 63)}
    kinds = [L.rate_kind(k) for k in range(64)]
    assert {(kinds[k], int(counts[k])) for k in range(64)} == {(kd, c) for kd in L.RATE_KINDS for c in set(counts.tolist())}
    at_bound = silent = burst_both = 0
    for k in range(64):
        n = int(counts[k])
        rb = S.round_bytes(FMT_R64, freqs, 16, contents[k], 2)
        full = rb[:n // 2]  # rounds with both states
        if kinds[k] == "rare":
            assert np.all(np.isin(contents[k], np.nonzero(freqs == 1)[0]))
            if n >= 16:
                w = S.group_bytes(full, 2)
                assert w.size >= 1 and w.min() == 32 and w.max() == 32, (k, n, w.min(), w.max())
                at_bound += 1
        elif kinds[k] == "common":
            assert np.all(contents[k] == S.COMMON) and rb.sum() == 0 and S.longest_silence(rb) == (n + 1) // 2, (k, n)
            silent += n > 0
        elif n >= 64:
            w = S.group_bytes(full, 2)
            assert w.max() == 32 and S.longest_silence(rb) >= 7, (k, n, w.max(), S.longest_silence(rb))
            burst_both += 1
    assert at_bound >= 12 and silent >= 12 and burst_both >= 8, (at_bound, silent, burst_both)
    # the 14-bit batch is the same input under 255 x 1 + 16129: 24 to 32 bytes per group
    freqs14, _, contents14, _ = L.rate_batch(14)
    assert S.rare_group_bytes(FMT_R64, 14, 2) == (24, 32)
    k = next(k for k in range(64) if kinds[k] == "rare" and counts[k] >= 320)
    w = S.group_bytes(S.round_bytes(FMT_R64, freqs14, 14, contents14[k], 2)[:int(counts[k]) // 2], 2)
    assert w.min() >= 24 and w.max() == 32


@pytest.mark.parametrize("n", L.DAMAGE_LOADS)
def test_every_damage_case_has_a_decisive_verdict(oracle, n):
    """Every case of the catalogue -- ten kinds of damage, applied to one stream, to one lane of each quad position, to every
    second stream and to every stream, on one wave-load and on three -- gets its verdict here: the index rule of the header
    for the four rejected kinds, the plain reference decoder for the six that are decoded, which must say BAD without needing
    a byte behind the stream's own slack (zeros that no damage touches).  The GPU file asserts exactly these."""
    hb = L.HostBatch(oracle, n)
    assert hb.container_bytes % 16 == 0 and np.all(hb.offs % 4 == 0) and hb.counts.min() >= 100 and hb.lens.min() > 24
    for c in (0, n - 1):  # the undamaged batch is good
        v = L.V.ref_decode(hb.ref, 2, hb.cont, int(hb.offs[c]), int(hb.counts[c]), int(hb.lens[c]),
                           L.V.granule_limit(int(hb.offs[c]), int(hb.lens[c])))
        assert v.good and np.array_equal(v.syms.astype(np.uint8), hb.syms[c])
    for kind in L.DAMAGE_KINDS:
        for pname, which in L.damage_patterns(n).items():
            d = L.Damaged(hb, kind, which)
            assert d.bad == list(which) and set(d.proofs) == set(which), (kind, pname)
            assert all(bad for _, bad in d.proofs.values()), (kind, pname, "a verdict that is not BAD")
            assert all(what == ("index" if kind in L.REJECTED else "stream") for what, _ in d.proofs.values())
            assert set(d.written) == (set() if kind in L.REJECTED else set(which))
            want = d.expected(hb, 0xA5)
            for c in which:
                lo, cnt = int(hb.sym_offs[c]), int(hb.counts[c])
                if kind in L.REJECTED:
                    assert np.all(want[lo:lo + cnt] == 0xA5)
                elif kind in ("len-4", "len+4"):
                    assert np.array_equal(want[lo:lo + cnt], hb.syms[c])  # all symbols right, the length wrong
                elif kind in ("count-1", "count-64"):
                    k = cnt - (1 if kind == "count-1" else 64)
                    assert np.array_equal(want[lo:lo + k], hb.syms[c][:k]) and np.all(want[lo + k:lo + cnt] == 0xA5)
