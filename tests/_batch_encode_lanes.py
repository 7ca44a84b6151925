"""What tests/test_batch_encode_lanes_host.py and tests/test_gpu_batch_encode_lanes.py share: the reader of the registry's SECOND
list (ryg_rans_amd/csrc/kernel_names.hpp, RANS_AMD_KERNEL_NAMES_ENCODE_LANES), the rows and the descriptor of the ragged 2-way
rans64 lane ENCODER (k_encode_batch_r64_lanes, RANS_AMD_OPT_BATCH_ENCODE_LANES), its single wave-loads, the rate inputs whose
bounds the host file proves, and the variants of tests/_batch.py's bodies that assume another layout.

Nothing here needs a GPU but PoolBatch64, which the GPU file alone builds."""
import functools
import os
import subprocess

import numpy as np

import _batch_lanes as L
import _stream_rate as S
import ryg_rans_amd as R
from _batch import GUARD, POISON, PoolBatch, mandatory_lengths, padded
from _kernel_rows import CSRC, HERE, LANE_SHAPES, ROOT, Family, registry
from _oracle import FMT_R64

BATCH_R64_LANES_ENCODE = "batch_r64_lanes_encode"
KERNEL = "k_encode_batch_r64_lanes"
OPT_BATCH_ENCODE_LANES = R.OPT_BATCH_ENCODE_LANES
# RANS_AMD_OPT_*, by value (tests/_kernel_rows.py's OPTIONS and the new one behind them)
OPTIONS = ("LANE_KERNELS", "LANE_FUSED_PLACEMENT", "FUSED_PLACEMENT", "DUAL_DECODE", "ENC_SCRATCH_RING", "BATCH_GROUPS",
           "BATCH_ENCODE_GROUPS", "BATCH_PAIRS", "BATCH_ENCODE_PAIRS", "BATCH_LANES", "BATCH_ENCODE_LANES")


@functools.lru_cache(maxsize=None)
def second_list():
    """[(family, name)]: every entry of the second list, as tests/kernel_names_batch_encode_lanes_driver.cpp prints them (the
    driver fails on a name or a family of the first list, and on an id that does not follow the first list's)."""
    build = os.path.join(ROOT, "build", "kernel_names")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "kernel_names_batch_encode_lanes_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "kernel_names_batch_encode_lanes_driver.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return [tuple(ln.split("\t")) for ln in out.splitlines()]


def second_list_names(family):
    return {name for f, name in second_list() if f == family}


# ---- sixty-four 2-way rans64 streams per wave: encoder (tests/test_gpu_batch_encode_lanes.py)
def _enc_lane_row(rid, sb, K):
    return {"id": rid, "fmt": FMT_R64, "sb": sb, "K": K, "ways": 2, "decode": "k_decode_batch<r64>", "encode": KERNEL}


ENC_LANE_ROWS = [
    _enc_lane_row("r64-2-enc-lanes", 14, 256),            # the reference's scale_bits (main64.cpp)
    _enc_lane_row("r64-2-enc-lanes-16bit", 16, 256),      # a frequency of 2^16 is inside the working range
    _enc_lane_row("r64-2-enc-lanes-12bit", 12, 256),
    _enc_lane_row("r64-2-enc-lanes-64sym-7bit", 7, 64),   # the smallest scale_bits; the record table is padded to 256
    _enc_lane_row("r64-2-enc-lanes-64sym-10bit", 10, 64),
]
ELROW = {r["id"]: r for r in ENC_LANE_ROWS}
ELMAIN, EL16 = ELROW["r64-2-enc-lanes"], ELROW["r64-2-enc-lanes-16bit"]
ENC_LANE_RATE_ROW = {14: ELMAIN, 16: EL16}
ENC_LANES = Family(OPT_BATCH_ENCODE_LANES, "encode", FMT_R64, 2, 64, ENC_LANE_ROWS, ELMAIN, "k_encode_batch<r64>", BATCH_R64_LANES_ENCODE,
                   LANE_SHAPES, ("FMT_R64", 14, "OPT_BATCH_ENCODE_LANES"))


def check_second_list_rows(d, rows=None):
    """tests/_kernel_rows.py check_family_rows for a family of the second list (registry() knows the first list's families
    alone): the family's names are the kernels of the rows on the family's side, in both directions; the rows are the
    family's shapes; the name is in no family of the first list."""
    rows = d.rows if rows is None else rows
    names, kernel = second_list_names(d.family), d.main[d.side]
    got = {r[d.side] for r in rows}
    assert names == got, ("kernels no row expects", sorted(names - got), "names no launcher reports", sorted(got - names))
    assert kernel in names
    assert all(r["ways"] == d.ways and r["fmt"] == d.fmt for r in rows)
    assert sorted((r["sb"], r["K"]) for r in rows) == d.shapes
    assert all(kernel not in ns for ns in registry().values()) and d.family not in registry()


# ---- single wave-loads: the smallest shapes at which finishing at different times can go wrong ------------------------------
WAVE_LOADS = {
    "one-block-each": [64] * 64,
    "boundaries": padded(64, [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]),
    "63-dead-one-flushing": [65536] + [63] * 63,
    "every-lane-finishes-elsewhere": [64 * (l % 16 + 1) + 3 * l for l in range(64)],
    "quad-mates-differ": [320, 0, 64, 193] * 16,
    "all-empty": [0] * 64,
    "second-load-of-one": [300] * 65,
    "mandatory-and-200s": padded(64, mandatory_lengths(2)),
}
ALIGNS = (1, 4, 16, 64)

# ---- rate extremes in one wave: 255 x 1 and one common symbol at 2^16 (S.lane_model) ----------------------------------------
RATE_WAVES = {
    "fast-beside-dead": ([65536] + [255] * 63, ["rare"] + ["common"] * 63),
    "stalled-beside-draining": ([65536] + [64 * (l % 16 + 1) for l in range(63)], ["common"] + ["rare"] * 63),
}


def rate_wave(sb, name):
    """-> (freqs, counts, {stream: symbols}): one wave-load, every stream rare-only or common-only (L.rate_content)."""
    freqs = S.lane_model(sb)
    counts, kinds = RATE_WAVES[name]
    return freqs, np.array(counts, dtype=np.uint32), {k: L.rate_content(freqs, kinds[k], counts[k], 900 + k) for k in range(64)}


NO_ZERO_LANE_LOADS = (14, 192)  # tests/_batch.py no_zero_batch: three wave-loads at 14 bits


class PoolBatch64(PoolBatch):
    """tests/_batch.py's PoolBatch lays its symbols out at sym_align = 4; this one moves them to sym_align = 64, the lane
    encoder's fast layout: the same streams, prototypes and container."""

    def __init__(self, R, ctx, torch, oracle, row, proto_counts, n, seed):
        super().__init__(R, ctx, torch, oracle, row, proto_counts, n, seed)
        old_sym, old_buf = self.d_sym, self.d_buf
        self.sym_offs, slot_offs = R.batch_layout(self.counts, row["fmt"], 2, 64)
        assert np.array_equal(slot_offs, self.slot_offs) and np.all(self.sym_offs % 64 == 0)
        self.d_sym = torch.from_numpy(self.sym_offs.astype(np.int64)).cuda()
        self.d_buf = torch.full((int(self.sym_offs[-1]) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        reps = self.d_counts.to(torch.int64)
        within = torch.arange(int(reps.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(reps, 0) - reps, reps)
        self.d_buf[torch.repeat_interleave(self.d_sym[:-1], reps) + within] = old_buf[torch.repeat_interleave(old_sym[:-1], reps) + within]
