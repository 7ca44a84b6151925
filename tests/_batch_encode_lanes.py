"""What tests/test_batch_encode_lanes_host.py and tests/test_gpu_batch_encode_lanes.py share beyond tests/_kernel_rows.py (the rows
and the descriptor) and tests/_batch.py (the bodies): the single wave-loads of the ragged 2-way rans64 lane ENCODER
(k_encode_batch_r64_lanes, RANS_AMD_OPT_BATCH_ENCODE_LANES) and the rate inputs whose bounds the host file proves.  Nothing here
needs a GPU."""
import numpy as np

import _batch_lanes as L
import _stream_rate as S
from _batch import mandatory_lengths, padded

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
