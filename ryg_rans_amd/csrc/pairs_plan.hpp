// pairs_plan.hpp -- the LDS plan of k_encode_batch_alias_pairs (encode_groups.hip), as plain arithmetic.  Host-only and free
// of HIP: tests/enc_alias_pairs_plan_driver.cpp prints it with g++.
//
// The block's LDS holds 256 16-byte records, remap16 (2 << scale_bits bytes) and one set of ring rows per wave (32 rows of 68
// bytes: groups_common.hpp kPairWaveLds).  Sixteen waves where the CU's 160 KiB leave room for them, else as many as fit -- at
// 16 bits 128 KiB of remap16 leave 13; two blocks per CU where two fit (up to 14 bits).
#pragma once

#include <cstdint>

namespace rans_amd {

constexpr uint32_t kEncAliasPairsRecBytes = 256 * 16;   // == encode_groups.hip kEncPairTable
constexpr uint32_t kEncAliasPairsWaveLds = 32 * 68;     // == groups_common.hpp kPairWaveLds
constexpr uint32_t kEncAliasPairsLdsCap = 160 * 1024;   // == groups_common.hpp kGrpLdsCap
constexpr uint32_t kEncAliasPairsMaxWaves = 16;         // == groups_common.hpp kGrpThreads / 64

struct EncAliasPairsPlan {
    uint32_t table_bytes;   // records + remap16: where the rows start
    uint32_t waves;         // per block; 0: the tables leave no room for a wave
    uint32_t lds_bytes;     // the block's dynamic LDS
    uint32_t blocks_per_cu; // what the grid is sized for
};

constexpr EncAliasPairsPlan enc_alias_pairs_plan(uint32_t scale_bits)
{
    if (scale_bits > 16) // (remap16 holds 16-bit slots)
        return EncAliasPairsPlan{0u, 0u, 0u, 0u};
    const uint32_t tables = kEncAliasPairsRecBytes + (2u << scale_bits);
    const uint32_t room = (kEncAliasPairsLdsCap - tables) / kEncAliasPairsWaveLds;
    const uint32_t waves = room < kEncAliasPairsMaxWaves ? room : kEncAliasPairsMaxWaves;
    const uint32_t lds = tables + waves * kEncAliasPairsWaveLds;
    return EncAliasPairsPlan{tables, waves, lds, waves == kEncAliasPairsMaxWaves && 2u * lds <= kEncAliasPairsLdsCap ? 2u : 1u};
}

} // namespace rans_amd
