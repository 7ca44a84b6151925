// launchers.hpp -- entry points of the kernel translation units (internal; the public launchers of
// kernels.h are assembled from these in dispatch.cpp).  Every launcher reports the kernel it launched as a KernelId
// through `name` (may be null): an entry of the one registry in kernel_names.hpp, which also holds its family.
#pragma once

#include "kernels.h"
#include "pairs_plan.hpp" // the alias pair encoder's block and LDS (host-only)

#include "../../include/ryg_rans_amd.h" // the option ids and public formats of kBatchFamilies

// Launch and report THIS launch's status: hipGetLastError() is per thread and sticky, so an error left
// behind by other code in the process (PyTorch probing a device, say) would otherwise be blamed on us.
#define RANS_LAUNCH(kern, grid, block, lds, stream, ...)                         \
    do {                                                                         \
        (void)hipGetLastError();                                                 \
        hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);         \
    } while (0)

#include <atomic>
#include <type_traits>

namespace rans_amd {

// Raise a kernel's dynamic-LDS limit once per (kernel, device): function attributes are per device, and
// one process may hold contexts on several GPUs.  `done` is a per-kernel bit set indexed by device.
inline hipError_t allow_large_lds(const void *kernel, int bytes, std::atomic<uint64_t> &done)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit)
        return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess)
        done.fetch_or(bit, std::memory_order_release);
    return e;
}

// The launch tail of the wave-per-chunk kernels, one instantiation per kernel: raise its dynamic-LDS limit to lds_cap (0: the
// kernel stays within the default), launch it with the geometry wave_shape.hpp worked out, report this launch's status.
template <auto KERN, class Params> hipError_t launch_wave_kernel(const WaveLaunch &g, uint64_t lds_cap, hipStream_t stream, const Params &p)
{
    static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
    if (lds_cap)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(KERN), (int)lds_cap, lds_ok); e != hipSuccess)
            return e;
    RANS_LAUNCH(KERN, dim3(g.grid), dim3(g.threads), (size_t)g.lds, stream, p);
    return hipGetLastError();
}

// wave_states_per_lane's K as a template argument: f(std::integral_constant<int, K>)
template <class F> hipError_t with_states_per_lane(int K, F &&f)
{
    switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}

// wave-per-chunk kernels (N-way streams with N = 64 K lanes): decode_wave.hip, encode_wave.hip
hipError_t launch_decode_wave(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
hipError_t launch_encode_wave(int format, const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);

// ... their ragged forms (one stream per wave, per-stream symbol ranges)
hipError_t launch_decode_batch_wave(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
hipError_t launch_encode_batch_wave(int format, const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... and the ragged decoder with one model per stream (format: kKernelFormatByteAdaptive / kKernelFormatWordAdaptive)
hipError_t launch_decode_batch_models_wave(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);

// two chunks per wave, 64-way, byte-stream formats (decode_dual.hip); format: kKernelFormatAlias2[W] or RANS_AMD_FMT_BYTE
hipError_t launch_decode_dual(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);

// eight chunks per wave, the reference's 8-way word layout over u8 symbols (decode_groups.hip): chunks of a multiple of 4
// symbols on a 4-byte aligned output, a partial last octet and a ragged last chunk included
bool decode_word_groups_applicable(const DecParams &p);
hipError_t launch_decode_word_groups(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... its ragged form (rans_amd_decode_batch, kBatchFamilies): eight STREAMS per wave, each with its own symbol count
// and output address, from eight streams on
bool decode_batch_word_groups_applicable(const DecParams &p);
hipError_t launch_decode_batch_word_groups(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
// 32 chunks per wave, the byte format's 2-way layout over u8 symbols (cum2sym tables), same file
bool decode_byte_pairs_applicable(const DecParams &p);
hipError_t launch_decode_byte_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... its ragged form (rans_amd_decode_batch, kBatchFamilies): 32 STREAMS per wave, each with its own symbol count and
// output address, from 32 streams on, the tables and the wave rings inside the CU's 160 KiB of LDS
bool decode_batch_byte_pairs_applicable(const DecParams &p);
hipError_t launch_decode_batch_byte_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... and the same plan for the alias format's 2-way layout (main_alias.cpp; rans_amd_decode_batch, kBatchFamilies): 32 STREAMS
// per wave over the FMT_ALIAS tables (divider + half-bucket records, about 5 KiB for 256 symbols at any scale_bits), u8
// symbols, a power-of-two alphabet of at most 256 symbols, scale_bits 8..16, from 32 streams on
bool decode_batch_alias_pairs_applicable(const DecParams &p);
hipError_t launch_decode_batch_alias_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);

// the 8-way word layout's encoder, eight chunks per wave (encode_groups.hip): chunks of a multiple of 4 u8 symbols, the
// three-kernel placement, the slot layout or sized slots (no fused placement)
bool encode_word_groups_applicable(const EncParams &p);
hipError_t launch_encode_word_groups(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... its ragged form (rans_amd_encode_batch[_ordered], kBatchFamilies): eight STREAMS per wave, each with its own
// symbol count, symbol address and slot, from eight streams on
bool encode_batch_word_groups_applicable(const EncParams &p);
hipError_t launch_encode_batch_word_groups(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// the byte format's 2-way layout, ragged (rans_amd_encode_batch[_ordered], kBatchFamilies): 32 STREAMS per wave, each
// with its own symbol count, symbol address and slot, from 32 streams on, scale_bits 8..16
bool encode_batch_byte_pairs_applicable(const EncParams &p);
hipError_t launch_encode_batch_byte_pairs(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... and the same plan for the alias format's 2-way layout (main_alias.cpp; rans_amd_encode_batch[_ordered], kBatchFamilies): 32
// STREAMS per wave over the encoder's LDS tables (records + remap16, 2 << scale_bits bytes: the launcher sizes the block from what
// they leave, pairs_plan.hpp), u8 symbols, a power-of-two alphabet of at most 256 symbols, scale_bits 8..16, from 32 streams on
bool encode_batch_alias_pairs_applicable(const EncParams &p);
hipError_t launch_encode_batch_alias_pairs(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);

// lane-per-stream kernels (N = 1, 2, 4, 8 with at least kLaneKernelMinChunks chunks): decode_lanes.hip, encode_lanes.hip
constexpr uint64_t kLaneKernelMinChunks = 64;
inline bool lanes_applicable(uint64_t nchunks, uint32_t n_ways)
{
    return nchunks >= kLaneKernelMinChunks && (n_ways == 1 || n_ways == 2 || n_ways == 4 || n_ways == 8);
}
hipError_t launch_decode_lanes(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
hipError_t launch_encode_lanes(int format, const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// the ragged form of the 2-way rans64 lane decoder (rans_amd_decode_batch, kBatchFamilies; decode_lanes.hip): 64 STREAMS
// per wave, one per lane, each with its own symbol count and output address, from 64 streams on, scale_bits 7..16, the tables
// and at least one wave's rings inside the CU's 160 KiB of LDS (the launcher sizes the block from what the tables leave)
bool decode_batch_r64_lanes_applicable(const DecParams &p);
hipError_t launch_decode_batch_r64_lanes(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
// ... and of the 2-way rans64 lane encoder (rans_amd_encode_batch[_ordered], kBatchFamilies; encode_lanes.hip): 64 STREAMS per
// wave, one per lane, each with its own symbol count, symbol address and slot, from 64 streams on, scale_bits 7..16 (the
// launcher sizes the block: 8 KiB of records and 8 KiB of ring per wave)
bool encode_batch_r64_lanes_applicable(const EncParams &p);
hipError_t launch_encode_batch_r64_lanes(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name);
// the ragged form of the staged 1-way lane decoder (rans_amd_decode_batch, kBatchFamilies; decode_lanes.hip): 64 STREAMS per wave,
// one per lane with ONE state each, for the non-interleaved layout of the byte, word, rans64 (cum2sym) and alias formats over u8
// symbols, from 64 streams on; scale_bits 8..16 (byte, alias: a power-of-two alphabet of at most 256 symbols), 12 (word), 7..16
// (rans64); the tables and at least one wave's rings inside the CU's 160 KiB of LDS (the launcher sizes the block from what the
// tables leave).  `format` is the kernel-side one; a row of kBatchFamilies names an instantiation of the templates.
bool decode_batch_singles_applicable(int format, const DecParams &p);
hipError_t launch_decode_batch_singles(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name);
template <int FORMAT> bool decode_batch_singles_applicable(const DecParams &p) { return decode_batch_singles_applicable(FORMAT, p); }
template <int FORMAT> hipError_t launch_decode_batch_singles(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    return launch_decode_batch_singles(FORMAT, p, num_cus, stream, name);
}
// true when launch_encode_lanes would take the staged kernel for this request -- the one that can place its chunks
// itself (EncParams::status); everything but status / offsets / out / out_cap must be filled in
bool encode_lanes_fused(const EncParams &p, int num_cus);
// true when launch_encode_lanes would take a staged kernel for this SIZED-slot request (EncParams::ovf_ctl): encode_lanes.hip
bool encode_lanes_sized_ok(int format, const EncParams &p, int num_cus);

// The streams-per-wave families of the ragged batches, in the order the launchers ask them: a context option sets the bit, and
// a batch of the row's public format that the row's *_applicable accepts goes to the row's kernel; every other batch takes the
// wave-per-stream kernels, under the options as well.  A decoder's row leaves the encoder's pair null and the other way round.
// The format is the KERNEL-side one that the launchers are handed: an alias model with the encoder's LDS tables encodes under
// kKernelFormatAliasLds, not RANS_AMD_FMT_ALIAS.
// `streams` completes the option's E_ARG text.  The rows of the 1-way layout, one per format under one option and one bit, stand
// behind the other decoders' rows: a batch that had a family keeps it.  (The 1-way ENCODER, the 2-way scalar word layout and the
// ragged forms of the 4- and 8-way lane kernels are later work: one more row each.)
struct BatchFamily {
    int option; // RANS_AMD_OPT_*
    const char *option_name;
    uint32_t bit; // kVarBatch* in DecParams::variant / EncParams::variant
    int format;
    bool (*decode_applicable)(const DecParams &);
    hipError_t (*launch_decode)(const DecParams &, int, hipStream_t, KernelId *);
    bool (*encode_applicable)(const EncParams &);
    hipError_t (*launch_encode)(const EncParams &, int, hipStream_t, KernelId *);
    const char *streams;
};
#define RANS_BATCH_DECODER(opt, bit, fmt, kern, streams) {opt, #opt, bit, fmt, kern##_applicable, launch_##kern, nullptr, nullptr, streams}
#define RANS_BATCH_ENCODER(opt, bit, fmt, kern, streams) {opt, #opt, bit, fmt, nullptr, nullptr, kern##_applicable, launch_##kern, streams}
#define RANS_BATCH_SINGLES(fmt)                                                                                                                \
    {RANS_AMD_OPT_BATCH_SINGLES, "RANS_AMD_OPT_BATCH_SINGLES", kVarBatchSingles, fmt, decode_batch_singles_applicable<fmt>, launch_decode_batch_singles<fmt>, \
     nullptr, nullptr, "sixty-four 1-way streams per wave"}
constexpr BatchFamily kBatchFamilies[] = {
    RANS_BATCH_DECODER(RANS_AMD_OPT_BATCH_GROUPS, kVarBatchGroups, RANS_AMD_FMT_WORD, decode_batch_word_groups, "eight 8-way word streams per wave"),
    RANS_BATCH_DECODER(RANS_AMD_OPT_BATCH_PAIRS, kVarBatchPairs, RANS_AMD_FMT_BYTE, decode_batch_byte_pairs, "thirty-two 2-way byte streams per wave"),
    RANS_BATCH_DECODER(RANS_AMD_OPT_BATCH_LANES, kVarBatchLanes, RANS_AMD_FMT_R64, decode_batch_r64_lanes, "sixty-four 2-way rans64 streams per wave"),
    RANS_BATCH_DECODER(RANS_AMD_OPT_BATCH_ALIAS_PAIRS, kVarBatchAliasPairs, RANS_AMD_FMT_ALIAS, decode_batch_alias_pairs, "thirty-two 2-way alias streams per wave"),
    RANS_BATCH_SINGLES(RANS_AMD_FMT_BYTE),
    RANS_BATCH_SINGLES(RANS_AMD_FMT_WORD),
    RANS_BATCH_SINGLES(RANS_AMD_FMT_R64),
    RANS_BATCH_SINGLES(RANS_AMD_FMT_ALIAS),
    RANS_BATCH_ENCODER(RANS_AMD_OPT_BATCH_ENCODE_GROUPS, kVarBatchEncGroups, RANS_AMD_FMT_WORD, encode_batch_word_groups, "eight 8-way word streams per wave"),
    RANS_BATCH_ENCODER(RANS_AMD_OPT_BATCH_ENCODE_PAIRS, kVarBatchEncPairs, RANS_AMD_FMT_BYTE, encode_batch_byte_pairs, "thirty-two 2-way byte streams per wave"),
    RANS_BATCH_ENCODER(RANS_AMD_OPT_BATCH_ENCODE_LANES, kVarBatchEncLanes, RANS_AMD_FMT_R64, encode_batch_r64_lanes, "sixty-four 2-way rans64 streams per wave"),
    RANS_BATCH_ENCODER(RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS, kVarBatchEncAliasPairs, kKernelFormatAliasLds, encode_batch_alias_pairs, "thirty-two 2-way alias streams per wave"),
};
#undef RANS_BATCH_DECODER
#undef RANS_BATCH_ENCODER
#undef RANS_BATCH_SINGLES

// the first family whose option is on and that takes this batch, or null: the wave-per-stream kernels
inline const BatchFamily *decode_batch_family(uint32_t variant, int format, const DecParams &p)
{
    for (const BatchFamily &f : kBatchFamilies)
        if (f.launch_decode && (variant & f.bit) && format == f.format && f.decode_applicable(p))
            return &f;
    return nullptr;
}
inline const BatchFamily *encode_batch_family(uint32_t variant, int format, const EncParams &p)
{
    for (const BatchFamily &f : kBatchFamilies)
        if (f.launch_encode && (variant & f.bit) && format == f.format && f.encode_applicable(p))
            return &f;
    return nullptr;
}

} // namespace rans_amd
