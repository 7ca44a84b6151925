// wave_shape.hpp -- which instance of the wave-per-chunk kernels (decode_wave.hip, encode_wave.hip, encode_adaptive.hip) a
// request gets and with what geometry it is launched, as functions of plain values.  Host-only (no HIP): the launchers
// dispatch on these results, and tests/test_wave_shape.py enumerates them without a GPU.
#pragma once

#include <cstdint>

#include "kernel_formats.hpp"

namespace rans_amd {

// Per-wave LDS stream window (see decode_wave.hip "stream window").
constexpr uint32_t kRingBytes = 2048;   // two 1 KiB blocks
constexpr uint32_t kRingBlock = 1024;   // 64 lanes x 16 B
constexpr uint32_t kRingMirror = 768;   // copy of ring[0..768) after the end: no wrap between checkpoints
constexpr uint32_t kRingStride = kRingBytes + kRingMirror;

constexpr uint32_t kCuLdsBytes = 160 * 1024;
constexpr int kDecBlockThreads = 1024; // 16 waves share one table image
constexpr int kEncBlockThreads = 256;
constexpr int kEncAliasLdsThreads = 1024;  // FMT_ALIAS_LDS: 16 waves share the (up to 160 KiB) tables of a CU
constexpr uint32_t kEncFusedThreads = 512; // 7 encoder waves + 1 copier wave; 4 blocks per CU
constexpr uint32_t kEncFusedCopiers16 = 2; // copier waves of a 16-wave block
constexpr uint32_t kEncMailboxBytes = 16 + 64 * 8;
// Wave-per-chunk encoders, fused placement: behind the mailbox, one "drained" counter per coding wave of the block (the
// scratch ring protocol, EncParams::ring_slots)
constexpr uint32_t kEncDrainBytes = 64;
constexpr uint32_t kEncFusedLdsBytes = kEncMailboxBytes + kEncDrainBytes;
// word encoder, one state per lane: the emitted words of sixteen rounds are staged in a window of LDS per wave
// (encode_wave.hip, enc_word_full_staged); the windows follow the 8 KiB of record tables
constexpr uint32_t kEncStageBytes = 2048;
constexpr uint32_t kEncRecBytes = 16; // sizeof(EncRec), model.h
// waves per SIMD the fused kernel is compiled for: 8 (64 VGPRs: 4 blocks of 8 waves per CU) with one state per lane, 4 and 2
// with 2-4 and 8 states per lane -- at 64 VGPRs those spilled 20 to 785 registers (the 512-way rans64 encoder)
constexpr int enc_fused_waves_per_simd(int K) { return K == 1 ? 8 : (K <= 4 ? 4 : 2); }

// per-chunk models (device_common.hpp): scale_bits 8..12, every wave's own tables in LDS
constexpr uint32_t kAdaptMaxScaleBits = 12;
constexpr uint32_t kAdaptDecWaveLds = (1u << kAdaptMaxScaleBits) + 256u * 4u; // cum2sym + packed {freq | start << 16} records
constexpr uint32_t kAdaptEncWaveLds = 256u * 16u;                             // EncRec per symbol
// encode_adaptive.hip: six waves per SIMD (80 registers), 24 one-wave workgroups per CU (the LDS would allow 25): measured the
// same from 20 to 25 per CU, and with 1, 4 or 8 count loads in flight (profiles/r06_adaptive_encoder_variants.log: the
// launch is bound by the LDS pipe -- one ds_add per symbol on top of the coder's record gather -- not by latency)
constexpr int kAdaptWavesPerSimd = 6, kAdaptPerCu = 24;
constexpr uint32_t kAdaptRecBytes = 256u * 16u;                     // the records, at LDS address 0
constexpr uint32_t kAdaptEncLds = kAdaptRecBytes + kEncStageBytes; // 6 KiB; the counters of step 1 lie over the records
// (waves per SIMD by the registers a resident chunk needs -- 64 / 32 / 16 VGPRs of symbols beside ~90 of working set, no spills:
//  at RR = 16 three spill-free waves beat four that spill 22 registers, 0.874 against 0.984 ms for the word format)
constexpr int adapt_waves_per_simd(int K, int RR) { return K != 1 ? (K <= 4 ? 4 : 2) : RR >= 16 ? 3 : RR >= 4 ? 4 : kAdaptWavesPerSimd; }

// K states per lane for an N-way stream: the smallest of 1, 2, 4, 8 with 64 K >= N (lane counts that are no multiple of 64
// leave the tail lanes idle); 0: no wave kernel takes this interleave
constexpr int wave_states_per_lane(uint32_t n_ways)
{
    return n_ways < 1 ? 0 : n_ways <= 64 ? 1 : n_ways <= 128 ? 2 : n_ways <= 256 ? 4 : n_ways <= 512 ? 8 : 0;
}

// threads == 0: the request has no launch
struct WaveLaunch {
    uint32_t threads, grid;
    uint64_t lds;                    // dynamic LDS bytes
    uint32_t mailbox_off, stage_off; // the encoder's EncParams fields of these names
};
constexpr uint32_t wave_grid(uint64_t want, uint64_t cap) { return (uint32_t)(want < cap ? (want ? want : 1) : cap); }

// ---- decoder ----------------------------------------------------------------------------------------------------------
// Does k_decode<fmt, K, out, ragged> exist?  Element stores always; the search decoder has nothing else; paired u16 stores
// up to K = 4, but up to K = 2 for the word-u16 format and in ragged batches, where only it and the alias format have them;
// transposed u8 stores for every other format (word, K = 1: in the form of k_decode_word64).
constexpr bool decode_has(int fmt, int K, int out, bool ragged)
{
    if (out == OUT_SLOW || fmt == FMT_R64S)
        return out == OUT_SLOW;
    if (out == OUT_FAST16)
        return fmt == FMT_WORD16 ? K <= 2 : ragged ? fmt == FMT_ALIAS && K <= 2 : K <= 4;
    return fmt != FMT_WORD16;
}
constexpr bool decode_is_word64(int fmt, int K, int out) { return fmt == FMT_WORD && K == 1 && out == OUT_FAST8; }

// "output pointer and chunk size aligned": what a uniform call's fast stores need (the word-u16 format counts the chunk in bytes)
constexpr bool decode_out_aligned(int fmt, uint64_t out_addr, uint32_t chunk_syms)
{
    return ((out_addr | (uint64_t)chunk_syms * (fmt == FMT_WORD16 ? 2u : 1u)) & 3u) == 0;
}

struct DecodeShape {
    int K, out; // K == 0: invalid
    bool word64;
};
// The fast stores are for full waves (N = 64 K).  A uniform call needs the alignment as well; a ragged batch chooses per
// stream inside the kernel, so its launcher goes by the interleave and the symbol width alone.
// (alternatives that were measured and lost -- compiler-scheduled renormalisation -2 %, output through an LDS tile -7 %,
//  per-round byte stores -5 %, groups without the pipelined chunk hand-over, the byte format's byte stores: HISTORY.md,
//  profiles/r04_byte_decoder_variants.log -- are no longer in the sources)
constexpr DecodeShape decode_shape(int fmt, uint32_t n_ways, uint32_t sym_bytes, bool aligned, bool ragged)
{
    const int K = wave_states_per_lane(n_ways);
    const int want = (fmt == FMT_WORD16 || sym_bytes == 2) ? OUT_FAST16 : sym_bytes == 1 ? OUT_FAST8 : OUT_SLOW;
    const bool fast = K && n_ways == 64u * K && (ragged || aligned) && decode_has(fmt, K, want, ragged);
    const int out = fast ? want : OUT_SLOW;
    return {K, out, K && decode_is_word64(fmt, K, out)};
}

constexpr WaveLaunch decode_launch(bool word64, bool adaptive, uint32_t table0_bytes, uint32_t table1_bytes, uint64_t nchunks, int num_cus)
{
    // per-chunk models: every wave owns its tables (5 KiB) and window, nothing is shared -- workgroups of FOUR waves, five of
    // them per CU: 20 waves where one 16-wave workgroup held 16, and one wave per SIMD from every workgroup (one- and two-wave
    // workgroups spread unevenly over the CUs when the grid does not fill them: 0.84 / 0.80 ms against 0.73 for the word
    // format, profiles/r06_adaptive_decoder_variants.log)
    constexpr uint32_t kAdaptDecThreads = 256;
    const uint32_t threads = adaptive ? kAdaptDecThreads : kDecBlockThreads;
    const uint32_t waves = threads / 64;
    const uint32_t t0 = adaptive ? waves * kAdaptDecWaveLds : (table0_bytes + 15u) & ~15u;
    const uint32_t t1 = adaptive || word64 ? 0u : (table1_bytes + 15u) & ~15u;
    const uint64_t lds = (uint64_t)t0 + t1 + (uint64_t)waves * kRingStride;
    if (lds > kCuLdsBytes && !word64) // (k_decode_word64: one 32 KiB table, two workgroups per CU)
        return {};
    uint64_t blocks_per_cu = word64 || lds * 2 <= kCuLdsBytes ? 2 : 1;
    if (adaptive) { // small workgroups: what the LDS allows, within 32 waves per CU
        blocks_per_cu = kCuLdsBytes / ((lds + 255) & ~(uint64_t)255);
        blocks_per_cu = blocks_per_cu * waves > 32 ? 32 / waves : blocks_per_cu;
    }
    return {threads, wave_grid((nchunks + waves - 1) / waves, (uint64_t)num_cus * blocks_per_cu), lds, 0, 0};
}

// ---- encoder ----------------------------------------------------------------------------------------------------------
// k_encode's MODE (encode_wave.hip) from what the request carries, -1: no such kernel.  The per-chunk word models
// (FMT_WORDA) exist in MODE 0 only, as rans_amd_encode_adaptive launches them.
constexpr int encode_mode(bool fused, bool slot_layout, bool claims, bool slot_offsets, bool ovf_ctl, bool sym_ranges, bool worda)
{
    const bool slots = !fused && slot_layout && claims; // dynamic claims, no copiers
    if (worda && (fused || slots))
        return -1;
    if (fused)
        return 1;
    if (slots && slot_offsets) // per-stream symbol ranges and slots
        return sym_ranges && !ovf_ctl ? 4 : -1;
    if (slots)
        return ovf_ctl ? 3 : 2; // slots of the caller's size : worst-case slots
    return slot_offsets ? -1 : 0; // (a ragged request that did not reach MODE 4)
}

constexpr uint64_t encode_lds_cap(int fmt) { return fmt == FMT_ALIAS_LDS ? kCuLdsBytes : 128 * 1024; }

// per_chunk: EncParams::chunk_freqs is set; redo: the second launch of sized slots
constexpr WaveLaunch encode_launch(int fmt, int K, int mode, bool redo, uint32_t nsyms, uint32_t scale_bits, uint32_t sym_bytes,
                                   bool per_chunk, bool mailbox_global, uint64_t nchunks, int num_cus)
{
    const bool fused = mode == 1, dynamic = mode != 0;
    const uint32_t threads = fmt == FMT_ALIAS_LDS ? kEncAliasLdsThreads : (dynamic ? kEncFusedThreads : kEncBlockThreads);
    const uint32_t waves = threads / 64;
    const uint32_t enc_waves = fused ? waves - (waves >= 16 ? kEncFusedCopiers16 : 1) : waves;
    const uint64_t nrecs = nsyms < 256 ? 256 : nsyms;
    uint64_t lds = fmt == FMT_ALIAS_LDS ? nrecs * 8 + ((uint64_t)2 << scale_bits)
                   : ((fmt == FMT_BYTE && per_chunk) || fmt == FMT_WORDA) ? (uint64_t)waves * kAdaptEncWaveLds
                                                        : nrecs * kEncRecBytes + ((fmt == FMT_WORD || fmt == FMT_BYTE) ? 256 * 16 : 0);
    if ((fmt == FMT_WORD || (fmt == FMT_BYTE && !per_chunk)) && K == 1 && sym_bytes == 1 && nrecs == 256)
        lds += (uint64_t)waves * kEncStageBytes; // stream staging windows (4 + 4 KiB of tables in front)
    uint32_t mailbox_off = 0, stage_off = 0;
    if (fused && !mailbox_global) {
        lds = (lds + 15) & ~(uint64_t)15;
        mailbox_off = (uint32_t)lds;
        lds += kEncFusedLdsBytes;
    }
    if (fmt == FMT_ALIAS_LDS && K == 1 && sym_bytes == 1) { // windows of the coding waves, where there is room
        const uint64_t at = (lds + 15) & ~(uint64_t)15;
        if (at + (uint64_t)enc_waves * kEncStageBytes <= kCuLdsBytes) {
            stage_off = (uint32_t)at;
            lds = at + (uint64_t)enc_waves * kEncStageBytes;
        }
    }
    if (lds > encode_lds_cap(fmt))
        return {};
    // blocks per CU: what the LDS allows, within the 32 resident waves of a CU
    uint64_t per_cu = lds ? kCuLdsBytes / lds : 8;
    per_cu = per_cu < 1 ? 1 : per_cu;
    per_cu = per_cu * waves > 32 ? 32 / waves : per_cu;
    if (dynamic && fmt != FMT_ALIAS_LDS) { // ... and within the waves per SIMD the kernel's register budget was chosen for
        const uint64_t fit = (uint64_t)enc_fused_waves_per_simd(K) * 4 / waves;
        per_cu = per_cu > fit ? (fit ? fit : 1) : per_cu;
    }
    uint64_t cap = (uint64_t)num_cus * (fmt == FMT_ALIAS_LDS || dynamic ? per_cu : 8);
    if (mode == 3 && redo) // (a handful of chunks at most, usually none: one block per CU finds that out quickly)
        cap = (uint64_t)num_cus;
    return {threads, wave_grid((nchunks + enc_waves - 1) / enc_waves, cap), lds, mailbox_off, stage_off};
}

// ---- fused per-chunk-model encoder (encode_adaptive.hip) -----------------------------------------------------------------
struct AdaptShape {
    int K, RR; // K == 0: invalid; RR > 0: register-resident chunks of RR x 1024 symbols
};
// whole_chunk: n >= chunk_syms.  Ragged batches: the two-pass form for every stream, by the interleave alone
constexpr AdaptShape adapt_shape(uint32_t n_ways, bool syms_aligned, bool whole_chunk, uint32_t chunk_syms, bool ragged)
{
    const bool resident = !ragged && n_ways == 64 && syms_aligned && whole_chunk &&
                          (chunk_syms == 4096u || chunk_syms == 8192u || chunk_syms == 16384u);
    return {wave_states_per_lane(n_ways), resident ? (int)(chunk_syms / 1024u) : 0};
}

constexpr WaveLaunch adapt_launch(int K, int RR, uint64_t nchunks, int num_cus)
{
    // workgroups per CU: 6 KiB of LDS each allow 25 (profiles/r06_wg_residency.log), the registers kAdaptPerCu and fewer
    const uint64_t per_cu = K != 1 ? (K <= 4 ? 16 : 8) : (uint64_t)adapt_waves_per_simd(K, RR) * 4;
    const uint64_t cap = (uint64_t)num_cus * (per_cu < (uint64_t)kAdaptPerCu ? per_cu : (uint64_t)kAdaptPerCu);
    return {64, wave_grid(nchunks, cap), kAdaptEncLds, 0, 0};
}

} // namespace rans_amd
