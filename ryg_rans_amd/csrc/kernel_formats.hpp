// kernel_formats.hpp -- the kernel-side format numbers and the decoders' store modes: what the kernels are instantiated
// over (device_common.hpp) and what the launchers choose among (wave_shape.hpp).  Host-only: no HIP.
#pragma once

#include "../../include/ryg_rans_amd.h"

namespace rans_amd {

constexpr int FMT_BYTE = RANS_AMD_FMT_BYTE;
constexpr int FMT_WORD = RANS_AMD_FMT_WORD;
constexpr int FMT_R64 = RANS_AMD_FMT_R64;
constexpr int FMT_ALIAS = RANS_AMD_FMT_ALIAS;
// Internal kernel format: rans64 (RANS_AMD_FMT_R64 to the caller) for the scale_bits the cum2sym decoder
// cannot take -- 17..31, where a 2^scale_bits lookup table fits no LDS, and 1..6, where its 24-bit partial
// products do not hold.  The symbol comes from a binary search over the cumulative frequencies
// (nsyms + 1 words in LDS), the state updates use full 64 x 32 multiplies.  Same stream, any
// scale_bits rans64.h accepts (rans64.h:169: <= 31); several times slower than the table decoder.
constexpr int FMT_R64S = 4;
// Internal kernel format of the ENCODER: alias coding (RANS_AMD_FMT_ALIAS to the caller) with the slot
// permutation alias_remap (main_alias.cpp:63,225-228) held in LDS as u16 next to 8-byte symbol records, for the
// models where both fit (2 M + 8 nsyms <= 160 KiB: every model up to 4096 symbols at 16 bits).  The general
// alias encoder gathers alias_remap from L2: 64 random dwords per sub-step drag 64 cache lines through the L1.
constexpr int FMT_ALIAS_LDS = 5;
// Internal kernel format of the DECODER: the word format (RANS_AMD_FMT_WORD to the caller) over an alphabet of more
// than 256 symbols -- SURVEY 8(f)4's "16-bit-symbol word format"; rans_word_sse41.h:41 fixes 256, the stream
// format itself does not care.  Slot record {freq, bias | sym << 16}: one more v_and than the byte-symbol record.
constexpr int FMT_WORD16 = 6;
// Internal kernel format of the DECODER: byte format with one model PER CHUNK: every wave builds
// cum2sym + symbol records of its chunk in its own LDS region from the chunk's 256 normalised frequencies
// (scale_bits <= 12: 4 KiB + 2 KiB per wave), so the tables are addressed through per-wave pointers.
constexpr int FMT_BYTEA = 7;
// Internal kernel formats of the two-chunks-per-wave DECODER (decode_dual.hip) for alias models: the half-bucket
// record is {sym | (M - freq) << 16, adjust} -- the update x' = x - adjust - (M - freq) * (x >> scale_bits) needs
// neither x mod M nor a mask on the frequency, and the low half IS the symbol a 16-bit store writes -- and the divider
// is held as the bucket's own-slot count (main_alias.cpp:209 `divider[i] = i * tgt + h0`, here h0 alone), one byte per
// bucket at LDS address 0 (FMT_ALIAS2, M / nsyms <= 255) or two (FMT_ALIAS2W).
constexpr int FMT_ALIAS2 = 8;
constexpr int FMT_ALIAS2W = 9;
// Internal kernel format of the DECODER: the byte format (RANS_AMD_FMT_BYTE to the caller) with the slot table of the word
// format -- one 8-byte record {freq | sym << 24, slot - start} per cumulative slot at LDS address 8 * slot -- for models whose
// table fits beside the stream windows (scale_bits <= 13).  D step: v_and, v_lshlrev, ds_read_b64, v_lshrrev, v_mad_u32_u24
// (rans_byte.h:125-128 + :291-298 as rans_word_sse41.h:123-131 does it): one gather instead of two dependent ones.
constexpr int FMT_BYTEF = 11;
// Internal kernel format: the WORD format (rans_word_sse41.h, 12-bit probabilities, 16-bit renormalisation) with one model
// PER CHUNK (SURVEY 8(f)3 on the headline's format): the decoder's waves build cum2sym + {freq, start} of their chunk as
// FMT_BYTEA does (a 4096-slot table per wave, rans_word_sse41.h:64-72, would be 32 KiB each) -- slot = x & 4095,
// x = freq * (x >> 12) + (slot - start) is the very update of rans_word_sse41.h:123-131; the encoder's waves build the
// general path's {freq, start, reciprocal} records.
constexpr int FMT_WORDA = 12;

// OUT_SLOW: element stores (any N, any alignment, u16 symbols).  OUT_FAST8: 4 rounds of u8 symbols transposed in
// registers, one dword store per lane.  OUT_FAST16: u16 symbols, 2 rounds packed per dword and swapped between lane pairs.
// (The 64-way word decoder has a kernel of its own: decode_wave.hip k_decode_word64.)
enum OutMode { OUT_SLOW = 0, OUT_FAST8 = 1, OUT_FAST16 = 4 };

} // namespace rans_amd
