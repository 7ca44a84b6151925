// encode_groups.hip -- the mirror image of decode_groups.hip's k_decode_word_groups: the reference's 8-way word layout
// (rans_word_sse41.h:57-100, main_simd.cpp:287-300: eight states, one pointer that moves DOWN), EIGHT chunks per wave, lane
// 8 g + i holds state i of chunk g of the wave's octet.
//
// The lane-per-chunk encoder (encode_lanes.hip k_encode_lanes_staged) walks a whole chunk per lane: 10 KiB of staging rows and
// rings per wave, 11..13 waves per CU, 1.2 ms per GiB.  Here a round codes one symbol per lane:
//   * symbols: sixteen rounds are one 128-byte line of the chunk, 16 bytes per lane, taken apart into per-state bytes by
//     the inverse of the decoder's output exchange (v_cndmask_b32_dpp between the halves of the group, then the quad
//     transposes, which are their own inverse); the next line is in flight while this one is coded, rounds run from the
//     chunk's last to its first (main_simd.cpp:287-300);
//   * "who emits" (x > thresh, rans_word_sse41.h:85) is a ballot; t = its bits of MY group, in place; a lane's rank among
//     its group's emitters is v_mbcnt over t, the group's running word count c (a VGPR) moves on by v_bcnt(t); the
//     lane's word lands 2 (c' - rank) bytes below the end of the stream (ascending lane = ascending address inside a round,
//     later rounds below earlier ones: rans_word_sse41.h:93-99);
//   * a group's words go to a 256-byte ring in LDS; eight rounds emit at most 8 x 8 words = one 128-byte block, so every
//     eight rounds at most one finished block per group leaves, 16 bytes per lane, to its place below the end of the
//     chunk's slot.  The flushed states (RansWordEncFlush, state 0 lowest) follow the same way;
//   * the division x / freq is the wave encoder's (encode_common.hpp: Alverson or round-up reciprocal from the 16-byte
//     WordEncRec, exact), one ds_read_b128 per symbol.
// Slots: worst-case scratch slots (k_layout / k_compact_small behind the launch), the caller's container (slot layout), or
// sized slots -- a store that would start below the slot's first byte is dropped, and a chunk whose stream turns out longer
// than its slot is listed for the redo launch exactly as the lane encoders list theirs (EncParams::ovf_ctl).
// Chunks of a multiple of 4 symbols (launcher: the symbol loads are dword-aligned); what a chunk size off 128 leaves, and the
// input's last octet when its last chunk is a ragged one, go round by round.  The ragged form for rans_amd_encode_batch --
// eight STREAMS per wave, each with its own symbol count, symbol address and slot -- is k_encode_batch_word_groups, behind the
// uniform kernel.  Behind that one: k_encode_batch_byte_pairs, the ragged encoder of the byte format's 2-way layout
// (main.cpp:226-246), thirty-two STREAMS per wave; it has no uniform form here (the uniform byte 2-way encoder is the lane kernel).
//
// No MFMA: integer, table-driven, serial per state.

#include "decode_common.hpp"
#include "groups_common.hpp"

namespace rans_amd {

namespace {

constexpr uint32_t kEncGrpTable = 256 * 16;          // WordEncRec[256] at LDS address 0

// Eight rounds, odd-numbered round first (accumulator B: rounds 15, 13, 11, 9 or 7, 5, 3, 1 -- bytes 3..0; accumulator A the
// even ones).  Per round 15 VALU (18 with the round-up reciprocal, + 1 where symbols without a record have to be found) + 2 LDS:
//   v_lshlrev (SDWA byte J)    LDS address of the symbol's record (the table starts at LDS address 0)
//   ds_read_b128               {m', thresh, cmpl | sh << 24, bias}
//   v_cmp                      vcc = the lanes that emit a word
//   v_and, v_and_or            t = my group's bits of the ballot (in one half of the wave)
//   v_mbcnt x2, v_bcnt, v_sub  rank among my group's emitters; c' = words so far; rank - c' = the word's place from the end
//   v_lshlrev, v_and_or        -> LDS byte address in the group's ring
//   ds_write_b16, v_lshrrev    under exec = vcc: the low half leaves, x >>= 16
//   v_mul_hi .. v_add          x = x + bias + (x / freq) * cmpl (encode_common.hpp RANS_ENC_WORD_TAIL_*)
// Fixed registers v56..v59 hold the record: the parts of a 128-bit asm operand cannot be named.
#define RANS_GE_HEAD(ACC, SEL, TRACKSTR)                                                                               \
    "v_lshlrev_b32_sdwa %[t0], %[k4], " ACC " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t"   \
    "ds_read_b128 v[56:59], %[t0]\n\t"                                                                                 \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    "v_cmp_gt_u32_e32 vcc, %[x], v57\n\t"                                                                              \
    TRACKSTR                                                                                                           \
    "s_nop 0\n\t"                                                                                                      \
    "v_and_b32_e32 %[t0], vcc_lo, %[gmlo]\n\t"                                                                         \
    "v_and_or_b32 %[t1], vcc_hi, %[gmhi], %[t0]\n\t"                                                                   \
    "v_mbcnt_lo_u32_b32 %[t0], %[t0], 0\n\t"                                                                           \
    "v_mbcnt_hi_u32_b32 %[t0], %[t1], %[t0]\n\t"                                                                       \
    "v_bcnt_u32_b32 %[c], %[t1], %[c]\n\t"                                                                             \
    "v_sub_u32_e32 %[t0], %[t0], %[c]\n\t"                                                                             \
    "v_lshlrev_b32_e32 %[t0], 1, %[t0]\n\t"                                                                            \
    "v_and_or_b32 %[t0], %[t0], %[k255], %[ring]\n\t"                                                                  \
    "s_mov_b64 exec, vcc\n\t"                                                                                          \
    "ds_write_b16 %[t0], %[x]\n\t"                                                                                     \
    "v_lshrrev_b32_e32 %[x], 16, %[x]\n\t"                                                                             \
    "s_mov_b64 exec, -1\n\t"                                                                                           \
    "v_mul_hi_u32 %[t1], %[x], v56\n\t"
#define RANS_GE_TAIL_SMALL                                                                                             \
    "v_lshrrev_b32_sdwa %[t1], v58, %[t1] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t"        \
    "v_mad_u32_u24 %[t1], %[t1], v58, %[x]\n\t"                                                                        \
    "v_add_u32_e32 %[x], %[t1], v59\n\t"
#define RANS_GE_TAIL_GM                                                                                                \
    "v_sub_u32_e32 %[t0], %[x], %[t1]\n\t"                                                                             \
    "v_lshrrev_b32_e32 %[t0], 1, %[t0]\n\t"                                                                            \
    "v_add_u32_e32 %[t1], %[t1], %[t0]\n\t"                                                                            \
    RANS_GE_TAIL_SMALL
#define RANS_GE_TRACK "v_or_b32_e32 %[worst], %[worst], v58\n\t"
#define RANS_GE_PAIR(SEL, TRACKSTR, TAIL)                                                                              \
    RANS_GE_HEAD("%[pb]", SEL, TRACKSTR) TAIL RANS_GE_HEAD("%[pa]", SEL, TRACKSTR) TAIL
#define RANS_GE_EIGHT(TRACKSTR, TAIL)                                                                                  \
    asm volatile(RANS_GE_PAIR("BYTE_3", TRACKSTR, TAIL) RANS_GE_PAIR("BYTE_2", TRACKSTR, TAIL)                           \
                 RANS_GE_PAIR("BYTE_1", TRACKSTR, TAIL) RANS_GE_PAIR("BYTE_0", TRACKSTR, TAIL)                           \
                 : [x] "+v"(x), [c] "+v"(c), [worst] "+v"(worst), [t0] "=&v"(t0), [t1] "=&v"(t1)                         \
                 : [pa] "v"(acc_a), [pb] "v"(acc_b), [k4] "v"(k4), [gmlo] "v"(gm_lo), [gmhi] "v"(gm_hi), [k255] "v"(k255), \
                   [ring] "v"(ring)                                                                                    \
                 : "vcc", "memory", "v56", "v57", "v58", "v59")
template <bool SMALL, bool TRACK>
__device__ __forceinline__ void encode_octet_8rounds(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t acc_a, uint32_t acc_b,
                                                     uint32_t k4, uint32_t gm_lo, uint32_t gm_hi, uint32_t k255, uint32_t ring)
{
    uint32_t t0, t1;
    if constexpr (SMALL && TRACK)
        RANS_GE_EIGHT(RANS_GE_TRACK, RANS_GE_TAIL_SMALL);
    else if constexpr (SMALL)
        RANS_GE_EIGHT("s_nop 0\n\t", RANS_GE_TAIL_SMALL);
    else if constexpr (TRACK)
        RANS_GE_EIGHT(RANS_GE_TRACK, RANS_GE_TAIL_GM);
    else
        RANS_GE_EIGHT("s_nop 0\n\t", RANS_GE_TAIL_GM);
}
#undef RANS_GE_EIGHT
#undef RANS_GE_PAIR
#undef RANS_GE_TRACK
#undef RANS_GE_TAIL_GM
#undef RANS_GE_TAIL_SMALL
#undef RANS_GE_HEAD

// One 128-byte line of a group, last round first: the exchange and the transposes take the line apart into per-state bytes
// (byte J of a_k: round 8 (k >> 1) + 2 J + (k & 1)), then two times eight rounds.  flush(have_bytes) is the kernel's
// flush_block: the block that the LAST eight rounds of the line before may have finished leaves behind the wait for this
// line's symbols -- in front of it the wait (s_waitcnt vmcnt(0), the compiler cannot count conditional stores) would be for a
// store that has only just been issued.  (Never true for a dead group: it left with 64 fb >= c, and its c stands still.)
template <bool SMALL, bool TRACK, class FLUSH>
__device__ __forceinline__ void encode_line(const u32x4 &v, uint32_t &x, uint32_t &c, uint32_t &worst, const uint32_t &fb, uint32_t sel1, uint32_t sel2,
                                            uint32_t k4, uint32_t m_lo, uint32_t m_hi, uint32_t k255, uint32_t ring, FLUSH &&flush)
{
    uint32_t a0, a1, a2, a3;
    line_to_halves(v, a0, a1, a2, a3);
    a0 = quad_transpose(a0, sel1, sel2);
    a1 = quad_transpose(a1, sel1, sel2);
    a2 = quad_transpose(a2, sel1, sel2);
    a3 = quad_transpose(a3, sel1, sel2);
    if (c >= 64u * (fb + 1u))
        flush(2u * c);
    encode_octet_8rounds<SMALL, TRACK>(x, c, worst, a2, a3, k4, m_lo, m_hi, k255, ring); // rounds 15 .. 8
    if (c >= 64u * (fb + 1u))
        flush(2u * c);
    encode_octet_8rounds<SMALL, TRACK>(x, c, worst, a0, a1, k4, m_lo, m_hi, k255, ring); // rounds 7 .. 0
}

template <bool SMALL, bool TRACK>
__global__ void __launch_bounds__(kGrpThreads, 8) k_encode_word_groups(const EncParams p)
{
    using Tr = FmtTraits<FMT_WORD>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stage_table(smem, p.word_enc_recs, kEncGrpTable);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never code on a wrong assumption
        if (threadIdx.x == 0)
            atomicOr(p.flags, 1u);
        return;
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t g = lane >> 3, i = lane & 7u;
    const uint32_t ring_c = kEncGrpTable + wave * kGrpWaveLds + g * kGrpRing; // raw LDS address of the group's ring (256-byte aligned)
    uint32_t ring = ring_c;
    uint32_t gm_lo, gm_hi, k255 = 255u, k4 = 4u;
    pin_vgpr(ring);
    group_ballot_bits(g, gm_lo, gm_hi);
    pin_vgpr(k255);
    pin_vgpr(k4);
    const uint32_t sel1 = (lane & 1u) ? 0x03070105u : 0x06020400u;
    const uint32_t sel2 = (lane & 2u) ? 0x03020706u : 0x05040100u;
    const uint32_t lines = uniform(p.chunk_syms >> 7); // 16 rounds of 8 symbols each
    const uint64_t octets = (p.nchunks + 7u) >> 3;     // (the last one may hold fewer than eight chunks)
    const uint32_t slot = (uint32_t)p.slot_bytes;
    const bool ragged = p.n % p.chunk_syms != 0; // the input's last chunk is short: its octet takes the round-by-round path

    uint32_t worst = 0;
    WorkClaims work;
    work.init(p.claims, wave, waves_per_block); // (the dynamic hand-out as in the decoders)
    // a claim covers at least 8192 symbols (one atomic unit retires ~90 claims per microsecond)
    const uint32_t per_claim = uniform(p.chunk_syms >= 1024u ? 1u : (1024u + p.chunk_syms - 1u) / p.chunk_syms);
    const uint64_t claims = (octets + per_claim - 1u) / per_claim;
    for (;;) {
        const uint64_t claim = work.take(lane);
        if (claim >= claims)
            break;
        const uint64_t o_end = (claim + 1u) * per_claim < octets ? (claim + 1u) * per_claim : octets;
        for (uint64_t vk = claim * per_claim; vk < o_end; ++vk) {
            // (a ragged last chunk: its octet takes three times an octet's usual time -- the work is dealt back to front then, and
            //  that one starts first; 1 GiB + 8191 symbols in 16 Ki-symbol chunks: 0.76 -> 0.63 ms)
            const uint64_t octet = ragged ? octets - 1u - vk : vk;
            const uint64_t chunk = octet * 8u + g;
            const bool valid = chunk < p.nchunks;
            // symbols through a descriptor of the octet's input (the running offset is an SGPR), stream blocks through one of its slots
            const rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t *>(p.syms) + octet * 8u * p.chunk_syms, 0, 8u * p.chunk_syms, kRsrcFlags);
            const rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(p.scratch + octet * 8u * p.slot_bytes, 0, 8u * slot, kRsrcFlags);
            const uint32_t in_off = valid ? g * p.chunk_syms + 16u * i : 0x80000000u; // (a chunk that does not exist reads zeros)
            const uint32_t slot_end = (g + 1u) * slot;                                 // offset of the END of my chunk's slot in the octet's
            uint32_t x = Tr::kL, c = 0, fb = 0; // state, words emitted so far (the group's), blocks flushed
            // block fb of the ring -> its place below the slot's end; a piece that would start below the slot's first byte is dropped
            // (sized slots: the chunk then does not fit, its length says so at the end)
            auto flush_block = [&](uint32_t have_bytes) { // have_bytes: the group's stream so far
                const uint32_t below = kGrpBlock * (fb + 1u) - 16u * i; // this lane's piece starts `below` bytes under the slot's end
                if (valid && below <= slot && below - 16u < have_bytes) {
                    const u32x4 v = *reinterpret_cast<RANS_LDS const u32x4 *>((uintptr_t)(ring_c + ((fb & 1u) ? 0u : kGrpBlock) + 16u * i));
                    __builtin_amdgcn_raw_buffer_store_b128(v, orsrc, slot_end - below, 0, 0);
                }
                fb += 1u;
            };
            auto sixteen = [&](const u32x4 &v) { // one 128-byte line of the chunk, last round first
                encode_line<SMALL, TRACK>(v, x, c, worst, fb, sel1, sel2, k4, gm_lo, gm_hi, k255, ring, flush_block);
            };
            // (for what a chunk size off 128 leaves, and for the input's last octet when its last chunk is a ragged one)
            auto one_round = [&](uint32_t sym, bool active) { encode_word_round<SMALL>(x, c, worst, sym, active, gm_lo, gm_hi, ring_c); };
            const uint8_t RANS_GLOBAL *src = (const uint8_t RANS_GLOBAL *)p.syms + chunk * p.chunk_syms;
            if (octet + 1u == octets && ragged) { // one octet of the whole input: a byte load per lane and round
                uint32_t nsym = 0;
                if (valid)
                    nsym = chunk + 1u == p.nchunks ? (uint32_t)(p.n - chunk * p.chunk_syms) : p.chunk_syms;
                for (uint32_t r = (p.chunk_syms + 7u) >> 3; r-- > 0;) {
                    const bool active = r * 8u + i < nsym;
                    one_round(active ? (uint32_t)src[r * 8u + i] : 0u, active);
                    if ((r & 7u) == 0 && c >= 64u * (fb + 1u))
                        flush_block(2u * c);
                }
            } else {
                for (uint32_t r = (p.chunk_syms + 7u) >> 3; r-- > 16u * lines;) { // the rounds behind the chunk's last whole line
                    const bool active = valid && r * 8u + i < p.chunk_syms;
                    one_round(active ? (uint32_t)src[r * 8u + i] : 0u, active);
                    if ((r & 7u) == 0 && c >= 64u * (fb + 1u))
                        flush_block(2u * c);
                }
                if (lines) {
                    u32x4 next = __builtin_amdgcn_raw_buffer_load_b128(irsrc, in_off, 128u * (lines - 1u), kAuxNt);
                    for (uint32_t q = lines; q-- > 0;) {
                        const u32x4 cur = next;
                        if (q)
                            next = __builtin_amdgcn_raw_buffer_load_b128(irsrc, in_off, 128u * (q - 1u), kAuxNt);
                        sixteen(cur);
                    }
                }
            }
            if (c >= 64u * (fb + 1u)) // (the last eight rounds' block)
                flush_block(2u * c);
            // the final states, state 0 lowest (RansWordEncFlush: rans_word_sse41.h:104-113 reads them back in that order): lane
            // i's dword ends 32 - 4 i bytes ... starts 2 c + 32 - 4 i bytes below the slot's end
            {
                const uint32_t at = 0u - (2u * c + 32u - 4u * i);
                *reinterpret_cast<RANS_LDS uint16_t *>((uintptr_t)(ring_c | (at & 255u))) = (uint16_t)x;
                *reinterpret_cast<RANS_LDS uint16_t *>((uintptr_t)(ring_c | ((at + 2u) & 255u))) = (uint16_t)(x >> 16);
                c += 16u;
            }
            const uint32_t len = 2u * c;
            if (64u * fb < c)
                flush_block(len);
            if (64u * fb < c)
                flush_block(len);
            if (valid && i == 0) {
                p.lengths[chunk] = len;
                if (len > slot) { // (sized slots only: a worst-case slot holds every stream)
                    if (p.ovf_ctl)
                        p.ovf_list[atomicAdd(p.ovf_ctl, 1u)] = (uint32_t)chunk;
                } else if (p.slot_layout) {
                    p.offsets[chunk] = (chunk + 1u) * p.slot_bytes - len;
                    if (chunk + 1 == p.nchunks)
                        p.offsets[p.nchunks] = p.nchunks * p.slot_bytes;
                }
            }
        }
    }
    if (TRACK && __builtin_amdgcn_ballot_w64((worst >> 31) != 0) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

// ---------------------------------------------------------------------------
// k_encode_batch_word_groups -- the ragged form of k_encode_word_groups (rans_amd_encode_batch[_ordered] under
// RANS_AMD_OPT_BATCH_ENCODE_GROUPS): a wave's eight groups hold eight STREAMS, each with its own symbol count, symbol address
// and slot.  The unit of work is one octet of the hand-out order: lane 8 g + i holds state i of the stream at position
// 8 o + g -- stream order[8 o + g], or 8 o + g without an order; a position at or past nchunks has no stream.  The rounds, the
// record table, the ring and its blocks, the transposes and the half-group exchange are k_encode_word_groups'.  The coder
// works from a stream's last symbol to its first, so the eight groups START together and finish at different times:
//   * tail first: the count_g - 128 blocks_g symbols behind the stream's last whole 128-byte line (all of them where the
//     stream's first symbol is not 4-byte aligned: blocks_g = 0) go one round at a time, a byte load per lane, lanes without a
//     symbol sitting out; the wave runs max_g(ceil(tail_g / 8)) iterations, iteration k is round ceil(tail_g / 8) - 1 - k of
//     group g.  Nothing of a group that sits out is touched: one_round emits and tracks under `active` only;
//   * then lines: the wave runs the sixteen-round sequence max_g(blocks_g) times with FULL exec (the sequence sets exec = -1
//     itself, and the DPP moves of the exchange read zeros from lanes an exec mask has switched off); iteration q is line
//     blocks_g - 1 - q of group g while q < blocks_g.
// A group is FINALISED -- its last block check, the eight flushed states, the last one or two blocks, lengths[s] and
// offsets[s] -- at the top of the iteration q == blocks_g: right behind its last round (behind the tail when it has no whole
// line), before the wave runs another round.  From then on it is DEAD, and so is, from the start, a group without a stream
// or with a rejected one.  That answers the two hazards of a group that has to ride along under full exec:
//   1. the sequence's ds_write_b16 runs under exec = vcc, the whole wave's emitters, whatever the group's bits of the ballot
//      are.  A dead group's bits are zeroed (its c stands still, its rank is 0), but its lanes still write, at
//      ring | (-2 c & 255): the place of the word the stream emitted last.  Because the group was finalised before the first
//      such round, that word has left; flush_block and the index stores are closed to a dead group for good, so what its ring,
//      its x and its c become is of no consequence: the record address comes from the symbol byte (zero: inside the table),
//      the ring address is masked into the group's own 256 bytes, and it reads and writes no global memory;
//   2. TRACK ORs the record's third word into `worst`, and a dead group is fed the record of byte value 0, which a model
//      need not have: `worst` is put back from a copy behind every line for the groups that did not run it.
// Index entries are the caller's data and checked exactly as k_encode's MODE 4 checks them (encode_wave.hip): a slot that
// fails is not written, lengths[s] = 0, offsets[s] = the slot's end, bit 1 of the flags; an order entry that names no stream
// codes nothing, writes no index entry and sets bit 11 (RANS_AMD_E_ARG).  Every lane addresses symbols and slots in 64 bits.
// ---------------------------------------------------------------------------
typedef uint32_t u32x4_sym __attribute__((ext_vector_type(4), aligned(4))); // a line piece on the 4-byte grid

template <bool SMALL, bool TRACK>
__global__ void __launch_bounds__(kGrpThreads, 8) k_encode_batch_word_groups(const EncParams p)
{
    using Tr = FmtTraits<FMT_WORD>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stage_table(smem, p.word_enc_recs, kEncGrpTable);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never code on a wrong assumption
        if (threadIdx.x == 0)
            atomicOr(p.flags, 4u);
        return;
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t g = lane >> 3, i = lane & 7u;
    const uint32_t ring_c = kEncGrpTable + wave * kGrpWaveLds + g * kGrpRing; // (as in k_encode_word_groups)
    uint32_t ring = ring_c;
    uint32_t gm_lo, gm_hi, k255 = 255u, k4 = 4u;
    pin_vgpr(ring);
    group_ballot_bits(g, gm_lo, gm_hi);
    pin_vgpr(k255);
    pin_vgpr(k4);
    const uint32_t sel1 = (lane & 1u) ? 0x03070105u : 0x06020400u;
    const uint32_t sel2 = (lane & 2u) ? 0x03020706u : 0x05040100u;
    const uint64_t octets = (p.nchunks + 7u) >> 3; // one per claim (the last one may hold fewer than eight streams)

    uint32_t worst = 0;
    WorkClaims work;
    work.init(p.claims, wave, waves_per_block);
    for (;;) {
        const uint64_t octet = work.take(lane);
        if (octet >= octets)
            break;
        // ---- this group's stream: its index entries, all of them the caller's data
        const uint64_t pos = octet * 8u + g;
        const bool exists = pos < p.nchunks;
        uint64_t s = pos;
        if (exists && p.order)
            s = p.order[pos];
        const bool named = exists && s < p.nchunks;
        if (exists && !named && i == 0) // an order entry that names no stream: nothing coded, no index entry
            atomicOr(p.flags, 2048u);
        uint64_t first = 0, slot_at = 0, slot_end = 0;
        uint32_t count = 0;
        if (named) {
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
            slot_at = p.slot_offsets[s];
            slot_end = p.slot_offsets[s + 1];
        }
        // what rans_amd_chunk_bound() asks for this stream: two bytes per symbol + the eight flushed states
        const uint64_t need = ((uint64_t)count * 2u + 8u * 4u + 15u) & ~15ull;
        const uint64_t slot_size = slot_end - slot_at;
        const bool fits = ((slot_at | slot_end) & 15u) == 0 && slot_end >= slot_at && slot_end <= p.out_cap && slot_size >= need &&
                          slot_size <= 0xfffffff0ull;
        if (named && !fits && i == 0) { // nothing of this stream is written
            atomicOr(p.flags, 2u);
            p.lengths[s] = 0u;
            p.offsets[s] = slot_end;
        }
        bool live = named && fits; // the group holds a stream that is still being coded
        const uint32_t slot = (uint32_t)slot_size;
        const uint64_t out_end = reinterpret_cast<uint64_t>(p.scratch) + slot_end; // (live: 16-byte aligned, inside the container)
        const uint64_t src = reinterpret_cast<uint64_t>(p.syms) + first;
        const uint32_t blocks = (live && (src & 3u) == 0) ? count >> 7 : 0u;
        const uint32_t tail = live ? count - (blocks << 7) : 0u;
        const uint32_t tail_rounds = (uint32_t)(((uint64_t)tail + 7u) >> 3);
        const uint32_t max_blocks = wave_max8(blocks), max_tail_rounds = wave_max8(tail_rounds);

        uint32_t x = Tr::kL, c = 0, fb = 0; // state, words emitted so far (the group's), blocks flushed
        uint32_t m_lo = live ? gm_lo : 0u, m_hi = live ? gm_hi : 0u; // my group's bits of the ballot; none once it is dead
        // block fb of the ring -> its place below the slot's end; a piece that would start below the slot's first byte is dropped,
        // and so is one that lies wholly below the stream (k_encode_word_groups' two guards); nothing leaves a dead group
        auto flush_block = [&](uint32_t have_bytes) { // have_bytes: the group's stream so far
            const uint64_t below = (uint64_t)kGrpBlock * (fb + 1u) - 16u * i; // this lane's piece starts `below` bytes under the slot's end
            if (live && below <= slot && below - 16u < have_bytes) {
                const u32x4 v = *reinterpret_cast<RANS_LDS const u32x4 *>((uintptr_t)(ring_c + ((fb & 1u) ? 0u : kGrpBlock) + 16u * i));
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(out_end - below) = v;
            }
            fb += 1u;
        };
        auto one_round = [&](uint32_t sym, bool active) { encode_word_round<SMALL>(x, c, worst, sym, active, m_lo, m_hi, ring_c); };
        // ---- tail: the rounds behind the stream's last whole line, the group's last round first
        {
            const uint8_t RANS_GLOBAL *tsrc = reinterpret_cast<const uint8_t RANS_GLOBAL *>(src + ((uint64_t)blocks << 7) + i);
            for (uint32_t k = 0; k < max_tail_rounds; ++k) {
                const bool in = k < tail_rounds; // (the same for the eight lanes of a group)
                const uint32_t r = tail_rounds - 1u - k;
                const bool active = in && r * 8u + i < tail; // (r < 2^29: count < 2^31 follows from the slot's size)
                one_round(active ? (uint32_t)tsrc[(uint64_t)r * 8u] : 0u, active);
                // (at least every eight rounds of any group; never true for a group that sits out: its c stands still)
                if ((k & 7u) == 7u && c >= 64u * (fb + 1u))
                    flush_block(2u * c);
            }
        }
        // ---- lines: sixteen rounds each, the group's last line first
        uint64_t lp = src + ((uint64_t)blocks << 7) + 16u * i; // 128 bytes above this lane's piece of the next line to load
        auto load_line = [&](bool want) -> u32x4 {
            u32x4 v = {0u, 0u, 0u, 0u}; // (a dead group codes zeros)
            if (want) {
                lp -= kGrpBlock;
                const u32x4_sym t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_sym RANS_GLOBAL *>(lp));
                v = u32x4{t.x, t.y, t.z, t.w};
            }
            return v;
        };
        u32x4 next = load_line(blocks != 0u);
        for (uint32_t q = 0;; ++q) {
            if (live && q == blocks) { // ---- finalise: this group's last round is behind it
                if (c >= 64u * (fb + 1u)) // (the last eight rounds' block)
                    flush_block(2u * c);
                // the final states, state 0 lowest (RansWordEncFlush): lane i's dword starts 2 c + 32 - 4 i bytes below the slot's end
                const uint32_t at = 0u - (2u * c + 32u - 4u * i);
                *reinterpret_cast<RANS_LDS uint16_t *>((uintptr_t)(ring_c | (at & 255u))) = (uint16_t)x;
                *reinterpret_cast<RANS_LDS uint16_t *>((uintptr_t)(ring_c | ((at + 2u) & 255u))) = (uint16_t)(x >> 16);
                c += 16u;
                const uint32_t len = 2u * c;
                if (64u * fb < c)
                    flush_block(len);
                if (64u * fb < c)
                    flush_block(len);
                if (i == 0) {
                    p.lengths[s] = len;
                    p.offsets[s] = slot_end - len;
                }
                live = false; // dead: no block, no index store ever again
                m_lo = m_hi = 0u;
            }
            if (q == max_blocks)
                break;
            const bool run = q < blocks;
            const u32x4 v = next;
            next = load_line(q + 1u < blocks);
            const uint32_t worst_keep = worst;
            encode_line<SMALL, TRACK>(v, x, c, worst, fb, sel1, sel2, k4, m_lo, m_hi, k255, ring, flush_block); // (under full exec: see there)
            worst = run ? worst : worst_keep;
        }
    }
    if (TRACK && __builtin_amdgcn_ballot_w64((worst >> 31) != 0) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

// ---------------------------------------------------------------------------
// k_encode_batch_byte_pairs -- the byte format's 2-way layout (rans_byte.h:62-90, main.cpp:226-246: two states, one pointer
// that moves DOWN) for rans_amd_encode_batch[_ordered] under RANS_AMD_OPT_BATCH_ENCODE_PAIRS: THIRTY-TWO streams per wave,
// the mirror image of decode_groups.hip's k_decode_batch_byte_pairs.  The unit of work is one wave-load of the hand-out
// order: lane 2 g + i holds state i of the stream at position 32 w + g -- stream order[32 w + g], or 32 w + g without an
// order; a position at or past nchunks has no stream.
//   * the coder runs from a stream's last symbol to its first; round r holds symbols 2 r (state 0) and 2 r + 1 (state 1), an
//     odd count's last symbol is state 0's alone and is coded first (main.cpp:232-236);
//   * a state emits 0, 1 or 2 bytes (`while x >= x_max`, scale_bits <= 16), its low byte first -- highest.  Inside a round
//     state 1 puts first: the odd lane writes from the pair's cursor c (bytes emitted so far), the even lane from c + the odd
//     lane's count, which comes through one DPP swap of the pair (the decoder's sequence with odd and even exchanged); a lane's
//     count is its own two compares, there is no ballot;
//   * stream byte k (0 = the first emitted) lives at offset 63 - (k & 63) of the pair's 64-byte ring in LDS, two 32-byte
//     blocks; rows kPairRow = 68 bytes apart, so that equal positions of the 32 pairs fall on 32 banks.  Eight rounds emit at
//     most 8 x 2 x 2 = 32 bytes per pair: one compare per lane every eight rounds decides whether a finished block leaves,
//     16 bytes per lane, to its place below the end of the stream's slot (slot_end is a multiple of 16, blocks are counted
//     down from it: k_encode_batch_word_groups' flush_block with its two guards);
//   * records {rcp, cmpl | rshift << 24, bias, x_max} (encode_common.hpp enc_byte_full's), 256 of them at LDS address 0, built
//     in the prologue from EncParams::enc_recs; a byte value without a record never emits, leaves x alone and carries bit 31
//     in its second word: TRACK (models that have such values) ORs those words together, bit 0 of the flags at the end;
//   * symbols: whole 32-byte pieces of a stream whose first symbol is 4-byte aligned -- sixteen rounds, 16 bytes per lane, the
//     next piece in flight while this one is coded -- are taken apart into per-state dwords by the inverse of the decoder's
//     pair_lines and coded by a hand-scheduled eight-round sequence under FULL exec (it sets exec = -1 itself, and its DPP
//     moves read the pair's other lane).  The count_g - 32 pieces_g symbols behind the last whole piece (all of them where
//     the first symbol is not 4-byte aligned) go one compiler-scheduled round at a time, a byte load per lane, lanes without
//     a symbol sitting out -- FIRST, because they are the end of the stream.
// The 32 pairs START together and finish at different times.  A pair is FINALISED -- its last block check, the two flushed
// states (RansEncFlush(rans1), then rans0: state 0's dword lowest), the last one or two blocks, lengths[s] and offsets[s]
// -- at the top of the iteration q == pieces_g: right behind its last round, before the wave runs another one.  From then
// on it is DEAD, and so is, from the start, a pair without a stream or with a rejected one.  A dead pair rides along under
// full exec and, unlike a dead group of the word encoder, its cursor DOES move (its count is its own compares).  It is left
// to run free -- it is never resumed, so there is nothing to put back -- and that is safe:
//   * nothing of it ever leaves: flush_block and the index stores test `live`, which is cleared for good;
//   * its ring writes go to top - (position & 63), inside its own row whatever its cursor is, and everything of its
//     stream had left the ring when it was finalised;
//   * it loads no symbol (load_piece fetches under q + 1 < pieces_g) and codes zeros: it reads only the record of byte value 0;
//   * it cannot raise the model flag, even when byte value 0 has no record: `worst` is put back from a copy behind every
//     piece for the pairs that did not run it (the rounds of the tail track under `active` only);
//   * it cannot raise any other flag: bits 1 and 11 are set in the claim's set-up alone.
// Index entries are the caller's data and checked exactly as k_encode_batch_word_groups checks them, with need = align16(2 *
// count + 2 * 4) = rans_amd_chunk_bound(): a slot that fails is not written, lengths[s] = 0, offsets[s] = the slot's end, bit
// 1 of the flags; an order entry that names no stream codes nothing, writes no index entry and sets bit 11.  Every lane
// addresses symbols and slots in 64 bits.  A stream of 0 symbols is the two flushed initial states.
// What follows from the lane number is worked out per claim (lane_number_now) and the claim compare is scalar, as in the pair
// decoder: nothing of it stays in registers across the piece loop.  No MFMA: integer, table-driven, serial per state.
// ---------------------------------------------------------------------------
constexpr uint32_t kEncPairTable = 256 * 16; // the records, at LDS address 0

// One round of the eight, 21 VALU (+ 1 with TRACK) + 3 LDS; vcc = the odd lanes for the whole sequence, v56..v59 the record:
//   v_lshlrev (SDWA byte J)     LDS address of the symbol's record
//   ds_read_b128, v_lshrrev     {rcp, cmpl | rshift << 24, bias, x_max}; t1 = x >> 8
//   v_cmp x2                    n1 = x >= x_max (at least one byte leaves), n2 = x >> 8 >= x_max (two)
//   v_addc x2                   t2 = c + n1 + n2: where this lane's bytes END if it is the pair's first
//   v_cndmask_dpp               my position = odd lane: the cursor; even lane: the odd lane's t2
//   v_add_dpp, v_sub            the pair's next cursor = t2 + the other lane's t2 - c
//   v_and, v_sub / v_add, v_and, v_sub   position, position + 1 -> LDS addresses in the pair's ring (downwards from `top`)
//   ds_write_b8 x2, v_mov, v_lshrrev     under exec = n1 / n2: the low byte leaves, then the next one
//   v_mul_hi .. v_add           x = x + bias + (x / freq) * cmpl (enc_byte_full's tail)
#define RANS_PE_ROUND(ACC, SEL, TRACKSTR)                                                                              \
    "v_lshlrev_b32_sdwa %[t0], %[k4], " ACC " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t"   \
    "ds_read_b128 v[56:59], %[t0]\n\t"                                                                                 \
    "v_lshrrev_b32_e32 %[t1], 8, %[x]\n\t"                                                                             \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    "v_cmp_ge_u32_e64 %[n1], %[x], v59\n\t"                                                                            \
    "v_cmp_ge_u32_e64 %[n2], %[t1], v59\n\t"                                                                           \
    TRACKSTR                                                                                                           \
    "v_addc_co_u32_e64 %[t2], %[dm], %[c], 0, %[n1]\n\t"                                                               \
    "v_addc_co_u32_e64 %[t2], %[dm], %[t2], 0, %[n2]\n\t"                                                              \
    "s_nop 1\n\t"                                                                                                      \
    "v_cndmask_b32_dpp %[t3], %[t2], %[c], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_add_u32_dpp %[t0], %[t2], %[t2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                              \
    "v_sub_u32_e32 %[c], %[t0], %[c]\n\t"                                                                              \
    "v_and_b32_e32 %[t0], 63, %[t3]\n\t"                                                                               \
    "v_sub_u32_e32 %[t0], %[top], %[t0]\n\t"                                                                           \
    "v_add_u32_e32 %[t3], 1, %[t3]\n\t"                                                                                \
    "v_and_b32_e32 %[t3], 63, %[t3]\n\t"                                                                               \
    "v_sub_u32_e32 %[t3], %[top], %[t3]\n\t"                                                                           \
    "s_mov_b64 exec, %[n1]\n\t"                                                                                        \
    "ds_write_b8 %[t0], %[x]\n\t"                                                                                      \
    "v_mov_b32_e32 %[x], %[t1]\n\t"                                                                                    \
    "s_mov_b64 exec, %[n2]\n\t"                                                                                        \
    "ds_write_b8 %[t3], %[t1]\n\t"                                                                                     \
    "v_lshrrev_b32_e32 %[x], 8, %[x]\n\t"                                                                              \
    "s_mov_b64 exec, -1\n\t"                                                                                           \
    "v_mul_hi_u32 %[t0], %[x], v56\n\t"                                                                                \
    "v_lshrrev_b32_sdwa %[t0], v57, %[t0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t"        \
    "v_mad_u32_u24 %[t0], %[t0], v57, %[x]\n\t"                                                                        \
    "v_add_u32_e32 %[x], %[t0], v58\n\t"
#define RANS_PE_FOUR(ACC, TRACKSTR)                                                                                    \
    RANS_PE_ROUND(ACC, "BYTE_3", TRACKSTR) RANS_PE_ROUND(ACC, "BYTE_2", TRACKSTR) RANS_PE_ROUND(ACC, "BYTE_1", TRACKSTR) \
    RANS_PE_ROUND(ACC, "BYTE_0", TRACKSTR)
#define RANS_PE_EIGHT(TRACKSTR)                                                                                        \
    asm volatile("s_mov_b64 vcc, %[odds]\n\t" RANS_PE_FOUR("%[hi]", TRACKSTR) RANS_PE_FOUR("%[lo]", TRACKSTR)            \
                 : [x] "+v"(x), [c] "+v"(c), [worst] "+v"(worst), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), \
                   [n1] "=&s"(n1), [n2] "=&s"(n2), [dm] "=&s"(dm)                                                       \
                 : [hi] "v"(hi), [lo] "v"(lo), [k4] "v"(k4), [top] "v"(top), [odds] "s"(0xaaaaaaaaaaaaaaaaull)         \
                 : "vcc", "memory", "v56", "v57", "v58", "v59")
// eight rounds of a pair, the last first: bytes 3 .. 0 of `hi` (four rounds of this lane's state), then of `lo`
template <bool TRACK>
__device__ __forceinline__ void encode_pairs_8rounds(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t hi, uint32_t lo, uint32_t k4, uint32_t top)
{
    uint32_t t0, t1, t2, t3;
    uint64_t n1, n2, dm;
    if constexpr (TRACK)
        RANS_PE_EIGHT("v_or_b32_e32 %[worst], %[worst], v57\n\t");
    else
        RANS_PE_EIGHT("s_nop 0\n\t");
}
#undef RANS_PE_EIGHT
#undef RANS_PE_FOUR
#undef RANS_PE_ROUND

// The alias format's round (k_encode_batch_alias_pairs, behind the byte kernel; RansEncPutAlias, main_alias.cpp:241-250: the byte
// format's renormalisation, then x = ((x / freq) << scale_bits) + alias_remap[(x % freq) + start]).  The renormalisation, the DPP
// exchange of the counts and the two ds_write_b8 are RANS_PE_ROUND's, instruction for instruction; the put is new.  Records
// {rcp, (2^24 - freq) | rshift << 24, start | inc << 16, x_max} at LDS address sym << 4, remap16 behind them (the ds_read_u16's
// offset field is its base), v56..v59 the record:
//   v_mul_hi, v_lshrrev (SDWA)  q0 = mulhi(x, rcp) >> rshift: Alverson's reciprocal, exact for x < 2^31 -- but for freq == 1,
//   v_add (SDWA word 1)         where mulhi(x, 2^32 - 1) = x - 1: that record's inc is 1.  q = q0 + inc
//   v_mad_u32_u24               t2 = q * (2^24 - freq) + x: its low 24 bits are x - q * freq = x % freq (q < 2^23, freq < 2^16)
//   v_add_lshl, v_and           byte offset of the gather = 2 (t2 + start) under mask2 = (2^scale_bits - 1) << 1: whatever the
//                               lane holds -- a dead pair, no stream, no record -- the read stays inside remap16 (inc << 16 is
//                               shifted to bit 17, the high bits of t2 above that: both outside the mask)
//   ds_read_u16                 the one new LDS round trip; the NEXT round's record is asked for behind it (its address comes
//                               from the symbol byte alone, v56..v59 are free from here), so the wait for the gather --
//   s_waitcnt lgkmcnt(1)        -- leaves that read in flight, and the next round's lgkmcnt(0) finds it (nearly) there
//   v_lshl_add                  x = (q << scale_bits) + remap16[...]
// 23 VALU (+ 1 with TRACK) + 4 LDS per round (profiles/batch_encode_alias_pairs_isa.md).  A byte value without a record: {0, ~0, 0, ~0} -- it never emits (the count is
// still the lane's own two compares: at most 2 bytes per lane and round, whatever x is), q = 0, and bit 31 of its second word is
// TRACK's.
#define RANS_AE_LOAD(ACC, SEL)                                                                                         \
    "v_lshlrev_b32_sdwa %[t3], %[k4], " ACC " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t"   \
    "ds_read_b128 v[56:59], %[t3]\n\t"
#define RANS_AE_ROUND(NEXT, WAIT, TRACKSTR)                                                                            \
    "v_lshrrev_b32_e32 %[t1], 8, %[x]\n\t"                                                                             \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    "v_cmp_ge_u32_e64 %[n1], %[x], v59\n\t"                                                                            \
    "v_cmp_ge_u32_e64 %[n2], %[t1], v59\n\t"                                                                           \
    TRACKSTR                                                                                                           \
    "v_addc_co_u32_e64 %[t2], %[dm], %[c], 0, %[n1]\n\t"                                                               \
    "v_addc_co_u32_e64 %[t2], %[dm], %[t2], 0, %[n2]\n\t"                                                              \
    "s_nop 1\n\t"                                                                                                      \
    "v_cndmask_b32_dpp %[t3], %[t2], %[c], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_add_u32_dpp %[t0], %[t2], %[t2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"                              \
    "v_sub_u32_e32 %[c], %[t0], %[c]\n\t"                                                                              \
    "v_and_b32_e32 %[t0], 63, %[t3]\n\t"                                                                               \
    "v_sub_u32_e32 %[t0], %[top], %[t0]\n\t"                                                                           \
    "v_add_u32_e32 %[t3], 1, %[t3]\n\t"                                                                                \
    "v_and_b32_e32 %[t3], 63, %[t3]\n\t"                                                                               \
    "v_sub_u32_e32 %[t3], %[top], %[t3]\n\t"                                                                           \
    "s_mov_b64 exec, %[n1]\n\t"                                                                                        \
    "ds_write_b8 %[t0], %[x]\n\t"                                                                                      \
    "v_mov_b32_e32 %[x], %[t1]\n\t"                                                                                    \
    "s_mov_b64 exec, %[n2]\n\t"                                                                                        \
    "ds_write_b8 %[t3], %[t1]\n\t"                                                                                     \
    "v_lshrrev_b32_e32 %[x], 8, %[x]\n\t"                                                                              \
    "s_mov_b64 exec, -1\n\t"                                                                                           \
    "v_mul_hi_u32 %[t0], %[x], v56\n\t"                                                                                \
    "v_lshrrev_b32_sdwa %[t0], v57, %[t0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t"        \
    "v_add_u32_sdwa %[t0], %[t0], v58 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n\t"            \
    "v_mad_u32_u24 %[t2], %[t0], v57, %[x]\n\t"                                                                        \
    "v_add_lshl_u32 %[t2], %[t2], v58, 1\n\t"                                                                          \
    "v_and_b32_e32 %[t2], %[mask2], %[t2]\n\t"                                                                         \
    "ds_read_u16 %[t2], %[t2] offset:4096\n\t"                                                                         \
    NEXT                                                                                                               \
    WAIT                                                                                                               \
    "v_lshl_add_u32 %[x], %[t0], %[sbv], %[t2]\n\t"
#define RANS_AE_NEXT(ACC, SEL, TRACKSTR) RANS_AE_ROUND(RANS_AE_LOAD(ACC, SEL), "s_waitcnt lgkmcnt(1)\n\t", TRACKSTR)
#define RANS_AE_EIGHT(TRACKSTR)                                                                                        \
    asm volatile("s_mov_b64 vcc, %[odds]\n\t" RANS_AE_LOAD("%[hi]", "BYTE_3")                                            \
                 RANS_AE_NEXT("%[hi]", "BYTE_2", TRACKSTR) RANS_AE_NEXT("%[hi]", "BYTE_1", TRACKSTR)                     \
                 RANS_AE_NEXT("%[hi]", "BYTE_0", TRACKSTR) RANS_AE_NEXT("%[lo]", "BYTE_3", TRACKSTR)                     \
                 RANS_AE_NEXT("%[lo]", "BYTE_2", TRACKSTR) RANS_AE_NEXT("%[lo]", "BYTE_1", TRACKSTR)                     \
                 RANS_AE_NEXT("%[lo]", "BYTE_0", TRACKSTR) RANS_AE_ROUND("", "s_waitcnt lgkmcnt(0)\n\t", TRACKSTR)       \
                 : [x] "+v"(x), [c] "+v"(c), [worst] "+v"(worst), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), \
                   [n1] "=&s"(n1), [n2] "=&s"(n2), [dm] "=&s"(dm)                                                       \
                 : [hi] "v"(hi), [lo] "v"(lo), [k4] "v"(k4), [top] "v"(top), [sbv] "v"(sbv), [mask2] "v"(mask2),       \
                   [odds] "s"(0xaaaaaaaaaaaaaaaaull)                                                                   \
                 : "vcc", "memory", "v56", "v57", "v58", "v59")
// eight rounds of an alias pair, the last first (encode_pairs_8rounds' arguments + the two constants of the put)
template <bool TRACK>
__device__ __forceinline__ void encode_alias_pairs_8rounds(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t hi, uint32_t lo, uint32_t k4, uint32_t top,
                                                           uint32_t sbv, uint32_t mask2)
{
    uint32_t t0, t1, t2, t3;
    uint64_t n1, n2, dm;
    if constexpr (TRACK)
        RANS_AE_EIGHT("v_or_b32_e32 %[worst], %[worst], v57\n\t");
    else
        RANS_AE_EIGHT("s_nop 0\n\t");
}
#undef RANS_AE_EIGHT
#undef RANS_AE_NEXT
#undef RANS_AE_ROUND
#undef RANS_AE_LOAD

// One compiler-scheduled round of an alias pair: groups_common.hpp's encode_pair_round with the alias put (the same
// instructions as RANS_AE_ROUND's, in C++).  Lanes without a symbol sit the round out; an active lane whose byte value has no
// record emits nothing, tracks bit 31 and gathers under the mask like every other.
__device__ __forceinline__ void encode_alias_pair_round(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t sym, bool active, uint32_t odd, uint32_t top,
                                                        int lane_o, uint32_t sbv, uint32_t mask2)
{
    const u32x4 rec = *reinterpret_cast<RANS_LDS const u32x4 *>((uintptr_t)(sym << 4));
    uint32_t n = 0;
    if (active)
        n = (uint32_t)(x >= rec.w) + (uint32_t)((x >> 8) >= rec.w);
    const uint32_t n_other = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_o, (int)n);
    const uint32_t at = c + (odd ? 0u : n_other);
    c += n + n_other;
    if (n >= 1u)
        *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)(top - (at & 63u))) = (uint8_t)x;
    if (n >= 2u)
        *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)(top - ((at + 1u) & 63u))) = (uint8_t)(x >> 8);
    x >>= 8u * n;
    if (active) {
        const uint32_t q = (__umulhi(x, rec.x) >> ((rec.y >> 24) & 31u)) + (rec.z >> 16);
        const uint32_t t = (q & 0xffffffu) * (rec.y & 0xffffffu) + x; // low 24 bits: x - q * freq
        const uint32_t at2 = ((t + rec.z) << 1) & mask2;              // inside remap16 whatever the lane holds
        x = (q << sbv) + *reinterpret_cast<RANS_LDS const uint16_t *>((uintptr_t)(kEncPairTable + at2));
        worst |= rec.y;
    }
}

// The inverse of decode_groups.hip's pair_lines: 32 bytes of a pair's stream of symbols, bytes [0, 16) in the even lane and
// [16, 32) in the odd one, -> d0..d3, the four dwords of this lane's state (byte J of d_m: round 4 m + J of the piece's
// sixteen).  The lanes first swap dwords so that the even lane holds dwords 0, 2, 4, 6 of the piece and the odd lane 1, 3, 5,
// 7; then every lane picks its state's bytes out of its own dword and the other lane's (sel: v_perm(theirs, mine)).
__device__ __forceinline__ void piece_to_states(const u32x4 &v, uint32_t &d0, uint32_t &d1, uint32_t &d2, uint32_t &d3, uint32_t sel)
{
    uint32_t e0, e1, e2, e3;
    asm volatile("s_nop 1\n\t"
                 "s_mov_b64 vcc, %[evens]\n\t"
                 "v_cndmask_b32_dpp %[e0], %[vy], %[vx], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" // even ? mine : the even lane's y
                 "v_cndmask_b32_dpp %[e1], %[vw], %[vz], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_mov_b64 vcc, %[odds]\n\t"
                 "v_cndmask_b32_dpp %[e2], %[vx], %[vy], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" // odd ? mine : the odd lane's x
                 "v_cndmask_b32_dpp %[e3], %[vz], %[vw], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_mov_b32_dpp %[d0], %[e0] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[d1], %[e1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[d2], %[e2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[d3], %[e3] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_perm_b32 %[d0], %[d0], %[e0], %[sel]\n\t" // even: [mine.0, mine.2, theirs.0, theirs.2]; odd: [theirs.1, theirs.3, mine.1, mine.3]
                 "v_perm_b32 %[d1], %[d1], %[e1], %[sel]\n\t"
                 "v_perm_b32 %[d2], %[d2], %[e2], %[sel]\n\t"
                 "v_perm_b32 %[d3], %[d3], %[e3], %[sel]"
                 : [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [e0] "=&v"(e0), [e1] "=&v"(e1), [e2] "=&v"(e2),
                   [e3] "=&v"(e3)
                 : [vx] "v"(v.x), [vy] "v"(v.y), [vz] "v"(v.z), [vw] "v"(v.w), [sel] "v"(sel), [evens] "s"(0x5555555555555555ull),
                   [odds] "s"(0xaaaaaaaaaaaaaaaaull)
                 : "vcc");
}

// The sixteen rounds of a piece that piece_to_states has taken apart, last round first.  flush(have_bytes) is the kernel's
// flush_block: the block that the eight rounds before may have finished leaves in front of the next eight.  (A dead pair's
// check may be true -- its cursor moves -- and its flush_block then only counts the block.)
// ALIAS: the alias format's rounds (sbv, mask2: the constants of their put; the byte kernel passes zeros that nobody reads).
template <bool ALIAS, bool TRACK, class FLUSH>
__device__ __forceinline__ void encode_piece(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t &x, uint32_t &c, uint32_t &worst,
                                             const uint32_t &fb, uint32_t k4, uint32_t top, uint32_t sbv, uint32_t mask2, FLUSH &&flush)
{
    if (c >= kPairBlock * (fb + 1u))
        flush(c);
    if constexpr (ALIAS)
        encode_alias_pairs_8rounds<TRACK>(x, c, worst, d3, d2, k4, top, sbv, mask2);
    else
        encode_pairs_8rounds<TRACK>(x, c, worst, d3, d2, k4, top); // rounds 15 .. 8
    if (c >= kPairBlock * (fb + 1u))
        flush(c);
    if constexpr (ALIAS)
        encode_alias_pairs_8rounds<TRACK>(x, c, worst, d1, d0, k4, top, sbv, mask2);
    else
        encode_pairs_8rounds<TRACK>(x, c, worst, d1, d0, k4, top); // rounds 7 .. 0
}

// The body of k_encode_batch_byte_pairs and, with ALIAS, of k_encode_batch_alias_pairs (behind it): everything but the tables, the
// rings' base and the rounds is the same code.
template <bool ALIAS, bool TRACK> __device__ __forceinline__ void encode_batch_pairs(const EncParams p)
{
    using Tr = FmtTraits<FMT_BYTE>; // (the alias format's states are the byte format's: RANS_BYTE_L, 32 bits)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if constexpr (ALIAS) {
        // {freq | start << 16, floor(2^32 / freq)} (padded to 256 by the host) -> the sequence's records {rcp, (2^24 - freq) | rshift
        // << 24, start | inc << 16, x_max}: Alverson's reciprocal (rans_byte.h:201-243) from the frequency, inc = 1 for freq == 1
        const uint2 *g0 = reinterpret_cast<const uint2 *>(p.alias_recs8);
        uint4 *l0 = reinterpret_cast<uint4 *>(smem);
        for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) {
            const uint2 r = g0[k];
            const uint32_t freq = k < p.nsyms ? r.x & 0xffffu : 0u, start = r.x >> 16;
            uint4 rec = {0u, 0xffffffffu, 0u, 0xffffffffu}; // no frequency: nothing leaves, q = 0, bit 31 for TRACK
            if (freq == 1u) {
                rec = uint4{0xffffffffu, 0xffffffu, start | 0x10000u, 1u << (31u - p.scale_bits)};
            } else if (freq) {
                const uint32_t sh = 32u - (uint32_t)__builtin_clz(freq - 1u); // ceil(log2 freq), 1..16
                const uint32_t rcp = (uint32_t)(((1ull << (sh + 31u)) + freq - 1u) / freq);
                rec = uint4{rcp, (0x1000000u - freq) | ((sh - 1u) << 24), start, freq << (31u - p.scale_bits)};
            }
            l0[k] = rec;
        }
        stage_table(smem + kEncPairTable, p.alias_remap16, 2u << p.scale_bits); // remap16 behind the records
    } else { // EncRec {freq | rshift << 24, bias, rcp, -} -> the sequence's records (k_encode<byte>'s prologue), 256 of them
        const uint4 *g0 = reinterpret_cast<const uint4 *>(p.enc_recs);
        uint4 *l0 = reinterpret_cast<uint4 *>(smem);
        for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) {
            const uint4 r = k < p.nsyms ? g0[k] : uint4{0u, 0u, 0u, 0u};
            const uint32_t freq = r.x & 0xffffffu;
            l0[k] = freq ? uint4{r.z, (((1u << p.scale_bits) - freq) & 0xffffffu) | (r.x & 0xff000000u), r.y, freq << (31u - p.scale_bits)}
                         : uint4{0u, 0xffffffffu, 0u, 0xffffffffu}; // no frequency: nothing leaves, x stays, bit 31 for TRACK
        }
    }
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never code on a wrong assumption
        if (threadIdx.x == 0)
            atomicOr(p.flags, 4u);
        return;
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    uint32_t rings_at = kEncPairTable; // the rows, behind the tables
    if constexpr (ALIAS)
        rings_at += 2u << p.scale_bits;
    uint32_t ring = rings_at + wave * kPairWaveLds + (lane >> 1) * kPairRow; // raw LDS byte address of the pair's ring
    uint32_t ring_i = ring + 16u * (lane & 1u);                              // where this lane's 16 bytes of a block lie
    uint32_t top = ring + (kPairRing - 1u), k4 = 4u;
    uint32_t sel = (lane & 1u) ? 0x03010705u : 0x06040200u;
    uint32_t sbv = 0u, mask2 = 0u; // ALIAS: the put's shift, and what keeps its gather inside remap16
    pin_vgpr(ring);
    pin_vgpr(ring_i);
    pin_vgpr(top);
    pin_vgpr(k4);
    pin_vgpr(sel);
    if constexpr (ALIAS) {
        sbv = p.scale_bits;
        mask2 = ((1u << p.scale_bits) - 1u) << 1;
        pin_vgpr(sbv);
        pin_vgpr(mask2);
    }
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 31u) >> 5); // wave-loads, one per claim (the last one may hold fewer than 32
                                                                         // streams); stream indices are 32-bit

    uint32_t worst = 0;
    WorkClaims work;
    work.init(p.claims, wave, waves_per_block);
    for (;;) {
        const uint64_t load = work.take(lane);
        if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
            break;
        // ---- this pair's stream: its index entries, all of them the caller's data
        const uint32_t ln = lane_number_now();
        const uint32_t g = ln >> 1, i = ln & 1u;
        const uint64_t pos = load * 32u + g;
        const bool exists = pos < p.nchunks;
        uint64_t s = pos;
        if (exists && p.order)
            s = p.order[pos];
        const bool named = exists && s < p.nchunks;
        if (exists && !named && i == 0) // an order entry that names no stream: nothing coded, no index entry
            atomicOr(p.flags, 2048u);
        uint64_t first = 0, slot_at = 0, slot_end = 0;
        uint32_t count = 0;
        if (named) {
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
            slot_at = p.slot_offsets[s];
            slot_end = p.slot_offsets[s + 1];
        }
        // what rans_amd_chunk_bound() asks for this stream: two bytes per symbol + the two flushed states
        const uint64_t need = ((uint64_t)count * 2u + 2u * 4u + 15u) & ~15ull;
        const uint64_t slot_size = slot_end - slot_at;
        const bool fits = ((slot_at | slot_end) & 15u) == 0 && slot_end >= slot_at && slot_end <= p.out_cap && slot_size >= need &&
                          slot_size <= 0xfffffff0ull;
        if (named && !fits && i == 0) { // nothing of this stream is written
            atomicOr(p.flags, 2u);
            p.lengths[s] = 0u;
            p.offsets[s] = slot_end;
        }
        bool live = named && fits; // the pair holds a stream that is still being coded
        const uint32_t slot = (uint32_t)slot_size;
        const uint64_t out_end = reinterpret_cast<uint64_t>(p.scratch) + slot_end; // (live: 16-byte aligned, inside the container)
        const uint64_t src = reinterpret_cast<uint64_t>(p.syms) + first;
        const uint32_t pieces = (live && (src & 3u) == 0) ? count >> 5 : 0u;
        const uint32_t tail = live ? count - (pieces << 5) : 0u; // (< 2^31: count < 2^31 follows from the slot's size)
        const uint32_t tail_rounds = (tail + 1u) >> 1;
        const uint32_t max_pieces = wave_max32(pieces), max_tail_rounds = wave_max32(tail_rounds);

        uint32_t x = Tr::kL, c = 0, fb = 0; // state, bytes emitted so far (the pair's), blocks flushed
        // block fb of the ring -> its place below the slot's end; a piece that would start below the slot's first byte is dropped,
        // and so is one that lies wholly below the stream (k_encode_batch_word_groups' two guards); nothing leaves a dead pair
        auto flush_block = [&](uint32_t have_bytes) { // have_bytes: the pair's stream so far
            const uint64_t below = (uint64_t)kPairBlock * (fb + 1u) - (ring_i - ring); // this lane's 16 bytes start `below` bytes under the slot's end
            if (live && below <= slot && below - 16u < have_bytes) {
                RANS_LDS const uint32_t *b = reinterpret_cast<RANS_LDS const uint32_t *>((uintptr_t)(ring_i + ((fb & 1u) ? 0u : kPairBlock)));
                const u32x4 v = {b[0], b[1], b[2], b[3]}; // (rows are 4-byte aligned: four dword reads)
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(out_end - below) = v;
            }
            fb += 1u;
        };
        // ---- tail: the rounds behind the stream's last whole piece, the pair's last round first
        {
            const uint8_t RANS_GLOBAL *tsrc = reinterpret_cast<const uint8_t RANS_GLOBAL *>(src + ((uint64_t)pieces << 5) + i);
            const int lane_o = (int)(4u * (ln ^ 1u)); // the pair's other lane
            for (uint32_t k = 0; k < max_tail_rounds; ++k) {
                const bool in = k < tail_rounds; // (the same for both lanes of a pair)
                const uint32_t r = tail_rounds - 1u - k;
                const bool active = in && 2u * r + i < tail; // (an odd count: state 1 sits the first round out)
                if constexpr (ALIAS)
                    encode_alias_pair_round(x, c, worst, active ? (uint32_t)tsrc[(uint64_t)r * 2u] : 0u, active, i, top, lane_o, sbv, mask2);
                else
                    encode_pair_round(x, c, worst, active ? (uint32_t)tsrc[(uint64_t)r * 2u] : 0u, active, i, top, lane_o);
                // (at least every eight rounds of any pair; never true for a pair that sits out: its c stands still)
                if ((k & 7u) == 7u && c >= kPairBlock * (fb + 1u))
                    flush_block(c);
            }
        }
        // ---- pieces: sixteen rounds each, the pair's last piece first
        uint64_t lp = src + ((uint64_t)pieces << 5) + (ring_i - ring); // 32 bytes above this lane's half of the next piece to load
        auto load_piece = [&](bool want) -> u32x4 {
            u32x4 v = {0u, 0u, 0u, 0u}; // (a dead pair codes zeros)
            if (want) {
                lp -= kPairBlock;
                const u32x4_sym t = *reinterpret_cast<const u32x4_sym RANS_GLOBAL *>(lp);
                v = u32x4{t.x, t.y, t.z, t.w};
            }
            return v;
        };
        u32x4 next = load_piece(pieces != 0u);
        for (uint32_t q = 0;; ++q) {
            if (live && q == pieces) { // ---- finalise: this pair's last round is behind it
                if (c >= kPairBlock * (fb + 1u)) // (the last eight rounds' block)
                    flush_block(c);
                // RansEncFlush(rans1), then (rans0): state 1's dword ends c bytes below the slot's end, state 0's dword below it;
                // byte J of a dword is stream byte k + 3 - J, k the position of its top byte
                const uint32_t k = c + (ring_i == ring ? 4u : 0u);
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j)
                    *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)(top - ((k + 3u - j) & 63u))) = (uint8_t)(x >> (8u * j));
                c += 2u * 4u;
                const uint32_t len = c;
                if (kPairBlock * fb < c)
                    flush_block(len);
                if (kPairBlock * fb < c)
                    flush_block(len);
                if (ring_i == ring) {
                    p.lengths[s] = len;
                    p.offsets[s] = slot_end - len;
                }
                live = false; // dead: no block, no index store ever again
            }
            if (q == max_pieces)
                break;
            const bool run = q < pieces;
            // (the next piece is asked for BEHIND the exchange that consumes this one: the compiler cannot count a conditional
            //  load, its s_waitcnt vmcnt(0) stands in front of the first use of a loaded register -- the exchange -- and in
            //  this order the load it waits for was issued sixteen rounds ago)
            uint32_t d0, d1, d2, d3;
            piece_to_states(next, d0, d1, d2, d3, sel);
            next = load_piece(q + 1u < pieces);
            const uint32_t worst_keep = worst;
            encode_piece<ALIAS, TRACK>(d0, d1, d2, d3, x, c, worst, fb, k4, top, sbv, mask2, flush_block); // (under full exec: see the head)
            worst = run ? worst : worst_keep;
        }
    }
    if (TRACK && __builtin_amdgcn_ballot_w64((worst >> 31) != 0) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

template <bool TRACK> __global__ void __launch_bounds__(kGrpThreads, 8) k_encode_batch_byte_pairs(const EncParams p)
{
    encode_batch_pairs<false, TRACK>(p);
}

// ---------------------------------------------------------------------------
// k_encode_batch_alias_pairs -- the alias format's 2-way layout (main_alias.cpp:241-250, 306-330: two states, one pointer that
// moves DOWN) for rans_amd_encode_batch[_ordered] under RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS: THIRTY-TWO streams per wave, the
// mirror image of decode_groups.hip's k_decode_batch_alias_pairs.  An alias stream IS a byte-format stream -- the same
// renormalisation, the same two states, one pointer, the same flush -- so this is k_encode_batch_byte_pairs' body
// (encode_batch_pairs<ALIAS = true>): the unit of work, tail first and then 32-byte pieces, piece_to_states and load_piece, the
// rings and flush_block with its two guards, the finalise, "dead from then on", the slot check, the flags, 64-bit addressing,
// the scalar claim compare.  Only the put differs (RANS_AE_ROUND): x = ((x / freq) << scale_bits) + remap16[x % freq + start],
// one more LDS gather in sequence.  Two hazards the byte kernel does not have, and their answers:
//   1. the gather's index.  A dead pair, a pair without a stream, a tail lane that sits out (the tail's round gathers under
//      `active` only) and a byte value without a record all run the sequence under full exec, and their start + rem is garbage:
//      the byte offset is ANDed with (2^scale_bits - 1) << 1 in front of every read, so it lies inside remap16 whatever the lane
//      holds.  Nothing relies on what an out-of-range LDS read returns.
//   2. a byte value without a record (frequency 0, or >= nsyms of a 64-symbol model): its record's x_max is ~0, and the count is
//      still the lane's own two compares -- never more than 2 bytes per lane and round, so the slot bound holds by construction.
//      TRACK ORs bit 31 of its second word into `worst` (the call reports RANS_AMD_E_MODEL; what the state becomes is free); a
//      DEAD pair reading the record of byte value 0 raises nothing: `worst` is put back behind every piece, as in the byte kernel.
// LDS: 4 KiB of records at address 0, remap16 (2 << scale_bits bytes) behind them, then the waves' rows (kPairWaveLds each).  The
// block is the launcher's (pairs_plan.hpp enc_alias_pairs_plan): 16 waves, twice per CU up to 14 bits, once at 15; at 16 bits
// the tables leave room for 13 waves.  The kernel works from blockDim.x.
// ---------------------------------------------------------------------------
template <bool TRACK> __global__ void __launch_bounds__(kGrpThreads, 8) k_encode_batch_alias_pairs(const EncParams p)
{
    encode_batch_pairs<true, TRACK>(p);
}

} // namespace

// (api.cpp asks this while it still fills the parameters in: only what it sets first counts -- the shape, the symbol buffer, the
//  slot size, and that neither the fused placement nor a redo is asked for; scratch and container are 16-byte aligned by then)
bool encode_word_groups_applicable(const EncParams &p)
{
    return p.n_ways == 8 && p.sym_bytes == 1 && !p.status && !p.redo && !p.no_lanes && p.nsyms <= 256 && (p.chunk_syms & 3u) == 0 &&
           p.chunk_syms >= 32 && p.chunk_syms <= (1u << 20) && p.nchunks >= 8 && (reinterpret_cast<uintptr_t>(p.syms) & 15u) == 0 &&
           (p.slot_bytes & 15u) == 0 && p.slot_bytes >= 48 && p.slot_bytes < (1ull << 28);
}

// The SMALL / TRACK instantiation a request takes, out of the kernel's four launches [SMALL][TRACK] (word_small: the round-up
// reciprocal is not needed; dense256: every byte value has a record, nothing to track), and its launch: one octet per wave,
// the default dynamic-LDS limit, two blocks per CU.
using EncGroupLaunch = hipError_t (*)(uint64_t, size_t, uint32_t, int, hipStream_t, const EncParams &);
static hipError_t launch_encode_groups(const EncGroupLaunch (&launches)[2][2], const EncParams &p, int num_cus, hipStream_t stream)
{
    const size_t lds = kEncGrpTable + (size_t)(kGrpThreads / 64) * kGrpWaveLds;
    return launches[p.word_small != 0][p.dense256 == 0]((p.nchunks + 7u) / 8u, lds, 0, num_cus, stream, p);
}

hipError_t launch_encode_word_groups(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!p.word_enc_recs || (reinterpret_cast<uintptr_t>(p.scratch) & 15u) != 0)
        return hipErrorInvalidValue;
    if (name)
        *name = KernelId::encode_word_groups;
    static const EncGroupLaunch launches[2][2] = {
        {launch_group_kernel<k_encode_word_groups<false, false>, EncParams>, launch_group_kernel<k_encode_word_groups<false, true>, EncParams>},
        {launch_group_kernel<k_encode_word_groups<true, false>, EncParams>, launch_group_kernel<k_encode_word_groups<true, true>, EncParams>}};
    return launch_encode_groups(launches, p, num_cus, stream);
}

// the ragged form: the reference's 8-way word layout over u8 symbols at 12 bits, from eight streams on (everything else stays
// with the wave-per-stream kernels); counts, symbol addresses and slots are the kernel's to check
bool encode_batch_word_groups_applicable(const EncParams &p)
{
    return p.n_ways == 8 && p.sym_bytes == 1 && p.nsyms <= 256 && p.word_enc_recs && p.scale_bits == 12 && p.nchunks >= 8 &&
           (reinterpret_cast<uintptr_t>(p.scratch) & 15u) == 0;
}

hipError_t launch_encode_batch_word_groups(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!encode_batch_word_groups_applicable(p) || !p.sym_offsets || !p.sym_counts || !p.slot_offsets || !p.lengths || !p.offsets || !p.flags)
        return hipErrorInvalidValue;
    if (name)
        *name = KernelId::encode_batch_word_groups;
    static const EncGroupLaunch launches[2][2] = {
        {launch_group_kernel<k_encode_batch_word_groups<false, false>, EncParams>, launch_group_kernel<k_encode_batch_word_groups<false, true>, EncParams>},
        {launch_group_kernel<k_encode_batch_word_groups<true, false>, EncParams>, launch_group_kernel<k_encode_batch_word_groups<true, true>, EncParams>}};
    return launch_encode_groups(launches, p, num_cus, stream);
}

// the ragged form of the byte format's 2-way layout over u8 symbols, from 32 streams on, at the scale_bits the pair decoder
// takes (a batch that decodes on pairs also encodes on pairs); counts, symbol addresses and slots are the kernel's to check
bool encode_batch_byte_pairs_applicable(const EncParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.nsyms <= 256 && p.scale_bits >= 8 && p.scale_bits <= 16 && p.nchunks >= 32 &&
           (reinterpret_cast<uintptr_t>(p.scratch) & 15u) == 0;
}

// one wave-load per wave; 4 KiB of records and sixteen waves of ring rows: inside the default dynamic-LDS limit, two blocks
// per CU whatever the model's scale_bits
hipError_t launch_encode_batch_byte_pairs(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!encode_batch_byte_pairs_applicable(p) || !p.enc_recs || !p.sym_offsets || !p.sym_counts || !p.slot_offsets || !p.lengths || !p.offsets ||
        !p.flags)
        return hipErrorInvalidValue;
    if (name)
        *name = KernelId::encode_batch_byte_pairs;
    const size_t lds = kEncPairTable + (size_t)(kGrpThreads / 64) * kPairWaveLds;
    const uint64_t loads = (p.nchunks + 31u) / 32u;
    return p.dense256 ? launch_group_kernel<k_encode_batch_byte_pairs<false>, EncParams>(loads, lds, 0, num_cus, stream, p)
                      : launch_group_kernel<k_encode_batch_byte_pairs<true>, EncParams>(loads, lds, 0, num_cus, stream, p);
}

// the ragged form of the alias format's 2-way layout over u8 symbols, from 32 streams on, at the shapes the alias pair decoder
// takes (a batch that decodes on pairs also encodes on pairs), for models that carry the encoder's LDS tables; counts, symbol
// addresses and slots are the kernel's to check
bool encode_batch_alias_pairs_applicable(const EncParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.nsyms >= 2 && p.nsyms <= 256 && (p.nsyms & (p.nsyms - 1u)) == 0 && p.scale_bits >= 8 &&
           p.scale_bits <= 16 && p.nchunks >= 32 && (reinterpret_cast<uintptr_t>(p.scratch) & 15u) == 0 && p.alias_recs8 && p.alias_remap16;
}

// One wave-load per wave; the block and its LDS are enc_alias_pairs_plan's (pairs_plan.hpp) -- launch_group_kernel's blocks are
// kGrpThreads wide, and at 16 bits the tables leave room for 13 waves only, so the few lines of the launch stand here.
template <auto KERN> static hipError_t launch_alias_pairs_kernel(const EncAliasPairsPlan &plan, const EncParams &p, int num_cus, hipStream_t stream)
{
    static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
    if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(KERN), (int)kGrpLdsCap, lds_ok); e != hipSuccess)
        return e;
    const uint64_t loads = (p.nchunks + 31u) / 32u;
    const uint64_t want_blocks = (loads + plan.waves - 1u) / plan.waves;
    const uint64_t cap = (uint64_t)num_cus * plan.blocks_per_cu;
    const uint32_t grid = (uint32_t)(want_blocks < cap ? want_blocks : cap);
    RANS_LAUNCH(KERN, dim3(grid), dim3(64u * plan.waves), (size_t)plan.lds_bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_encode_batch_alias_pairs(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!encode_batch_alias_pairs_applicable(p) || !p.sym_offsets || !p.sym_counts || !p.slot_offsets || !p.lengths || !p.offsets || !p.flags)
        return hipErrorInvalidValue;
    const EncAliasPairsPlan plan = enc_alias_pairs_plan(p.scale_bits);
    static_assert(kEncAliasPairsRecBytes == kEncPairTable && kEncAliasPairsWaveLds == kPairWaveLds && kEncAliasPairsLdsCap == kGrpLdsCap &&
                      kEncAliasPairsMaxWaves * 64u == kGrpThreads && kEncPairTable == 4096u,
                  "pairs_plan.hpp restates these; RANS_AE_ROUND's gather carries kEncPairTable as its offset");
    if (plan.waves == 0 || plan.lds_bytes > kGrpLdsCap || num_cus <= 0)
        return hipErrorInvalidValue;
    if (name)
        *name = KernelId::encode_batch_alias_pairs;
    return p.dense256 ? launch_alias_pairs_kernel<k_encode_batch_alias_pairs<false>>(plan, p, num_cus, stream)
                      : launch_alias_pairs_kernel<k_encode_batch_alias_pairs<true>>(plan, p, num_cus, stream);
}

} // namespace rans_amd
