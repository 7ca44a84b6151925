// decode_groups.hip -- decoders for two of the reference's own narrow layouts with 64 / N chunks per wave and ONE STATE PER
// LANE: k_decode_word_groups, the 8-way word layout (rans_word_sse41.h:151-227: two SSE registers of four states, one shared
// cursor) with lane 8 g + i = state i of chunk g of the wave's octet, and further down k_decode_byte_pairs, the 2-way byte
// layout of main.cpp:226-280 with lane 2 g + i.
//
// The lane-per-chunk kernels (decode_lanes.hip) give every lane a whole chunk: 64 private streams per wave, a 136-byte ring
// row per lane in LDS (8.7 KiB per wave beside the 32 KiB slot table: 13..14 waves per CU), and their pace is set by
// how few waves a CU can hold (profiles/r06_small_abs.md).  Here a chunk is decoded the way the wave-per-chunk
// kernels do it (decode_wave.hip) -- one symbol per lane per round, "who renormalises" is a ballot, a lane's place in
// its stream is a population count over the lanes below it -- only that the ballot is cut into eight bytes, one per
// chunk:
//   * mask_g = ballot & (bits of group g), held per lane in a VGPR; v_mbcnt counts ITS bits below the lane, and with
//     the group's cursor as the instruction's addend the result is the lane's word position outright; v_bcnt with the
//     cursor as addend is the group's next cursor (every lane of the group computes the same);
//   * a group's stream goes through a 256-byte ring in LDS (2 KiB per wave: 32 waves per CU beside the table), fetched
//     in aligned 128-byte blocks, 16 bytes per lane, the next block parked in registers one refill ahead.  Eight rounds
//     consume at most 8 x 8 x 2 = 128 bytes per group, so a group needs at most one block per eight rounds: one
//     compare per lane every eight rounds, the refill itself runs under the exec mask of the groups that need it;
//   * sixteen rounds are one 128-byte line of the chunk: four rounds of symbols are transposed inside the quads (as in
//     decode_wave.hip), the halves of the group exchange dwords (v_cndmask_b32_dpp), and every lane stores 16 bytes -- pieces
//     of a line that leave at different times reach memory as partial lines (profiles/r06_word8_groups.md: 2.05 ms with
//     one dword per lane every four rounds, 0.51 with whole lines).
// Chunks of a multiple of 4 symbols -- the output is stored in dwords -- (the launcher hands everything else to the lane
// kernel); a ragged last chunk sends the input's last octet one round at a time; what a chunk size off 128 leaves goes four rounds, then one round
// at a time.  The mirror image, the 8-way encoder: encode_groups.hip.  The ragged form for rans_amd_decode_batch -- eight
// STREAMS per wave, each with its own symbol count -- is k_decode_batch_word_groups, behind the uniform kernel; the 2-way byte
// layout's, thirty-two streams per wave, is k_decode_batch_byte_pairs behind k_decode_byte_pairs, and the alias format's 2-way
// layout's k_decode_batch_alias_pairs behind that.
//
// No MFMA: integer, table-driven, serial per state.

#include "decode_common.hpp"
#include "groups_common.hpp"

namespace rans_amd {

namespace {

constexpr uint32_t kGrpClaimSyms = 8192;        // symbols one claim of the work counter covers, at least
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes on the 4-byte grid (the ragged kernel's lines)

// Eight rounds of the eight chunks as one hand-scheduled sequence: rans_word_sse41.h:123-141 (the D step and the
// renormalisation of RansWordDecSym / RansWordDecRenorm), 14 VALU + 2 LDS per round:
//   v_and, v_lshlrev            slot = x & 4095 -> LDS byte address of the slot record (the table starts at LDS address 0)
//   ds_read_b64                 {freq | sym << 24, bias}
//   v_lshrrev, v_mad_u32_u24    x = freq * (x >> 12) + bias
//   v_cmp                       vcc = the lanes that renormalise (x < 2^16)
//   v_perm                      the symbol joins its accumulator (rounds 2..7; it also is one of the two wait states a
//                               VALU read of a VALU-written vcc needs on gfx940+, s_nop the other)
//   v_and, v_and_or             t_lo = vcc_lo & my group's bits, t = (vcc_hi & my group's bits) | t_lo -- a group lies in
//                               one half of the wave, so t is the group's byte of the ballot in place
//   v_mbcnt_lo(t_lo, cursor), v_mbcnt_hi(t, .)   cursor + renormalising lanes of MY group below me: for lanes 0..31
//                               v_mbcnt_hi adds nothing, for lanes 32..63 t_lo is zero and v_mbcnt_lo adds nothing
//   v_bcnt(t, cursor)           the group's next cursor (words)
//   v_lshlrev, v_and_or         word position -> LDS byte address inside the group's 256-byte ring
//   ds_read_u16, v_perm         under exec = vcc: x = (x << 16) | word
// Rounds alternate between two accumulators (A: rounds 0, 2, 4, 6; B: 1, 3, 5, 7), see the output transposition below.
// Fixed registers v56..v63: the halves of a 64-bit asm operand cannot be named.
#define RANS_G_LOOKUP(PAIR, LO, HI)                        \
    "v_and_b32_e32 v62, %[m12], %[x]\n\t"                  \
    "v_lshlrev_b32_e32 v62, 3, v62\n\t"                    \
    "ds_read_b64 " PAIR ", v62\n\t"                        \
    "v_lshrrev_b32_e32 v63, 12, %[x]\n\t"                  \
    "s_waitcnt lgkmcnt(0)\n\t"                             \
    "v_mad_u32_u24 %[x], " LO ", v63, " HI "\n\t"
#define RANS_G_RENORM(FILL)                                \
    "v_cmp_gt_u32_e32 vcc, %[lim], %[x]\n\t"               \
    FILL                                                   \
    "v_and_b32_e32 v62, vcc_lo, %[gmlo]\n\t"               \
    "v_and_or_b32 v63, vcc_hi, %[gmhi], v62\n\t"           \
    "v_mbcnt_lo_u32_b32 v62, v62, %[cur]\n\t"              \
    "v_mbcnt_hi_u32_b32 v62, v63, v62\n\t"                 \
    "v_bcnt_u32_b32 %[cur], v63, %[cur]\n\t"               \
    "v_lshlrev_b32_e32 v62, 1, v62\n\t"                    \
    "v_and_or_b32 v62, v62, %[k255], %[ring]\n\t"          \
    "s_mov_b64 exec, vcc\n\t"                              \
    "ds_read_u16 v63, v62\n\t"                             \
    "s_waitcnt lgkmcnt(0)\n\t"                             \
    "v_perm_b32 %[x], %[x], v63, %[selm]\n\t"              \
    "s_mov_b64 exec, -1\n\t"
__device__ __forceinline__ void decode_octet_8rounds(uint32_t &x, uint32_t &curw, uint32_t &acc_a, uint32_t &acc_b, uint32_t m12,
                                                     uint32_t lim, uint32_t gm_lo, uint32_t gm_hi, uint32_t k255, uint32_t ring,
                                                     uint32_t sel_a, uint32_t sel_b, uint32_t sel_c)
{
    asm volatile(
        RANS_G_LOOKUP("v[56:57]", "v56", "v57") RANS_G_RENORM("s_nop 1\n\t")
        RANS_G_LOOKUP("v[58:59]", "v58", "v59") RANS_G_RENORM("s_nop 1\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pa], v60, v56, %[selA]\n\ts_nop 0\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pb], v60, v58, %[selA]\n\ts_nop 0\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pa], v60, %[pa], %[selB]\n\ts_nop 0\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pb], v60, %[pb], %[selB]\n\ts_nop 0\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pa], v60, %[pa], %[selC]\n\ts_nop 0\n\t")
        RANS_G_LOOKUP("v[60:61]", "v60", "v61") RANS_G_RENORM("v_perm_b32 %[pb], v60, %[pb], %[selC]\n\ts_nop 0\n\t")
        : [x] "+v"(x), [cur] "+v"(curw), [pa] "=&v"(acc_a), [pb] "=&v"(acc_b)
        : [m12] "v"(m12), [lim] "v"(lim), [gmlo] "v"(gm_lo), [gmhi] "v"(gm_hi), [k255] "v"(k255), [ring] "v"(ring),
          [selA] "v"(sel_a), [selB] "v"(sel_b), [selC] "v"(sel_c), [selm] "s"(0x05040100u)
        : "vcc", "memory", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63");
}
#undef RANS_G_LOOKUP
#undef RANS_G_RENORM

__global__ void __launch_bounds__(kGrpThreads, 8) k_decode_word_groups(const DecParams p)
{
    using Tr = FmtTraits<FMT_WORD>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // WordSlot[4096]: 32 KiB, a multiple of the ring size
    stage_table(smem, p.table0, t0_bytes);
    __syncthreads();
    DecTables<FMT_WORD> T;
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t g = lane >> 3, i = lane & 7u;
    const WordGroupLane L(t0_bytes, wave, g);
    const uint32_t ring = L.ring, bias = L.bias, gm_lo = L.gm_lo, gm_hi = L.gm_hi, k255 = L.k255, k65536 = L.k65536;
    const uint32_t sel_a = L.sel_a, sel_b = L.sel_b, sel_c = L.sel_c;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glo = cbase & ~uint64_t(15), glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t sel1 = (lane & 1u) ? 0x03070105u : 0x06020400u;
    const uint32_t sel2 = (lane & 2u) ? 0x03020706u : 0x05040100u;
    const uint32_t groups16 = uniform(p.chunk_syms >> 7);      // 16 rounds of 8 symbols
    const uint32_t rem4 = uniform((p.chunk_syms >> 5) & 3u);   // + up to three times 4 rounds
    const uint32_t left_syms = uniform(p.chunk_syms & 31u);    // + up to 31 symbols
    const uint64_t octets = (p.nchunks + 7u) >> 3; // (the last one may hold fewer than eight chunks)
    const uint32_t per_claim = uniform(p.chunk_syms >= kGrpClaimSyms / 8u ? 1u : (kGrpClaimSyms / 8u + p.chunk_syms - 1u) / p.chunk_syms);
    const uint64_t claims = (octets + per_claim - 1u) / per_claim;

    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    // A ragged last chunk (p.n % p.chunk_syms != 0) is decoded here as well: its octet, the input's last, goes one round at a
    // time with the lanes that have no symbol sitting out -- three times an octet's usual time, so the octets are handed out
    // back to front then and that one starts first.
    const bool ragged = p.n % p.chunk_syms != 0;
    auto octet_of = [&](uint64_t k) -> uint64_t { return ragged ? octets - 1u - k : k; }; // k: the order of the hand-out
    uint64_t vk, o_end;
    bool have;
    {
        const uint64_t c = work.take(lane);
        have = c < claims;
        vk = c * per_claim;
        o_end = (c + 1u) * per_claim < octets ? (c + 1u) * per_claim : octets;
    }
    uint64_t off = 0;
    uint32_t len = 0;
    if (have && octet_of(vk) * 8u + g < p.nchunks) {
        off = p.offsets[octet_of(vk) * 8u + g];
        len = p.lengths[octet_of(vk) * 8u + g];
    }
    while (have) {
        {
            const uint64_t octet = octet_of(vk);
            const bool exists = octet * 8u + g < p.nchunks;
            const bool valid = exists && (off & 1u) == 0 && len >= 8u * 4u && off <= p.container_bytes && len <= p.container_bytes - off;
            if (exists && !valid && i == 0)
                nbad++;
            const uint64_t src = cbase + (valid ? off : 0u);
            uint32_t x = Tr::kL;
            if (valid) // RansDecInit order: state 0 first (rans_word_sse41.h:104-113)
                x = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[i];
            WordRing R;
            const uint32_t start = R.open(src, i, ring, bias, true, glo, glimit);
            uint32_t &curw = R.curw;
            auto checkpoint = [&]() { R.checkpoint(); };

            // symbol stores through a descriptor of the octet's output: the running offset is an SGPR
            const rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<void *>(reinterpret_cast<uint64_t>(p.out) + octet * 8u * p.chunk_syms), 0, 8u * p.chunk_syms, kRsrcFlags);
            const uint32_t out_off16 = valid ? g * p.chunk_syms + 16u * i : 0x80000000u; // (an invalid chunk's stores: dropped by the range check)
            uint32_t osoff = 0;
            const bool by_rounds = ragged && octet + 1u == octets; // (wave-uniform)
            for (uint32_t q = 0; q < (by_rounds ? 0u : groups16); ++q) {
                uint32_t a0, a1, a2, a3;
                // (the refill check BEHIND each eight rounds, not in front: the store of the line before then is eight rounds old when a
                //  refill's s_waitcnt vmcnt(0) comes -- in front of the rounds it had just been issued; 0.519 -> 0.503 ms)
                decode_octet_8rounds(x, curw, a0, a1, T.mask12v, k65536, gm_lo, gm_hi, k255, ring, sel_a, sel_b, sel_c);
                checkpoint();
                decode_octet_8rounds(x, curw, a2, a3, T.mask12v, k65536, gm_lo, gm_hi, k255, ring, sel_a, sel_b, sel_c);
                checkpoint();
                a0 = quad_transpose(a0, sel1, sel2);
                a1 = quad_transpose(a1, sel1, sel2);
                a2 = quad_transpose(a2, sel1, sel2);
                a3 = quad_transpose(a3, sel1, sel2);
                const u32x4 v = halves_to_line(a0, a1, a2, a3);
                // (chunk sizes off 64: a chunk's lines straddle the memory's at odd places, and the pieces of a memory line arrive
                //  sixteen rounds apart -- plain stores let L2 put them together: 1000-symbol chunks 1.10 -> 0.77 ms, 4000: 0.90 ->
                //  0.65; on the 64-byte grid `nt sc1` wins: 960-symbol chunks 0.52 against 0.59)
                if (p.chunk_syms & 63u)
                    __builtin_amdgcn_raw_buffer_store_b128(v, orsrc, out_off16, osoff, 0);
                else
                    __builtin_amdgcn_raw_buffer_store_b128(v, orsrc, out_off16, osoff, kAuxStore);
                osoff += 128u;
            }
            for (uint32_t q = 0; q < (by_rounds ? 0u : rem4); ++q) { // what is left of a chunk that is not a multiple of 128 symbols: 4 rounds a time
                uint32_t acc = 0;
                acc = acc_symbol<Tr::kSymByte, 0>(decode_word_round(T, x, curw, true, gm_lo, gm_hi, k255, k65536, ring), acc);
                acc = acc_symbol<Tr::kSymByte, 1>(decode_word_round(T, x, curw, true, gm_lo, gm_hi, k255, k65536, ring), acc);
                acc = acc_symbol<Tr::kSymByte, 2>(decode_word_round(T, x, curw, true, gm_lo, gm_hi, k255, k65536, ring), acc);
                acc = acc_symbol<Tr::kSymByte, 3>(decode_word_round(T, x, curw, true, gm_lo, gm_hi, k255, k65536, ring), acc);
                if (q & 1u)
                    checkpoint();
                const uint32_t v = quad_transpose(acc, sel1, sel2);
                const uint32_t li = lane_id() & 7u; // lane (m, h) of the group holds row m, states 4 h .. 4 h + 3
                __builtin_amdgcn_raw_buffer_store_b32(v, orsrc, out_off16 - 16u * li + (li & 3u) * 8u + (li >> 2) * 4u, osoff, 0);
                osoff += 32u;
            }
            // what a chunk size off 32 leaves (at most 31 symbols: three rounds and a partial one, main_simd.cpp:313-332 with
            // in_size % 8 != 0) -- or, in the ragged chunk's octet, every round: lanes without a symbol sit the round out, a byte
            // store per lane
            uint32_t nsym = valid ? p.chunk_syms : 0u, r_first = p.chunk_syms - left_syms;
            if (by_rounds) {
                r_first = 0u;
                if (valid && octet * 8u + g + 1u == p.nchunks)
                    nsym = (uint32_t)(p.n - (octet * 8u + g) * p.chunk_syms);
            }
            for (uint32_t r0 = r_first; r0 < p.chunk_syms; r0 += 8u) {
                if (by_rounds && (r0 & 63u) == 0)
                    checkpoint();
                const bool active = r0 + i < nsym;
                const uint32_t raw = decode_word_round(T, x, curw, active, gm_lo, gm_hi, k255, k65536, ring);
                if (active)
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(raw >> 24), orsrc, out_off16 - 16u * i + r0 + i, 0, 0);
            }
            // integrity: every state back at L, the cursor exactly at the end of the chunk's stream
            const bool bad = valid && (x != Tr::kL || 2u * curw - bias - (start - 8u * 4u) != len);
            const uint64_t bm = __builtin_amdgcn_ballot_w64(bad);
            if (i == 0 && ((bm >> (8u * g)) & 0xffu) != 0)
                nbad++;
            // the octet after this one
            uint64_t n_vk = vk + 1u, n_end = o_end;
            bool n_have = true;
            if (n_vk >= o_end) {
                const uint64_t c = work.take(lane);
                n_have = c < claims;
                n_vk = c * per_claim;
                n_end = (c + 1u) * per_claim < octets ? (c + 1u) * per_claim : octets;
            }
            uint64_t n_off = 0;
            uint32_t n_len = 0;
            if (n_have && octet_of(n_vk) * 8u + g < p.nchunks) {
                n_off = p.offsets[octet_of(n_vk) * 8u + g];
                n_len = p.lengths[octet_of(n_vk) * 8u + g];
            }
            vk = n_vk;
            o_end = n_end;
            have = n_have;
            off = n_off;
            len = n_len;
        }
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
}

// ---------------------------------------------------------------------------
// k_decode_batch_word_groups -- the ragged form of k_decode_word_groups (rans_amd_decode_batch under
// RANS_AMD_OPT_BATCH_GROUPS): a wave's eight groups hold eight STREAMS, each with its own symbol count and its own output
// address.  The unit of work is one octet of the hand-out order: lane 8 g + i holds state i of the stream at position
// 8 o + g -- stream order[8 o + g], or 8 o + g without an order; a position at or past nchunks has no stream.  The rounds,
// the ring and its refills, the transposes and the half-group exchange are k_decode_word_groups'; what is new is that the
// groups' loop counts differ:
//   * the wave runs the 16-round sequence max_g(blocks_g) times with FULL exec, blocks_g = count_g >> 7 whole 128-byte
//     lines.  The sequence sets exec = -1 itself, and the DPP moves of the exchange read zeros from lanes an exec mask has
//     switched off, so a group that has run out of lines cannot be masked off: it is PARKED.  Its bits of the ballot are
//     zeroed (gm_lo = gm_hi = 0): its cursor then stands still, checkpoint() never fires for it, and its ring, pend, ld,
//     left, wr and thr stay as they are; its state is put back from a copy behind every block (one select); its line is
//     not stored.
//     A parked group keeps running the rounds on whatever its state becomes, and that is safe: a round reads the slot
//     table at 8 (x & 4095), inside the 32 KiB table whatever x is, and the ring at (position & 255) | ring, inside the
//     group's own 256 bytes whatever the position is; it reads no global memory (refills are checkpoint()'s) and writes
//     nothing but its own registers.  The same holds for a group without a stream or with a rejected one, which is parked
//     from the start and whose ring is never filled from memory.
//   * behind the common loop every group decodes its count_g & 127 remaining symbols one round at a time, lanes without a
//     symbol sitting out, a byte store per lane (the uniform kernel's path for a ragged last chunk).
// Every lane addresses its output in 64 bits (out_syms is 64-bit, and the eight streams of a wave may lie anywhere in it).
// A stream whose output is not 4-byte aligned takes the round-by-round path for all of its symbols (blocks_g = 0): the
// rule of the wave kernels -- sym_align = 4 is the fast layout, anything else is correct and slower.
// Index entries are the caller's data and checked as k_decode's RAGGED form and the kernel above check theirs: the order
// entry names a stream, the offset is even, the stream holds its eight states and lies inside the container, the symbol
// range lies inside [0, out_syms).  A stream that fails is counted once; nothing of it is fetched, nothing stored.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGrpThreads, 8) k_decode_batch_word_groups(const DecParams p)
{
    using Tr = FmtTraits<FMT_WORD>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long t_start = p.span ? wall_clock64() : 0ull;
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // WordSlot[4096]: 32 KiB, a multiple of the ring size
    stage_table(smem, p.table0, t0_bytes);
    __syncthreads();
    DecTables<FMT_WORD> T;
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t g = lane >> 3, i = lane & 7u;
    const WordGroupLane L(t0_bytes, wave, g);
    const uint32_t ring = L.ring, bias = L.bias, gm_lo = L.gm_lo, gm_hi = L.gm_hi, k255 = L.k255, k65536 = L.k65536;
    const uint32_t sel_a = L.sel_a, sel_b = L.sel_b, sel_c = L.sel_c;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glo = cbase & ~uint64_t(15), glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t sel1 = (lane & 1u) ? 0x03070105u : 0x06020400u;
    const uint32_t sel2 = (lane & 2u) ? 0x03020706u : 0x05040100u;
    const uint64_t octets = (p.nchunks + 7u) >> 3; // one per claim (the last one may hold fewer than eight streams)

    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    for (;;) {
        const uint64_t octet = work.take(lane);
        if (octet >= octets)
            break;
        // ---- this group's stream: its index entries, all of them the caller's data
        bool exists, valid;
        uint64_t off, first;
        uint32_t len, count;
        fetch_stream_entry<8u * 4u, true>(p, octet * 8u + g, exists, valid, off, first, len, count);
        if (exists && !valid && i == 0)
            nbad++;
        const uint64_t src = cbase + (valid ? off : 0u);
        uint32_t x = Tr::kL;
        if (valid) // RansDecInit order: state 0 first (rans_word_sse41.h:104-113)
            x = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[i];
        WordRing R; // (a group without a valid stream fetches nothing)
        const uint32_t start = R.open(src, i, ring, bias, valid, glo, glimit);
        uint32_t &curw = R.curw;
        auto checkpoint = [&]() { R.checkpoint(); };
        const uint32_t end2 = len + bias + (start - 8u * 4u); // twice the (biased) cursor at the end of the stream

        // ---- the group's own counts: whole lines through the common loop, the rest a round at a time
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + first; // (valid: [dst, dst + count) lies inside the output)
        const uint32_t blocks = (valid && (dst & 3u) == 0) ? count >> 7 : 0u;
        const uint32_t tail = valid ? count - (blocks << 7) : 0u;
        const uint32_t max_blocks = wave_max8(blocks), max_tail = wave_max8(tail);
        uint64_t line = dst + 16u * i; // this lane's 16 bytes of the group's next line
        uint32_t m_lo = gm_lo, m_hi = gm_hi;
        for (uint32_t q = 0; q < max_blocks; ++q) {
            const bool run = q < blocks;
            if (!run) // parked: no bit of the ballot is this group's
                m_lo = m_hi = 0u;
            const uint32_t x_keep = x;
            uint32_t a0, a1, a2, a3;
            decode_octet_8rounds(x, curw, a0, a1, T.mask12v, k65536, m_lo, m_hi, k255, ring, sel_a, sel_b, sel_c);
            checkpoint();
            decode_octet_8rounds(x, curw, a2, a3, T.mask12v, k65536, m_lo, m_hi, k255, ring, sel_a, sel_b, sel_c);
            checkpoint();
            a0 = quad_transpose(a0, sel1, sel2);
            a1 = quad_transpose(a1, sel1, sel2);
            a2 = quad_transpose(a2, sel1, sel2);
            a3 = quad_transpose(a3, sel1, sel2);
            const u32x4 v = halves_to_line(a0, a1, a2, a3); // (under full exec: see there)
            // (plain stores: a stream starts anywhere on the 4-byte grid, so its lines straddle the memory's -- the case in which
            //  k_decode_word_groups leaves it to L2 to put the pieces together)
            if (run) {
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line) = v;
                line += kGrpBlock;
            }
            x = run ? x : x_keep;
        }
        // ---- count & 127 symbols (all of them where the output is not 4-byte aligned): one round at a time
        const uint64_t tail_dst = line - 16u * i; // (`line` has moved on by the group's own blocks, no further)
        const uint32_t tail_rounds = (uint32_t)(((uint64_t)max_tail + 7u) >> 3);
        for (uint32_t rr = 0; rr < tail_rounds; ++rr) {
            if ((rr & 7u) == 0)
                checkpoint();
            const uint32_t r0 = rr << 3; // < max_tail
            const bool active = r0 < tail && i < tail - r0;
            const uint32_t raw = decode_word_round(T, x, curw, active, gm_lo, gm_hi, k255, k65536, ring);
            if (active)
                *reinterpret_cast<uint8_t RANS_GLOBAL *>(tail_dst + r0 + i) = (uint8_t)(raw >> 24);
        }
        // integrity: every state back at L, the cursor exactly at the end of the stream
        const bool bad = valid && (x != Tr::kL || 2u * curw != end2);
        const uint64_t bm = __builtin_amdgcn_ballot_w64(bad);
        if (i == 0 && ((bm >> (8u * g)) & 0xffu) != 0)
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
    record_span(p, t_start, smem);
}

// ---------------------------------------------------------------------------
// Byte format, 2-way (main.cpp:226-280: two states, one pointer): THIRTY-TWO chunks per wave, lane 2 g + i holds state i of
// chunk g of the wave's batch.  The same plan as above with the group cut down to a pair:
//   * a state takes 0, 1 or 2 bytes (rans_byte.h:307-318, scale_bits <= 16); state 1's bytes follow state 0's, so the odd
//     lane's position is the cursor + what the even lane takes (its count through a DPP swap of the pair, masked to the even
//     lanes' counts beforehand), and the next cursor is the odd lane's position + count, broadcast to the pair (DPP);
//   * a pair's stream goes through a 64-byte ring in LDS (rows 68 bytes apart: byte 64 mirrors byte 0, so that the second
//     byte of a lane can be read at offset 1 without wrapping), fetched in aligned 32-byte blocks, 16 bytes per lane, the
//     next block parked in registers.  Eight rounds consume at most 8 x 2 x 2 = 32 bytes per pair: the refill check again is
//     one compare per lane every eight rounds;
//   * tables as in the lane kernels: cum2sym (LDS address 0) and {freq, start} records -- two dependent gathers per symbol;
//   * four rounds of a state's symbols are one dword; the pair interleaves them (DPP swap + v_perm), sixteen rounds are 32
//     bytes of the chunk, 16 per lane, and after thirty-two rounds two 16-byte stores per lane leave back to back: 64
//     contiguous bytes per chunk.
// Full chunks of a multiple of 4 symbols (what a size off 64 leaves goes one round at a time).
// ---------------------------------------------------------------------------
constexpr int kPairAux = kAuxStore; // nt sc1, as the other decoders' symbol stores (plain stores: 0.94 ms against 0.73)

// Eight rounds (one symbol per lane and round) as one hand-scheduled sequence; rans_byte.h:125-128 (get), :291-298 (advance),
// :307-318 (renormalise).  17 VALU + 4 LDS per round:
//   v_and                       cf = x & mask
//   ds_read_u8                  s = cum2sym[cf]
//   v_lshrrev                   q = x >> scale_bits
//   v_lshl_or                   the symbol joins its accumulator (rounds 1..3 of four; round 0's lands there directly)
//   v_lshl_add, ds_read_b64     {freq, start} of s
//   v_mad_u32_u24, v_sub        x = freq * q + cf - start
//   v_cmp x2                    n1 = x < 2^23 (at least one byte), n2 = x < 2^15 (two)
//   v_addc x2                   t = cursor + n1 + n2: where this lane's bytes END if it is the pair's first
//   v_cndmask_dpp               my position = even lane: the cursor; odd lane: the even lane's t (vcc = the even lanes)
//   v_add_dpp, v_sub            the pair's next cursor = t + the other lane's t - cursor
//   v_and, v_add                position -> LDS address in the pair's ring
//   ds_read_u8 x2, v_lshl_or x2 under exec = n1 / n2: x = (x << 8) | byte
#define RANS_P_RECORD(SREG)                                                                        \
    "v_lshl_add_u32 %[t1], " SREG ", 3, %[rec]\n\t"                                                \
    "ds_read_b64 v[60:61], %[t1]\n\t"                                                              \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    "v_mad_u32_u24 %[x], v60, %[t2], %[t0]\n\t"                                                    \
    "v_sub_u32_e32 %[x], %[x], v61\n\t"
#define RANS_P_ROUND(SREG, FILL)                                                                   \
    "v_and_b32_e32 %[t0], %[maskv], %[x]\n\t"                                                      \
    "ds_read_u8 " SREG ", %[t0]\n\t"                                                               \
    "v_lshrrev_b32_e32 %[t2], %[sbv], %[x]\n\t"                                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    RANS_P_RECORD(SREG)                                                                            \
    RANS_P_RENORM(FILL)
// (the renormalisation on its own: the alias pairs' round below ends with the same text)
#define RANS_P_RENORM(FILL)                                                                        \
    "v_cmp_gt_u32_e64 %[n1], %[l23], %[x]\n\t"                                                     \
    "v_cmp_gt_u32_e64 %[n2], %[l15], %[x]\n\t"                                                     \
    FILL                                                                                           \
    "v_addc_co_u32_e64 %[t1], %[dm], %[cur], 0, %[n1]\n\t"                                         \
    "v_addc_co_u32_e64 %[t1], %[dm], %[t1], 0, %[n2]\n\t"                                          \
    "s_nop 1\n\t"                                                                                  \
    "v_cndmask_b32_dpp %[t2], %[t1], %[cur], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_u32_dpp %[t0], %[t1], %[t1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"         \
    "v_sub_u32_e32 %[cur], %[t0], %[cur]\n\t"                                                      \
    "v_and_b32_e32 %[t2], 63, %[t2]\n\t"                                                           \
    "v_add_u32_e32 %[t2], %[ring], %[t2]\n\t"                                                      \
    "s_mov_b64 exec, %[n1]\n\t"                                                                    \
    "ds_read_u8 %[t1], %[t2]\n\t"                                                                  \
    "s_mov_b64 exec, %[n2]\n\t"                                                                    \
    "ds_read_u8 %[t0], %[t2] offset:1\n\t"                                                         \
    "s_mov_b64 exec, %[n1]\n\t"                                                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    "v_lshl_or_b32 %[x], %[x], 8, %[t1]\n\t"                                                       \
    "s_mov_b64 exec, %[n2]\n\t"                                                                    \
    "v_lshl_or_b32 %[x], %[x], 8, %[t0]\n\t"                                                       \
    "s_mov_b64 exec, -1\n\t"
#define RANS_P_FOUR(ACC)                                                                           \
    RANS_P_ROUND(ACC, "s_nop 0\n\t")                                                               \
    RANS_P_ROUND("%[t3]", "v_lshl_or_b32 " ACC ", %[t3], 8, " ACC "\n\t")                          \
    RANS_P_ROUND("%[t3]", "v_lshl_or_b32 " ACC ", %[t3], 16, " ACC "\n\t")                         \
    RANS_P_ROUND("%[t3]", "v_lshl_or_b32 " ACC ", %[t3], 24, " ACC "\n\t")
__device__ __forceinline__ void decode_pairs_8rounds(uint32_t &x, uint32_t &cur, uint32_t &acc_a, uint32_t &acc_b, uint32_t maskv,
                                                     uint32_t sbv, uint32_t rec, uint32_t l23, uint32_t l15, uint32_t ring)
{
    uint32_t t0, t1, t2, t3;
    uint64_t n1, n2, dm;
    asm volatile("s_mov_b64 vcc, %[evens]\n\t" // the even lanes (the pair's state 0), for the whole sequence
                 RANS_P_FOUR("%[pa]") RANS_P_FOUR("%[pb]")
                 : [x] "+v"(x), [cur] "+v"(cur), [pa] "=&v"(acc_a), [pb] "=&v"(acc_b), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
                   [t3] "=&v"(t3), [n1] "=&s"(n1), [n2] "=&s"(n2), [dm] "=&s"(dm)
                 : [maskv] "v"(maskv), [sbv] "v"(sbv), [rec] "v"(rec), [l23] "v"(l23), [l15] "v"(l15), [ring] "v"(ring),
                   [evens] "s"(0x5555555555555555ull)
                 : "vcc", "memory", "v60", "v61");
}
#undef RANS_P_FOUR
#undef RANS_P_RECORD
#undef RANS_P_ROUND

// The same eight rounds for the ALIAS format's 2-way layout (main_alias.cpp:252-267 for the symbol, then rans_byte.h:307-318:
// the stream IS the byte format's, so RANS_P_RENORM follows unchanged).  The tables are the FMT_ALIAS ones of
// fill_decoder_tables: {freq | sym << 16, adjust} per half bucket at LDS address 0, divider u32[nsyms] at `div`.  A bucket's two
// halves lie side by side -- 2 b the donor's, 2 b + 1 the bucket's own symbol's --, so ONE 16-byte read at 16 b brings both
// records, and it does not wait for the divider: the two gathers of a round leave together where the byte format's second
// gather waits for the first, and the divider only SELECTS.  The symbol step is 13 VALU + 2 LDS where the byte format's is
// 6 + 2 -- 24 VALU + 4 LDS per round -- but one LDS round trip shorter in sequence, and a launch of ragged streams lasts as
// long as the rounds of its longest stream one after the other:
//   v_and                       xm = x & mask
//   v_lshrrev                   bucket = xm >> (scale_bits - log2 nsyms)                     (< nsyms for ANY x)
//   v_lshl_add, ds_read_b32     divider[bucket]
//   v_lshlrev, ds_read_b128     both half records of the bucket, at 16 bucket                (< 16 nsyms for ANY x)
//   v_lshrrev                   q = x >> scale_bits
//   v_sub, v_ashrrev            xm - divider (both < 2^17) as a mask: all ones where the slot is the bucket's own symbol's
//   v_bfi x2                    {freq | sym << 16, adjust} of the half the mask selects
//   v_mul_u32_u24 (sdwa)        freq * q, freq the record's low word (freq < 2^16, q < 2^23 for a state in the working range)
//   v_sub, v_add                x = freq * q + (xm - adjust)
//   v_perm                      the symbol, byte 2 of the record, goes straight into its byte of the accumulator (in the
//                               renormalisation's fill slot; bytes not written yet are zeroed by the selector)
//   + the 11 VALU and 2 LDS of RANS_P_RENORM.
// Both gathers stay inside the tables whatever x is -- the bucket comes out of log2 nsyms bits of x and nothing else goes into
// either address -- and the symbol comes out of the record: no further lookup depends on what a table holds.  That is what lets
// a parked or rejected pair free-run (k_decode_batch_alias_pairs).  DPP and exec as above: the s_nop in front of the DPP reads of
// freshly written VGPRs is RANS_P_RENORM's, and exec is -1 again at the end of every round.
#define RANS_A_ROUND(ACC, SEL)                                                                     \
    "v_and_b32_e32 %[t0], %[maskv], %[x]\n\t"                                                      \
    "v_lshrrev_b32_e32 %[t1], %[bsh], %[t0]\n\t"                                                   \
    "v_lshl_add_u32 %[t3], %[t1], 2, %[div]\n\t"                                                   \
    "ds_read_b32 %[t3], %[t3]\n\t"                                                                 \
    "v_lshlrev_b32_e32 %[t1], 4, %[t1]\n\t"                                                        \
    "ds_read_b128 v[56:59], %[t1]\n\t"                                                             \
    "v_lshrrev_b32_e32 %[t2], %[sbv], %[x]\n\t"                                                    \
    "s_waitcnt lgkmcnt(1)\n\t"                                                                     \
    "v_sub_u32_e32 %[t3], %[t0], %[t3]\n\t"                                                        \
    "v_ashrrev_i32_e32 %[t3], 31, %[t3]\n\t"                                                       \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    "v_bfi_b32 v56, %[t3], v58, v56\n\t"                                                           \
    "v_bfi_b32 v57, %[t3], v59, v57\n\t"                                                           \
    "v_mul_u32_u24_sdwa %[x], v56, %[t2] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t" \
    "v_sub_u32_e32 %[t0], %[t0], v57\n\t"                                                          \
    "v_add_u32_e32 %[x], %[x], %[t0]\n\t"                                                          \
    RANS_P_RENORM("v_perm_b32 " ACC ", v56, " ACC ", " SEL "\n\t")
#define RANS_A_FOUR(ACC) RANS_A_ROUND(ACC, "%[s0]") RANS_A_ROUND(ACC, "%[s1]") RANS_A_ROUND(ACC, "%[s2]") RANS_A_ROUND(ACC, "%[s3]")
// div: the dividers' LDS address (PairLane::rec); bsh = scale_bits - log2 nsyms (wave-uniform)
__device__ __forceinline__ void decode_alias_pairs_8rounds(uint32_t &x, uint32_t &cur, uint32_t &acc_a, uint32_t &acc_b, uint32_t maskv,
                                                           uint32_t sbv, uint32_t div, uint32_t bsh, uint32_t l23, uint32_t l15, uint32_t ring)
{
    uint32_t t0, t1, t2, t3;
    uint64_t n1, n2, dm;
    asm volatile("s_mov_b64 vcc, %[evens]\n\t" // the even lanes (the pair's state 0), for the whole sequence
                 RANS_A_FOUR("%[pa]") RANS_A_FOUR("%[pb]")
                 : [x] "+v"(x), [cur] "+v"(cur), [pa] "=&v"(acc_a), [pb] "=&v"(acc_b), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
                   [t3] "=&v"(t3), [n1] "=&s"(n1), [n2] "=&s"(n2), [dm] "=&s"(dm)
                 : [maskv] "v"(maskv), [sbv] "v"(sbv), [div] "v"(div), [bsh] "s"(bsh), [l23] "v"(l23), [l15] "v"(l15), [ring] "v"(ring),
                   [evens] "s"(0x5555555555555555ull),
                   // v_perm(record, accumulator): byte 2 of the record -> byte k, the bytes below kept, those above zero
                   [s0] "s"(0x0c0c0c06u), [s1] "s"(0x0c0c0600u), [s2] "s"(0x0c060100u), [s3] "s"(0x06020100u)
                 : "vcc", "memory", "v56", "v57", "v58", "v59");
}
#undef RANS_A_FOUR
#undef RANS_A_ROUND
#undef RANS_P_RENORM

// sixteen rounds of a pair -> 32 bytes of its chunk, 16 per lane: d0..d3 are the four 4-round accumulators of this lane's
// state.  Pair-interleave (the even lane keeps the first dword of every eight bytes, the odd lane the second), then the even
// lane collects bytes [0, 16) and the odd lane [16, 32).
__device__ __forceinline__ u32x4 pair_lines(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t sel_p)
{
    u32x4 v;
    uint32_t e0, e1, e2, e3;
    asm volatile("s_nop 1\n\t"
                 "v_mov_b32_dpp %[e0], %[d0] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[e1], %[d1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[e2], %[d2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %[e3], %[d3] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_perm_b32 %[e0], %[e0], %[d0], %[sel]\n\t" // even: [mine0, theirs0, mine1, theirs1]; odd: [theirs2, mine2, theirs3, mine3]
                 "v_perm_b32 %[e1], %[e1], %[d1], %[sel]\n\t"
                 "v_perm_b32 %[e2], %[e2], %[d2], %[sel]\n\t"
                 "v_perm_b32 %[e3], %[e3], %[d3], %[sel]\n\t"
                 "s_mov_b64 vcc, %[evens]\n\t"
                 "v_cndmask_b32_dpp %[vx], %[e2], %[e0], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" // even ? mine : the even lane's
                 "v_cndmask_b32_dpp %[vz], %[e3], %[e1], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_mov_b64 vcc, %[odds]\n\t"
                 "v_cndmask_b32_dpp %[vy], %[e0], %[e2], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" // odd ? mine : the odd lane's
                 "v_cndmask_b32_dpp %[vw], %[e1], %[e3], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
                 : [vx] "=&v"(v.x), [vy] "=&v"(v.y), [vz] "=&v"(v.z), [vw] "=&v"(v.w), [e0] "=&v"(e0), [e1] "=&v"(e1), [e2] "=&v"(e2),
                   [e3] "=&v"(e3)
                 : [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [d3] "v"(d3), [sel] "v"(sel_p), [evens] "s"(0x5555555555555555ull),
                   [odds] "s"(0xaaaaaaaaaaaaaaaaull)
                 : "vcc");
    return v;
}

// Four lanes (two pairs, chunks A and B) hold, per chunk, the eight 16-byte pieces of a 128-byte line: piece 2 r + i in
// register set r of the pair's lane i.  quad_half<HI, R> gathers what lane t of the quad stores with ONE instruction so that the
// quad writes 64 contiguous bytes: piece t of half R (pieces 4 R .. 4 R + 3) of chunk HI -- lane (2 HI + (t & 1))'s register set
// 2 R + (t >> 1).  Two DPP operations per dword.
template <int HI>
__device__ __forceinline__ u32x4 quad_half(const u32x4 &lo, const u32x4 &hi)
{
    u32x4 o;
    uint32_t t0, t1, t2, t3;
    if constexpr (HI) {
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %[t0], %[h0] quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t1], %[h1] quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t2], %[h2] quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t3], %[h3] quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "s_mov_b64 vcc, %[upper]\n\t" // lanes 2, 3 of every quad: the register set 2 R + 1
                     "v_cndmask_b32_dpp %[o0], %[l0], %[t0], vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o1], %[l1], %[t1], vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o2], %[l2], %[t2], vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o3], %[l3], %[t3], vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf"
                     : [o0] "=&v"(o.x), [o1] "=&v"(o.y), [o2] "=&v"(o.z), [o3] "=&v"(o.w), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
                       [t3] "=&v"(t3)
                     : [l0] "v"(lo.x), [l1] "v"(lo.y), [l2] "v"(lo.z), [l3] "v"(lo.w), [h0] "v"(hi.x), [h1] "v"(hi.y), [h2] "v"(hi.z),
                       [h3] "v"(hi.w), [upper] "s"(0xccccccccccccccccull)
                     : "vcc");
    } else {
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %[t0], %[h0] quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t1], %[h1] quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t2], %[h2] quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[t3], %[h3] quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "s_mov_b64 vcc, %[upper]\n\t"
                     "v_cndmask_b32_dpp %[o0], %[l0], %[t0], vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o1], %[l1], %[t1], vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o2], %[l2], %[t2], vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %[o3], %[l3], %[t3], vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf"
                     : [o0] "=&v"(o.x), [o1] "=&v"(o.y), [o2] "=&v"(o.z), [o3] "=&v"(o.w), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
                       [t3] "=&v"(t3)
                     : [l0] "v"(lo.x), [l1] "v"(lo.y), [l2] "v"(lo.z), [l3] "v"(lo.w), [h0] "v"(hi.x), [h1] "v"(hi.y), [h2] "v"(hi.z),
                       [h3] "v"(hi.w), [upper] "s"(0xccccccccccccccccull)
                     : "vcc");
    }
    return o;
}

// sixteen rounds of a pair -> this lane's 16 of the pair's 32 bytes; the ring's row as PairRing takes it
// (the refill check in front of the rounds here: behind them k_decode_byte_pairs is 1.5 % slower, k_decode_word_groups 3 % faster)
template <class ROW> __device__ __forceinline__ u32x4 pair_sixteen(PairRing &R, uint32_t &x, const PairLane &L, const ROW &row, bool live)
{
    uint32_t a0, a1, a2, a3;
    R.checkpoint(row, live);
    decode_pairs_8rounds(x, R.cur, a0, a1, L.maskv, L.sbv, L.rec, L.l23, L.l15, L.ring);
    R.checkpoint(row, live);
    decode_pairs_8rounds(x, R.cur, a2, a3, L.maskv, L.sbv, L.rec, L.l23, L.l15, L.ring);
    return pair_lines(a0, a1, a2, a3, L.sel_p);
}

__global__ void __launch_bounds__(kGrpThreads, 8) k_decode_byte_pairs(const DecParams p)
{
    using Tr = FmtTraits<FMT_BYTE>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // cum2sym u8[M]
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u; // {freq, start}[nsyms]
    stage_table(smem, p.table0, t0_bytes);
    stage_table(smem + t0_bytes, p.table1, t1_bytes);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t g = lane >> 1, i = lane & 1u;
    const uint32_t ring_c = t0_bytes + t1_bytes + wave * kPairWaveLds + g * kPairRow; // raw LDS byte address of the pair's ring
    const PairLane L(ring_c, p.scale_bits, t0_bytes, i);
    const uint32_t ring = L.ring, maskv = L.maskv, sbv = L.sbv, rec = L.rec, l23 = L.l23, l15 = L.l15, sel_p = L.sel_p;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glo = cbase & ~uint64_t(15), glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t groups64 = uniform(p.chunk_syms >> 7);    // 64 rounds of 2 symbols
    const uint32_t rem32 = uniform((p.chunk_syms >> 6) & 1u); // + 32 rounds
    const uint32_t left_syms = uniform(p.chunk_syms & 63u);   // + up to 31 rounds, one at a time
    const uint64_t batches = (p.nchunks + 31u) >> 5;      // (the last one may hold fewer than 32 chunks)
    const uint32_t per_claim = uniform(p.chunk_syms >= kGrpClaimSyms / 32u ? 1u : (kGrpClaimSyms / 32u + p.chunk_syms - 1u) / p.chunk_syms);
    const uint64_t claims = (batches + per_claim - 1u) / per_claim;

    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    const bool ragged = p.n % p.chunk_syms != 0; // (as in k_decode_word_groups)
    for (;;) {
        const uint64_t claim = work.take(lane);
        if (claim >= claims)
            break;
        const uint64_t b_end = (claim + 1u) * per_claim < batches ? (claim + 1u) * per_claim : batches;
        for (uint64_t vb = claim * per_claim; vb < b_end; ++vb) {
            const uint64_t batch = ragged ? batches - 1u - vb : vb; // (a ragged last chunk: its batch goes round by round -- first)
            const uint64_t chunk = batch * 32u + g;
            const bool exists = chunk < p.nchunks;
            const uint64_t off = exists ? p.offsets[chunk] : 0u;
            const uint32_t len = exists ? p.lengths[chunk] : 0u;
            const bool valid = exists && len >= 2u * 4u && off <= p.container_bytes && len <= p.container_bytes - off;
            if (exists && !valid && i == 0)
                nbad++;
            const uint64_t src = cbase + (valid ? off : 0u);
            uint32_t x = Tr::kL;
            if (valid) // RansDecInit order: state 0 first (main.cpp:261-262)
                x = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[i];
            PairRing R;
            const PairRowOfLane row{ring_c, i};
            const uint32_t start = R.open(src, i, row, true, glo, glimit);
            uint32_t &cur = R.cur;
            auto checkpoint = [&]() { R.checkpoint(row, true); };

            const rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<void *>(reinterpret_cast<uint64_t>(p.out) + batch * 32u * p.chunk_syms), 0, 32u * p.chunk_syms, kRsrcFlags);
            const uint32_t out_off16 = valid ? g * p.chunk_syms + 16u * i : 0x80000000u; // (an invalid chunk's stores: dropped by the range check)
            // the quad's two chunks A = g & ~1 and B = A + 1, as lane t = lane & 3 of the quad addresses them: 16 t bytes in
            const bool valid_a = __shfl((int)valid, (int)(lane & ~3u)) != 0, valid_b = __shfl((int)valid, (int)(lane | 2u)) != 0;
            const uint32_t off_a = valid_a ? (g & ~1u) * p.chunk_syms + 16u * (lane & 3u) : 0x80000000u;
            const uint32_t off_b = valid_b ? (g | 1u) * p.chunk_syms + 16u * (lane & 3u) : 0x80000000u;
            uint32_t osoff = 0;
            auto sixteen = [&]() -> u32x4 { return pair_sixteen(R, x, L, row, true); };
            // 64 rounds = one 128-byte line of the chunk: four 16-byte stores per lane leave back to back (a pair writes 32
            // contiguous bytes per instruction; pieces of a line that leave 16 or 32 rounds apart reach memory as partial
            // lines -- measured 1.18 ms against 0.70 without stores)
            const bool by_rounds = ragged && batch + 1u == batches; // (wave-uniform)
            for (uint32_t q = 0; q < (by_rounds ? 0u : groups64); ++q) {
                const u32x4 v0 = sixteen();
                const u32x4 v1 = sixteen();
                const u32x4 v2 = sixteen();
                const u32x4 v3 = sixteen();
                // a quad writes 64 contiguous bytes per instruction, a chunk's line with two instructions back to back
                // (64-byte pieces off the 64-byte grid: plain stores, as in k_decode_word_groups -- 1000-symbol chunks 1.67 -> 1.42 ms;
                //  on the grid `nt sc1` wins: 960-symbol chunks 0.79 against 1.15)
                if (p.chunk_syms & 63u) {
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<0>(v0, v1), orsrc, off_a, osoff, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<0>(v2, v3), orsrc, off_a, osoff + 64u, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<1>(v0, v1), orsrc, off_b, osoff, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<1>(v2, v3), orsrc, off_b, osoff + 64u, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<0>(v0, v1), orsrc, off_a, osoff, kPairAux);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<0>(v2, v3), orsrc, off_a, osoff + 64u, kPairAux);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<1>(v0, v1), orsrc, off_b, osoff, kPairAux);
                    __builtin_amdgcn_raw_buffer_store_b128(quad_half<1>(v2, v3), orsrc, off_b, osoff + 64u, kPairAux);
                }
                osoff += 128u;
            }
            if (rem32 && !by_rounds) { // a chunk of an odd multiple of 64 symbols: its last half line
                const u32x4 v0 = sixteen();
                const u32x4 v1 = sixteen();
                __builtin_amdgcn_raw_buffer_store_b128(v0, orsrc, out_off16, osoff, 0);
                __builtin_amdgcn_raw_buffer_store_b128(v1, orsrc, out_off16, osoff + 32u, 0);
            }
            // what a chunk size off 64 leaves (at most 31 rounds) -- or, in the ragged chunk's batch, every round: compiler-scheduled,
            // one round at a time, lanes without a symbol sit the round out, a byte store per lane
            uint32_t nsym = valid ? p.chunk_syms : 0u, s_first = p.chunk_syms - left_syms;
            if (by_rounds) {
                s_first = 0u;
                if (valid && chunk + 1u == p.nchunks)
                    nsym = (uint32_t)(p.n - chunk * p.chunk_syms);
            }
            for (uint32_t s0 = s_first; s0 < p.chunk_syms; s0 += 2u) {
                if (((s0 - s_first) & 15u) == 0)
                    checkpoint();
                const bool active = s0 + i < nsym;
                const uint32_t sy = decode_pair_round<false>(x, cur, active, i, maskv, sbv, rec, l23, l15, ring_c, 0);
                if (active)
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)sy, orsrc, out_off16 - 16u * i + s0 + i, 0, 0);
            }
            // integrity: both states back at L, the cursor exactly at the end of the chunk's stream
            const bool bad = valid && (x != Tr::kL || cur - (start - 2u * 4u) != len);
            const uint64_t bm = __builtin_amdgcn_ballot_w64(bad);
            if (i == 0 && ((bm >> (2u * g)) & 3u) != 0)
                nbad++;
        }
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
}

// ---------------------------------------------------------------------------
// k_decode_batch_byte_pairs -- the ragged form of k_decode_byte_pairs (rans_amd_decode_batch under
// RANS_AMD_OPT_BATCH_PAIRS): a wave's thirty-two pairs hold thirty-two STREAMS, each with its own symbol count and its own
// output address.  The unit of work is one wave-load of the hand-out order: lane 2 g + i holds state i of the stream at
// position 32 w + g -- stream order[32 w + g], or 32 w + g without an order; a position at or past nchunks has no stream.
// The rounds, the 68-byte ring rows and their refills, the pair interleave and the quad gather are k_decode_byte_pairs';
// what is new is that the pairs' loop counts differ, as the groups' do in k_decode_batch_word_groups:
//   * the wave runs the 64-round line body max_g(blocks_g) times with FULL exec, blocks_g = count_g >> 7 whole 128-byte
//     lines.  The sequence sets exec = -1 itself and its DPP moves read the pair's other lane, so a pair that has run out of
//     lines cannot be masked off: it is PARKED.  There is no per-pair ballot to zero here (a lane's byte count comes from
//     its own two compares), so a parked pair's cursor does move; instead
//       - its checkpoint() is gated by q < blocks_g: it writes no ring byte and issues no global load, and its ring, pend,
//         ld, left and thr stay exactly what they were when it parked -- it still owes its tail;
//       - its state x and its cursor cur are put back from copies behind every line (two selects);
//       - its line is not stored.
//     A parked pair keeps running the rounds on whatever its state becomes, and that is safe: a round reads only LDS and
//     writes nothing but the pair's own registers.  It reads cum2sym at x & mask, inside table 0 whatever x is; a record at
//     rec + 8 s with s a byte of cum2sym, i.e. a symbol of the model, inside table 1 for every table the model builder
//     makes; and the ring at ring + (position & 63) and one byte further, inside the pair's own 68-byte row whatever the
//     cursor is.  It reads no global memory: refills are checkpoint()'s, and that is gated.  The same holds for a pair
//     without a stream or with a rejected one, which is parked from the start and whose ring is never filled from memory
//     (b0, b1 and pend are zero, left = 0).
//   * behind the common loop every pair decodes its count_g - 128 blocks_g remaining symbols one round at a time, lanes
//     without a symbol sitting out, a byte store per lane (the uniform kernel's path for a ragged last chunk).
// Every lane addresses its output in 64 bits (out_syms is 64-bit, and the 32 streams of a wave may lie anywhere in it).  A
// stream whose output is not 4-byte aligned takes the round-by-round path for all of its symbols (blocks_g = 0).
// Index entries are the caller's data and checked per pair as k_decode_batch_word_groups checks them per group: the order
// entry names a stream, the stream holds its two states and lies inside the container, the symbol range lies inside
// [0, out_syms); no parity rule on the offset (the byte format's unit is 1).  A stream that fails is counted once, by the
// pair's even lane; nothing of it is fetched, nothing stored.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGrpThreads, 8) k_decode_batch_byte_pairs(const DecParams p)
{
    using Tr = FmtTraits<FMT_BYTE>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long t_start = p.span ? wall_clock64() : 0ull;
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // cum2sym u8[M]
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u; // {freq, start}[nsyms]
    stage_table(smem, p.table0, t0_bytes);
    stage_table(smem + t0_bytes, p.table1, t1_bytes);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t ring_c = t0_bytes + t1_bytes + wave * kPairWaveLds + (lane >> 1) * kPairRow; // (as in k_decode_byte_pairs, the constants as well)
    uint32_t ring_i = ring_c + 16u * (lane & 1u); // where this lane's 16 bytes of a block go
    pin_vgpr(ring_i);
    const PairLane L(ring_c, p.scale_bits, t0_bytes, lane & 1u);
    const uint32_t ring = L.ring, maskv = L.maskv, sbv = L.sbv, rec = L.rec, l23 = L.l23, l15 = L.l15, sel_p = L.sel_p;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glo = cbase & ~uint64_t(15), glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 31u) >> 5); // wave-loads, one per claim (the last one may hold fewer than 32
                                                                         // streams); stream indices are 32-bit

    // over the 32 pairs (v is the same in a pair's lanes): a butterfly over lane ^ 2, 4, 8, 16 inside each half of the wave
    // (ds_swizzle in bit-mask mode: and 0x1f, or 0, xor d -- no address register), then the larger of the two halves
    auto wave_max = [&](uint32_t v) -> uint32_t {
        uint32_t t;
        t = (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x081f);
        v = t > v ? t : v;
        t = (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101f);
        v = t > v ? t : v;
        t = (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x201f);
        v = t > v ? t : v;
        t = (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401f);
        v = t > v ? t : v;
        const uint32_t lo = __builtin_amdgcn_readlane(v, 0), hi = __builtin_amdgcn_readlane(v, 32);
        return lo > hi ? lo : hi;
    };
    // the lane number, worked out where it is needed: what follows from it -- index addresses, shuffle addresses, 16 t -- is
    // then worked out per claim as well and not kept in registers across the line loop (volatile: not hoisted)
    auto lane_now = [&]() -> uint32_t {
        uint32_t l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };

    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    for (;;) {
        const uint64_t load = work.take(lane);
        if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
            break;
        // ---- this pair's stream: its index entries, all of them the caller's data
        const uint32_t ln = lane_now();
        const uint32_t g = ln >> 1, i = ln & 1u;
        // (fetch_stream_entry<2 * 4, false>, written out: see the ring below)
        const uint64_t pos = load * 32u + g;
        const bool exists = pos < p.nchunks;
        uint64_t s = pos;
        if (exists && p.order)
            s = p.order[pos];
        bool valid = exists && s < p.nchunks;
        uint64_t off = 0, first = 0;
        uint32_t len = 0, count = 0;
        if (valid) {
            off = p.offsets[s];
            len = p.lengths[s];
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
        }
        valid = valid && len >= 2u * 4u && off <= p.container_bytes && len <= p.container_bytes - off && first <= p.out_syms &&
                count <= p.out_syms - first;
        if (exists && !valid && i == 0)
            nbad++;
        const uint64_t src = cbase + (valid ? off : 0u);
        uint32_t x = Tr::kL;
        if (valid) // RansDecInit order: state 0 first (main.cpp:261-262)
            x = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[i];
        // The ring: PairRing's, but opened and checked here, on locals (a pair without a valid stream fetches nothing).  Through
        // PairRing::open() / checkpoint() this kernel's claim set-up compiles differently and the launch is 0.4 % slower
        // (profiles/groups_common_isa.md); put() and refill() are the shared ones.
        const uint64_t abase = src & ~uint64_t(kPairBlock - 1u);
        const uint32_t start = (uint32_t)(src - abase) + 2u * 4u; // < 40
        uint32_t cur = start;
        uint64_t ld = abase + 16u * i;
        u32x4 b0 = {0u, 0u, 0u, 0u}, b1 = b0, pend = b0;
        if (valid) {
            b0 = load16(ld, glo, glimit);
            b1 = load16(ld + kPairBlock, glo, glimit);
            pend = load16(ld + 2u * kPairBlock, glo, glimit);
        }
        ld += 3u * kPairBlock;
        uint32_t left = 0;
        if (valid && ld < glimit) {
            const uint64_t pieces = (glimit - ld + (kPairBlock - 1u)) / kPairBlock;
            left = pieces < 0x7fffffffu ? (uint32_t)pieces : 0x7fffffffu;
        }
        const PairRowPinned row{ring, ring_i};
        PairRing R;
        auto put = [&](uint32_t at, const u32x4 &v) { R.put(row, at, v); };
        put(0, b0);
        put(kPairBlock, b1);
        uint32_t thr = kPairBlock;
        auto checkpoint = [&](bool live) { // live: the pair runs (the same for both of its lanes); a parked pair's ring stays as it is
            if (live && cur >= thr) {
                put(~thr & kPairBlock, pend);
                thr += kPairBlock;
                R.ld = ld;
                R.pend = pend;
                R.left = left;
                R.refill();
                ld = R.ld;
                pend = R.pend;
                left = R.left;
            }
        };
        checkpoint(valid); // the states may end in block 1
        const uint32_t end = len + (start - 2u * 4u); // the cursor at the end of the stream

        // ---- the pair's own counts: whole lines through the common loop, the rest a round at a time
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + first; // (valid: [dst, dst + count) lies inside the output)
        const uint32_t blocks = (valid && (dst & 3u) == 0) ? count >> 7 : 0u;
        const uint32_t tail = valid ? count - (blocks << 7) : 0u;
        const uint32_t max_blocks = wave_max(blocks), max_tail = wave_max(tail);
        // the quad's two streams A = g & ~1 and B = A + 1, as lane t = lane & 3 of the quad addresses them: 16 t bytes in
        // (ds_bpermute with the byte address of the lane to read: __shfl keeps a lane number of its own in a register)
        auto from = [&](uint32_t v, int addr) -> uint32_t { return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v); };
        const int lane_a = (int)(4u * (ln & ~3u)), lane_b = (int)(4u * (ln | 2u));
        const uint32_t blocks_a = from(blocks, lane_a), blocks_b = from(blocks, lane_b);
        uint64_t line_a = ((uint64_t)from((uint32_t)(dst >> 32), lane_a) << 32 | from((uint32_t)dst, lane_a)) + 16u * (ln & 3u);
        uint64_t line_b = ((uint64_t)from((uint32_t)(dst >> 32), lane_b) << 32 | from((uint32_t)dst, lane_b)) + 16u * (ln & 3u);
        const bool pair_b = (ln & 2u) != 0; // this lane's own stream is the quad's B
        bool run = false;
        auto sixteen = [&]() -> u32x4 { // pair_sixteen() with this kernel's own checkpoint()
            uint32_t a0, a1, a2, a3;
            checkpoint(run);
            decode_pairs_8rounds(x, cur, a0, a1, maskv, sbv, rec, l23, l15, ring);
            checkpoint(run);
            decode_pairs_8rounds(x, cur, a2, a3, maskv, sbv, rec, l23, l15, ring);
            return pair_lines(a0, a1, a2, a3, sel_p);
        };
        for (uint32_t q = 0; q < max_blocks; ++q) {
            run = pair_b ? q < blocks_b : q < blocks_a; // q < this pair's blocks
            const uint32_t x_keep = x, cur_keep = cur;
            const u32x4 v0 = sixteen();
            const u32x4 v1 = sixteen();
            const u32x4 v2 = sixteen();
            const u32x4 v3 = sixteen();
            // a quad writes 64 contiguous bytes per instruction, a stream's line with two instructions back to back; the
            // gathers run under full exec (their DPP moves read all four lanes), the stores under q < blocks of the stream
            // they belong to.  Plain stores: a stream starts anywhere on the 4-byte grid, so its lines straddle the memory's
            // -- the case in which k_decode_byte_pairs leaves it to L2 to put the pieces together.
            const u32x4 ha0 = quad_half<0>(v0, v1), ha1 = quad_half<0>(v2, v3);
            if (q < blocks_a) {
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_a) = ha0;
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_a + 64u) = ha1;
            }
            const u32x4 hb0 = quad_half<1>(v0, v1), hb1 = quad_half<1>(v2, v3);
            if (q < blocks_b) {
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_b) = hb0;
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_b + 64u) = hb1;
            }
            line_a += 128u; // (past a stream's last line the address is not used any more)
            line_b += 128u;
            x = run ? x : x_keep;
            cur = run ? cur : cur_keep;
        }
        // ---- count - 128 blocks symbols (all of them where the output is not 4-byte aligned): one round at a time, compiler-scheduled
        // (this pair's address from the quad's: the lines have moved on by max_blocks, the pair's tail follows its own blocks)
        const uint32_t lt = lane_now();
        const uint32_t gt = lt >> 1, it = lt & 1u;
        const bool tail_b = (lt & 2u) != 0;
        const int lane_o = (int)(4u * (lt ^ 1u)); // the pair's other lane
        const uint64_t tail_dst = (tail_b ? line_b : line_a) - 16u * (lt & 3u) - ((uint64_t)(max_blocks - (tail_b ? blocks_b : blocks_a)) << 7);
        const uint32_t tail_rounds = (uint32_t)(((uint64_t)max_tail + 1u) >> 1);
        for (uint32_t rr = 0; rr < tail_rounds; ++rr) {
            if ((rr & 7u) == 0)
                checkpoint(valid);
            const uint32_t s0 = rr << 1; // < max_tail
            const bool active = s0 < tail && it < tail - s0;
            const uint32_t sy = decode_pair_round<true>(x, cur, active, it, maskv, sbv, rec, l23, l15, ring, lane_o);
            if (active)
                *reinterpret_cast<uint8_t RANS_GLOBAL *>(tail_dst + s0 + it) = (uint8_t)sy;
        }
        // integrity: both states back at L, the cursor exactly at the end of the stream
        const bool bad = valid && (x != Tr::kL || cur != end);
        const uint64_t bm = __builtin_amdgcn_ballot_w64(bad);
        if (it == 0 && ((bm >> (2u * gt)) & 3u) != 0)
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
    record_span(p, t_start, smem, wave * 64u + lane_now());
}

// ---------------------------------------------------------------------------
// k_decode_batch_alias_pairs -- k_decode_batch_byte_pairs' plan for the ALIAS format's 2-way layout (main_alias.cpp;
// rans_amd_decode_batch under RANS_AMD_OPT_BATCH_ALIAS_PAIRS).  An alias stream is a byte-format stream -- the same
// renormalisation, the same pair interleave, 0, 1 or 2 bytes per state and round -- so everything but the symbol step is the
// byte kernel's: lane 2 g + i holds state i of the stream at position 32 load + g of the hand-out order; 68-byte ring rows fed
// through load16 and refills behind the pair's own checkpoint(); whole 128-byte lines in the common loop under full exec, pairs
// that have run out of lines PARKED (no checkpoint, x and the cursor put back from copies behind every line, no store); tails
// a round at a time with byte stores; an output off the 4-byte grid by rounds entirely; 64-bit output addresses in every lane;
// index entries checked per pair (fetch_stream_entry) and counted once by the even lane; the stream accepted when both states
// are back at L and the cursor stands at its end.  Here all of that comes through the shared pieces (PairRing, PairRowPinned,
// PairLane, fetch_stream_entry, wave_max32, lane_number_now, pair_lines, quad_half), which the byte kernel, left as it compiles,
// partly keeps written out.
// The tables are the FMT_ALIAS ones fill_decoder_tables hands every alias decoder: {freq | sym << 16, adjust} per half bucket
// (table 0, LDS address 0, 16 nsyms bytes) and divider u32[nsyms] (table 1) -- 5 KiB for 256 symbols at ANY scale_bits, where
// the byte kernel's cum2sym is 64 KiB at 16 bits and leaves one block per CU: here two blocks share a CU at every scale_bits.
// A parked pair, and one without a stream or with a rejected one, free-runs the rounds on whatever its state becomes, as in the
// byte kernel, and that is safe for the same reason: a round reads only LDS and writes only the pair's own registers.  It reads
// divider[bucket] with bucket = (x & mask) >> (scale_bits - log2 nsyms) < nsyms, inside table 1 whatever x is; the 16 bytes at
// 16 bucket, the records of halves 2 bucket and 2 bucket + 1 < 2 nsyms, inside table 0 whatever x is (the divider selects
// between them and goes into no address); the symbol comes out of the selected record, so no further address depends on a
// table's content; and the ring at ring + (position & 63) and one byte further, inside the pair's
// own 68-byte row whatever the cursor is.  No global memory: refills are checkpoint()'s, and that is gated.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGrpThreads, 8) k_decode_batch_alias_pairs(const DecParams p)
{
    using Tr = FmtTraits<FMT_ALIAS>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long t_start = p.span ? wall_clock64() : 0ull;
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // {freq | sym << 16, adjust}[2 nsyms]
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u; // divider u32[nsyms]
    stage_table(smem, p.table0, t0_bytes);
    stage_table(smem + t0_bytes, p.table1, t1_bytes);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t ring_c = t0_bytes + t1_bytes + wave * kPairWaveLds + (lane >> 1) * kPairRow; // raw LDS byte address of the pair's ring
    uint32_t ring_i = ring_c + 16u * (lane & 1u); // where this lane's 16 bytes of a block go
    pin_vgpr(ring_i);
    const PairLane L(ring_c, p.scale_bits, t0_bytes, lane & 1u); // (L.rec: the dividers' address)
    const uint32_t bsh = uniform(p.scale_bits - p.log2nsyms);     // slot -> bucket (the launcher: log2nsyms <= 8 <= scale_bits)
    const PairRowPinned row{L.ring, ring_i};

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glo = cbase & ~uint64_t(15), glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 31u) >> 5); // wave-loads, one per claim (the last one may hold fewer than 32
                                                                         // streams); stream indices are 32-bit
    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    for (;;) {
        const uint64_t load = work.take(lane);
        if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
            break;
        // ---- this pair's stream: its index entries, all of them the caller's data
        const uint32_t ln = lane_number_now();
        const uint32_t g = ln >> 1, i = ln & 1u;
        bool exists, valid;
        uint64_t off, first;
        uint32_t len, count;
        fetch_stream_entry<2u * 4u, false>(p, load * 32u + g, exists, valid, off, first, len, count);
        if (exists && !valid && i == 0)
            nbad++;
        const uint64_t src = cbase + (valid ? off : 0u);
        uint32_t x = Tr::kL;
        if (valid) // RansDecInit order: state 0 first (main_alias.cpp: as main.cpp:261-262)
            x = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[i];
        PairRing R; // (a pair without a valid stream fetches nothing, now or later)
        const uint32_t start = R.open(src, i, row, valid, glo, glimit);
        uint32_t &cur = R.cur;
        const uint32_t end = len + (start - 2u * 4u); // the cursor at the end of the stream

        // ---- the pair's own counts: whole lines through the common loop, the rest a round at a time
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + first; // (valid: [dst, dst + count) lies inside the output)
        const uint32_t blocks = (valid && (dst & 3u) == 0) ? count >> 7 : 0u;
        const uint32_t tail = valid ? count - (blocks << 7) : 0u;
        const uint32_t max_blocks = wave_max32(blocks), max_tail = wave_max32(tail);
        // the quad's two streams A = g & ~1 and B = A + 1, as lane t = lane & 3 of the quad addresses them: 16 t bytes in
        auto from = [&](uint32_t v, int addr) -> uint32_t { return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v); };
        const int lane_a = (int)(4u * (ln & ~3u)), lane_b = (int)(4u * (ln | 2u));
        const uint32_t blocks_a = from(blocks, lane_a), blocks_b = from(blocks, lane_b);
        uint64_t line_a = ((uint64_t)from((uint32_t)(dst >> 32), lane_a) << 32 | from((uint32_t)dst, lane_a)) + 16u * (ln & 3u);
        uint64_t line_b = ((uint64_t)from((uint32_t)(dst >> 32), lane_b) << 32 | from((uint32_t)dst, lane_b)) + 16u * (ln & 3u);
        const bool pair_b = (ln & 2u) != 0; // this lane's own stream is the quad's B
        bool run = false;
        auto sixteen = [&]() -> u32x4 { // sixteen rounds -> this lane's 16 of the pair's 32 bytes
            uint32_t a0, a1, a2, a3;
            R.checkpoint(row, run);
            decode_alias_pairs_8rounds(x, cur, a0, a1, L.maskv, L.sbv, L.rec, bsh, L.l23, L.l15, L.ring);
            R.checkpoint(row, run);
            decode_alias_pairs_8rounds(x, cur, a2, a3, L.maskv, L.sbv, L.rec, bsh, L.l23, L.l15, L.ring);
            return pair_lines(a0, a1, a2, a3, L.sel_p);
        };
        for (uint32_t q = 0; q < max_blocks; ++q) {
            run = pair_b ? q < blocks_b : q < blocks_a; // q < this pair's blocks
            const uint32_t x_keep = x, cur_keep = cur;
            const u32x4 v0 = sixteen();
            const u32x4 v1 = sixteen();
            const u32x4 v2 = sixteen();
            const u32x4 v3 = sixteen();
            // the gathers under full exec (their DPP moves read all four lanes), the stores under q < blocks of the stream they
            // belong to; plain stores: a stream starts anywhere on the 4-byte grid
            const u32x4 ha0 = quad_half<0>(v0, v1), ha1 = quad_half<0>(v2, v3);
            if (q < blocks_a) {
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_a) = ha0;
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_a + 64u) = ha1;
            }
            const u32x4 hb0 = quad_half<1>(v0, v1), hb1 = quad_half<1>(v2, v3);
            if (q < blocks_b) {
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_b) = hb0;
                *reinterpret_cast<u32x4_a4 RANS_GLOBAL *>(line_b + 64u) = hb1;
            }
            line_a += 128u; // (past a stream's last line the address is not used any more)
            line_b += 128u;
            x = run ? x : x_keep;
            cur = run ? cur : cur_keep;
        }
        // ---- count - 128 blocks symbols (all of them where the output is not 4-byte aligned): one round at a time, compiler-scheduled
        // (this pair's address from the quad's: the lines have moved on by max_blocks, the pair's tail follows its own blocks)
        const uint32_t lt = lane_number_now();
        const uint32_t gt = lt >> 1, it = lt & 1u;
        const bool tail_b = (lt & 2u) != 0;
        const int lane_o = (int)(4u * (lt ^ 1u)); // the pair's other lane
        const uint64_t tail_dst = (tail_b ? line_b : line_a) - 16u * (lt & 3u) - ((uint64_t)(max_blocks - (tail_b ? blocks_b : blocks_a)) << 7);
        const uint32_t tail_rounds = (uint32_t)(((uint64_t)max_tail + 1u) >> 1);
        for (uint32_t rr = 0; rr < tail_rounds; ++rr) {
            if ((rr & 7u) == 0)
                R.checkpoint(row, valid);
            const uint32_t s0 = rr << 1; // < max_tail
            const bool active = s0 < tail && it < tail - s0;
            const uint32_t sy = decode_pair_round<true, true>(x, cur, active, it, L.maskv, L.sbv, L.rec, L.l23, L.l15, L.ring, lane_o, bsh);
            if (active)
                *reinterpret_cast<uint8_t RANS_GLOBAL *>(tail_dst + s0 + it) = (uint8_t)sy;
        }
        // integrity: both states back at L, the cursor exactly at the end of the stream
        const bool bad = valid && (x != Tr::kL || cur != end);
        const uint64_t bm = __builtin_amdgcn_ballot_w64(bad);
        if (it == 0 && ((bm >> (2u * gt)) & 3u) != 0)
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
    record_span(p, t_start, smem, wave * 64u + lane_number_now());
}

} // namespace

// (a ragged last chunk included: its octet goes one round at a time and is handed out first)
bool decode_word_groups_applicable(const DecParams &p)
{
    return p.n_ways == 8 && p.sym_bytes == 1 && p.scale_bits == 12 && (p.chunk_syms & 3u) == 0 && p.chunk_syms >= 32 && p.chunk_syms <= (1u << 20) &&
           (reinterpret_cast<uintptr_t>(p.out) & 3u) == 0 && p.n / p.chunk_syms >= 8 && !p.trace &&
           ((p.table0_bytes + 15u) & ~15u) % kGrpRing == 0;
}

hipError_t launch_decode_word_groups(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    const size_t lds = ((p.table0_bytes + 15u) & ~15u) + (size_t)(kGrpThreads / 64) * kGrpWaveLds;
    if (name)
        *name = KernelId::decode_word_groups;
    return launch_group_kernel<k_decode_word_groups>((p.nchunks + 7u) / 8u, lds, kGrpLdsCap, num_cus, stream, p);
}

// The ragged form: word format over u8 symbols (the caller has checked the format: the u16 kernel format is another one),
// from eight streams on; any symbol count, any output address.
bool decode_batch_word_groups_applicable(const DecParams &p)
{
    return p.n_ways == 8 && p.sym_bytes == 1 && p.scale_bits == 12 && p.nchunks >= 8 && p.sym_offsets && p.sym_counts && !p.trace &&
           ((p.table0_bytes + 15u) & ~15u) % kGrpRing == 0;
}

hipError_t launch_decode_batch_word_groups(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    const size_t lds = ((p.table0_bytes + 15u) & ~15u) + (size_t)(kGrpThreads / 64) * kGrpWaveLds;
    if (name)
        *name = KernelId::decode_batch_word_groups;
    return launch_group_kernel<k_decode_batch_word_groups>((p.nchunks + 7u) / 8u, lds, kGrpLdsCap, num_cus, stream, p); // one octet per wave
}

// The same for the byte format's 2-way layout (cum2sym tables, scale_bits 8..16, u8 symbols).
static size_t pair_lds(const DecParams &p) // both tables and the waves' ring rows
{
    return (size_t)((p.table0_bytes + 15u) & ~15u) + ((p.table1_bytes + 15u) & ~15u) + (size_t)(kGrpThreads / 64) * kPairWaveLds;
}
bool decode_byte_pairs_applicable(const DecParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.scale_bits >= 8 && p.scale_bits <= 16 && (p.chunk_syms & 3u) == 0 &&
           p.chunk_syms >= 64 && p.chunk_syms <= (1u << 20) && (reinterpret_cast<uintptr_t>(p.out) & 3u) == 0 && p.n / p.chunk_syms >= 32 && !p.trace &&
           pair_lds(p) <= kGrpLdsCap;
}

hipError_t launch_decode_byte_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (name)
        *name = KernelId::decode_byte_pairs;
    return launch_group_kernel<k_decode_byte_pairs>((p.nchunks + 31u) / 32u, pair_lds(p), kGrpLdsCap, num_cus, stream, p);
}

// The ragged form: byte format over u8 symbols with the cum2sym tables (the caller has checked the format: the fused slot
// records are another kernel format), from 32 streams on; any symbol count, any output address.
bool decode_batch_byte_pairs_applicable(const DecParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.scale_bits >= 8 && p.scale_bits <= 16 && p.nchunks >= 32 && p.sym_offsets && p.sym_counts &&
           !p.trace && pair_lds(p) <= kGrpLdsCap;
}

hipError_t launch_decode_batch_byte_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (name)
        *name = KernelId::decode_batch_byte_pairs;
    return launch_group_kernel<k_decode_batch_byte_pairs>((p.nchunks + 31u) / 32u, pair_lds(p), kGrpLdsCap, num_cus, stream, p); // one wave-load per wave
}

// The alias format's 2-way layout over u8 symbols with the FMT_ALIAS tables (the caller has checked the format): the alphabet
// a power of two of at most 256 symbols -- what the alias builder accepts, with 16 nsyms bytes of half-bucket records and
// 4 nsyms of dividers, so that the table sizes say it --, from 32 streams on; any symbol count, any output address.
bool decode_batch_alias_pairs_applicable(const DecParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.scale_bits >= 8 && p.scale_bits <= 16 && p.log2nsyms <= 8 &&
           p.table0_bytes == (16u << p.log2nsyms) && p.table1_bytes == (4u << p.log2nsyms) && p.nchunks >= 32 && p.sym_offsets && p.sym_counts &&
           !p.trace && pair_lds(p) <= kGrpLdsCap;
}

hipError_t launch_decode_batch_alias_pairs(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (name)
        *name = KernelId::decode_batch_alias_pairs;
    return launch_group_kernel<k_decode_batch_alias_pairs>((p.nchunks + 31u) / 32u, pair_lds(p), kGrpLdsCap, num_cus, stream, p); // one wave-load per wave
}

} // namespace rans_amd
