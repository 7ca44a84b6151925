// groups_common.hpp -- what the nine group kernels share (internal): decode_groups.hip's k_decode_word_groups,
// k_decode_batch_word_groups, k_decode_byte_pairs, k_decode_batch_byte_pairs, k_decode_batch_alias_pairs and encode_groups.hip's k_encode_word_groups,
// k_encode_batch_word_groups, k_encode_batch_byte_pairs, k_encode_batch_alias_pairs.  Every piece is written once here, forceinline, and where the kernels differ the difference is
// an argument or a template parameter that is constant at the call site (profiles/groups_common_isa.md: what each kernel
// compiles to with them).  The hand-scheduled sequences stay with their kernels.  Helpers that took the place of a lambda
// take their arguments as the lambda did -- what it captured by `const T &`, its own parameters by value: the register
// allocation of these kernels (64 VGPRs, some bytes of scratch) follows such details, and the note says which ones.  Such a
// signature is tagged "(by reference: see head)": do not tidy it into by-value scalars without running
// tools/compare_kernel_isa.py --ranges on both files.
#pragma once

#include "decode_common.hpp"

namespace rans_amd {

constexpr uint32_t kGrpBlock = 128;             // bytes a group moves at a time: 8 lanes x 16 B
constexpr uint32_t kGrpRing = 2 * kGrpBlock;    // per group
constexpr uint32_t kGrpWaveLds = 8 * kGrpRing;  // per wave
constexpr uint32_t kGrpThreads = 1024;
constexpr uint32_t kGrpLdsCap = 160 * 1024;     // the CU's LDS: what a group kernel's dynamic-LDS limit is raised to

// ---- prologue ------------------------------------------------------------------------------------------------------
// A table into LDS, 16 bytes per thread and trip.  The kernel's __syncthreads() follows, and its lds_starts_at_zero()
// guard with the early return (left in the kernel bodies: inside a helper the return costs 7..11 instructions).
// (by reference: see head)
__device__ __forceinline__ void stage_table(uint8_t *const &lds, const void *const &table, const uint32_t &bytes)
{
    const uint4 *g0 = reinterpret_cast<const uint4 *>(table);
    uint4 *l0 = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = threadIdx.x; i < bytes / 16u; i += blockDim.x)
        l0[i] = g0[i];
}

// the next launch's work counters and the span record, zeroed by block 0
__device__ __forceinline__ void reset_for_next_launch(const DecParams &p)
{
    if (p.work_counter_reset && blockIdx.x == 0 && threadIdx.x < kWorkPools)
        p.work_counter_reset[threadIdx.x * kWorkPoolStride] = 0u;
    if (p.span_reset && blockIdx.x == 0 && threadIdx.x < 2)
        p.span_reset[threadIdx.x] = 0ull;
}

// opaque to the compiler: a per-lane constant stays in its VGPR (a VALU operand from an SGPR or a literal issues slower:
// profiles/r01_ubench.log; the hand-scheduled sequences name them as "v" operands)
__device__ __forceinline__ void pin_vgpr(uint32_t &v) { asm volatile("v_mov_b32 %0, %0" : "+v"(v)); }

// group g's bits of the ballot's halves (a group of eight lanes lies in one half of the wave: one of the two is zero)
__device__ __forceinline__ void group_ballot_bits(uint32_t g, uint32_t &gm_lo, uint32_t &gm_hi)
{
    uint32_t lo = g < 4 ? 0xffu << (8u * g) : 0u, hi = g >= 4 ? 0xffu << (8u * (g - 4u)) : 0u;
    pin_vgpr(lo);
    pin_vgpr(hi);
    gm_lo = lo;
    gm_hi = hi;
}

// What lane 8 g + i of a word decoder keeps per lane, in VGPRs: the group's ring, its bits of the ballot, the constants of
// decode_octet_8rounds.
struct WordGroupLane {
    // raw LDS byte address of this group's ring (LDS starts at zero; 256-byte aligned: positions wrap with an and-or)
    uint32_t ring;
    // Ring positions carry a per-group bias of 16 g bytes: the groups' cursors move at the same average pace, and eight
    // rings 256 bytes apart would otherwise sit on the same banks.
    uint32_t bias;
    uint32_t gm_lo, gm_hi;
    uint32_t k255 = 255u, k65536 = 0x10000u;
    // v_perm selectors of the symbol accumulators (decode_common.hpp acc_symbol for byte 3 of the slot record's first word)
    uint32_t sel_a = 0x03020703u, sel_b = 0x03070100u, sel_c = 0x07020100u;
    __device__ __forceinline__ WordGroupLane(uint32_t t0_bytes, uint32_t wave, uint32_t g)
        : ring(t0_bytes + wave * kGrpWaveLds + g * kGrpRing), bias(16u * g)
    {
        group_ballot_bits(g, gm_lo, gm_hi);
        pin_vgpr(sel_a);
        pin_vgpr(sel_b);
        pin_vgpr(sel_c);
        pin_vgpr(k255);
        pin_vgpr(k65536);
    }
};

// ---- work hand-out -------------------------------------------------------------------------------------------------
// Work is handed out dynamically, as in decode_wave.hip k_decode (pool = blockIdx % 8 owns the claims c with c % 8 == pool),
// or by a static stride over the grid's waves where the launch has no counters.
// Nothing is claimed or fetched ahead of its unit: the kernels are bound by VALU and LDS issue (eight waves per SIMD), a
// wave's trips to memory in front of an octet are covered by the other seven, and measured (profiles/r06_word8_groups.md)
// a claim held while another octet is decoded keeps work from the waves that run dry: + 6 % at 16 octets per wave, + 15 %
// at one; index entries fetched during the last rounds only add to what the refills' s_waitcnt vmcnt(0) waits for.
struct WorkClaims {
    uint32_t *counter; // the pooled counters, or null
    uint64_t total_waves, claim_v;
    uint32_t npools, pool;
    __device__ __forceinline__ void init(uint32_t *work_counter, uint32_t wave, uint32_t waves_per_block)
    {
        counter = work_counter;
        total_waves = (uint64_t)gridDim.x * waves_per_block;
        claim_v = (uint64_t)blockIdx.x * waves_per_block + wave;
        npools = gridDim.x < kWorkPools ? gridDim.x : kWorkPools;
        pool = blockIdx.x % npools;
    }
    __device__ __forceinline__ uint64_t take(uint32_t lane) // wave-uniform; the caller compares it with its number of claims
    {
        if (counter) {
            uint32_t got = 0;
            if (lane == 0)
                got = atomicAdd(counter + pool * kWorkPoolStride, 1u);
            return (uint64_t)uniform(got) * npools + pool;
        }
        const uint64_t c = claim_v;
        claim_v += total_waves;
        return uniform64(c);
    }
};

// ---- the ballot, cut into groups -------------------------------------------------------------------------------------
// `pred` of the lanes of MY group (m_lo, m_hi: its bits of the ballot's halves; none for a parked or dead group): returns
// addend + the number of them below this lane (v_mbcnt adds its second operand) and moves the group's count on by all of them.
__device__ __forceinline__ uint32_t group_rank(bool pred, uint32_t m_lo, uint32_t m_hi, uint32_t addend, uint32_t &count)
{
    const uint64_t m = __builtin_amdgcn_ballot_w64(pred);
    const uint32_t t_lo = (uint32_t)m & m_lo, t_hi = (uint32_t)(m >> 32) & m_hi;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(t_hi, __builtin_amdgcn_mbcnt_lo(t_lo, addend));
    count += (uint32_t)__builtin_popcount(t_lo) + (uint32_t)__builtin_popcount(t_hi);
    return rank;
}

__device__ __forceinline__ uint32_t wave_max8(uint32_t v) // over the eight groups (v is the same in a group's lanes)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t t = __builtin_amdgcn_readlane(v, 8 * k);
        m = t > m ? t : m;
    }
    return m;
}

// ---- the decoders' stream rings ------------------------------------------------------------------------------------
// (by reference: see head)
__device__ __forceinline__ u32x4 load16(const uint64_t &a, const uint64_t &glo, const uint64_t &glimit) // 16 bytes of the container, zeros beyond its granules
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (a >= glo && a < glimit)
        v = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(a));
    return v;
}

// What a ring is fed from: aligned blocks of BLOCK bytes, 16 bytes per lane, the next block parked in registers one refill
// ahead.  The ring holds blocks nb - 2 and nb - 1, pend is block nb, ld the address of this lane's piece of block nb + 1.
template <uint32_t BLOCK> struct RingFeed {
    uint64_t ld;
    u32x4 pend;
    uint32_t left;
    // blocks 0, 1 (-> b0, b1: the ring's first content) and 2 (-> pend) from `at`; fetch: the ragged kernels' streams that
    // do not exist or were rejected fetch nothing, now or later (zeros, left = 0).  (The members assigned directly, `ld < glimit`
    // tested first: the shape with which all four decoders keep their loops and registers, profiles/groups_common_isa.md.)
    // (by reference: see head)
    __device__ __forceinline__ void open(const uint64_t &at, const bool &fetch, const uint64_t &glo, const uint64_t &glimit, u32x4 &b0, u32x4 &b1)
    {
        b0 = u32x4{0u, 0u, 0u, 0u};
        b1 = b0;
        pend = b0;
        if (fetch) {
            b0 = load16(at, glo, glimit);
            b1 = load16(at + BLOCK, glo, glimit);
            pend = load16(at + 2u * BLOCK, glo, glimit);
        }
        ld = at + 3u * BLOCK;
        // 16-byte pieces at ld, ld + BLOCK, ... that still lie inside the container's granules: the refills count them down instead
        // of comparing addresses (a piece beyond the end is not fetched; the ring then keeps what it had -- only a damaged
        // stream reads that far, and the integrity check is what catches those)
        left = 0;
        if (ld < glimit && fetch) {
            const uint64_t pieces = (glimit - ld + (BLOCK - 1u)) / BLOCK;
            left = pieces < 0x7fffffffu ? (uint32_t)pieces : 0x7fffffffu;
        }
    }
    __device__ __forceinline__ void refill() // pend has gone to the ring: the block after it
    {
        if (left) {
            pend = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(ld));
            left--;
        }
        ld += BLOCK;
    }
};

// A word group's ring: 256 bytes of LDS at `ring` (raw LDS address, 256-byte aligned: positions wrap with an and-or).
// Positions count from the 128-byte line of the stream's first byte and carry the group's bias; curw is the cursor in words.
struct WordRing : RingFeed<kGrpBlock> {
    uint32_t curw, wr, thr; // wr: where block nb goes; thr: cursor (words) from which block nb has to be in the ring
    // lane i of the group; returns the position behind the eight states
    // (by reference: see head)
    __device__ __forceinline__ uint32_t open(const uint64_t &src, const uint32_t &i, const uint32_t &ring, const uint32_t &bias, const bool &fetch, const uint64_t &glo,
                                            const uint64_t &glimit)
    {
        const uint64_t abase = src & ~uint64_t(kGrpBlock - 1u);
        const uint32_t start = (uint32_t)(src - abase) + 8u * 4u; // < 160
        curw = (start + bias) >> 1;
        u32x4 b0, b1;
        RingFeed::open(abase + 16u * i, fetch, glo, glimit, b0, b1);
        *reinterpret_cast<RANS_LDS u32x4 *>((uintptr_t)(ring | ((16u * i + bias) & 255u))) = b0;
        *reinterpret_cast<RANS_LDS u32x4 *>((uintptr_t)(ring | ((kGrpBlock + 16u * i + bias) & 255u))) = b1;
        wr = ring | ((16u * i + bias) & 255u);
        thr = (kGrpBlock + bias) >> 1;
        checkpoint(); // the states may end in block 1
        return start;
    }
    // Eight rounds consume at most one block per group: one compare per lane every eight rounds, the refill itself runs under
    // the exec mask of the groups that need it (the same for the eight lanes of a group; never true for a parked group: its
    // cursor stands still)
    __device__ __forceinline__ void checkpoint()
    {
        if (curw >= thr) {
            *reinterpret_cast<RANS_LDS u32x4 *>((uintptr_t)wr) = pend;
            wr ^= kGrpBlock;
            thr += kGrpBlock / 2u;
            refill();
        }
    }
};

__device__ __forceinline__ uint32_t lds_u16(uint32_t addr)
{
    return *reinterpret_cast<RANS_LDS const uint16_t *>((uintptr_t)addr);
}

// One compiler-scheduled round of a word group (what the eight-round sequence does, for the rounds it does not cover):
// rans_word_sse41.h:123-141.  Lanes without a symbol sit the round out; returns the slot record's first word (the symbol in
// its byte 3), 0 for those.
__device__ __forceinline__ uint32_t decode_word_round(const DecTables<FMT_WORD> &T, uint32_t &x, uint32_t &curw, bool active, uint32_t gm_lo,
                                                      uint32_t gm_hi, uint32_t k255, uint32_t k65536, uint32_t ring)
{
    uint32_t raw = 0;
    if (active)
        raw = dec_step<FMT_WORD>(T, x);
    const bool need = active && x < k65536;
    const uint32_t at = group_rank(need, gm_lo, gm_hi, curw, curw); // the cursor + this group's renormalising lanes below me
    if (need)
        x = (x << 16) | lds_u16(((at << 1) & k255) | ring);
    return raw;
}

// ---- the byte format's pairs ----------------------------------------------------------------------------------------
constexpr uint32_t kPairBlock = 32;              // bytes a pair fetches at a time: 2 lanes x 16 B
constexpr uint32_t kPairRing = 2 * kPairBlock;   // per pair
constexpr uint32_t kPairRow = kPairRing + 4;     // ring + the mirror byte; 17 dwords: equal positions of the 32 pairs on 32 banks
constexpr uint32_t kPairWaveLds = 32 * kPairRow; // per wave

// What a lane of a pair keeps in VGPRs: the constants of decode_pairs_8rounds and pair_lines.
struct PairLane {
    uint32_t ring, maskv, sbv, rec; // raw LDS byte address of the pair's ring; x & maskv, x >> sbv; the records' LDS address
    uint32_t l23 = 1u << 23, l15 = 1u << 15;
    uint32_t sel_p; // v_perm(theirs, mine): the pair's bytes in stream order
    // (by reference: see head)
    __device__ __forceinline__ PairLane(const uint32_t &ring_c, const uint32_t &scale_bits, const uint32_t &t0_bytes, const uint32_t &odd)
        : ring(ring_c), maskv((1u << scale_bits) - 1u), sbv(scale_bits), rec(t0_bytes), sel_p(odd ? 0x03070206u : 0x05010400u)
    {
        pin_vgpr(ring);
        pin_vgpr(maskv);
        pin_vgpr(sbv);
        pin_vgpr(rec);
        pin_vgpr(l23);
        pin_vgpr(l15);
    }
};

// A pair's ring: 64 bytes of LDS in a 68-byte row (byte 64 mirrors byte 0, so that the second byte of a lane can be read at
// offset 1 without wrapping).  Positions count from the 32-byte block of the stream's first byte; cur is the cursor in bytes.
// How a lane addresses the row is the kernel's, a ROW argument constant at every call: the uniform kernel from the row's
// address and its lane of the pair; the ragged kernel, which must not keep the lane number live across its line loop, from
// the two addresses it has pinned in VGPRs.
struct PairRowOfLane {
    uint32_t ring_c, i;
    __device__ __forceinline__ uint32_t piece(uint32_t at) const { return ring_c + at + 16u * i; } // where this lane's 16 bytes of a block go
    __device__ __forceinline__ bool even() const { return i == 0; }
    __device__ __forceinline__ uint32_t mirror() const { return ring_c + kPairRing; }
};
struct PairRowPinned {
    uint32_t ring, ring_i; // ring_i = ring + 16 i
    __device__ __forceinline__ uint32_t piece(uint32_t at) const { return ring_i + at; }
    __device__ __forceinline__ bool even() const { return ring_i == ring; }
    __device__ __forceinline__ uint32_t mirror() const { return ring + kPairRing; }
};
// (k_decode_batch_byte_pairs takes put() and refill() from here and keeps open() and the checkpoint condition in its body:
// profiles/groups_common_isa.md, "Left in place".  A fix to open() or checkpoint() has to be made there as well.)
struct PairRing : RingFeed<kPairBlock> {
    uint32_t cur, thr; // thr: cursor from which block nb has to be in the ring; block nb goes to ring offset ~thr & 32
    template <class ROW> __device__ __forceinline__ void put(const ROW &row, uint32_t at, const u32x4 &v)
    {
        RANS_LDS uint32_t *d = reinterpret_cast<RANS_LDS uint32_t *>((uintptr_t)row.piece(at)); // (rows are 4-byte aligned: four dword writes)
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
        if (at == 0 && row.even())
            *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)row.mirror()) = (uint8_t)v.x;
    }
    // lane i of the pair; returns the position behind the two states
    // (by reference: see head)
    template <class ROW>
    __device__ __forceinline__ uint32_t open(const uint64_t &src, const uint32_t &i, const ROW &row, const bool &fetch, const uint64_t &glo, const uint64_t &glimit)
    {
        const uint64_t abase = src & ~uint64_t(kPairBlock - 1u);
        const uint32_t start = (uint32_t)(src - abase) + 2u * 4u; // < 40
        cur = start;
        u32x4 b0, b1;
        RingFeed::open(abase + 16u * i, fetch, glo, glimit, b0, b1);
        put(row, 0, b0);
        put(row, kPairBlock, b1);
        thr = kPairBlock;
        checkpoint(row, fetch); // the states may end in block 1
        return start;
    }
    // Eight rounds consume at most 8 x 2 x 2 = 32 bytes per pair: one compare per lane every eight rounds (the same for both
    // lanes of a pair).  live: the pair runs; a parked pair's ring stays as it is.
    template <class ROW> __device__ __forceinline__ void checkpoint(const ROW &row, bool live)
    {
        if (live && cur >= thr) {
            put(row, ~thr & kPairBlock, pend);
            thr += kPairBlock;
            refill();
        }
    }
};

// One compiler-scheduled round of a pair: rans_byte.h:125-128 (get), :291-298 (advance), :307-318 (renormalise: state 0's
// bytes first).  Lanes without a symbol sit the round out; returns the symbol.  The other lane's byte count comes through
// __shfl_xor, or (BPERMUTE) through ds_bpermute with lane_o, the byte address of the lane to read: __shfl keeps a lane
// number of its own in a register.
// ALIAS: the alias format's symbol step instead (main_alias.cpp:252-267, dec_step's FMT_ALIAS form): the half-bucket records
// {freq | sym << 16, adjust} at LDS address 0, `rec` the dividers' address, bsh = scale_bits - log2 nsyms.
// (by reference: see head)
template <bool BPERMUTE, bool ALIAS = false>
__device__ __forceinline__ uint32_t decode_pair_round(uint32_t &x, uint32_t &cur, const bool &active, const uint32_t &odd, const uint32_t &maskv,
                                                      const uint32_t &sbv, const uint32_t &rec, const uint32_t &l23, const uint32_t &l15,
                                                      const uint32_t &ring, const int &lane_o, const uint32_t &bsh = 0u)
{
    uint32_t sy = 0, n = 0;
    if (active) {
        const uint32_t cf = x & maskv;
        if constexpr (ALIAS) {
            const uint32_t bucket = cf >> bsh;
            const uint32_t div = *reinterpret_cast<RANS_LDS const uint32_t *>((uintptr_t)(rec + 4u * bucket));
            const uint32_t half = 2u * bucket + ((cf - div) >> 31); // + 1: the bucket's own symbol (cf < divider; both < 2^17)
            const u32x2 e = *reinterpret_cast<RANS_LDS const u32x2 *>((uintptr_t)(8u * half));
            sy = e.x >> 16;
            x = (e.x & 0xffffu) * ((x >> sbv) & 0xffffffu) + cf - e.y;
        } else {
            sy = *reinterpret_cast<RANS_LDS const uint8_t *>((uintptr_t)cf);
            const u32x2 fr = *reinterpret_cast<RANS_LDS const u32x2 *>((uintptr_t)(rec + 8u * sy));
            x = (fr.x & 0xffffffu) * ((x >> sbv) & 0xffffffu) + cf - fr.y;
        }
        n = (uint32_t)(x < l23) + (uint32_t)(x < l15);
    }
    const uint32_t n_other = BPERMUTE ? (uint32_t)__builtin_amdgcn_ds_bpermute(lane_o, (int)n) : (uint32_t)__shfl_xor((int)n, 1, 64);
    const uint32_t pos = cur + (odd ? n_other : 0u);
    cur += n + n_other;
    if (n >= 1u)
        x = (x << 8) | *reinterpret_cast<RANS_LDS const uint8_t *>((uintptr_t)(ring + (pos & 63u)));
    if (n >= 2u)
        x = (x << 8) | *reinterpret_cast<RANS_LDS const uint8_t *>((uintptr_t)(ring + ((pos + 1u) & 63u)));
    return sy;
}

// Sixteen rounds = one 128-byte line per group.  Round r's symbols go to byte (r >> 1) & 3 of accumulator
// (r & 1) + 2 (r >> 3): after the quad transposes lane (m = i & 3, h = i >> 2) holds the dwords (row 2 m, half h),
// (row 2 m + 1, half h), (row 8 + 2 m, h), (row 9 + 2 m, h) of the line's sixteen 8-byte rows; the halves h = 0
// keep the first two and take their other halves from lane i + 4, the halves h = 1 the last two from lane i - 4:
// lane i then holds bytes [16 i, 16 i + 16) of the line, one 16-byte store per lane.
// (v_cndmask_b32_dpp by hand: left to the compiler, the select becomes a branch around the DPP move, and a DPP
// move under an exec mask reads zeros from the lanes the mask has switched off -- the very lanes it is after.  For the
// same reason the ragged kernels run it under full exec.)
__device__ __forceinline__ u32x4 halves_to_line(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3)
{
    u32x4 v;
    asm volatile("s_nop 1\n\t"
                 "s_mov_b64 vcc, %[lower]\n\t"
                 "v_cndmask_b32_dpp %[vx], %[a2], %[a0], vcc row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" // lower ? a0 : a2 of lane - 4
                 "v_cndmask_b32_dpp %[vz], %[a3], %[a1], vcc row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "s_mov_b64 vcc, %[upper]\n\t"
                 "v_cndmask_b32_dpp %[vy], %[a0], %[a2], vcc row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" // upper ? a2 : a0 of lane + 4
                 "v_cndmask_b32_dpp %[vw], %[a1], %[a3], vcc row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : [vx] "=&v"(v.x), [vy] "=&v"(v.y), [vz] "=&v"(v.z), [vw] "=&v"(v.w)
                 : [a0] "v"(a0), [a1] "v"(a1), [a2] "v"(a2), [a3] "v"(a3), [lower] "s"(0x0f0f0f0f0f0f0f0full),
                   [upper] "s"(0xf0f0f0f0f0f0f0f0ull)
                 : "vcc");
    return v;
}

// The encoders' inverse: rows 2 i, 2 i + 1 of the line -> this state's column.  The halves of the group swap what
// halves_to_line gave them; the quad transposes, which are their own inverse, follow at the call.
__device__ __forceinline__ void line_to_halves(const u32x4 &v, uint32_t &a0, uint32_t &a1, uint32_t &a2, uint32_t &a3)
{
    asm volatile("s_nop 1\n\t"
                 "s_mov_b64 vcc, %[lower]\n\t"
                 "v_cndmask_b32_dpp %[a0], %[vy], %[vx], vcc row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" // lower ? mine : y of lane - 4
                 "v_cndmask_b32_dpp %[a1], %[vw], %[vz], vcc row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "s_mov_b64 vcc, %[upper]\n\t"
                 "v_cndmask_b32_dpp %[a2], %[vx], %[vy], vcc row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" // upper ? mine : x of lane + 4
                 "v_cndmask_b32_dpp %[a3], %[vz], %[vw], vcc row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3)
                 : [vx] "v"(v.x), [vy] "v"(v.y), [vz] "v"(v.z), [vw] "v"(v.w), [lower] "s"(0x0f0f0f0f0f0f0f0full),
                   [upper] "s"(0xf0f0f0f0f0f0f0f0ull)
                 : "vcc");
}

// ---- the encoders' rounds and blocks ---------------------------------------------------------------------------------
// One round of the compiler-scheduled kind: lanes without a symbol sit it out (main_simd.cpp:287-300 with in_size % 8 != 0:
// the partial round belongs to states 0 .. in_size % 8 - 1); it emits and tracks under `active` only.  m_lo, m_hi: the
// group's bits of the ballot, none once it is dead.  The group's words go to its ring at ring_c, the lane's 2 (c' - rank)
// bytes below the end of the stream.
// (by reference: see head)
template <bool SMALL>
__device__ __forceinline__ void encode_word_round(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t sym, bool active, const uint32_t &m_lo,
                                                  const uint32_t &m_hi, const uint32_t &ring_c)
{
    const u32x4 rec = *reinterpret_cast<RANS_LDS const u32x4 *>((uintptr_t)(sym << 4));
    const bool emit = active && x > rec.y; // rans_word_sse41.h:85
    const uint32_t rank = group_rank(emit, m_lo, m_hi, 0u, c);
    if (emit) {
        *reinterpret_cast<RANS_LDS uint16_t *>((uintptr_t)(ring_c | ((2u * (rank - c)) & 255u))) = (uint16_t)x;
        x >>= 16;
    }
    if (active) { // encode_common.hpp RANS_ENC_WORD_TAIL_*: x += bias + (x / freq) * cmpl
        uint32_t q = __umulhi(x, rec.x);
        if constexpr (!SMALL)
            q += (x - q) >> 1;
        q >>= rec.z >> 24;
        x = x + rec.w + (q & 0xffffffu) * (rec.z & 0xffffffu);
        worst |= rec.z;
    }
}

// The byte format's pair (rans_byte.h:62-90, main.cpp:226-246), one compiler-scheduled round: state 1 puts first, so the odd
// lane's bytes start at the pair's cursor c (bytes emitted so far) and the even lane's behind them -- the other lane's count
// comes through ds_bpermute with lane_o, the byte address of the lane to read.  Stream byte k (0 = the first emitted, the
// stream's LAST byte) lives at `top` - (k & 63) of the pair's 64-byte ring (top: raw LDS address of the ring's byte 63); a
// state emits its low byte first.  Lanes without a symbol sit the round out: they emit nothing, track nothing, keep their x.
// Record {rcp, cmpl | rshift << 24, bias, x_max} at LDS address sym << 4 (encode_common.hpp enc_byte_full's).
__device__ __forceinline__ void encode_pair_round(uint32_t &x, uint32_t &c, uint32_t &worst, uint32_t sym, bool active, uint32_t odd, uint32_t top,
                                                  int lane_o)
{
    const u32x4 rec = *reinterpret_cast<RANS_LDS const u32x4 *>((uintptr_t)(sym << 4));
    uint32_t n = 0;
    if (active)
        n = (uint32_t)(x >= rec.w) + (uint32_t)((x >> 8) >= rec.w); // `while (x >= x_max)`: never more than twice for scale_bits <= 16
    const uint32_t n_other = (uint32_t)__builtin_amdgcn_ds_bpermute(lane_o, (int)n);
    const uint32_t at = c + (odd ? 0u : n_other);
    c += n + n_other;
    if (n >= 1u)
        *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)(top - (at & 63u))) = (uint8_t)x;
    if (n >= 2u)
        *reinterpret_cast<RANS_LDS uint8_t *>((uintptr_t)(top - ((at + 1u) & 63u))) = (uint8_t)(x >> 8);
    x >>= 8u * n;
    if (active) { // x = bias + x + (x / freq) * cmpl_freq, the quotient by Alverson's reciprocal: exact for x < 2^31
        const uint32_t q = __umulhi(x, rec.x) >> ((rec.y >> 24) & 31u);
        x = x + rec.z + q * (rec.y & 0xffffffu);
        worst |= rec.y;
    }
}

// The lane number, worked out on the spot (volatile: not hoisted out of a claim loop, so that nothing that follows from it
// stays in registers across the loop's hand-scheduled part).
__device__ __forceinline__ uint32_t lane_number_now()
{
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// over the 32 pairs (v is the same in a pair's lanes): a butterfly over lane ^ 2, 4, 8, 16 inside each half of the wave
// (ds_swizzle in bit-mask mode: and 0x1f, or 0, xor d -- no address register), then the larger of the two halves
// (k_decode_batch_byte_pairs keeps its own copy of this and of the lane number as lambdas: it is left as it compiles)
__device__ __forceinline__ uint32_t wave_max32(uint32_t v)
{
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
}

// ---- index entries of a ragged stream (the decoders') --------------------------------------------------------------
// The entries of the stream at position `pos` of the hand-out order -- stream order[pos], or pos without an order; a
// position at or past nchunks has no stream.  All of them are the caller's data and checked as k_decode's RAGGED form checks
// them: the order entry names a stream, the offset is a multiple of the format's unit (EVEN: the word format's 2), the stream
// holds its states (MIN_LEN bytes) and lies inside the container, the symbol range lies inside [0, out_syms).  Nothing of a
// stream that fails is fetched or stored; the caller counts it once.
// (k_decode_batch_byte_pairs writes the same out in its body with MIN_LEN = 2 * 4 and no parity rule: through this helper, in
// either shape tried, its tail loop or its claim set-up compile differently -- profiles/groups_common_isa.md.  A fix here
// has to be made there as well.)
// (by reference: see head)
template <uint32_t MIN_LEN, bool EVEN>
__device__ __forceinline__ void fetch_stream_entry(const DecParams &p, const uint64_t &pos, bool &exists, bool &valid, uint64_t &off, uint64_t &first,
                                                   uint32_t &len, uint32_t &count)
{
    exists = pos < p.nchunks;
    uint64_t s = pos;
    if (exists && p.order)
        s = p.order[pos];
    valid = exists && s < p.nchunks;
    off = first = 0;
    len = count = 0;
    if (valid) {
        off = p.offsets[s];
        len = p.lengths[s];
        first = p.sym_offsets[s];
        count = p.sym_counts[s];
    }
    valid = valid && (!EVEN || (off & 1u) == 0) && len >= MIN_LEN && off <= p.container_bytes && len <= p.container_bytes - off &&
            first <= p.out_syms && count <= p.out_syms - first;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The launch of a group kernel, one instantiation per kernel: `units` of work (octets or wave-loads), one per wave, in blocks of
// kGrpThreads.  lds_cap: what the kernel's dynamic-LDS limit is raised to, and then a CU takes two blocks only where two fit
// under it; 0: the kernel stays within the default limit, two blocks per CU (the encoders).
template <auto KERN, class Params>
hipError_t launch_group_kernel(uint64_t units, size_t lds, uint32_t lds_cap, int num_cus, hipStream_t stream, const Params &p)
{
    static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
    if (lds_cap)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(KERN), (int)lds_cap, lds_ok); e != hipSuccess)
            return e;
    const uint32_t per_cu = lds_cap && 2u * lds > lds_cap ? 1u : 2u;
    const uint64_t want_blocks = (units + kGrpThreads / 64 - 1) / (kGrpThreads / 64);
    const uint64_t cap = (uint64_t)num_cus * per_cu;
    const uint32_t grid = (uint32_t)(want_blocks < cap ? want_blocks : cap);
    RANS_LAUNCH(KERN, dim3(grid), dim3(kGrpThreads), lds, stream, p);
    return hipGetLastError();
}

} // namespace rans_amd
