// decode_lanes.hip -- lane-per-stream decoders for narrow interleaves (N = 1, 2, 4, 8), all generations.

#include "lanes_common.hpp"
#include "groups_common.hpp" // the ragged kernel's prologue, work hand-out and span record

namespace rans_amd {

namespace {

// Per-lane stream window for the lane-per-stream decoder: 16 bytes of the lane's own stream
// in registers plus the next 16 prefetched, so that a lane touches global memory once per
// 16 stream bytes (a dword-per-unit walk would issue 4-16x as many scattered accesses).
// The window is consumed from its low end and shifted down after every unit -- positional
// indexing would be a chain of v_cndmask (~22 issue cycles each on gfx950) -- and the refill
// loads straight into `pre` under the lanes' exec mask, so the load issued at one refill is only
// waited for at the next one.
struct LaneWindow {
    u32x4 win, pre;
    uint64_t next;  // global address of the 16 bytes after `pre`
    uint64_t limit; // 16-byte aligned end of the readable container
    uint32_t left;  // bytes left in win (1..16)
    uint32_t used;  // stream bytes consumed so far

    template <int UNIT> __device__ __forceinline__ void shift()
    {
        if constexpr (UNIT == 4) {
            win.x = win.y;
            win.y = win.z;
            win.z = win.w;
        } else {
            win.x = __builtin_amdgcn_alignbit(win.y, win.x, 8 * UNIT);
            win.y = __builtin_amdgcn_alignbit(win.z, win.y, 8 * UNIT);
            win.z = __builtin_amdgcn_alignbit(win.w, win.z, 8 * UNIT);
            win.w >>= 8 * UNIT;
        }
    }
    __device__ __forceinline__ void refill()
    {
        win = pre;
        left = 16;
        if (next < limit) // past the container: `pre` keeps stale bytes, which only a corrupt chunk consumes
            pre = *reinterpret_cast<const u32x4 RANS_GLOBAL *>(next);
        next += 16;
    }
    template <int UNIT> __device__ __forceinline__ void open(uint64_t addr, uint64_t lim)
    {
        limit = lim;
        const uint64_t base = addr & ~uint64_t(15);
        used = 0;
        win = u32x4{0u, 0u, 0u, 0u};
        pre = win;
        if (base < limit)
            win = *reinterpret_cast<const u32x4 RANS_GLOBAL *>(base);
        if (base + 16 < limit)
            pre = *reinterpret_cast<const u32x4 RANS_GLOBAL *>(base + 16);
        next = base + 32;
        left = 16;
        for (uint32_t skip = (uint32_t)(addr & 15u); skip != 0; skip -= UNIT) { // once per chunk
            shift<UNIT>();
            left -= UNIT;
        }
    }
    template <int UNIT> __device__ __forceinline__ uint32_t take()
    {
        uint32_t w = win.x;
        if constexpr (UNIT == 2)
            w &= 0xffffu;
        else if constexpr (UNIT == 1)
            w &= 0xffu;
        shift<UNIT>();
        used += UNIT;
        left -= UNIT;
        if (left == 0)
            refill();
        return w;
    }
};

template <int FMT>
__device__ __forceinline__ void lane_renorm(typename FmtTraits<FMT>::state_t &x, LaneWindow &W, bool active)
{
    if constexpr (FMT == FMT_WORD) {
        if (active && x < (1u << 16)) // rans_word_sse41.h:134-141
            x = (x << 16) | W.take<2>();
    } else if constexpr (FMT == FMT_R64) {
        if (active && x < (1ull << 31)) // rans64.h:305-316
            x = (x << 32) | W.take<4>();
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) // rans_byte.h:307-318, at most two bytes for scale_bits <= 16
            if (active && x < (1u << 23))
                x = (x << 8) | W.take<1>();
    }
}

// ---------------------------------------------------------------------------
// Staged lane-per-stream decoder.  Per-lane 16-byte loads pull a whole memory line for every
// 16 bytes used, and the line is long evicted when the lane comes back for its next 16 bytes
// (measured: >= 4x over-fetch, the kernel sat on the fabric at ~3.3 TB/s); and a lane that
// refills on its own stalls its whole wave.  Here the WAVE refills for all of its 64 chunks at
// once, every 16 symbols: a lane's stream lives in a 128-byte ring in LDS (two 64-byte lines),
// lanes publish which line they need next, and 4 lanes fetch one chunk's line with coalesced
// 16-byte loads (4 load instructions cover 64 chunks x 64 B).  16 symbols consume at most one
// line (rans64: <= 4 B per symbol), so "at least 64 bytes ahead" before every group is all the
// invariant there is.  (What a VALID stream reaches is half of that: symbols of frequency 1 at
// 16 bits take 32 bytes per group in every format -- tests/test_lane_rate_cpu.py --, so the
// invariant has 32 bytes to spare; a refill threshold of 31 decodes wrongly.)  Ring rows are 136
// bytes apart: equal positions of the 64 lanes spread over 32 banks.  Positions are 32-bit offsets
// from the line of the wave's first chunk.
// ---------------------------------------------------------------------------
constexpr uint32_t kLaneWaveLds = 64 * kLaneRingStride + 64 * 4; // rings + one request word per lane

template <int FMT> struct LaneRing {
    const uint8_t *row; // this lane's ring in LDS
    uint32_t cur;       // read position (offset from the wave's region base)
    uint32_t used;      // stream bytes consumed

    template <int UNIT> __device__ __forceinline__ uint32_t take()
    {
        const uint8_t *at = row + (cur & (2 * kLaneLine - 1));
        cur += UNIT;
        used += UNIT;
        if constexpr (UNIT == 4)
            return *reinterpret_cast<const uint32_t *>(at);
        else if constexpr (UNIT == 2)
            return *reinterpret_cast<const uint16_t *>(at);
        else
            return *at;
    }
    __device__ __forceinline__ void renorm(typename FmtTraits<FMT>::state_t &x, bool active)
    {
        // the branch bodies hold an LDS read, so they stay exec-masked branches (no v_cndmask)
        if constexpr (FMT == FMT_WORD) {
            if (active && x < (1u << 16)) // rans_word_sse41.h:134-141
                x = (x << 16) | take<2>();
        } else if constexpr (FMT == FMT_R64) {
            if (active && x < (1ull << 31)) // rans64.h:305-316
                x = (x << 32) | take<4>();
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) // rans_byte.h:307-318, at most two bytes for scale_bits <= 16
                if (active && x < (1u << 23))
                    x = (x << 8) | take<1>();
        }
    }
};

// Smallest stream offset among the lanes that hold a chunk (wave-uniform): the base of the wave's 32-bit window
// onto the container.  Offsets need not ascend with the chunk index.  A wave addresses its batch through 32-bit offsets
// from the batch's lowest chunk: chunks that lie 1 GiB or more above it (an overflowed chunk of a large sized-slot
// container, a scattered hand-made index) wait for another trip of the same wave over the same batch, whose window starts
// at the lowest of THEM (`again` below) -- every well-formed index decodes, the usual batch in one trip.
__device__ __forceinline__ uint64_t wave_min_offset(uint64_t off, bool valid)
{
    uint32_t lo = valid ? (uint32_t)off : 0xffffffffu, hi = valid ? (uint32_t)(off >> 32) : 0xffffffffu;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t olo = (uint32_t)__shfl_xor((int)lo, d), ohi = (uint32_t)__shfl_xor((int)hi, d);
        const bool less = ohi < hi || (ohi == hi && olo < lo);
        lo = less ? olo : lo;
        hi = less ? ohi : hi;
    }
    return uniform64(((uint64_t)hi << 32) | lo);
}

template <int FMT, int NW>
__global__ void __launch_bounds__(1024) k_decode_lanes_staged(const DecParams p)
{
    using Tr = FmtTraits<FMT>;
    using state_t = typename Tr::state_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u;
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u;
    {
        const uint4 *g0 = reinterpret_cast<const uint4 *>(p.table0);
        uint4 *l0 = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < t0_bytes / 16u; i += blockDim.x)
            l0[i] = g0[i];
        const uint4 *g1 = reinterpret_cast<const uint4 *>(p.table1);
        uint4 *l1 = reinterpret_cast<uint4 *>(smem + t0_bytes);
        for (uint32_t i = threadIdx.x; i < t1_bytes / 16u; i += blockDim.x)
            l1[i] = g1[i];
    }
    __syncthreads();

    DecTables<FMT> T;
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }

    if (p.work_counter_reset && blockIdx.x == 0 && threadIdx.x < kWorkPools)
        p.work_counter_reset[threadIdx.x * kWorkPoolStride] = 0u; // keep the wave kernels' counter ring consistent
    if (p.span_reset && blockIdx.x == 0 && threadIdx.x < 2)
        p.span_reset[threadIdx.x] = 0ull;
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    uint8_t *rings = smem + t0_bytes + t1_bytes + wave * kLaneWaveLds;
    uint32_t *req = reinterpret_cast<uint32_t *>(rings + 64u * kLaneRingStride);
    const uint32_t part = lane & 3u, grp = lane >> 2;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glimit = (cbase + p.container_bytes + 15u) & ~uint64_t(15);
    const bool wide_out = p.sym_bytes == 1 && ((reinterpret_cast<uintptr_t>(p.out) | p.chunk_syms) & 15u) == 0;
    uint32_t nbad = 0;
    const uint64_t nbatches = (p.nchunks + 63u) / 64u;
    const uint64_t total_waves = (uint64_t)gridDim.x * waves_per_block;
    uint64_t again = 0; // lanes of the batch in hand whose chunks lay beyond the last trip's window
    for (uint64_t batch_v = (uint64_t)blockIdx.x * waves_per_block + wave; batch_v < nbatches; batch_v += again ? 0 : total_waves) {
        const uint64_t batch = uniform64(batch_v);
        const uint64_t chunk = batch * 64u + lane;
        bool valid = chunk < p.nchunks && (again == 0 || ((again >> lane) & 1u));
        const uint64_t off = valid ? p.offsets[chunk] : 0;
        const uint32_t len = valid ? p.lengths[chunk] : 0;
        const uint64_t first = chunk * p.chunk_syms;
        if (valid && ((off & (Tr::kUnit - 1u)) != 0 || len < NW * Tr::kStateBytes || off > p.container_bytes || len > p.container_bytes - off)) {
            nbad++; // (a malformed entry is seen in one trip only: it never joins `again`)
            valid = false;
        }
        // region base: the line of the lowest chunk of this trip
        const uint64_t rb = wave_min_offset(off, valid) & ~uint64_t(kLaneLine - 1);
        const bool far = valid && off - rb >= (1u << 30);
        again = __builtin_amdgcn_ballot_w64(far);
        valid = valid && !far;
        const uint32_t nsym = valid ? (uint32_t)((p.n - first) < p.chunk_syms ? (p.n - first) : p.chunk_syms) : 0u;
        uint8_t RANS_GLOBAL *dst = (uint8_t RANS_GLOBAL *)p.out + first * p.sym_bytes;

        state_t x[NW];
#pragma unroll
        for (int l = 0; l < NW; ++l) { // RansDecInit order: lane 0's state first
            x[l] = Tr::kL;
            if (valid) {
                const uint8_t RANS_GLOBAL *src = (const uint8_t RANS_GLOBAL *)p.container + off;
                if constexpr (FMT == FMT_R64) {
                    const u32x2 v = reinterpret_cast<const u32x2 RANS_GLOBAL *>(src)[l];
                    x[l] = (uint64_t)v.x | ((uint64_t)v.y << 32);
                } else {
                    x[l] = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[l];
                }
            }
        }
        LaneRing<FMT> W;
        W.row = rings + lane * kLaneRingStride;
        W.cur = (uint32_t)(off - rb) + NW * Tr::kStateBytes;
        W.used = 0;
        uint32_t ld = W.cur & ~(kLaneLine - 1u); // next line this lane has not staged yet

        // the whole wave takes part (also lanes without a chunk): lane -> which line its chunk needs,
        // then lane (4 g + part) moves 16 bytes of chunk (16 j + g)'s line, j = 0..3
        auto refill = [&]() {
            const bool need = valid && (int32_t)(ld - W.cur) < (int32_t)kLaneLine;
            req[lane] = need ? (ld | 1u) : 0u;
            if (need)
                ld += kLaneLine;
            uint32_t r[4];
            u32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = req[16 * j + grp]; // LDS ops of one wave execute in order: sees the writes above
                v[j] = u32x4{0u, 0u, 0u, 0u};
                const uint64_t a = cbase + rb + (r[j] & ~(kLaneLine - 1u)) + part * 16u;
                if ((r[j] & 1u) && a < glimit)
                    v[j] = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(a));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r[j] & 1u) {
                    uint8_t *at = rings + (16u * j + grp) * kLaneRingStride + (r[j] & kLaneLine) + part * 16u;
                    reinterpret_cast<u32x2 *>(at)[0] = u32x2{v[j].x, v[j].y}; // rows are 8-byte aligned
                    reinterpret_cast<u32x2 *>(at)[1] = u32x2{v[j].z, v[j].w};
                }
        };

        // 16 symbols into four dwords: 16/NW rounds of NW steps + renormalisations
        auto decode16 = [&]() -> u32x4 {
            uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int rr = 0; rr < 16 / NW; ++rr) {
#pragma unroll
                for (int l = 0; l < NW; ++l) {
                    uint32_t sy = dec_step<FMT>(T, x[l]);
                    if constexpr (Tr::kSymByte == 3)
                        sy >>= 24;
                    const int pos = rr * NW + l;
                    pk[pos / 4] |= (sy & 0xffu) << (8 * (pos % 4));
                }
#pragma unroll
                for (int l = 0; l < NW; ++l)
                    W.renorm(x[l], true);
            }
            return u32x4{pk[0], pk[1], pk[2], pk[3]};
        };

        // store addresses of the transposed output: instruction t writes the line of the quad's lane t
        uint64_t at[4];
        bool vq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int src = (int)((lane & ~3u) + t);
            const uint64_t d64 = reinterpret_cast<uint64_t>(dst);
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)d64, src), hi = (uint32_t)__shfl((int)(uint32_t)(d64 >> 32), src);
            at[t] = (((uint64_t)hi << 32) | lo) + (lane & 3u) * 16u;
            vq[t] = __shfl((int)valid, src) != 0;
        }
        refill(); // two lines ahead to start with
        // 64 symbols per trip: four groups of 16 (a refill before each), then the lane writes its 64
        // bytes with four back-to-back 16-byte stores.  One 16-byte store per group left every line
        // dirty in L2 for four groups -- long enough to be evicted half-written: 3.2x the bytes on
        // the write side (WRITE_SIZE 0.87 GB for 0.27 GB of symbols).
        for (uint32_t i0 = 0; __builtin_amdgcn_ballot_w64(i0 < nsym) != 0; i0 += 64u) {
            const uint32_t left = i0 < nsym ? nsym - i0 : 0u;
            if (__builtin_amdgcn_ballot_w64(!(left >= 64u && wide_out) && valid) == 0) { // wave-uniform
                u32x4 q0 = {0u, 0u, 0u, 0u}, q1 = q0, q2 = q0, q3 = q0;
                refill();
                if (left)
                    q0 = decode16();
                refill();
                if (left)
                    q1 = decode16();
                refill();
                if (left)
                    q2 = decode16();
                refill();
                if (left)
                    q3 = decode16();
                // (every valid lane has its 64 symbols here; lanes without a chunk carry zeros)
                quad_transpose(q0, q1, q2, q3, lane);
                const uint32_t o = i0;
                if (vq[0])
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[0] + o) = q0;
                if (vq[1])
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[1] + o) = q1;
                if (vq[2])
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[2] + o) = q2;
                if (vq[3])
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[3] + o) = q3;
                continue;
            }
            // ragged end of a chunk, unaligned or 16-bit output: 16 symbols at a time
            for (uint32_t g = 0; g < 4u; ++g) {
                refill();
                const uint32_t j0 = i0 + 16u * g;
                if (j0 >= nsym)
                    continue;
                const uint32_t cnt = nsym - j0 < 16u ? nsym - j0 : 16u;
                if (cnt == 16u && wide_out) {
                    const u32x4 q = decode16();
                    __builtin_nontemporal_store(q, reinterpret_cast<u32x4 RANS_GLOBAL *>(dst + j0)); // written once, never read back
                } else {
                    for (uint32_t i = 0; i < cnt; i += NW) {
                        const uint32_t c = cnt - i < (uint32_t)NW ? cnt - i : (uint32_t)NW;
#pragma unroll
                        for (int l = 0; l < NW; ++l)
                            if ((uint32_t)l < c) {
                                uint32_t sy = dec_step<FMT>(T, x[l]);
                                if constexpr (Tr::kSymByte == 3)
                                    sy >>= 24;
                                if (p.sym_bytes == 1)
                                    dst[j0 + i + l] = (uint8_t)sy;
                                else
                                    reinterpret_cast<uint16_t RANS_GLOBAL *>(dst)[j0 + i + l] = (uint16_t)sy;
                            }
#pragma unroll
                        for (int l = 0; l < NW; ++l)
                            W.renorm(x[l], (uint32_t)l < c);
                    }
                }
            }
        }
        bool bad = false;
#pragma unroll
        for (int l = 0; l < NW; ++l)
            bad = bad || (x[l] != Tr::kL);
        if (valid && (bad || W.used + NW * Tr::kStateBytes != len))
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
}

// ---------------------------------------------------------------------------
// k_decode_lanes_r64x2: the reference's 2-way rans64 loop (main64.cpp:261-282), one chunk per lane, third
// generation.  What bounds the staged kernel above (rocprofv3 counters, profiles/r02_lanes_counters.md): neither the
// VALU (30 % busy) nor the LDS pipe (42 %) but the vector-memory ADDRESS path -- TA busy 86 % of the kernel: every
// lane's 16-byte store is its own request (64 per instruction, 16.8 M write requests for 256 MiB), and so is every
// 16-byte piece a lane fetches for itself.  And, per wave, four DEPENDENT LDS round trips per pair of symbols.  Here
//  * global accesses are made by QUADS of lanes: the four lanes of a quad fetch the four 16-byte pieces of ONE
//    chunk's 64-byte line (instruction t serves the quad's lane t: address and exec mask by DPP broadcast) and write
//    them straight into that lane's ring row; the 64 symbols a lane has decoded are transposed inside the quad (4 x 4
//    pieces, v_cndmask_b32_dpp) so that store instruction t writes chunk (quad, t)'s whole line: 64-byte requests;
//  * the next 8 stream bytes of a lane sit in two registers (the "window"); a renormalisation takes the first
//    dword under an exec mask (v_cmpx), and only the lanes that consumed something re-read their window
//    (ds_read2_b32, exec-masked) while the NEXT pair's table lookups are in flight: two LDS round trips per pair;
//  * a line is requested as soon as the ring has room for it (<= 64 B staged ahead), ONE GROUP (16 symbols) before
//    it is written to the ring: the pieces stay in registers over the group.  A valid stream consumes <= 40 B per
//    group (5 renormalisations per state: 8 x 16 bits out, 32 bits in each) and the window reads 8 B ahead, so
//    >= 48 B ahead at a group boundary is the invariant; a lane below that (streams of 2^-16 symbols) is served
//    synchronously on a side path.  (The 40 is a loose bound: a state that loses 8 x 16 bits and stays inside its
//    32-bit-wide interval takes at most FOUR dwords, 32 B per group for both -- tests/test_lane_rate_cpu.py -- so a valid
//    stream needs 40 B ahead and the invariant has a dword per state to spare; a threshold of 36 decodes wrongly.)
//  * the whole trip loop is ONE asm statement: states, window, parked pieces, packed symbols and temporaries in
//    fixed registers (64-bit operands need their halves named; nothing in flight crosses a statement the compiler
//    schedules).  The 64 symbols of a trip are stored at the start of the next trip, after its first vmcnt wait, so
//    that the stores have a whole group to complete.
// Requirements (launcher): scale_bits 7..16 (cum2sym), u8 symbols, chunk_syms % 64 == 0, 64-byte aligned output,
// every chunk full (a ragged last chunk goes through the staged kernel in a second launch).
// ---------------------------------------------------------------------------
constexpr uint32_t kR64RingStride = 2 * kLaneLine + 8; // 128-byte ring + mirror of its first dword (+ 4 pad)
constexpr uint32_t kR64WaveLds = 64 * kR64RingStride;

// Registers of the trip loop: v[8:23] packed symbols of the trip (set g = group g = piece g of the lane's line),
// v[24:39] parked pieces (set t = fetch instruction t), v[40:41] state 0, v[42:43] state 1, v[44:45] window,
// v46..v62 temporaries, v[64:67] ring addresses of the parked pieces; s[36:39] renormalisation masks,
// s[40:47] lanes with a parked piece per fetch instruction, s50 "not the first trip".
//
// One pair of symbols, first half: slots, cum2sym, records (rans64.h:286-292 for both states)
#define R64_LOOKUP                                                                                                      \
    "v_and_b32 v46, %[maskv], v40\n\t"                                                                                  \
    "v_and_b32 v47, %[maskv], v42\n\t"                                                                                  \
    "ds_read_u8 v48, v46\n\t"                                                                                           \
    "ds_read_u8 v49, v47\n\t"                                                                                           \
    "v_lshrrev_b64 v[50:51], %[sbv], v[40:41]\n\t"                                                                      \
    "v_lshrrev_b64 v[52:53], %[sbv], v[42:43]\n\t"                                                                      \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                          \
    "v_lshl_add_u32 v62, v48, 3, %[t1v]\n\t"                                                                            \
    "v_lshl_add_u32 v63, v49, 3, %[t1v]\n\t"                                                                            \
    "ds_read_b64 v[54:55], v62\n\t"                                                                                     \
    "ds_read_b64 v[56:57], v63\n\t"
// second half: x = freq * (x >> scale_bits) + slot - start, renormalisation (rans64.h:305-316: x < 2^31 -> x = x << 32
// | next dword) from the window under an exec mask, window re-read by the lanes that took from it
#define R64_UPDATE                                                                                                      \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                          \
    "v_sub_u32 v58, v46, v55\n\t"                                                                                       \
    "v_mul_u32_u24 v59, v54, v51\n\t"           /* freq * (q >> 32): freq <= 2^16, q >> 32 < 2^24 */                    \
    "v_mad_u64_u32 v[40:41], vcc, v50, v54, v[58:59]\n\t"                                                               \
    "v_cmpx_gt_u64 s[36:37], %[kL], v[40:41]\n\t"                                                                       \
    "v_mov_b32 v41, v40\n\t"                                                                                            \
    "v_mov_b32 v40, v44\n\t"                                                                                            \
    "v_mov_b32 v44, v45\n\t"                                                                                            \
    "v_add_u32 %[cur], 4, %[cur]\n\t"                                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                                            \
    "v_sub_u32 v60, v47, v57\n\t"                                                                                       \
    "v_mul_u32_u24 v61, v56, v53\n\t"                                                                                   \
    "v_mad_u64_u32 v[42:43], vcc, v52, v56, v[60:61]\n\t"                                                               \
    "v_cmpx_gt_u64 s[38:39], %[kL], v[42:43]\n\t"                                                                       \
    "v_mov_b32 v43, v42\n\t"                                                                                            \
    "v_mov_b32 v42, v44\n\t"                                                                                            \
    "v_add_u32 %[cur], 4, %[cur]\n\t"                                                                                   \
    "s_or_b64 exec, s[36:37], s[38:39]\n\t"                                                                             \
    "v_and_b32 v62, 0x7f, %[cur]\n\t"                                                                                   \
    "v_add_u32 v62, %[row], v62\n\t"                                                                                    \
    "ds_read2_b32 v[44:45], v62 offset1:1\n\t"                                                                          \
    "s_mov_b64 exec, -1\n\t"
// four symbols into one dword of the trip's output
#define R64_QUAD(PK)                                                                                                    \
    R64_LOOKUP "v_lshl_or_b32 " PK ", v49, 8, v48\n\t" R64_UPDATE                                                       \
    R64_LOOKUP "v_lshl_or_b32 " PK ", v48, 16, " PK "\n\tv_lshl_or_b32 " PK ", v49, 24, " PK "\n\t" R64_UPDATE
#define R64_GROUP(P0, P1, P2, P3) R64_QUAD(P0) R64_QUAD(P1) R64_QUAD(P2) R64_QUAD(P3)
// Round 3, the same pair of symbols with ONE gather each: a 4-byte slot record {freq:12 | slot - start:12 | sym:8} per
// cumulative slot (the layout rans_word_sse41.h:64-72 uses for the word format, applied to rans64's tables; it holds every
// model whose largest frequency is below 4096 -- at 14 bits every model whose most probable symbol stays below 25 %), at LDS
// address 4 * slot.  One LDS round trip per pair of symbols instead of two dependent ones, one gather instead of two
// (the LDS pipe was 74 % busy, half of it bank conflicts of the two gathers); one more VALU instruction per symbol.
#define R64P_LOOKUP                                                                                                     \
    "v_and_b32 v46, %[maskv], v40\n\t"                                                                                  \
    "v_and_b32 v47, %[maskv], v42\n\t"                                                                                  \
    "v_lshlrev_b32 v46, 2, v46\n\t"                                                                                     \
    "v_lshlrev_b32 v47, 2, v47\n\t"                                                                                     \
    "ds_read_b32 v54, v46\n\t"                                                                                          \
    "ds_read_b32 v56, v47\n\t"                                                                                          \
    "v_lshrrev_b64 v[50:51], %[sbv], v[40:41]\n\t"                                                                      \
    "v_lshrrev_b64 v[52:53], %[sbv], v[42:43]\n\t"
// PACK: the instruction(s) that put the two symbols (top bytes of v54, v56) into the trip's output dword
#define R64P_UPDATE(PACK)                                                                                               \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                          \
    PACK                                                                                                                \
    "v_and_b32 v48, %[m12v], v54\n\t"                                                                                   \
    "v_bfe_u32 v58, v54, 12, 12\n\t"                                                                                    \
    "v_mul_u32_u24 v59, v48, v51\n\t"                                                                                   \
    "v_mad_u64_u32 v[40:41], vcc, v50, v48, v[58:59]\n\t"                                                               \
    "v_cmpx_gt_u64 s[36:37], %[kL], v[40:41]\n\t"                                                                       \
    "v_mov_b32 v41, v40\n\t"                                                                                            \
    "v_mov_b32 v40, v44\n\t"                                                                                            \
    "v_mov_b32 v44, v45\n\t"                                                                                            \
    "v_add_u32 %[cur], 4, %[cur]\n\t"                                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                                            \
    "v_and_b32 v49, %[m12v], v56\n\t"                                                                                   \
    "v_bfe_u32 v60, v56, 12, 12\n\t"                                                                                    \
    "v_mul_u32_u24 v61, v49, v53\n\t"                                                                                   \
    "v_mad_u64_u32 v[42:43], vcc, v52, v49, v[60:61]\n\t"                                                               \
    "v_cmpx_gt_u64 s[38:39], %[kL], v[42:43]\n\t"                                                                       \
    "v_mov_b32 v43, v42\n\t"                                                                                            \
    "v_mov_b32 v42, v44\n\t"                                                                                            \
    "v_add_u32 %[cur], 4, %[cur]\n\t"                                                                                   \
    "s_or_b64 exec, s[36:37], s[38:39]\n\t"                                                                             \
    "v_and_b32 v62, 0x7f, %[cur]\n\t"                                                                                   \
    "v_add_u32 v62, %[row], v62\n\t"                                                                                    \
    "ds_read2_b32 v[44:45], v62 offset1:1\n\t"                                                                          \
    "s_mov_b64 exec, -1\n\t"
#define R64P_QUAD(PK)                                                                                                   \
    R64P_LOOKUP R64P_UPDATE("v_perm_b32 " PK ", v56, v54, %[selA]\n\t")                                                 \
    R64P_LOOKUP R64P_UPDATE("v_perm_b32 v63, v56, v54, %[selB]\n\tv_or_b32 " PK ", " PK ", v63\n\t")
#define R64P_GROUP(P0, P1, P2, P3) R64P_QUAD(P0) R64P_QUAD(P1) R64P_QUAD(P2) R64P_QUAD(P3)
// parked pieces -> ring.  Lane 4k+m holds piece m of the line of lane 4k+t (fetch instruction t): it goes to that
// lane's row, rq0 + 136 t + slot (rq0 = own row - 136 m + 16 m); piece 0 of slot 0 also refreshes the mirror dword.
#define R64_COMMIT                                                                                                      \
    "s_waitcnt vmcnt(0)\n\t" \
    "s_mov_b64 exec, s[40:41]\n\t" \
    "ds_write2_b64 v64, v[24:25], v[26:27] offset0:0 offset1:1\n\t" \
    "s_and_b64 exec, exec, %[m0]\n\t" \
    "v_cmpx_eq_u32 vcc, %[rq0], v64\n\t" \
    "ds_write_b32 %[rq0], v24 offset:128\n\t" \
    "s_mov_b64 exec, s[42:43]\n\t" \
    "ds_write2_b64 v65, v[28:29], v[30:31] offset0:17 offset1:18\n\t" \
    "s_and_b64 exec, exec, %[m0]\n\t" \
    "v_cmpx_eq_u32 vcc, %[rq0], v65\n\t" \
    "ds_write_b32 %[rq0], v28 offset:264\n\t" \
    "s_mov_b64 exec, s[44:45]\n\t" \
    "ds_write2_b64 v66, v[32:33], v[34:35] offset0:34 offset1:35\n\t" \
    "s_and_b64 exec, exec, %[m0]\n\t" \
    "v_cmpx_eq_u32 vcc, %[rq0], v66\n\t" \
    "ds_write_b32 %[rq0], v32 offset:400\n\t" \
    "s_mov_b64 exec, s[46:47]\n\t" \
    "ds_write2_b64 v67, v[36:37], v[38:39] offset0:51 offset1:52\n\t" \
    "s_and_b64 exec, exec, %[m0]\n\t" \
    "v_cmpx_eq_u32 vcc, %[rq0], v67\n\t" \
    "ds_write_b32 %[rq0], v36 offset:536\n\t" \
    "s_mov_b64 exec, -1\n\t"
// bytes staged ahead in v46 -> lanes with room for their next line (<= 64 ahead) ask for it: ld advances, the quad
// fetches (a = ld of the quad's lane t + 16 m by DPP; the sign bit marks "nothing asked")
#define R64_FETCH                                                                                                       \
    "v_bfrev_b32 v63, 1\n\t" \
    "v_cmp_ge_i32 vcc, 64, v46\n\t" \
    "v_cndmask_b32 v47, v63, %[ld], vcc\n\t" \
    "s_mov_b64 exec, vcc\n\t" \
    "v_add_u32 %[ld], 64, %[ld]\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "s_nop 4\n\t" \
    "v_add_u32_dpp v64, v47, %[l16] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_u32_dpp v65, v47, %[l16] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_u32_dpp v66, v47, %[l16] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_u32_dpp v67, v47, %[l16] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cmpx_le_i32 s[40:41], 0, v64\n\t" \
    "buffer_load_dwordx4 v[24:27], v64, %[rsrc], 0 offen nt\n\t" \
    "v_and_b32 v64, 64, v64\n\t" \
    "v_add_u32 v64, %[rq0], v64\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "v_cmpx_le_i32 s[42:43], 0, v65\n\t" \
    "buffer_load_dwordx4 v[28:31], v65, %[rsrc], 0 offen nt\n\t" \
    "v_and_b32 v65, 64, v65\n\t" \
    "v_add_u32 v65, %[rq0], v65\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "v_cmpx_le_i32 s[44:45], 0, v66\n\t" \
    "buffer_load_dwordx4 v[32:35], v66, %[rsrc], 0 offen nt\n\t" \
    "v_and_b32 v66, 64, v66\n\t" \
    "v_add_u32 v66, %[rq0], v66\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "v_cmpx_le_i32 s[46:47], 0, v67\n\t" \
    "buffer_load_dwordx4 v[36:39], v67, %[rsrc], 0 offen nt\n\t" \
    "v_and_b32 v67, 64, v67\n\t" \
    "v_add_u32 v67, %[rq0], v67\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "s_nop 4\n\t"
// a group boundary: the ring's invariant is >= 48 bytes ahead here (N: the boundary's number within its statement, for the label)
#define R64_BOUNDARY(N)                                                                                                 \
    "v_sub_u32 v46, %[ld], %[cur]\n\t"                                                                                  \
    "v_cmp_gt_i32 vcc, 48, v46\n\t"                                                                                     \
    "s_cbranch_vccz .Lr64ok" N "_%=\n\t"                                                                                \
    /* side path (some lane is about to starve): everybody with room asks now, and we wait */                          \
    R64_FETCH R64_COMMIT                                                                                                \
    "v_sub_u32 v46, %[ld], %[cur]\n\t"                                                                                  \
    ".Lr64ok" N "_%=:\n\t" R64_FETCH
// LINES lines fetched and committed at once, a statement of its own (the opening's two, the one ahead of a tail group); the
// names are the kernels' own: ld, cur, l16, rq0, m0, rsrc4
#define R64_ASK "v_sub_u32 v46, %[ld], %[cur]\n\t" R64_FETCH R64_COMMIT
#define R64_FETCH_NOW(LINES)                                                                                            \
    asm volatile(LINES "s_waitcnt lgkmcnt(0)"                                                                           \
                 : [ld] "+v"(ld)                                                                                        \
                 : [cur] "v"(cur), [l16] "v"(l16), [rq0] "v"(rq0), [m0] "s"(m0), [rsrc] "s"(rsrc4)                      \
                 : R64_CLOBBERS)
// 4 x 4 transpose of 16-byte pieces inside every quad: lane 4k+m, set t  <->  lane 4k+t, set m
#define R64_TRANSPOSE                                                                                                   \
    "v_mov_b32 v46, v8\n\t" \
    "v_mov_b32 v47, v9\n\t" \
    "v_mov_b32 v48, v10\n\t" \
    "v_mov_b32 v49, v11\n\t" \
    "v_mov_b32 v50, v16\n\t" \
    "v_mov_b32 v51, v17\n\t" \
    "v_mov_b32 v52, v18\n\t" \
    "v_mov_b32 v53, v19\n\t" \
    "s_mov_b32 vcc_lo, 0x55555555\n\t" \
    "s_mov_b32 vcc_hi, 0x55555555\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_dpp v8, v12, v8, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v9, v13, v9, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v10, v14, v10, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v11, v15, v11, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v16, v20, v16, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v17, v21, v17, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v18, v22, v18, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v19, v23, v19, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t" \
    "s_mov_b32 vcc_lo, 0xaaaaaaaa\n\t" \
    "s_mov_b32 vcc_hi, 0xaaaaaaaa\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_dpp v12, v46, v12, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v13, v47, v13, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v14, v48, v14, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v15, v49, v15, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v20, v50, v20, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v21, v51, v21, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v22, v52, v22, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v23, v53, v23, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_mov_b32 v46, v8\n\t" \
    "v_mov_b32 v47, v9\n\t" \
    "v_mov_b32 v48, v10\n\t" \
    "v_mov_b32 v49, v11\n\t" \
    "v_mov_b32 v50, v12\n\t" \
    "v_mov_b32 v51, v13\n\t" \
    "v_mov_b32 v52, v14\n\t" \
    "v_mov_b32 v53, v15\n\t" \
    "s_mov_b32 vcc_lo, 0x33333333\n\t" \
    "s_mov_b32 vcc_hi, 0x33333333\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_dpp v8, v16, v8, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v9, v17, v9, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v10, v18, v10, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v11, v19, v11, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v12, v20, v12, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v13, v21, v13, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v14, v22, v14, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v15, v23, v15, vcc quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "s_mov_b32 vcc_lo, 0xcccccccc\n\t" \
    "s_mov_b32 vcc_hi, 0xcccccccc\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_dpp v16, v46, v16, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v17, v47, v17, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v18, v48, v18, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v19, v49, v19, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v20, v50, v20, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v21, v51, v21, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v22, v52, v22, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_dpp v23, v53, v23, vcc quad_perm:[2,3,2,3] row_mask:0xf bank_mask:0xf\n\t"
// store instruction t: the line of chunk (quad, t), 16 bytes per lane of the quad
#define R64_STORES                                                                                                      \
    "s_mov_b64 exec, %[vq0]\n\t" \
    "global_store_dwordx4 %[at0], v[8:11], off\n\t" \
    "s_mov_b64 exec, %[vq1]\n\t" \
    "global_store_dwordx4 %[at1], v[12:15], off\n\t" \
    "s_mov_b64 exec, %[vq2]\n\t" \
    "global_store_dwordx4 %[at2], v[16:19], off\n\t" \
    "s_mov_b64 exec, %[vq3]\n\t" \
    "global_store_dwordx4 %[at3], v[20:23], off\n\t" \
    "s_mov_b64 exec, -1\n\t" \
    "v_lshl_add_u64 %[at0], %[at0], 0, 64\n\t" \
    "v_lshl_add_u64 %[at1], %[at1], 0, 64\n\t" \
    "v_lshl_add_u64 %[at2], %[at2], 0, 64\n\t" \
    "v_lshl_add_u64 %[at3], %[at3], 0, 64\n\t"
// Paired stores (round 5): a trip leaves 64 bytes per chunk -- HALF a 128-byte line of L2 -- and the other half followed a
// whole trip later, by when the line could have left L2 half written (WRITE_SIZE 1.34 x the symbols).
// Now the transposed pieces of every other trip wait in v68..v83 and the pair goes out together: instruction t writes
// bytes [0, 64) and [64, 128) of chunk (quad, t)'s line back to back.
#define R64_HOLD                                                                                                        \
    "v_mov_b32 v68, v8\n\tv_mov_b32 v69, v9\n\tv_mov_b32 v70, v10\n\tv_mov_b32 v71, v11\n\t"                             \
    "v_mov_b32 v72, v12\n\tv_mov_b32 v73, v13\n\tv_mov_b32 v74, v14\n\tv_mov_b32 v75, v15\n\t"                           \
    "v_mov_b32 v76, v16\n\tv_mov_b32 v77, v17\n\tv_mov_b32 v78, v18\n\tv_mov_b32 v79, v19\n\t"                           \
    "v_mov_b32 v80, v20\n\tv_mov_b32 v81, v21\n\tv_mov_b32 v82, v22\n\tv_mov_b32 v83, v23\n\t"
#define R64_STORES2                                                                                                     \
    "s_mov_b64 exec, %[vq0]\n\t"                                                                                        \
    "global_store_dwordx4 %[at0], v[68:71], off\n\t"                                                                    \
    "global_store_dwordx4 %[at0], v[8:11], off offset:64\n\t"                                                           \
    "s_mov_b64 exec, %[vq1]\n\t"                                                                                        \
    "global_store_dwordx4 %[at1], v[72:75], off\n\t"                                                                    \
    "global_store_dwordx4 %[at1], v[12:15], off offset:64\n\t"                                                          \
    "s_mov_b64 exec, %[vq2]\n\t"                                                                                        \
    "global_store_dwordx4 %[at2], v[76:79], off\n\t"                                                                    \
    "global_store_dwordx4 %[at2], v[16:19], off offset:64\n\t"                                                          \
    "s_mov_b64 exec, %[vq3]\n\t"                                                                                        \
    "global_store_dwordx4 %[at3], v[80:83], off\n\t"                                                                    \
    "global_store_dwordx4 %[at3], v[20:23], off offset:64\n\t"                                                          \
    "s_mov_b64 exec, -1\n\t"                                                                                            \
    "v_lshl_add_u64 %[at0], %[at0], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at1], %[at1], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at2], %[at2], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at3], %[at3], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at0], %[at0], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at1], %[at1], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at2], %[at2], 0, 64\n\t"                                                                          \
    "v_lshl_add_u64 %[at3], %[at3], 0, 64\n\t"
// s50 = trips decoded and not stored yet (0, 1: in v8..v23, 2: the older one transposed in v68..v83).  At the top of a trip:
#define R64_TRIP_TOP                                                                                                    \
    "s_cmp_eq_u32 s50, 0\n\t"                                                                                           \
    "s_cbranch_scc1 .Lr64first_%=\n\t" R64_TRANSPOSE                                                                    \
    "s_cmp_eq_u32 s50, 1\n\t"                                                                                           \
    "s_cbranch_scc1 .Lr64hold_%=\n\t" R64_STORES2                                                                       \
    "s_mov_b32 s50, 0\n\t"                                                                                              \
    "s_branch .Lr64first_%=\n\t"                                                                                        \
    ".Lr64hold_%=:\n\t" R64_HOLD ".Lr64first_%=:\n\t"
#define R64_TRIP_END                                                                                                    \
    "s_add_u32 s50, s50, 1\n\t"
#define R64_LAST                                                                                                        \
    R64_TRANSPOSE                                                                                                       \
    "s_cmp_eq_u32 s50, 2\n\t"                                                                                           \
    "s_cbranch_scc1 .Lr64pair_%=\n\t" R64_STORES                                                                        \
    "s_branch .Lr64done_%=\n\t"                                                                                         \
    ".Lr64pair_%=:\n\t" R64_STORES2 ".Lr64done_%=:\n\t"
#define R64_HOLD_CLOBBERS , "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83"
#define R64_CLOBBERS                                                                                                    \
    "vcc", "scc", "memory", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21",   \
        "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", \
        "v39", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", \
        "v62", "v63", "v64", "v65", "v66", "v67", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", \
        "s47", "s50"

// The window of a wave's sixty-four streams onto the container, a buffer resource at the line of the lowest one: offsets from
// rb, reads past the last 16-byte granule return 0.  Lanes 2^30 bytes and more beyond rb wait for another pass (`again`) and
// are not valid in this one.  Declares rb and rsrc4; the other names are the kernels' own.  (A macro: as a forceinline helper
// taking references it costs both kernels their code -- 1 and 3 instructions less, 2 VGPRs less in the ragged one, not equal:
// profiles/batch_families_isa.md.)
#define R64_WINDOW                                                                                                      \
    const uint64_t rb = wave_min_offset(off, valid) & ~uint64_t(kLaneLine - 1);                                         \
    const bool far = valid && off - rb >= (1u << 30);                                                                   \
    again = __builtin_amdgcn_ballot_w64(far);                                                                           \
    valid = valid && !far;                                                                                              \
    const uint64_t span = cbytes16 - (rb < cbytes16 ? rb : cbytes16);                                                   \
    const uint32_t nrec = uniform((uint32_t)(span < 0x7ffffff0ull ? span : 0x7ffffff0ull));                             \
    const uint64_t wbase = uniform64(cbase + rb);                                                                       \
    const u32x4 rsrc4 = {uniform((uint32_t)wbase), uniform((uint32_t)(wbase >> 32)) & 0xffffu, nrec, 0x00020000u}

template <bool PACKED> __global__ void __launch_bounds__(1024) k_decode_lanes_r64x2(const DecParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u;
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u;
    // (groups_common.hpp's stage_table and reset_for_next_launch, written out: with either helper the claim loop's set-up is laid
    // out differently, 7 instructions more in both instantiations -- profiles/batch_families_isa.md.  The ragged kernel below
    // calls them.)
    {
        const uint4 *g0 = reinterpret_cast<const uint4 *>(p.table0);
        uint4 *l0 = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < t0_bytes / 16u; i += blockDim.x)
            l0[i] = g0[i];
        const uint4 *g1 = reinterpret_cast<const uint4 *>(p.table1);
        uint4 *l1 = reinterpret_cast<uint4 *>(smem + t0_bytes);
        for (uint32_t i = threadIdx.x; i < t1_bytes / 16u; i += blockDim.x)
            l1[i] = g1[i];
    }
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // the asm addresses LDS by raw offsets
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    if (p.work_counter_reset && blockIdx.x == 0 && threadIdx.x < kWorkPools)
        p.work_counter_reset[threadIdx.x * kWorkPoolStride] = 0u;
    if (p.span_reset && blockIdx.x == 0 && threadIdx.x < 2)
        p.span_reset[threadIdx.x] = 0ull;

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t row = t0_bytes + t1_bytes + wave * kR64WaveLds + lane * kR64RingStride; // LDS byte offset
    const uint32_t m = lane & 3u;
    const uint32_t rq0 = row - m * kR64RingStride + m * 16u; // piece m in the row of the quad's lane 0
    const uint32_t l16 = m * 16u;
    const uint8_t *rowp = smem + row;
    uint32_t maskv = (1u << p.scale_bits) - 1u, sbv = p.scale_bits, t1v = t0_bytes;
    asm volatile("v_mov_b32 %0, %0" : "+v"(maskv)); // VGPR copies: a VALU op with an SGPR operand issues slower
    asm volatile("v_mov_b32 %0, %0" : "+v"(sbv));
    asm volatile("v_mov_b32 %0, %0" : "+v"(t1v));
    uint32_t m12v = 0xfffu;
    asm volatile("v_mov_b32 %0, %0" : "+v"(m12v));
    (void)m12v;
    const uint64_t kL = 1ull << 31;
    const uint64_t m0 = 0x1111111111111111ull; // lane 0 of every quad

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t cbytes16 = (p.container_bytes + 15u) & ~uint64_t(15);
    uint32_t nbad = 0;
    const uint64_t nbatches = (p.nchunks + 63u) / 64u;
    const uint64_t total_waves = (uint64_t)gridDim.x * waves_per_block;
    uint64_t again = 0; // lanes of the batch in hand whose chunks lay beyond the last trip's window (wave_min_offset)
    for (uint64_t batch_v = (uint64_t)blockIdx.x * waves_per_block + wave; batch_v < nbatches; batch_v += again ? 0 : total_waves) {
        const uint64_t batch = uniform64(batch_v);
        const uint64_t chunk = batch * 64u + lane;
        bool valid = chunk < p.nchunks && (again == 0 || ((again >> lane) & 1u));
        const uint64_t off = valid ? p.offsets[chunk] : 0;
        const uint32_t len = valid ? p.lengths[chunk] : 0;
        if (valid && ((off & 3u) != 0 || len < 16u || off > p.container_bytes || len > p.container_bytes - off)) {
            nbad++;
            valid = false;
        }
        R64_WINDOW;
        // store addresses: instruction t writes the line of the quad's lane t, this lane its piece m
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + chunk * p.chunk_syms;
        uint64_t at[4], vq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int src = (int)((lane & ~3u) + t);
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)dst, src), hi = (uint32_t)__shfl((int)(uint32_t)(dst >> 32), src);
            at[t] = (((uint64_t)hi << 32) | lo) + l16;
            vq[t] = __builtin_amdgcn_ballot_w64(__shfl((int)valid, src) != 0);
        }

        uint32_t cur = valid ? (uint32_t)(off - rb) : 0u; // position in the batch's window (ring index = cur & 127)
        const uint32_t cur0 = cur;
        uint32_t ld = valid ? (cur & ~(kLaneLine - 1u)) : 0x40000000u; // next line not yet requested (never, without a chunk)
        // opening: the first two lines (the states are the first 16 bytes of the stream, rans64.h:251-262)
        R64_FETCH_NOW(R64_ASK R64_ASK);
        uint64_t xA, xB, win;
        {
            const u32x2 a = *reinterpret_cast<const u32x2 *>(rowp + (cur & 127u));
            const u32x2 b = *reinterpret_cast<const u32x2 *>(rowp + ((cur + 8u) & 127u));
            xA = (uint64_t)a.x | ((uint64_t)a.y << 32);
            xB = (uint64_t)b.x | ((uint64_t)b.y << 32);
            cur += 16u;
            const uint32_t w0 = *reinterpret_cast<const uint32_t *>(rowp + (cur & 127u));
            const uint32_t w1 = *reinterpret_cast<const uint32_t *>(rowp + ((cur + 4u) & 127u));
            win = (uint64_t)w0 | ((uint64_t)w1 << 32);
        }
        uint32_t trips = uniform(p.chunk_syms >> 6);
        // every trip of the chunk in one statement; GROUP and its own operands (...) are what the two slot layouts differ in
#define R64_ALL_TRIPS(GROUP, ...)                                                                                       \
    asm volatile("s_mov_b64 s[40:41], 0\n\t"                                                                            \
                 "s_mov_b64 s[42:43], 0\n\t"                                                                            \
                 "s_mov_b64 s[44:45], 0\n\t"                                                                            \
                 "s_mov_b64 s[46:47], 0\n\t"                                                                            \
                 "s_mov_b32 s50, 0\n\t"                                                                                 \
                 ".Lr64trip_%=:\n\t"                                                                                    \
                 R64_COMMIT                                                                                             \
                 R64_TRIP_TOP                                                                                           \
                 R64_BOUNDARY("0") GROUP("v8", "v9", "v10", "v11")                                                      \
                 R64_COMMIT R64_BOUNDARY("1") GROUP("v12", "v13", "v14", "v15")                                         \
                 R64_COMMIT R64_BOUNDARY("2") GROUP("v16", "v17", "v18", "v19")                                         \
                 R64_COMMIT R64_BOUNDARY("3") GROUP("v20", "v21", "v22", "v23")                                         \
                 R64_TRIP_END                                                                                           \
                 "s_sub_u32 %[trips], %[trips], 1\n\t"                                                                  \
                 "s_cmp_lg_u32 %[trips], 0\n\t"                                                                         \
                 "s_cbranch_scc1 .Lr64trip_%=\n\t"                                                                      \
                 R64_LAST                                                                                               \
                 "s_waitcnt vmcnt(0) lgkmcnt(0)"                                                                        \
                 : "+{v[40:41]}"(xA), "+{v[42:43]}"(xB), "+{v[44:45]}"(win), [cur] "+v"(cur), [ld] "+v"(ld), [at0] "+v"(at[0]),       \
                   [at1] "+v"(at[1]), [at2] "+v"(at[2]), [at3] "+v"(at[3]), [trips] "+s"(trips)                         \
                 : [maskv] "v"(maskv), [sbv] "v"(sbv), __VA_ARGS__, [row] "v"(row), [l16] "v"(l16), [rq0] "v"(rq0),     \
                   [kL] "s"(kL), [m0] "s"(m0), [vq0] "s"(vq[0]), [vq1] "s"(vq[1]), [vq2] "s"(vq[2]), [vq3] "s"(vq[3]),  \
                   [rsrc] "s"(rsrc4)                                                                                    \
                 : R64_CLOBBERS R64_HOLD_CLOBBERS)
        if constexpr (PACKED)
            R64_ALL_TRIPS(R64P_GROUP, [m12v] "v"(m12v), [selA] "s"(0x0c0c0703u), [selB] "s"(0x07030c0cu));
        else
            R64_ALL_TRIPS(R64_GROUP, [t1v] "v"(t1v));
#undef R64_ALL_TRIPS
        // RansDec end state: both states back at L, every byte of the chunk consumed (main64.cpp has no check; ours)
        if (valid && (xA != kL || xB != kL || cur - cur0 != len))
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
}

// ---------------------------------------------------------------------------
// k_decode_batch_r64_lanes -- the ragged form of k_decode_lanes_r64x2 (rans_amd_decode_batch under
// RANS_AMD_OPT_BATCH_LANES): a wave's sixty-four lanes hold sixty-four STREAMS of the reference's 2-way rans64 layout
// (main64.cpp:224-287), each with its own symbol count, output address, stream offset and length.  The unit of work is
// one wave-load of the hand-out order, claimed through the work counter: lane l of claim k holds stream
// order[64 k + l] -- 64 k + l without an order; a position at or past nchunks has no stream.  The rings (128 bytes +
// mirror per lane, rows 136 bytes apart), the quad fetches through the wave's buffer window, the commit of the parked
// pieces, the pair of symbols and the group of sixteen are k_decode_lanes_r64x2's, macro for macro; the ring's invariant
// is its invariant (>= 48 bytes ahead at a group boundary, the side path for a lane below that).  What is new:
//   * ONE TRIP (64 symbols) is one asm statement, not the whole loop: the wave runs it max_l(count_l >> 6) times, and
//     between two trips nothing is in flight (the trip ends with the commit of the pieces its last group asked for), so
//     the compiler's code between them sees plain registers.  That costs the uniform kernel's overlap of a trip's stores
//     and last fetch with the next trip's first group; other waves of the SIMD cover it.
//   * a lane whose stream has run out of whole trips -- or that has no stream -- is PARKED: the statement runs under full
//     exec (its DPP moves read the quad's other lanes), so the lane free-runs on whatever its state becomes.  That reads
//     LDS only: cum2sym at x & mask, inside table 0; a record at table 1 + 8 s with s a byte of cum2sym, a symbol of
//     the model; its own ring row at (cursor & 127) and the mirror dword behind it.  It requests no line: for the trip
//     its "next line" is put 2^29 bytes ahead of its cursor, so neither the fetch's test (<= 64 ahead) nor the side
//     path's (< 48 ahead) sees it, and a quad fetches for a member only what that member asked for.  Behind the trip its
//     states, window, cursor and next line are put back from copies: its ring holds what it held, its tail reads the
//     right bytes.  Its 64 bytes are not stored.
//   * stores: a lane whose output is 64-byte aligned has its line written by its quad (transpose, then instruction t
//     writes the line of the quad's lane t under "this trip < the trips of lane t": the uniform kernel's vq masks, per
//     trip); a lane on the 4-byte grid writes its own four 16-byte pieces, any other lane 64 bytes one by one -- before
//     the transpose, from its own registers.  rans_amd_batch_layout with sym_align = 64 is the fast layout.
//   * the tail: count & 63 symbols in groups of sixteen, compiler-scheduled, a pair at a time and the odd last symbol on
//     state 0 (main64.cpp's loops: i < (n & ~1) in pairs, then rans0); every group follows a fetch + commit of its own
//     (synchronous, the side path's), so it never relies on a line a parked lane did not request.  Byte stores.
//   * the window: a buffer resource at the line of the wave-load's lowest stream, lanes 2^30 bytes and more beyond it wait
//     for another pass over the same claim (`again`), as in the uniform kernel; reads behind the container's last 16-byte
//     granule return 0.  Ring positions are 32-bit: a stream longer than 2^30 bytes is counted as failed here.
// Index entries are the caller's data: the order entry names a stream, the offset is on the 4-byte grid, the stream holds
// its two states and lies inside the container, the symbol range lies inside [0, out_syms) -- a stream that fails any of
// these is counted once, nothing of it is fetched, nothing stored.  Behind the last symbol both states are 2^31 and the
// cursor stands at the stream's end, else the stream is counted.
// ---------------------------------------------------------------------------
// (R64_CLOBBERS without the sixteen output registers, which are operands here, and without s50)
#define R64B_CLOBBERS                                                                                                   \
    "vcc", "scc", "memory", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", \
        "v38", "v39", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", \
        "v61", "v62", "v63", "v64", "v65", "v66", "v67", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", \
        "s46", "s47"
typedef uint32_t lanes_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes on the 4-byte grid

__global__ void __launch_bounds__(1024) k_decode_batch_r64_lanes(const DecParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long t_start = p.span ? wall_clock64() : 0ull;
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u; // cum2sym u8[M]
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u; // {freq, start}[nsyms]
    stage_table(smem, p.table0, t0_bytes);
    stage_table(smem + t0_bytes, p.table1, t1_bytes);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // the asm addresses LDS by raw offsets
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);
    DecTables<FMT_R64> T; // the tail's compiler-scheduled steps
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t row = t0_bytes + t1_bytes + wave * kR64WaveLds + lane * kR64RingStride; // LDS byte offset
    const uint32_t m = lane & 3u;
    const uint32_t rq0 = row - m * kR64RingStride + m * 16u; // piece m in the row of the quad's lane 0
    const uint32_t l16 = m * 16u;
    const uint8_t *rowp = smem + row;
    uint32_t maskv = (1u << p.scale_bits) - 1u, sbv = p.scale_bits, t1v = t0_bytes;
    asm volatile("v_mov_b32 %0, %0" : "+v"(maskv)); // VGPR copies: a VALU op with an SGPR operand issues slower
    asm volatile("v_mov_b32 %0, %0" : "+v"(sbv));
    asm volatile("v_mov_b32 %0, %0" : "+v"(t1v));
    const uint64_t kL = 1ull << 31;
    const uint64_t m0 = 0x1111111111111111ull; // lane 0 of every quad
    constexpr uint32_t kParkAhead = 1u << 29;  // a lane that must not ask: its next line this far ahead of its cursor

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t cbytes16 = (p.container_bytes + 15u) & ~uint64_t(15);
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 63u) >> 6); // wave-loads, one per claim; stream indices are 32-bit
    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    uint64_t again = 0; // lanes of the wave-load in hand whose streams lay beyond the last pass's window (wave_min_offset)
    uint64_t load = 0;
    for (;;) {
        if (again == 0) {
            load = work.take(lane);
            if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
                break;
        }
        // ---- this lane's stream: its index entries, all of them the caller's data
        const uint64_t pos = load * 64u + lane;
        // (groups_common.hpp's fetch_stream_entry<16, false> with the 4-byte grid and the 2^30 limit behind it, written out: the
        // helper knows no `again`, so a later pass reads the entries of lanes it skips, and the kernel compiles to another
        // register allocation, 113 VGPRs for 115 -- profiles/batch_families_isa.md.  A fix there has to be made here as well.)
        const bool mine = pos < p.nchunks && (again == 0 || ((again >> lane) & 1u)); // a position this pass looks at
        uint64_t s = pos;
        if (mine && p.order)
            s = p.order[pos];
        bool valid = mine && s < p.nchunks;
        uint64_t off = 0, first = 0;
        uint32_t len = 0, count = 0;
        if (valid) {
            off = p.offsets[s];
            len = p.lengths[s];
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
        }
        valid = valid && (off & 3u) == 0 && len >= 16u && len <= (1u << 30) && off <= p.container_bytes && len <= p.container_bytes - off &&
                first <= p.out_syms && count <= p.out_syms - first;
        if (mine && !valid)
            nbad++; // (a rejected entry is seen in one pass only: it never joins `again`)
        R64_WINDOW;

        // ---- the lane's own counts and where its symbols go ([dst, dst + count) lies inside the output)
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + first;
        const uint32_t trips = valid ? count >> 6 : 0u;
        const uint32_t tail = valid ? count & 63u : 0u;
        const bool by_quad = (dst & 63u) == 0, by_dwords = (dst & 3u) == 0;
        // store instruction t writes the line of the quad's lane t, this lane its piece m -- while that lane has trips left
        const uint32_t qtrips = by_quad ? trips : 0u;
        uint64_t at[4];
        uint32_t tq[4];
        {
            const uint32_t dlo = (uint32_t)dst, dhi = (uint32_t)(dst >> 32);
            at[0] = (((uint64_t)quad_perm<0x00>(dhi) << 32) | quad_perm<0x00>(dlo)) + l16;
            at[1] = (((uint64_t)quad_perm<0x55>(dhi) << 32) | quad_perm<0x55>(dlo)) + l16;
            at[2] = (((uint64_t)quad_perm<0xAA>(dhi) << 32) | quad_perm<0xAA>(dlo)) + l16;
            at[3] = (((uint64_t)quad_perm<0xFF>(dhi) << 32) | quad_perm<0xFF>(dlo)) + l16;
            tq[0] = quad_perm<0x00>(qtrips);
            tq[1] = quad_perm<0x55>(qtrips);
            tq[2] = quad_perm<0xAA>(qtrips);
            tq[3] = quad_perm<0xFF>(qtrips);
        }

        uint32_t cur = valid ? (uint32_t)(off - rb) : 0u; // position in the wave-load's window (ring index = cur & 127)
        const uint32_t cur0 = cur;
        uint32_t ld = valid ? (cur & ~(kLaneLine - 1u)) : kParkAhead; // next line not yet requested (never, without a stream)
        // opening: the first two lines (the states are the first 16 bytes of the stream, rans64.h:251-262)
        R64_FETCH_NOW(R64_ASK R64_ASK);
        uint64_t xA = kL, xB = kL, win = 0;
        if (valid) {
            const u32x2 a = *reinterpret_cast<const u32x2 *>(rowp + (cur & 127u));
            const u32x2 b = *reinterpret_cast<const u32x2 *>(rowp + ((cur + 8u) & 127u));
            xA = (uint64_t)a.x | ((uint64_t)a.y << 32);
            xB = (uint64_t)b.x | ((uint64_t)b.y << 32);
            cur += 16u;
            const uint32_t w0 = *reinterpret_cast<const uint32_t *>(rowp + (cur & 127u));
            const uint32_t w1 = *reinterpret_cast<const uint32_t *>(rowp + ((cur + 4u) & 127u));
            win = (uint64_t)w0 | ((uint64_t)w1 << 32);
        }

        // ---- whole trips: 64 symbols per lane and statement
        for (uint32_t trip = 0; __builtin_amdgcn_ballot_w64(trip < trips) != 0; ++trip) {
            const bool run = trip < trips;
            const uint64_t xA_keep = xA, xB_keep = xB, win_keep = win;
            const uint32_t cur_keep = cur, ld_keep = ld;
            ld = run ? ld : cur + kParkAhead;
            u32x4 q0, q1, q2, q3;
            asm volatile("s_mov_b64 s[40:41], 0\n\t"
                         "s_mov_b64 s[42:43], 0\n\t"
                         "s_mov_b64 s[44:45], 0\n\t"
                         "s_mov_b64 s[46:47], 0\n\t"
                         R64_BOUNDARY("0") R64_GROUP("v8", "v9", "v10", "v11")
                         R64_COMMIT R64_BOUNDARY("1") R64_GROUP("v12", "v13", "v14", "v15")
                         R64_COMMIT R64_BOUNDARY("2") R64_GROUP("v16", "v17", "v18", "v19")
                         R64_COMMIT R64_BOUNDARY("3") R64_GROUP("v20", "v21", "v22", "v23")
                         R64_COMMIT
                         "s_waitcnt lgkmcnt(0)"
                         : "+{v[40:41]}"(xA), "+{v[42:43]}"(xB), "+{v[44:45]}"(win), [cur] "+v"(cur), [ld] "+v"(ld), "=&{v[8:11]}"(q0),
                           "=&{v[12:15]}"(q1), "=&{v[16:19]}"(q2), "=&{v[20:23]}"(q3)
                         : [maskv] "v"(maskv), [sbv] "v"(sbv), [t1v] "v"(t1v), [row] "v"(row), [l16] "v"(l16), [rq0] "v"(rq0),
                           [kL] "s"(kL), [m0] "s"(m0), [rsrc] "s"(rsrc4)
                         : R64B_CLOBBERS);
            xA = run ? xA : xA_keep;
            xB = run ? xB : xB_keep;
            win = run ? win : win_keep;
            cur = run ? cur : cur_keep;
            ld = run ? ld : ld_keep;
            const uint64_t o = (uint64_t)trip << 6;
            if (run && !by_quad) { // the lane's own 64 bytes, from its own registers
                if (by_dwords) {
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o) = q0;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 16u) = q1;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 32u) = q2;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 48u) = q3;
                } else {
                    uint8_t RANS_GLOBAL *d = reinterpret_cast<uint8_t RANS_GLOBAL *>(dst + o);
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        d[j] = (uint8_t)(q0[j >> 2] >> (8 * (j & 3)));
                        d[16 + j] = (uint8_t)(q1[j >> 2] >> (8 * (j & 3)));
                        d[32 + j] = (uint8_t)(q2[j >> 2] >> (8 * (j & 3)));
                        d[48 + j] = (uint8_t)(q3[j >> 2] >> (8 * (j & 3)));
                    }
                }
            }
            quad_transpose(q0, q1, q2, q3, lane); // (full exec: the moves read all four lanes)
            if (trip < tq[0])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[0] + o) = q0;
            if (trip < tq[1])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[1] + o) = q1;
            if (trip < tq[2])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[2] + o) = q2;
            if (trip < tq[3])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[3] + o) = q3;
        }

        // ---- count & 63 symbols: sixteen at a time behind a fetch + commit of their own, straight from the ring
        uint8_t RANS_GLOBAL *tdst = reinterpret_cast<uint8_t RANS_GLOBAL *>(dst + ((uint64_t)trips << 6));
        for (uint32_t j0 = 0; __builtin_amdgcn_ballot_w64(j0 < tail) != 0; j0 += 16u) {
            const bool live = j0 < tail;
            const uint32_t ld_keep = ld;
            ld = live ? ld : cur + kParkAhead;
            R64_FETCH_NOW(R64_ASK);
            ld = live ? ld : ld_keep;
            if (live) {
                const uint32_t cnt = tail - j0 < 16u ? tail - j0 : 16u;
                for (uint32_t i = 0; i < cnt; i += 2u) {
                    const bool two = i + 1u < cnt;
                    tdst[j0 + i] = (uint8_t)dec_step<FMT_R64>(T, xA);
                    if (two)
                        tdst[j0 + i + 1u] = (uint8_t)dec_step<FMT_R64>(T, xB);
                    if (xA < kL) { // rans64.h:305-316, state 0 first
                        xA = (xA << 32) | *reinterpret_cast<const uint32_t *>(rowp + (cur & 127u));
                        cur += 4u;
                    }
                    if (two && xB < kL) {
                        xB = (xB << 32) | *reinterpret_cast<const uint32_t *>(rowp + (cur & 127u));
                        cur += 4u;
                    }
                }
            }
        }
        // RansDec end state: both states back at L, every byte of the stream consumed (main64.cpp has no check; ours)
        if (valid && (xA != kL || xB != kL || cur - cur0 != len))
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
    record_span(p, t_start, smem, threadIdx.x);
}
#undef R64B_CLOBBERS

// ---------------------------------------------------------------------------
// k_decode_batch_singles: the ragged form of k_decode_lanes_staged<FMT, 1> (rans_amd_decode_batch under
// RANS_AMD_OPT_BATCH_SINGLES) -- the NON-INTERLEAVED stream every reference program writes first (main.cpp:173-182,
// main64.cpp:175-184, main_simd.cpp:161-169, main_alias.cpp:300-309), sixty-four STREAMS per wave, one per lane with its one
// state, each with its own symbol count, output address, stream offset and length.  Compiler-scheduled like the staged kernel
// (dec_step, DecTables, LaneRing); the plan is k_decode_batch_r64_lanes', piece by piece:
//   * a unit of work (WorkClaims) is one wave-load of the hand-out order: lane l of claim k holds stream order[64 k + l], or
//     64 k + l without an order; a position at or past nchunks has no stream.
//   * index entries are the caller's data, checked as fetch_stream_entry checks them with the format's own unit and state size
//     (written out for the `again` pass, as in the rans64 kernel: a fix there has to be made here as well): the order entry
//     names a stream, the offset is a multiple of the unit (1 byte/alias, 2 word, 4 rans64), the stream holds its state (4
//     bytes; rans64 8) and lies inside the container, the symbol range lies inside [0, out_syms).  A stream that fails is
//     counted once, nothing of it is fetched, nothing stored.  Ring positions are 32-bit: a stream of more than 2^30 bytes is
//     counted as failed as well -- the one rule the wave-per-stream kernels do not have.
//   * the window: 32-bit positions from the line of the wave-load's lowest valid stream (wave_min_offset); lanes 2^30 bytes and
//     more above it wait for another pass over the same claim (`again`).  Every fetch is compared against the container's end
//     rounded up to 16 bytes: reads behind it yield zeros and never touch memory.  Nothing here reads outside
//     [container, container + container_bytes rounded up to 16) -- the initial state is one load at the stream's own address
//     (unaligned for byte and alias streams, as in the uniform kernel), inside the stream because its length was checked first.
//   * the rings: kLaneWaveLds per wave, a 128-byte ring per lane in rows kLaneRingStride apart, one request word per lane.  The
//     WAVE refills before every group of 16 symbols, under full exec, exactly as the staged kernel does: lanes publish the line
//     they need, quads fetch one lane's 64-byte line with four 16-byte loads.  The invariant is the staged kernel's: at least 64
//     bytes ahead before a group, which is what 16 symbols can take at the most (rans64: 4 bytes per symbol); a VALID stream
//     reaches half of that -- symbols of frequency 1 at 16 bits take 32 bytes per group in the byte, alias and rans64 formats,
//     the word format at its 12 bits 24 (tests/test_batch_singles_host.py) --, so the invariant has 32 bytes to spare.  A lane
//     without a stream, or whose stream has no group in this trip or tail pass, requests nothing.
//   * whole trips: 64 symbols per lane, the wave runs max_l(count_l >> 6) of them, a lane takes part while
//     trip < count >> 6 (plain exec masking: nothing here is asm, so nobody has to be parked).
//   * stores: by the address of a lane's first symbol, as in the rans64 kernel.  On a 64-byte line the quad transposes
//     (quad_transpose, under full exec) and store instruction t writes the line of the quad's lane t under "this trip < the
//     trips of lane t"; on the 4-byte grid the lane writes its own four 16-byte pieces; any other address byte by byte.
//     sym_align = 64 is the fast layout.  Nothing is written outside a validated stream's own [sym_offset, sym_offset + count).
//   * the tail: count & 63 symbols in groups of sixteen, each behind a refill of its own, byte stores.
//   * the verdict: the state is back at the format's L and consumed + state bytes == len, else the stream is counted.
// FMT_ALIAS: the alias decoder's divider + half-bucket records over a power-of-two alphabet of at most 256 u8 symbols, as for
// the alias pairs.  FMT_R64 is the cum2sym form (the search variant is another kernel format and stays on the wave kernel).
// ---------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(1024) k_decode_batch_singles(const DecParams p)
{
    using Tr = FmtTraits<FMT>;
    using state_t = typename Tr::state_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long t_start = p.span ? wall_clock64() : 0ull;
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u;
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u;
    stage_table(smem, p.table0, t0_bytes);
    stage_table(smem + t0_bytes, p.table1, t1_bytes);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // dec_step addresses the first table by raw offsets
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }
    reset_for_next_launch(p);
    DecTables<FMT> T;
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);

    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    uint8_t *rings = smem + t0_bytes + t1_bytes + wave * kLaneWaveLds;
    uint32_t *req = reinterpret_cast<uint32_t *>(rings + 64u * kLaneRingStride);
    const uint32_t part = lane & 3u, grp = lane >> 2;
    const uint32_t l16 = part * 16u;

    const uint64_t cbase = reinterpret_cast<uint64_t>(p.container);
    const uint64_t glimit = cbase + ((p.container_bytes + 15u) & ~uint64_t(15)); // (the container is 16-byte aligned: api.cpp)
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 63u) >> 6); // wave-loads, one per claim; stream indices are 32-bit
    uint32_t nbad = 0;
    WorkClaims work;
    work.init(p.work_counter, wave, waves_per_block);
    uint64_t again = 0; // lanes of the wave-load in hand whose streams lay beyond the last pass's window (wave_min_offset)
    uint64_t load = 0;
    for (;;) {
        if (again == 0) {
            load = work.take(lane);
            if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
                break;
        }
        // ---- this lane's stream: its index entries, all of them the caller's data
        const uint64_t pos = load * 64u + lane;
        const bool mine = pos < p.nchunks && (again == 0 || ((again >> lane) & 1u)); // a position this pass looks at
        uint64_t s = pos;
        if (mine && p.order)
            s = p.order[pos];
        bool valid = mine && s < p.nchunks;
        uint64_t off = 0, first = 0;
        uint32_t len = 0, count = 0;
        if (valid) {
            off = p.offsets[s];
            len = p.lengths[s];
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
        }
        valid = valid && (off & (Tr::kUnit - 1u)) == 0 && len >= Tr::kStateBytes && len <= (1u << 30) && off <= p.container_bytes &&
                len <= p.container_bytes - off && first <= p.out_syms && count <= p.out_syms - first;
        if (mine && !valid)
            nbad++; // (a rejected entry is seen in one pass only: it never joins `again`)
        // the window: the line of the lowest valid stream of this pass
        const uint64_t rb = wave_min_offset(off, valid) & ~uint64_t(kLaneLine - 1);
        const bool far = valid && off - rb >= (1u << 30);
        again = __builtin_amdgcn_ballot_w64(far);
        valid = valid && !far;

        // ---- the lane's own counts and where its symbols go ([dst, dst + count) lies inside the output)
        const uint64_t dst = reinterpret_cast<uint64_t>(p.out) + first;
        const uint32_t trips = valid ? count >> 6 : 0u;
        const uint32_t tail = valid ? count & 63u : 0u;
        const bool by_quad = (dst & 63u) == 0, by_dwords = (dst & 3u) == 0;
        // store instruction t writes the line of the quad's lane t, this lane its piece -- while that lane has trips left
        const uint32_t qtrips = by_quad ? trips : 0u;
        uint64_t at[4];
        uint32_t tq[4];
        {
            const uint32_t dlo = (uint32_t)dst, dhi = (uint32_t)(dst >> 32);
            at[0] = (((uint64_t)quad_perm<0x00>(dhi) << 32) | quad_perm<0x00>(dlo)) + l16;
            at[1] = (((uint64_t)quad_perm<0x55>(dhi) << 32) | quad_perm<0x55>(dlo)) + l16;
            at[2] = (((uint64_t)quad_perm<0xAA>(dhi) << 32) | quad_perm<0xAA>(dlo)) + l16;
            at[3] = (((uint64_t)quad_perm<0xFF>(dhi) << 32) | quad_perm<0xFF>(dlo)) + l16;
            tq[0] = quad_perm<0x00>(qtrips);
            tq[1] = quad_perm<0x55>(qtrips);
            tq[2] = quad_perm<0xAA>(qtrips);
            tq[3] = quad_perm<0xFF>(qtrips);
        }

        // ---- the initial state (RansDecInit): one load at the stream's own address, inside the stream (len was checked)
        state_t x = Tr::kL;
        if (valid) {
            const uint8_t RANS_GLOBAL *src = (const uint8_t RANS_GLOBAL *)p.container + off;
            if constexpr (FMT == FMT_R64) {
                const u32x2 v = *reinterpret_cast<const u32x2 RANS_GLOBAL *>(src);
                x = (uint64_t)v.x | ((uint64_t)v.y << 32);
            } else {
                x = *reinterpret_cast<const uint32_t RANS_GLOBAL *>(src);
            }
        }
        LaneRing<FMT> W;
        W.row = rings + lane * kLaneRingStride;
        W.cur = valid ? (uint32_t)(off - rb) + Tr::kStateBytes : 0u;
        W.used = 0;
        uint32_t ld = W.cur & ~(kLaneLine - 1u); // next line this lane has not staged yet

        // the whole wave takes part (also lanes without a stream, under full exec): lane -> which line its stream needs
        // (live: it has a group to decode behind this refill), then lane (4 g + part) moves 16 bytes of stream (16 j + g)'s
        // line, j = 0..3
        auto refill = [&](bool live) {
            const bool need = live && (int32_t)(ld - W.cur) < (int32_t)kLaneLine;
            req[lane] = need ? (ld | 1u) : 0u;
            if (need)
                ld += kLaneLine;
            uint32_t r[4];
            u32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = req[16 * j + grp]; // LDS ops of one wave execute in order: sees the writes above
                v[j] = u32x4{0u, 0u, 0u, 0u};
                const uint64_t a = cbase + rb + (r[j] & ~(kLaneLine - 1u)) + l16;
                if ((r[j] & 1u) && a < glimit) // behind the container's last 16-byte granule: zeros, no access
                    v[j] = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(a));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r[j] & 1u) {
                    uint8_t *to = rings + (16u * j + grp) * kLaneRingStride + (r[j] & kLaneLine) + l16;
                    reinterpret_cast<u32x2 *>(to)[0] = u32x2{v[j].x, v[j].y}; // rows are 8-byte aligned
                    reinterpret_cast<u32x2 *>(to)[1] = u32x2{v[j].z, v[j].w};
                }
        };
        // 16 symbols into four dwords
        auto decode16 = [&]() -> u32x4 {
            uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                uint32_t sy = dec_step<FMT>(T, x);
                if constexpr (Tr::kSymByte == 3)
                    sy >>= 24;
                pk[k / 4] |= (sy & 0xffu) << (8 * (k % 4));
                W.renorm(x, true);
            }
            return u32x4{pk[0], pk[1], pk[2], pk[3]};
        };

        refill(valid && count != 0u); // two lines ahead before the first group: this one and the group's own

        // ---- whole trips: 64 symbols per lane, four groups of 16 with a refill before each
        for (uint32_t trip = 0; __builtin_amdgcn_ballot_w64(trip < trips) != 0; ++trip) {
            const bool run = trip < trips;
            u32x4 q0 = {0u, 0u, 0u, 0u}, q1 = q0, q2 = q0, q3 = q0;
            refill(run);
            if (run)
                q0 = decode16();
            refill(run);
            if (run)
                q1 = decode16();
            refill(run);
            if (run)
                q2 = decode16();
            refill(run);
            if (run)
                q3 = decode16();
            const uint64_t o = (uint64_t)trip << 6;
            if (run && !by_quad) { // the lane's own 64 bytes, from its own registers
                if (by_dwords) {
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o) = q0;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 16u) = q1;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 32u) = q2;
                    *reinterpret_cast<lanes_u32x4_a4 RANS_GLOBAL *>(dst + o + 48u) = q3;
                } else {
                    uint8_t RANS_GLOBAL *d = reinterpret_cast<uint8_t RANS_GLOBAL *>(dst + o);
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        d[j] = (uint8_t)(q0[j >> 2] >> (8 * (j & 3)));
                        d[16 + j] = (uint8_t)(q1[j >> 2] >> (8 * (j & 3)));
                        d[32 + j] = (uint8_t)(q2[j >> 2] >> (8 * (j & 3)));
                        d[48 + j] = (uint8_t)(q3[j >> 2] >> (8 * (j & 3)));
                    }
                }
            }
            quad_transpose(q0, q1, q2, q3, lane); // (full exec: the moves read all four lanes)
            if (trip < tq[0])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[0] + o) = q0;
            if (trip < tq[1])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[1] + o) = q1;
            if (trip < tq[2])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[2] + o) = q2;
            if (trip < tq[3])
                *reinterpret_cast<u32x4 RANS_GLOBAL *>(at[3] + o) = q3;
        }

        // ---- count & 63 symbols: sixteen at a time behind a refill of their own, byte stores
        uint8_t RANS_GLOBAL *tdst = reinterpret_cast<uint8_t RANS_GLOBAL *>(dst + ((uint64_t)trips << 6));
        for (uint32_t j0 = 0; __builtin_amdgcn_ballot_w64(j0 < tail) != 0; j0 += 16u) {
            const bool live = j0 < tail;
            refill(live);
            if (live) {
                const uint32_t cnt = tail - j0 < 16u ? tail - j0 : 16u;
                for (uint32_t i = 0; i < cnt; ++i) {
                    uint32_t sy = dec_step<FMT>(T, x);
                    if constexpr (Tr::kSymByte == 3)
                        sy >>= 24;
                    tdst[j0 + i] = (uint8_t)sy;
                    W.renorm(x, true);
                }
            }
        }
        // RansDec end state: the state back at L, every byte of the stream consumed (the reference has no check; ours)
        if (valid && (x != Tr::kL || W.used + Tr::kStateBytes != len))
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
    record_span(p, t_start, smem, threadIdx.x);
}

template <int FMT, int NW>
__global__ void __launch_bounds__(256) k_decode_lanes(const DecParams p)
{
    using Tr = FmtTraits<FMT>;
    using state_t = typename Tr::state_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t t0_bytes = (p.table0_bytes + 15u) & ~15u;
    const uint32_t t1_bytes = (p.table1_bytes + 15u) & ~15u;
    {
        const uint4 *g0 = reinterpret_cast<const uint4 *>(p.table0);
        uint4 *l0 = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < t0_bytes / 16u; i += blockDim.x)
            l0[i] = g0[i];
        const uint4 *g1 = reinterpret_cast<const uint4 *>(p.table1);
        uint4 *l1 = reinterpret_cast<uint4 *>(smem + t0_bytes);
        for (uint32_t i = threadIdx.x; i < t1_bytes / 16u; i += blockDim.x)
            l1[i] = g1[i];
    }
    __syncthreads();

    DecTables<FMT> T;
    T.init(smem, smem + t0_bytes, p.scale_bits, p.log2nsyms);
    if (!lds_starts_at_zero(smem)) { // cannot happen without static LDS; never decode on a wrong assumption
        if (threadIdx.x == 0)
            atomicAdd(p.err_count, 1ull << 32);
        return;
    }

    if (p.work_counter_reset && blockIdx.x == 0 && threadIdx.x < kWorkPools)
        p.work_counter_reset[threadIdx.x * kWorkPoolStride] = 0u; // keep the wave kernels' counter ring consistent
    if (p.span_reset && blockIdx.x == 0 && threadIdx.x < 2)
        p.span_reset[threadIdx.x] = 0ull;
    const uint8_t RANS_GLOBAL *cbase = (const uint8_t RANS_GLOBAL *)p.container;
    const uint64_t glimit = (reinterpret_cast<uint64_t>(p.container) + p.container_bytes + 15u) & ~uint64_t(15);
    const bool wide_out = p.sym_bytes == 1 && ((reinterpret_cast<uintptr_t>(p.out) | p.chunk_syms) & 15u) == 0;
    uint32_t nbad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t chunk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; chunk < p.nchunks; chunk += stride) {
        const uint64_t off = p.offsets[chunk];
        const uint32_t len = p.lengths[chunk];
        const uint64_t first = chunk * p.chunk_syms;
        const uint32_t nsym = (uint32_t)((p.n - first) < p.chunk_syms ? (p.n - first) : p.chunk_syms);
        if ((off & (Tr::kUnit - 1u)) != 0 || len < NW * Tr::kStateBytes || off > p.container_bytes || len > p.container_bytes - off) {
            nbad++;
            continue;
        }
        const uint8_t RANS_GLOBAL *src = cbase + off;
        uint8_t RANS_GLOBAL *dst = (uint8_t RANS_GLOBAL *)p.out + first * p.sym_bytes;

        state_t x[NW];
#pragma unroll
        for (int l = 0; l < NW; ++l) { // RansDecInit order: lane 0's state first
            if constexpr (FMT == FMT_R64) {
                const u32x2 v = reinterpret_cast<const u32x2 RANS_GLOBAL *>(src)[l];
                x[l] = (uint64_t)v.x | ((uint64_t)v.y << 32);
            } else {
                x[l] = reinterpret_cast<const uint32_t RANS_GLOBAL *>(src)[l];
            }
        }
        LaneWindow W;
        W.open<(int)Tr::kUnit>(reinterpret_cast<uint64_t>(p.container) + off + NW * Tr::kStateBytes, glimit);
        bool bad = false;

        const uint32_t rounds = nsym / NW;
        uint32_t i = 0; // symbol index inside the chunk
        if (wide_out) {
            // 16 symbols per 16-byte store: 16/NW rounds per group
            constexpr int kRoundsPerGroup = 16 / NW;
            const uint32_t groups = rounds / kRoundsPerGroup;
            for (uint32_t g = 0; g < groups; ++g) {
                u32x4 pack = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int rr = 0; rr < kRoundsPerGroup; ++rr) {
#pragma unroll
                    for (int l = 0; l < NW; ++l) {
                        uint32_t sy = dec_step<FMT>(T, x[l]);
                        if constexpr (Tr::kSymByte == 3)
                            sy >>= 24;
                        const int pos = rr * NW + l;
                        pack[pos / 4] |= (sy & 0xffu) << (8 * (pos % 4));
                    }
#pragma unroll
                    for (int l = 0; l < NW; ++l)
                        lane_renorm<FMT>(x[l], W, true);
                }
                __builtin_nontemporal_store(pack, reinterpret_cast<u32x4 RANS_GLOBAL *>(dst + i));
                i += 16;
            }
        }
        // remaining rounds + tail: element stores
        while (i < nsym) {
            const uint32_t cnt = nsym - i < (uint32_t)NW ? nsym - i : (uint32_t)NW;
#pragma unroll
            for (int l = 0; l < NW; ++l)
                if ((uint32_t)l < cnt) {
                    uint32_t sy = dec_step<FMT>(T, x[l]);
                    if constexpr (Tr::kSymByte == 3)
                        sy >>= 24;
                    if (p.sym_bytes == 1)
                        dst[i + l] = (uint8_t)sy;
                    else
                        reinterpret_cast<uint16_t RANS_GLOBAL *>(dst)[i + l] = (uint16_t)sy;
                }
#pragma unroll
            for (int l = 0; l < NW; ++l)
                lane_renorm<FMT>(x[l], W, (uint32_t)l < cnt);
            i += cnt;
        }
#pragma unroll
        for (int l = 0; l < NW; ++l)
            bad = bad || (x[l] != Tr::kL);
        if (bad || W.used + NW * Tr::kStateBytes != len)
            nbad++;
    }
    if (nbad)
        atomicAdd(p.err_count, (unsigned long long)nbad);
}

template <int FMT, int NW>
hipError_t launch_decode_lanes_t(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    const uint32_t t0 = (p.table0_bytes + 15u) & ~15u, t1 = (p.table1_bytes + 15u) & ~15u;
    // staged kernel: the tables are shared by the block, every wave adds kLaneWaveLds of rings, so one
    // large block per CU keeps the most waves resident (rans64, 14 bits: 15 waves; 4-wave blocks: 12)
    const size_t table_lds = (size_t)t0 + t1;
    uint32_t sw = table_lds + kLaneWaveLds <= 160 * 1024 ? (uint32_t)((160 * 1024 - table_lds) / kLaneWaveLds) : 0;
    sw = sw > 16 ? 16 : sw;
    // 64 chunks of one wave must lie within 2^30 bytes (32-bit ring positions): any sane chunk size
    // NAMED FALLBACK: chunks of 512 Ki symbols and more, or tables that leave no room for a wave's rings, go to the first
    // generation's per-lane register window (k_decode_lanes: >= 4 x over-fetch, one chunk per lane all the same -- a wave per
    // chunk would leave 62 of 64 lanes idle on a 2-way stream); tests/test_gpu_parity.py test_lane_decoder_fallback_*
    const bool staged = sw >= 1 && (uint64_t)p.chunk_syms * 8u < (1u << 22);
    const uint64_t batches = (p.nchunks + 63) / 64;
    if (staged)
        sw = lanes_even_waves(batches, num_cus, sw);
    if constexpr (FMT == FMT_R64 && NW == 2) {
        // third generation for the reference's own 2-way rans64 layout (config 2): full 64-symbol trips only; a ragged
        // last chunk is decoded by the staged kernel in a second launch
        const bool aligned = p.sym_bytes == 1 && ((reinterpret_cast<uintptr_t>(p.out) | p.chunk_syms) & 63u) == 0 &&
                             (reinterpret_cast<uintptr_t>(p.container) & 15u) == 0;
        if (staged && aligned && p.nchunks >= 64 && !p.trace) {
            const uint64_t full = p.n / p.chunk_syms; // chunks with chunk_syms symbols
            // packed slot records (one gather per symbol) where the model has them and at least 8 waves' rings fit beside
            // the table
            const size_t packed_lds = (p.packed_bytes + 15u) & ~(size_t)15;
            const bool packed = p.packed && packed_lds + 8u * kR64WaveLds <= 160 * 1024;
            const size_t table_lds3 = packed ? packed_lds : table_lds;
            const uint32_t room3 = (uint32_t)((160 * 1024 - table_lds3) / kR64WaveLds);
            const uint64_t batches3 = (full + 63) / 64;
            const uint32_t sw3 = lanes_even_waves(batches3, num_cus, room3 > 16 ? 16 : room3);
            auto kern3 = packed ? k_decode_lanes_r64x2<true> : k_decode_lanes_r64x2<false>;
            static std::atomic<uint64_t> lds_ok3[2] = {{0}, {0}};
            DecParams q = p;
            q.nchunks = full;
            q.n = full * p.chunk_syms;
            if (packed) { // the kernel stages "table 0" and "table 1": the packed records and nothing
                q.table0 = p.packed;
                q.table0_bytes = p.packed_bytes;
                q.table1_bytes = 0;
            }
            if (name)
                *name = packed ? KernelId::decode_lanes_r64x2_packed : KernelId::decode_lanes_r64x2;
            if (hipError_t e = launch_lanes(kern3, lds_ok3[packed], 160 * 1024, lanes_grid(batches3, sw3, num_cus), 64 * sw3,
                                            table_lds3 + (size_t)sw3 * kR64WaveLds, stream, q);
                e != hipSuccess)
                return e;
            if (full == p.nchunks)
                return hipSuccess;
            DecParams r = p; // the ragged last chunk
            r.offsets = p.offsets + full;
            r.lengths = p.lengths + full;
            r.out = static_cast<uint8_t *>(p.out) + full * p.chunk_syms;
            r.n = p.n - full * p.chunk_syms;
            r.nchunks = 1;
            r.work_counter_reset = nullptr;
            r.span_reset = nullptr;
            static std::atomic<uint64_t> lds_ok4{0};
            return launch_lanes(k_decode_lanes_staged<FMT, NW>, lds_ok4, 160 * 1024, 1, 64, table_lds + kLaneWaveLds, stream, r);
        }
    }
    static std::atomic<uint64_t> lds_ok[2] = {{0}, {0}}; // per kernel generation, one bit per device
    if (staged) {
        if (name)
            *name = KernelId::decode_lanes_staged;
        return launch_lanes(k_decode_lanes_staged<FMT, NW>, lds_ok[1], 160 * 1024, lanes_grid(batches, sw, num_cus), 64 * sw,
                            table_lds + (size_t)sw * kLaneWaveLds, stream, p);
    }
    const uint64_t want = (p.nchunks + 255) / 256;
    // 256-thread blocks: up to 8 per CU (32 waves) when the tables leave room in LDS; the kernel
    // is latency-bound (per-lane scattered loads), so residency matters more than anything else
    const size_t lds_room = table_lds ? (160 * 1024) / table_lds : 8;
    const uint64_t cap = (uint64_t)num_cus * (lds_room >= 8 ? 8 : (lds_room >= 1 ? lds_room : 1));
    if (name)
        *name = KernelId::decode_lanes;
    return launch_lanes(k_decode_lanes<FMT, NW>, lds_ok[0], 160 * 1024, (uint32_t)(want < cap ? want : cap), 256, table_lds, stream,
                        p);
}

template <int FMT> hipError_t launch_decode_lanes_f(const DecParams &p, int num_cus, hipStream_t s, KernelId *name)
{
    switch (p.n_ways) {
    case 1: return launch_decode_lanes_t<FMT, 1>(p, num_cus, s, name);
    case 2: return launch_decode_lanes_t<FMT, 2>(p, num_cus, s, name);
    case 4: return launch_decode_lanes_t<FMT, 4>(p, num_cus, s, name);
    case 8: return launch_decode_lanes_t<FMT, 8>(p, num_cus, s, name);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

hipError_t launch_decode_lanes(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    switch (format) {
    case FMT_WORD: return launch_decode_lanes_f<FMT_WORD>(p, num_cus, stream, name);
    case FMT_BYTE: return launch_decode_lanes_f<FMT_BYTE>(p, num_cus, stream, name);
    case FMT_R64: return launch_decode_lanes_f<FMT_R64>(p, num_cus, stream, name);
    case FMT_ALIAS: return launch_decode_lanes_f<FMT_ALIAS>(p, num_cus, stream, name);
    default: return hipErrorInvalidValue;
    }
}

// The ragged form of the 2-way rans64 lane decoder: rans64 over u8 symbols with the cum2sym tables (the caller has checked
// the format: the search variant is another kernel format), from 64 streams on; any symbol count, any output address.  Both
// tables and at least one wave's rings inside the CU's 160 KiB of LDS.
static size_t batch_lanes_tables(const DecParams &p) { return (size_t)((p.table0_bytes + 15u) & ~15u) + ((p.table1_bytes + 15u) & ~15u); }
bool decode_batch_r64_lanes_applicable(const DecParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.scale_bits >= 7 && p.scale_bits <= 16 && p.nchunks >= 64 && p.sym_offsets &&
           p.sym_counts && !p.trace && batch_lanes_tables(p) + kR64WaveLds <= 160 * 1024;
}

hipError_t launch_decode_batch_r64_lanes(const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    // one block per CU, as many waves as the tables leave rings for (14 bits: 16; 16 bits, 64 KiB of cum2sym: 11); a batch
    // that does not fill them spreads its wave-loads evenly (lanes_even_waves)
    const size_t table_lds = batch_lanes_tables(p);
    const uint32_t room = (uint32_t)((160 * 1024 - table_lds) / kR64WaveLds);
    const uint32_t max_waves = room > 16 ? 16 : room;
    const uint64_t loads = (p.nchunks + 63) / 64;
    const uint32_t sw = loads >= (uint64_t)num_cus * max_waves ? max_waves : lanes_even_waves(loads, num_cus, max_waves);
    static std::atomic<uint64_t> lds_ok{0};
    if (name)
        *name = KernelId::decode_batch_r64_lanes;
    return launch_lanes(k_decode_batch_r64_lanes, lds_ok, 160 * 1024, lanes_grid(loads, sw, num_cus), 64 * sw,
                        table_lds + (size_t)sw * kR64WaveLds, stream, p);
}

// The ragged form of the staged 1-way lane decoder, one instantiation per format (`format` is the kernel-side number, so the
// rans64 search variant and the word format over u16 symbols are not asked): u8 symbols, from 64 streams on, the scale_bits the
// format's uniform lane kernel takes -- byte and alias 8..16 (dec_step's 24-bit product; alias: the builder's power-of-two
// alphabet of at most 256 symbols, so that the table sizes say it, as for the alias pairs), word 12, rans64 7..16 (cum2sym) --,
// both tables and at least one wave's rings inside the CU's 160 KiB of LDS; any symbol count, any output address.
bool decode_batch_singles_applicable(int format, const DecParams &p)
{
    bool bits = false;
    switch (format) {
    case FMT_BYTE: bits = p.scale_bits >= 8 && p.scale_bits <= 16; break;
    case FMT_ALIAS:
        bits = p.scale_bits >= 8 && p.scale_bits <= 16 && p.log2nsyms <= 8 && p.table0_bytes == (16u << p.log2nsyms) &&
               p.table1_bytes == (4u << p.log2nsyms);
        break;
    case FMT_WORD: bits = p.scale_bits == 12; break;
    case FMT_R64: bits = p.scale_bits >= 7 && p.scale_bits <= 16; break;
    default: break;
    }
    return bits && p.n_ways == 1 && p.sym_bytes == 1 && p.nchunks >= 64 && p.sym_offsets && p.sym_counts && !p.trace &&
           batch_lanes_tables(p) + kLaneWaveLds <= 160 * 1024;
}

template <int FMT> static hipError_t launch_decode_batch_singles_t(const DecParams &p, int num_cus, hipStream_t stream)
{
    // one block per CU, as many waves as the tables leave rings for (16 up to 14 bits; byte at 16 bits, 64 KiB of cum2sym: 10); a
    // batch that does not fill them spreads its wave-loads evenly (lanes_even_waves)
    const size_t table_lds = batch_lanes_tables(p);
    const uint32_t room = (uint32_t)((160 * 1024 - table_lds) / kLaneWaveLds);
    const uint32_t max_waves = room > 16 ? 16 : room;
    const uint64_t loads = (p.nchunks + 63) / 64;
    const uint32_t sw = loads >= (uint64_t)num_cus * max_waves ? max_waves : lanes_even_waves(loads, num_cus, max_waves);
    static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
    return launch_lanes(k_decode_batch_singles<FMT>, lds_ok, 160 * 1024, lanes_grid(loads, sw, num_cus), 64 * sw,
                        table_lds + (size_t)sw * kLaneWaveLds, stream, p);
}

hipError_t launch_decode_batch_singles(int format, const DecParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!decode_batch_singles_applicable(format, p)) // (kBatchFamilies has asked; a missing kernel is an error, never another path)
        return hipErrorInvalidValue;
    switch (format) {
    case FMT_BYTE:
        if (name)
            *name = KernelId::decode_batch_singles_byte;
        return launch_decode_batch_singles_t<FMT_BYTE>(p, num_cus, stream);
    case FMT_WORD:
        if (name)
            *name = KernelId::decode_batch_singles_word;
        return launch_decode_batch_singles_t<FMT_WORD>(p, num_cus, stream);
    case FMT_R64:
        if (name)
            *name = KernelId::decode_batch_singles_r64;
        return launch_decode_batch_singles_t<FMT_R64>(p, num_cus, stream);
    default:
        if (name)
            *name = KernelId::decode_batch_singles_alias;
        return launch_decode_batch_singles_t<FMT_ALIAS>(p, num_cus, stream);
    }
}

#undef R64_LOOKUP
#undef R64_UPDATE
#undef R64_QUAD
#undef R64_GROUP
#undef R64P_LOOKUP
#undef R64P_UPDATE
#undef R64P_QUAD
#undef R64P_GROUP
#undef R64_COMMIT
#undef R64_FETCH
#undef R64_TRANSPOSE
#undef R64_STORES
#undef R64_HOLD
#undef R64_STORES2
#undef R64_TRIP_TOP
#undef R64_TRIP_END
#undef R64_LAST
#undef R64_HOLD_CLOBBERS
#undef R64_CLOBBERS

} // namespace rans_amd
