// encode_lanes.hip -- lane-per-stream encoders for narrow interleaves (N = 1, 2, 4, 8), all generations, and the fused
// placement of their chunks.  Behind k_encode_lanes_r64x2: k_encode_batch_r64_lanes, its ragged form for
// rans_amd_encode_batch[_ordered] (sixty-four STREAMS per wave, each with its own count, symbol address and slot).

#include "lanes_common.hpp"
#include "groups_common.hpp" // the ragged kernel's work hand-out and wave maximum

namespace rans_amd {

namespace {

// one symbol of the sequential reference encoder (RansEncPut / RansWordEncPut / Rans64EncPut /
// RansEncPutAlias) for a lane-private state and write pointer
template <int FMT>
__device__ __forceinline__ void lane_put(typename FmtTraits<FMT>::state_t &x, uint32_t sym, const uint4 *recs,
                                         const EncParams &p, uint8_t RANS_GLOBAL *&wp, bool &bad)
{
    const bool known = sym < p.nsyms;
    const uint4 rec = recs[known ? sym : 0u];
    const uint32_t freq = (FMT == FMT_R64 || FMT == FMT_BYTE) ? (rec.x & 0xffffffu) : rec.x, start = rec.y, rcp = rec.z;
    if (!known || freq == 0) {
        bad = true;
        return;
    }
    if constexpr (FMT == FMT_WORD) {
        uint32_t y = x;
        if (y >= (freq << 20)) {
            wp -= 2;
            *reinterpret_cast<uint16_t RANS_GLOBAL *>(wp) = (uint16_t)y;
            y >>= 16;
        }
        x = enc_update_word(y, rec);
    } else if constexpr (FMT == FMT_R64) {
        uint64_t y = x;
        if (y >= (((uint64_t)freq) << (63u - p.scale_bits))) {
            wp -= 4;
            *reinterpret_cast<uint32_t RANS_GLOBAL *>(wp) = (uint32_t)y;
            y >>= 32;
        }
        x = enc_update_r64(y, rec, p.scale_bits);
    } else {
        uint32_t y = x;
        const uint32_t x_max = freq << (31u - p.scale_bits);
#pragma unroll
        for (int b = 0; b < 2; ++b)
            if (y >= x_max) {
                *--wp = (uint8_t)y;
                y >>= 8;
            }
        if constexpr (FMT == FMT_ALIAS) {
            uint32_t q, rem;
            divmod_rcp(y, freq, rcp, q, rem);
            x = (q << p.scale_bits) + p.alias_remap[rem + start];
        } else {
            x = enc_update_byte(y, rec, p.scale_bits);
        }
    }
}

// ---------------------------------------------------------------------------
// Staged lane-per-stream encoder: the mirror image of k_decode_lanes_staged.  Per-lane stores of
// every emitted unit reached HBM as partial lines (measured 6.4x the stream bytes on the write
// side) and per-lane 16-byte symbol loads pulled whole lines (3.6x).  Here
//   * symbols: the wave loads one 64-byte block of each of its 64 chunks with coalesced 16-byte
//     loads (4 lanes per chunk) into per-lane rows in LDS; every lane then walks its row from
//     the top, 16 symbols per ds_read_b128;
//   * stream: units go into a 128-byte ring per lane (two 64-byte lines, written downwards); after
//     every 16 symbols (at most 64 bytes emitted) a line that has filled up is written out by 4
//     lanes with 16-byte stores -- whole 64-byte lines, each written once.
// Slots are whole lines (api.cpp, encode_slot_bytes); what lies below the stream start inside the
// lowest line is never read.
// ---------------------------------------------------------------------------
constexpr uint32_t kEncRowStride = 80; // 64 symbol bytes, rows 16-byte aligned, 20 dwords apart
constexpr uint32_t kEncWaveLds = 64 * kEncRowStride + 64 * kLaneRingStride + 64 * 4;

// slot layout (EncParams::slot_layout): the chunk stays in its slot, its stream is [slot end - len, slot end)
// (sized slots, EncParams::ovf_ctl: a lane whose chunk did not fit its slot -- ovf -- lists it for the redo launch instead;
//  whatever it stored lies inside its own slot and counts for nothing)
__device__ __forceinline__ void lanes_publish_slot(const EncParams &p, uint64_t chunk, uint32_t len, bool ovf = false)
{
    if (ovf) {
        p.ovf_list[atomicAdd(p.ovf_ctl, 1u)] = (uint32_t)chunk;
        return;
    }
    if (p.slot_layout) {
        p.offsets[chunk] = (chunk + 1u) * p.slot_bytes - len;
        if (chunk + 1 == p.nchunks)
            p.offsets[p.nchunks] = p.nchunks * p.slot_bytes;
    }
}

template <int FMT> struct LaneOut {
    uint8_t *row;  // this lane's output ring in LDS
    uint32_t w;    // write offset inside the chunk's slot, moves down
    template <int UNIT> __device__ __forceinline__ void emit(uint32_t v)
    {
        w -= UNIT;
        uint8_t *at = row + (w & (2 * kLaneLine - 1));
        if constexpr (UNIT == 4)
            *reinterpret_cast<uint32_t *>(at) = v;
        else if constexpr (UNIT == 2)
            *reinterpret_cast<uint16_t *>(at) = (uint16_t)v;
        else
            *at = (uint8_t)v;
    }
};

// one symbol of the sequential reference encoder for a lane-private state, emitting into the ring
template <int FMT>
__device__ __forceinline__ void lane_put_staged(typename FmtTraits<FMT>::state_t &x, uint32_t sym, const uint4 *recs,
                                                const EncParams &p, LaneOut<FMT> &O, bool &bad)
{
    const bool known = sym < p.nsyms;
    const uint4 rec = recs[known ? sym : 0u];
    const uint32_t freq = (FMT == FMT_R64 || FMT == FMT_BYTE) ? (rec.x & 0xffffffu) : rec.x, start = rec.y, rcp = rec.z;
    if (!known || freq == 0) {
        bad = true;
        return;
    }
    if constexpr (FMT == FMT_WORD) {
        uint32_t y = x;
        if (y >= (freq << 20)) { // rans_word_sse41.h:85-89
            O.template emit<2>(y);
            y >>= 16;
        }
        x = enc_update_word(y, rec);
    } else if constexpr (FMT == FMT_R64) {
        uint64_t y = x;
        if (y >= (((uint64_t)freq) << (63u - p.scale_bits))) { // rans64.h:83-88
            O.template emit<4>((uint32_t)y);
            y >>= 32;
        }
        x = enc_update_r64(y, rec, p.scale_bits);
    } else {
        uint32_t y = x;
        const uint32_t x_max = freq << (31u - p.scale_bits); // rans_byte.h:64-70
#pragma unroll
        for (int b = 0; b < 2; ++b)
            if (y >= x_max) {
                O.template emit<1>(y);
                y >>= 8;
            }
        if constexpr (FMT == FMT_ALIAS) {
            uint32_t q, rem;
            divmod_rcp(y, freq, rcp, q, rem);
            x = (q << p.scale_bits) + p.alias_remap[rem + start];
        } else {
            x = enc_update_byte(y, rec, p.scale_bits);
        }
    }
}

// ---------------------------------------------------------------------------
// Fused placement of the lane encoders (EncParams::status != NULL): no k_layout / k_compact_small afterwards.  The
// container's layout is the oracle's (chunk c starts at the sum of the 16-byte aligned lengths before it), so the
// chunks of a batch can be copied to their place once the total of everything before the batch is known.
//
// The unit of the scan is a ROUND OF A BLOCK: its C coding waves take C consecutive batches (one claim of the block's
// scanner wave on a counter behind the status words), code them, and post their totals in LDS; the scanner adds them
// up, publishes status[unit] = AGGREGATE | total, looks back over the units before it (decoupled look-back,
// device_common.hpp; kScanWords * 64 units per step) until it meets a PREFIX, publishes its own PREFIX and leaves the
// place of every coder's batch in LDS; kLaneCopyWaves copier waves -- no LDS of their own, so they come on top of the
// coding waves the rings allow -- then move the round's batches to the container while the coders are a round ahead.
// 256 units (one per CU) finish together and one look-back step resolves them all.
//
// What this replaced, all of them measured on config 2 (0.36-0.40 ms with the two extra kernels): the coding wave
// placing its own batch at once (0.54: every wave of the first round finishes at the same moment and the prefix travels
// 64 batches per memory round trip); a copier wave per block that scans and copies batch by batch through a mailbox
// (0.375-0.52: 6-8 us per batch where the coders deliver one every 8 us); a scanner wave per block working batch by
// batch while the coders copy (0.40-0.42: with 2816 batches ending together a scanner walks back thousands of status
// words for each of its 11 batches); the round-of-a-block units with the coders copying their previous batch (0.42-0.47:
// the protocol costs 0.01 ms then, the copy 0.13 -- these kernels run 3-4 waves per SIMD, each bound by its own
// dependency chain, and a wave that spends 40 us per batch in memory round trips is not replaced by anybody).  With
// the copier waves the fused launch is as fast as the three kernels (0.34-0.37 ms against 0.35-0.37: 11 coding waves in
// three rounds instead of 16 in two pay for what the copy no longer costs) -- hence still opt-in.
// Units are claimed in ascending order by running blocks and a scanner waits only for smaller units: the smallest
// unfinished unit always belongs to a running block.  The copy is quad-cooperative like every other access of these
// kernels: instruction t moves 64 bytes of the chunk of the quad's lane t (16 bytes per lane, source unaligned),
// kLaneCopyDepth pieces per chunk in flight.
//
// A word on control flow: none of the loops below ends in an `if (lane == 0) { ... }`.  With such a tail the compiler
// let lanes 1..63 run ahead into the next iteration -- whose readfirstlane then read a lane that had not taken part --
// and parked lane 0's store behind the loop, for ever (found with the watchdogs below: flags 0x40, every status word
// still AGGREGATE).  Stores that one lane would do are done by all of them with the same value.
// ---------------------------------------------------------------------------
constexpr uint32_t kLaneCopyWaves = 3; // copier waves per block
constexpr uint32_t kLaneCopiers = 1 + kLaneCopyWaves; // scanner + copier waves (on top of the coding waves, <= 16 in all)
constexpr int kLaneCopyDepth = 4;
constexpr int kScanWords = 4;

struct LaneRounds { // the block's control words in LDS (EncParams::mailbox_off), zero at kernel start; index = round & 1
    // (units: round & 3 -- the scanner names round r + 1's unit while a copier may still be busy with round r - 1)
    uint32_t unit[4];     // unit claimed for the round ...
    uint32_t unit_seq[4]; // ... valid when this is round + 1
    uint32_t posted[2];   // coding waves that have posted their total
    uint32_t base_seq[2]; // bases[] valid when this is round + 1
    uint32_t copied[2];   // copier waves that are through with the round
    uint32_t totals[2][16];
    unsigned long long bases[2][16];
};
static_assert(sizeof(LaneRounds) <= kEncMailboxBytes, "LaneRounds must fit the LDS reserved for the placement");

struct LaneCoder { // a coding wave's view
    uint32_t round; // rounds begun
};

// poll an LDS word until it has the value (whole wave; gives up after kWaitTicks and says so in flags)
__device__ __forceinline__ bool lanes_wait_lds(volatile uint32_t *word, uint32_t value, uint32_t *flags, uint32_t flag_bit, uint32_t lane,
                                               unsigned long long wait_ticks)
{
    for (SpinWatch watch(wait_ticks);;) {
        if (uniform(*word) == value)
            return true;
        if (watch.expired(flags)) {
            atomicOr(flags, lane == 0 ? flag_bit : 0u);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// coding wave, start of a round: its batch, ~0 - 1 when it has none in this (the last) unit, ~0 when the launch is over
__device__ __forceinline__ uint64_t lanes_round_begin(const EncParams &p, LaneRounds *ctl, const LaneCoder &cs, uint32_t wave,
                                                      uint32_t coders, uint32_t lane)
{
    const uint32_t r = cs.round;
    if (!lanes_wait_lds(&ctl->unit_seq[r & 3u], r + 1u, p.flags, 128u, lane, p.wait_ticks))
        return ~0ull;
    const uint64_t first = p.batch_begin + (uint64_t)uniform(*(volatile uint32_t *)&ctl->unit[r & 3u]) * coders;
    if (first >= p.batch_end)
        return ~0ull;
    return first + wave < p.batch_end ? first + wave : ~0ull - 1u;
}

// coding wave: offsets[] of a batch and its copy out of the scratch slots; base = where the batch starts
__device__ __forceinline__ void lanes_copy_batch(const EncParams &p, uint64_t batch, uint32_t len, unsigned long long base, uint32_t lane)
{
    const uint64_t chunk = batch * 64u + lane;
    const bool valid = chunk < p.nchunks;
    const uint32_t alen = (len + 15u) & ~15u;
    uint32_t incl = alen; // inclusive sum over the lanes below
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        incl += lane >= (uint32_t)d ? o : 0u;
    }
    const uint64_t off = base + incl - alen;
    if (valid) {
        p.offsets[chunk] = off;
        if (chunk + 1 == p.nchunks)
            p.offsets[p.nchunks] = off + len;
    }
    if (__builtin_amdgcn_ballot_w64(valid && off + alen > p.out_cap) != 0) { // (wave-uniform; alen: whole granules are stored below)
        atomicOr(p.flags, lane == 0 ? 2u : 0u);
        return;
    }
    const uint32_t m = lane & 3u;
    const uint64_t sa = reinterpret_cast<uint64_t>(p.scratch) + (chunk + 1u) * p.slot_bytes - len; // a stream ends at its slot's end
    const uint64_t da = reinterpret_cast<uint64_t>(p.out) + off;
    uint64_t s_t[4], d_t[4];
    uint32_t n16[4], most = 0; // (the last piece of a chunk may read up to 15 bytes of the next slot: the scratch is padded)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int from = (int)((lane & ~3u) + t);
        s_t[t] = (uint64_t)(uint32_t)__shfl((int)(uint32_t)sa, from, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(sa >> 32), from, 64) << 32);
        d_t[t] = (uint64_t)(uint32_t)__shfl((int)(uint32_t)da, from, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(da >> 32), from, 64) << 32);
        n16[t] = (uint32_t)__shfl((int)(valid ? alen >> 4 : 0u), from, 64);
        most = n16[t] > most ? n16[t] : most;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)most, d, 64);
        most = o > most ? o : most;
    }
    most = uniform(most);
    for (uint32_t i0 = 0; i0 < most; i0 += 4u * kLaneCopyDepth) {
        u32x4 v[4][kLaneCopyDepth];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < kLaneCopyDepth; ++j) {
                const uint32_t i = i0 + 4u * j + m;
                if (i < n16[t])
                    v[t][j] = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(s_t[t] + 16ull * i));
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < kLaneCopyDepth; ++j) {
                const uint32_t i = i0 + 4u * j + m;
                if (i < n16[t])
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(d_t[t] + 16ull * i) = v[t][j];
            }
    }
}

// coding wave, end of a round: post the total (len: this lane's chunk, 0 without one)
__device__ __forceinline__ void lanes_round_end(const EncParams &p, LaneRounds *ctl, LaneCoder &cs, uint32_t wave, uint32_t lane,
                                                uint64_t batch, uint32_t len)
{
    (void)batch;
    const uint32_t r = cs.round;
    uint32_t sum = (len + 15u) & ~15u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
        sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // lengths[] and every flushed line of the batch have left the wave
    *(volatile uint32_t *)&ctl->totals[r & 1u][wave] = sum; // (every lane, the same value)
    atomicAdd(&ctl->posted[r & 1u], lane == 0 ? 1u : 0u);
    cs.round = r + 1u;
}

// copier wave number k of the block: when the places of a round's batches are known, the batches k, k + kLaneCopyWaves,
// ... of the round go to the container
__device__ __forceinline__ void lanes_copier(const EncParams &p, LaneRounds *ctl, uint32_t k, uint32_t lane, uint32_t coders)
{
    for (uint32_t r = 0;; ++r) {
        if (!lanes_wait_lds(&ctl->unit_seq[r & 3u], r + 1u, p.flags, 128u, lane, p.wait_ticks))
            return;
        const uint64_t first = p.batch_begin + (uint64_t)uniform(*(volatile uint32_t *)&ctl->unit[r & 3u]) * coders;
        if (first >= p.batch_end)
            return;
        if (!lanes_wait_lds(&ctl->base_seq[r & 1u], r + 1u, p.flags, 64u, lane, p.wait_ticks))
            return;
        for (uint32_t w = k; w < coders && first + w < p.batch_end; w += kLaneCopyWaves) {
            const volatile uint32_t *b = reinterpret_cast<const volatile uint32_t *>(&ctl->bases[r & 1u][w]);
            const unsigned long long base = (unsigned long long)uniform(b[0]) | ((unsigned long long)uniform(b[1]) << 32);
            const uint64_t chunk = (first + w) * 64u + lane;
            // (written by a wave of this CU before it posted its total, read through L2)
            const uint32_t len = chunk < p.nchunks ? __hip_atomic_load(p.lengths + chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            lanes_copy_batch(p, first + w, len, base, lane);
        }
        atomicAdd(&ctl->copied[r & 1u], lane == 0 ? 1u : 0u);
    }
}

// the scanner wave's life
__device__ __forceinline__ void lanes_scanner(const EncParams &p, LaneRounds *ctl, uint32_t lane, uint32_t coders)
{
    const uint64_t nunits = (p.batch_end - p.batch_begin + coders - 1u) / coders;
    unsigned int *counter = reinterpret_cast<unsigned int *>(p.status + ((p.nchunks + 63u) / 64u) + 8u * p.claim_slot);
    auto claim = [&]() {
        uint32_t got = 0;
        if (lane == 0)
            got = atomicAdd(counter, 1u);
        return uniform(got);
    };
    const uint32_t slot = lane < 15u ? lane : 15u; // (coders <= 15: slot 15 is nobody's)
    uint32_t u = claim();
    *(volatile uint32_t *)&ctl->unit[0] = u;
    *(volatile uint32_t *)&ctl->unit_seq[0] = 1u;
    for (uint32_t r = 0; u < nunits; ++r) {
        const uint32_t un = claim(); // the coders find their next unit as soon as they are through with this one
        *(volatile uint32_t *)&ctl->unit[(r + 1u) & 3u] = un;
        *(volatile uint32_t *)&ctl->unit_seq[(r + 1u) & 3u] = r + 2u;
        if (!lanes_wait_lds(&ctl->posted[r & 1u], coders, p.flags, 16u, lane, p.wait_ticks))
            return;
        const uint32_t mine = *(volatile uint32_t *)&ctl->totals[r & 1u][slot];
        const uint32_t t = lane < coders ? mine : 0u;
        uint32_t incl = t;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            incl += lane >= (uint32_t)d ? o : 0u;
        }
        const unsigned long long total = (uint32_t)__shfl((int)incl, 15, 64);
        *(volatile uint32_t *)&ctl->posted[r & 1u] = 0u; // (for round r + 2)
        const uint64_t gu = p.unit_base + u;
        __hip_atomic_store(p.status + gu, kStAggregate | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (every lane)
        unsigned long long base = 0;
        SpinWatch watch(p.wait_ticks);
        for (uint64_t j = gu;;) { // status[j-1], status[j-2], ... are still to be added
            unsigned long long st[kScanWords];
            uint64_t ready[kScanWords], pref[kScanWords];
#pragma unroll
            for (int k = 0; k < kScanWords; ++k) {
                const uint64_t back = lane + 64u * k; // distance - 1
                st[k] = kStPrefix; // virtual predecessors of unit 0: an inclusive prefix of 0
                if (back < j)
                    st[k] = __hip_atomic_load(p.status + (j - 1 - back), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int k = 0; k < kScanWords; ++k) {
                ready[k] = __builtin_amdgcn_ballot_w64((st[k] >> 62) != 0);
                pref[k] = __builtin_amdgcn_ballot_w64((st[k] >> 62) == 2);
            }
            // the nearest PREFIX: word K, lane `first`; everything nearer must be there (AGGREGATE or PREFIX)
            int K = kScanWords;
            uint32_t first = 64u;
            bool all_ready = true;
#pragma unroll
            for (int k = 0; k < kScanWords; ++k) {
                if (K == kScanWords) {
                    if (pref[k]) {
                        K = k;
                        first = (uint32_t)__builtin_ctzll(pref[k]);
                        const uint64_t need = first >= 63u ? ~0ull : ((2ull << first) - 1ull); // lanes 0 .. first
                        all_ready = all_ready && (ready[k] & need) == need;
                    } else {
                        all_ready = all_ready && ready[k] == ~0ull;
                    }
                }
            }
            if (!all_ready) { // a unit in that range is still being coded
                if (watch.expired(p.flags)) { // (a protocol error must not hang the GPU)
                    atomicOr(p.flags, lane == 0 ? 32u : 0u);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
                continue;
            }
            unsigned long long v = 0;
#pragma unroll
            for (int k = 0; k < kScanWords; ++k)
                if (k < K || (k == K && lane <= first))
                    v += st[k] & kStValue;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
                const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
                v += (unsigned long long)lo | ((unsigned long long)hi << 32);
            }
            base += uniform64(v);
            if (K < kScanWords)
                break;
            j -= 64u * kScanWords;
        }
        __hip_atomic_store(p.status + gu, kStPrefix | (base + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (every lane)
        const unsigned long long place = base + incl - t; // of coder `lane`'s batch
        if (r >= 2u) { // the copiers are through with round r - 2, whose places these words still hold
            if (!lanes_wait_lds(&ctl->copied[r & 1u], kLaneCopyWaves, p.flags, 16u, lane, p.wait_ticks))
                return;
            *(volatile uint32_t *)&ctl->copied[r & 1u] = 0u;
        }
        volatile uint32_t *b = reinterpret_cast<volatile uint32_t *>(&ctl->bases[r & 1u][slot]);
        b[0] = (uint32_t)place; // (lanes >= 15 all write slot 15)
        b[1] = (uint32_t)(place >> 32);
        *(volatile uint32_t *)&ctl->base_seq[r & 1u] = r + 1u;
        u = un;
    }
}

template <int FMT, int NW>
__global__ void __launch_bounds__(1024) k_encode_lanes_staged(const EncParams p)
{
    using Tr = FmtTraits<FMT>;
    using state_t = typename Tr::state_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(p.enc_recs);
        uint4 *l = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < p.nsyms; i += blockDim.x)
            l[i] = g[i];
        if (p.status) // (a block may be as small as one coding wave + the scanner: 128 threads for 132 words)
            for (uint32_t i = threadIdx.x; i < kEncMailboxBytes / 4u; i += blockDim.x)
                reinterpret_cast<uint32_t *>(smem + p.mailbox_off)[i] = 0u;
    }
    __syncthreads();
    const uint4 *recs = reinterpret_cast<const uint4 *>(smem);
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const bool fused = p.status != nullptr;
    const uint32_t waves_per_block = (blockDim.x >> 6) - (fused ? kLaneCopiers : 0u); // coding waves
    LaneRounds *ctl = reinterpret_cast<LaneRounds *>(smem + p.mailbox_off);
    if (fused && wave >= waves_per_block) { // ---- the scanner wave and the copier waves
        if (wave == waves_per_block)
            lanes_scanner(p, ctl, lane, waves_per_block);
        else
            lanes_copier(p, ctl, wave - waves_per_block - 1u, lane, waves_per_block);
        return;
    }
    uint8_t *rows = smem + p.nsyms * (uint32_t)sizeof(EncRec) + wave * kEncWaveLds;
    uint8_t *rings = rows + 64u * kEncRowStride;
    uint32_t *req = reinterpret_cast<uint32_t *>(rings + 64u * kLaneRingStride);
    const uint32_t part = lane & 3u, grp = lane >> 2;
    const uint32_t slot_lines = (uint32_t)(p.slot_bytes / kLaneLine);

    bool bad = false;
    LaneCoder cs{0};
    const uint64_t total_waves = (uint64_t)gridDim.x * waves_per_block;
    for (uint64_t batch_v = p.batch_begin + (uint64_t)blockIdx.x * waves_per_block + wave;; batch_v += total_waves) {
        if (fused) { // the block's scanner hands out the rounds
            batch_v = lanes_round_begin(p, ctl, cs, wave, waves_per_block, lane);
            if (batch_v == ~0ull - 1u) { // nothing for this wave in the last unit
                lanes_round_end(p, ctl, cs, wave, lane, batch_v, 0u);
                continue;
            }
        }
        if (batch_v >= p.batch_end)
            break;
        const uint64_t chunk0 = uniform64(batch_v) * 64u;
        const uint64_t chunk = chunk0 + lane;
        const bool valid = chunk < p.nchunks;
        auto syms_of = [&](uint64_t c) -> uint32_t { // symbols in chunk c (0 past the end)
            if (c >= p.nchunks)
                return 0u;
            const uint64_t first = c * p.chunk_syms;
            return (uint32_t)((p.n - first) < p.chunk_syms ? (p.n - first) : p.chunk_syms);
        };
        const uint32_t nsym = syms_of(chunk);
        const uint8_t RANS_GLOBAL *src = (const uint8_t RANS_GLOBAL *)p.syms + chunk * (uint64_t)p.chunk_syms;
        uint8_t RANS_GLOBAL *slots0 = (uint8_t RANS_GLOBAL *)p.scratch + chunk0 * p.slot_bytes; // wave-uniform

        state_t x[NW];
#pragma unroll
        for (int l = 0; l < NW; ++l)
            x[l] = Tr::kL;
        LaneOut<FMT> O;
        O.row = rings + lane * kLaneRingStride;
        O.w = (uint32_t)p.slot_bytes;
        uint32_t flushed = slot_lines; // lines [flushed, slot_lines) are in memory

        // the whole wave takes part: lanes publish the line they have filled (or, at the end, the lines
        // that hold anything), lane (4 g + part) writes 16 bytes of chunk (16 j + g)'s line
        auto flush = [&](bool final) {
            const bool need = valid && flushed != 0u &&
                              (final ? O.w < flushed * kLaneLine : O.w <= (flushed - 1u) * kLaneLine);
            req[lane] = need ? (((flushed - 1u) << 1) | 1u) : 0u;
            if (need)
                flushed -= 1u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t q = 16u * j + grp;
                const uint32_t r = req[q]; // LDS ops of one wave execute in order
                if (r & 1u) {
                    const uint32_t line = r >> 1;
                    const uint8_t *at = rings + q * kLaneRingStride + (line & 1u) * kLaneLine + part * 16u;
                    const u32x2 a = reinterpret_cast<const u32x2 *>(at)[0], b = reinterpret_cast<const u32x2 *>(at)[1];
                    u32x4 RANS_GLOBAL *o = reinterpret_cast<u32x4 RANS_GLOBAL *>(
                        slots0 + (uint64_t)q * p.slot_bytes + (uint64_t)line * kLaneLine + part * 16u);
                    *o = u32x4{a.x, a.y, b.x, b.y};
                }
            }
        };

        // symbol i belongs to state i mod NW; visit i = nsym-1 .. 0 (main.cpp:233-243).  The top
        // nsym % 16 symbols come one by one from memory, the rest through the staged rows.
        const uint32_t nsym16 = nsym & ~15u;
        for (uint32_t i = nsym; i > nsym16; --i) {
            const uint32_t sym = (uint32_t)src[i - 1];
            const uint32_t l = (i - 1) % NW;
#pragma unroll
            for (int ll = 0; ll < NW; ++ll) // static register indexing
                if ((uint32_t)ll == l)
                    lane_put_staged<FMT>(x[ll], sym, recs, p, O, bad);
        }
        flush(false);

        const uint32_t my_blocks = (nsym16 + 63u) >> 6;
        uint32_t max_blocks = my_blocks;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)max_blocks, d, 64);
            max_blocks = o > max_blocks ? o : max_blocks;
        }
        max_blocks = uniform(max_blocks);
        for (uint32_t k = max_blocks; k-- > 0;) {
            // stage block k of every chunk: 16 bytes per lane, 4 instructions for 64 chunks
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t q = 16u * j + grp;
                const uint32_t qsyms16 = syms_of(chunk0 + q) & ~15u;
                const uint32_t at = 64u * k + 16u * part;
                if (at + 16u <= qsyms16) {
                    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(
                        reinterpret_cast<uint64_t>(p.syms) + (chunk0 + q) * (uint64_t)p.chunk_syms + at));
                    *reinterpret_cast<u32x4 *>(rows + q * kEncRowStride + 16u * part) = v;
                }
            }
            const uint8_t *row = rows + lane * kEncRowStride;
#pragma unroll
            for (int g = 3; g >= 0; --g) {
                if (64u * k + 16u * g + 16u <= nsym16) {
                    const u32x4 cur = *reinterpret_cast<const u32x4 *>(row + 16 * g);
#pragma unroll
                    for (int j = 15; j >= 0; --j) {
                        const uint32_t sym = (cur[j >> 2] >> (8 * (j & 3))) & 0xffu;
                        lane_put_staged<FMT>(x[j % NW], sym, recs, p, O, bad);
                    }
                }
                flush(false);
            }
        }
        // flush states NW-1 .. 0 (lane 0's first in memory), then whatever the ring still holds
        if (valid) {
#pragma unroll
            for (int l = NW - 1; l >= 0; --l) {
                if constexpr (FMT == FMT_R64) {
                    O.template emit<4>((uint32_t)(x[l] >> 32));
                    O.template emit<4>((uint32_t)x[l]);
                } else if constexpr (FMT == FMT_WORD) {
                    O.template emit<2>(x[l] >> 16);
                    O.template emit<2>(x[l]);
                } else {
                    O.template emit<1>(x[l] >> 24);
                    O.template emit<1>(x[l] >> 16);
                    O.template emit<1>(x[l] >> 8);
                    O.template emit<1>(x[l]);
                }
            }
            p.lengths[chunk] = (uint32_t)p.slot_bytes - O.w;
            // (sized slots: a write offset that went below 0 has wrapped -- the flushes stopped at line 0, the ring took the rest)
            lanes_publish_slot(p, chunk, (uint32_t)p.slot_bytes - O.w, O.w > (uint32_t)p.slot_bytes);
        }
        flush(true);
        flush(true);
        if (fused)
            lanes_round_end(p, ctl, cs, wave, lane, chunk0 / 64u, valid ? (uint32_t)p.slot_bytes - O.w : 0u);
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

// ---------------------------------------------------------------------------
// k_encode_lanes_r64x2: the reference's own 2-way rans64 layout (main64.cpp:224-246, config 2) on its own -- the mirror
// image of k_decode_lanes_r64x2.  The staged kernel above spends 38 VALU instructions per symbol (compiler-scheduled
// 64-bit arithmetic full of register-pair moves, a branch around every renormalisation, a wait after every record read);
// here one 16-symbol group is ONE asm statement:
//  * record {rcp lo, rcp hi, bias << 6 | rcp_shift, cmpl} (16 bytes, one ds_read_b128 per symbol; the LDS pipe could
//    not feed two), the records of the next pair of symbols are read while the current pair is worked on;
//  * renormalisation test (rans64.h:83: x >= ((L >> scale_bits) << 32) * freq) on the high dword alone: the low dword of
//    that bound is 0, and x.hi >= (M - cmpl) << k  <=>  x.hi + (cmpl << k) >= 2^31 (k = 31 - scale_bits): one
//    v_lshl_add + v_cmpx; the lanes that emit run under the exec mask (dword into the ring, x >>= 32 as two moves);
//  * q = mulhi64(x, rcp) >> rcp_shift (rans64.h:91, exact): v_mul_hi + 3 x v_mad_u64_u32, the middle sum's carry through
//    vcc (E64_BACK below); x += bias + q * cmpl (rans64.h:92, Rans64EncSymbolInit's identity) as v_lshl_add_u64 +
//    v_mad_u64_u32 + v_mad_u32_u24; 18.5 VALU per symbol (22.5 until late in round 4);
//  * output ring per lane: 32 dwords, dword d of lane l at ring + 256 d + 4 l (every ds_write_b32 conflict-free), the ring
//    8 KiB aligned so that the write position wraps with one v_bfi; a lane's bytes written are never counted per symbol,
//    the flush derives them from the ring position (at most 64 bytes per group);
//  * symbols: four 64-byte lines per quad and block (instruction t = the line of the quad's lane t), transposed in
//    registers, the next block in flight during the current one; flushes by quads as in the staged kernel.
// Requirements (launcher): rans64 with scale_bits 7..16, u8 symbols, chunk_syms % 64 == 0, 16-byte aligned input, full
// batches of full chunks (the rest goes through the staged kernel in a second launch, which continues the same status
// array).  A frequency of 2^16 -- a one-symbol model at 16 bits -- is inside the working range: its record is cmpl = 0,
// rcp = 2^63, rcp_shift = 15, the renormalisation test x.hi + (0 << 15) >= 2^31 never fires (rans64.h:83's bound is 2^63)
// and x + bias + q * 0 leaves the state where it is (tests/test_gpu_lane_extremes.py, the one-symbol case).
// ---------------------------------------------------------------------------
constexpr uint32_t kR64EncRing = 8192;   // per coding wave
constexpr uint32_t kR64EncTable = 8192;  // 256 records of 16 bytes at LDS address 0 (rings behind, 8 KiB aligned)

// state 0 = v[40:41], state 1 = v[42:43]; record sets v[48:51] / v[52:55] (pair in hand) and v[56:59] / v[60:63] (next);
// temporaries v64..v79 with the permanently zero v65, v69, v77 (the two states are worked on one after the other)
#define E64_ZERO                                                                                                        \
    "v_mov_b32 v65, 0\n\tv_mov_b32 v69, 0\n\tv_mov_b32 v77, 0\n\t"
// address of the record of byte J of symbol dword S: sym << 4 -- one SDWA shift of the selected byte (the count in a VGPR:
// SDWA takes no literal)
#define E64_SDWA(D, S, SEL)                                                                                             \
    "v_lshlrev_b32_sdwa " D ", %[k4], " S " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t"
#define E64_ADDR3(D, S) E64_SDWA(D, S, "BYTE_3")
#define E64_ADDR2(D, S) E64_SDWA(D, S, "BYTE_2")
#define E64_ADDR1(D, S) E64_SDWA(D, S, "BYTE_1")
#define E64_ADDR0(D, S) E64_SDWA(D, S, "BYTE_0")
// renormalisation of state {XL, XH} with record dword C = cmpl (T: temporary)
#define E64_FRONT(XL, XH, C, T)                                                                                         \
    "v_lshl_add_u32 " T ", " C ", %[kv], " XH "\n\t"                                                                    \
    "v_cmpx_gt_i32 vcc, 0, " T "\n\t"                                                                                   \
    "v_add_u32 %[wk], %[m256], %[wk]\n\t"                                                                               \
    "v_bfi_b32 %[wk], %[m1fff], %[wk], %[ring]\n\t"                                                                     \
    "ds_write_b32 %[wk], " XL "\n\t"                                                                                    \
    "v_mov_b32 " XL ", " XH "\n\t"                                                                                      \
    "v_mov_b32 " XH ", 0\n\t"                                                                                           \
    "s_mov_b64 exec, -1\n\t"
// x = x + bias + (mulhi64(x, rcp) >> rcp_shift) * cmpl; X = "v[a:b]" of {XL, XH}; record R0..R3 = {rcp lo, rcp hi,
// bias << 6 | rcp_shift, cmpl}; TA / BP: pairs whose high register is permanently zero (TAL, BPL their low registers),
// TZ = {TZL, TZH}: the high dword of the middle sum and its carry.  mulhi64 as
//   t  = hi(xl * r0)
//   P1 = xh * r0 + t                 (< 2^63 + 2^32: xh < 2^31)
//   P2 = xl * r1 + P1                (may pass 2^64: the carry comes out of v_mad_u64_u32 in vcc)
//   RR = xh * r1 + {hi(P2), carry}
// -- the second product takes the WHOLE first one as its addend instead of a {low dword, 0} pair (round 4; three moves and
// a 64-bit add less); the shift takes its count from the low six bits of the record's third dword as they are
// (v_lshrrev_b64 looks at no others).  11 VALU (14 before).  Two instructions stand between the v_mad_u64_u32 that
// writes vcc and the v_addc that reads it (gfx940: a VALU write of an SGPR needs two wait states before a VALU reads it).
#define E64_BACK(X, XL, XH, R0, R1, R2, R3, TA, TAL, P1, TZ, TZL, TZH, P2, P2H, RR, RRL, RRH, BP, BPL, ZERO)             \
    "v_mul_hi_u32 " TAL ", " XL ", " R0 "\n\t"                                                                          \
    "v_mad_u64_u32 " P1 ", vcc, " XH ", " R0 ", " TA "\n\t"                                                             \
    "v_mad_u64_u32 " P2 ", vcc, " XL ", " R1 ", " P1 "\n\t"                                                             \
    "v_lshrrev_b32 " BPL ", 6, " R2 "\n\t"                                                                              \
    "v_mov_b32 " TZL ", " P2H "\n\t"                                                                                    \
    "v_addc_co_u32 " TZH ", vcc, 0, " ZERO ", vcc\n\t"                                                                  \
    "v_mad_u64_u32 " RR ", vcc, " XH ", " R1 ", " TZ "\n\t"                                                             \
    "v_lshrrev_b64 " RR ", " R2 ", " RR "\n\t"                                                                          \
    "v_lshl_add_u64 " X ", " X ", 0, " BP "\n\t"                                                                        \
    "v_mad_u64_u32 " X ", vcc, " RRL ", " R3 ", " X "\n\t"                                                              \
    "v_mad_u32_u24 " XH ", " RRH ", " R3 ", " XH "\n\t"
#define E64_BACK_A(R0, R1, R2, R3)                                                                                      \
    E64_BACK("v[40:41]", "v40", "v41", R0, R1, R2, R3, "v[64:65]", "v64", "v[66:67]", "v[68:69]", "v68", "v69",          \
             "v[70:71]", "v71", "v[72:73]", "v72", "v73", "v[76:77]", "v76", "v65")
#define E64_BACK_B(R0, R1, R2, R3)                                                                                      \
    E64_BACK("v[42:43]", "v42", "v43", R0, R1, R2, R3, "v[64:65]", "v64", "v[66:67]", "v[68:69]", "v68", "v69",          \
             "v[70:71]", "v71", "v[72:73]", "v72", "v73", "v[76:77]", "v76", "v65")
// one pair of symbols (the odd one = state 1 first: it is the later symbol) with its records in set 0 (v48..v55: state 1
// in v[48:51], state 0 in v[52:55]) or set 1 (v56..v63); PRE = address + read instructions of the NEXT pair, WAIT = lgkmcnt
#define E64_PAIR0(PRE, WAIT)                                                                                            \
    PRE "s_waitcnt lgkmcnt(" WAIT ")\n\t"                                                                               \
    E64_TRACK0                                                                                                          \
    E64_FRONT("v42", "v43", "v51", "v74") E64_FRONT("v40", "v41", "v55", "v74")                                         \
    E64_BACK_B("v48", "v49", "v50", "v51") E64_BACK_A("v52", "v53", "v54", "v55")
#define E64_PAIR1(PRE, WAIT)                                                                                            \
    PRE "s_waitcnt lgkmcnt(" WAIT ")\n\t"                                                                               \
    E64_TRACK1                                                                                                          \
    E64_FRONT("v42", "v43", "v59", "v74") E64_FRONT("v40", "v41", "v63", "v74")                                         \
    E64_BACK_B("v56", "v57", "v58", "v59") E64_BACK_A("v60", "v61", "v62", "v63")
// reads of a pair into set 0 / set 1: bytes (JB, JA) of symbol dword S
#define E64_READ0(ADDRB, ADDRA, S)                                                                                      \
    ADDRB("v78", S) ADDRA("v79", S) "ds_read_b128 v[48:51], v78\n\tds_read_b128 v[52:55], v79\n\t"
#define E64_READ1(ADDRB, ADDRA, S)                                                                                      \
    ADDRB("v78", S) ADDRA("v79", S) "ds_read_b128 v[56:59], v78\n\tds_read_b128 v[60:63], v79\n\t"
#define E64_CLOBBERS                                                                                                    \
    "vcc", "memory", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62",  \
        "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79"

// 16 symbols (dwords s3 = the last four .. s0 = the first four of the group), last symbol first
#define E64_GROUP_ASM                                                                                                   \
    asm volatile(E64_ZERO                                                                                               \
                 E64_READ0(E64_ADDR3, E64_ADDR2, "%[s3]")                                                               \
                 E64_PAIR0(E64_READ1(E64_ADDR1, E64_ADDR0, "%[s3]"), "2")                                               \
                 E64_PAIR1(E64_READ0(E64_ADDR3, E64_ADDR2, "%[s2]"), "2")                                               \
                 E64_PAIR0(E64_READ1(E64_ADDR1, E64_ADDR0, "%[s2]"), "2")                                               \
                 E64_PAIR1(E64_READ0(E64_ADDR3, E64_ADDR2, "%[s1]"), "2")                                               \
                 E64_PAIR0(E64_READ1(E64_ADDR1, E64_ADDR0, "%[s1]"), "2")                                               \
                 E64_PAIR1(E64_READ0(E64_ADDR3, E64_ADDR2, "%[s0]"), "2")                                               \
                 E64_PAIR0(E64_READ1(E64_ADDR1, E64_ADDR0, "%[s0]"), "2")                                               \
                 E64_PAIR1("", "0")                                                                                     \
                 : "+{v[40:41]}"(xA), "+{v[42:43]}"(xB), [wk] "+v"(wk), [worst] "+v"(worst)                             \
                 : [s3] "v"(s3), [s2] "v"(s2), [s1] "v"(s1), [s0] "v"(s0), [k4] "v"(k4), [m256] "v"(m256),              \
                   [m1fff] "v"(m1fff), [ring] "v"(ring), [kv] "v"(kv)                                                   \
                 : E64_CLOBBERS)
// TRACK: the model has byte values without a record (their cmpl = M is the largest value any record holds: v_max3 over
// the pairs' cmpl words finds it); EncParams::dense256 models run without
template <bool TRACK>
__device__ __forceinline__ void r64x2_encode_group(uint64_t &xA, uint64_t &xB, uint32_t &wk, uint32_t &worst, uint32_t s3,
                                                   uint32_t s2, uint32_t s1, uint32_t s0, uint32_t k4, uint32_t m256,
                                                   uint32_t m1fff, uint32_t ring, uint32_t kv)
{
    if constexpr (TRACK) {
#define E64_TRACK0 "v_max3_u32 %[worst], %[worst], v51, v55\n\t"
#define E64_TRACK1 "v_max3_u32 %[worst], %[worst], v59, v63\n\t"
        E64_GROUP_ASM;
#undef E64_TRACK0
#undef E64_TRACK1
    } else {
#define E64_TRACK0 ""
#define E64_TRACK1 ""
        E64_GROUP_ASM;
#undef E64_TRACK0
#undef E64_TRACK1
    }
}

template <bool TRACK>
__global__ void __launch_bounds__(1024) k_encode_lanes_r64x2(const EncParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    {   // EncRec {freq | rcp_shift << 24, bias, rcp lo, rcp hi} (model.h) -> {rcp lo, rcp hi, bias << 6 | rcp_shift, cmpl};
        // a symbol without a frequency: cmpl = M (the largest value any record holds: v_max3 finds it), rcp = 0
        const uint4 *g = reinterpret_cast<const uint4 *>(p.enc_recs);
        uint4 *l = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) {
            uint4 r = i < p.nsyms ? g[i] : uint4{0u, 0u, 0u, 0u};
            const uint32_t freq = r.x & 0xffffffu;
            l[i] = freq ? uint4{r.z, r.w, (r.y << 6) | (r.x >> 24), (1u << p.scale_bits) - freq}
                        : uint4{0u, 0u, 0u, 1u << p.scale_bits};
        }
        if (p.status) // (a block may be as small as one coding wave + the scanner: 128 threads for 132 words)
            for (uint32_t i = threadIdx.x; i < kEncMailboxBytes / 4u; i += blockDim.x)
                reinterpret_cast<uint32_t *>(smem + p.mailbox_off)[i] = 0u;
    }
    __syncthreads();
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const bool fused = p.status != nullptr;
    const uint32_t waves_per_block = (blockDim.x >> 6) - (fused ? kLaneCopiers : 0u); // coding waves
    LaneRounds *ctl = reinterpret_cast<LaneRounds *>(smem + p.mailbox_off);
    if (!lds_starts_at_zero(smem)) { // the asm addresses the record table by raw LDS offsets
        if (threadIdx.x == 0)
            atomicOr(p.flags, 4u);
        return;
    }
    if (fused && wave >= waves_per_block) { // ---- the scanner wave and the copier waves
        if (wave == waves_per_block)
            lanes_scanner(p, ctl, lane, waves_per_block);
        else
            lanes_copier(p, ctl, wave - waves_per_block - 1u, lane, waves_per_block);
        return;
    }
    const uint32_t ringbase = kR64EncTable + wave * kR64EncRing; // LDS byte offset, 8 KiB aligned
    const uint32_t *ringp = reinterpret_cast<const uint32_t *>(smem + ringbase);
    uint32_t k4 = 4u, m256 = 0xffffff00u, m1fff = 0x1fffu, ringv = ringbase, kv = 31u - p.scale_bits;
    asm volatile("v_mov_b32 %0, %0" : "+v"(k4)); // VGPR copies: a VALU op with a literal or an SGPR operand issues slower
    asm volatile("v_mov_b32 %0, %0" : "+v"(m256));
    asm volatile("v_mov_b32 %0, %0" : "+v"(m1fff));
    asm volatile("v_mov_b32 %0, %0" : "+v"(ringv));
    asm volatile("v_mov_b32 %0, %0" : "+v"(kv));
    const uint32_t m = lane & 3u, q4 = lane & ~3u;
    const uint32_t slot_lines = (uint32_t)(p.slot_bytes / kLaneLine);
    const uint32_t nblocks = p.chunk_syms >> 6;
    uint32_t worst = 0;
    LaneCoder cs{0};

    const uint64_t total_waves = (uint64_t)gridDim.x * waves_per_block;
    for (uint64_t batch_v = p.batch_begin + (uint64_t)blockIdx.x * waves_per_block + wave;; batch_v += total_waves) {
        if (fused) { // the block's scanner hands out the rounds
            batch_v = lanes_round_begin(p, ctl, cs, wave, waves_per_block, lane);
            if (batch_v == ~0ull - 1u) { // nothing for this wave in the last unit
                lanes_round_end(p, ctl, cs, wave, lane, batch_v, 0u);
                continue;
            }
        }
        if (batch_v >= p.batch_end)
            break;
        const uint64_t batch = uniform64(batch_v);
        const uint64_t chunk0 = batch * 64u;
        const uint64_t slots0 = reinterpret_cast<uint64_t>(p.scratch) + chunk0 * p.slot_bytes; // wave-uniform
        // symbol lines: instruction t = the line of the quad's lane t, this lane its piece m
        const uint64_t src0 = reinterpret_cast<uint64_t>(p.syms) + chunk0 * (uint64_t)p.chunk_syms + 16u * m;
        auto load_block = [&](u32x4 (&q)[4], uint32_t b) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                q[t] = __builtin_nontemporal_load(
                    reinterpret_cast<gvec_cptr>(src0 + (uint64_t)(q4 + t) * p.chunk_syms + 64ull * b));
        };

        uint64_t xA = 1ull << 31, xB = 1ull << 31; // Rans64EncInit
        uint32_t wk = ringbase + ((((uint32_t)p.slot_bytes & 127u) >> 2) << 8) + lane * 4u; // ring position of slot offset w
        uint32_t flushed = slot_lines; // lines [flushed, slot_lines) of this lane's slot are in memory

        // bytes of this lane's stream that are in the ring only: below line `flushed`, at most 127
        auto pending = [&]() { return (((flushed & 1u) << 6) - ((wk >> 6) & 124u)) & 127u; };
        // the whole wave takes part: lanes say which line they have filled (or, at the end, hold anything of), the quad
        // writes the line of its lane t with instruction t
        bool ovf = false; // sized slots: this lane's chunk needs a line below its slot
        auto flush = [&](bool need) {
            if (need && flushed == 0u) {
                ovf = true;
                need = false;
            }
            const int32_t line = need ? (int32_t)(flushed - 1u) : -1;
            if (need)
                flushed -= 1u;
            if (__builtin_amdgcn_ballot_w64(need) == 0)
                return;
            const int32_t lts[4] = {(int32_t)quad_perm<0x00>((uint32_t)line), (int32_t)quad_perm<0x55>((uint32_t)line),
                                    (int32_t)quad_perm<0xAA>((uint32_t)line), (int32_t)quad_perm<0xFF>((uint32_t)line)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int32_t lt = lts[t]; // the line asked for by the quad's lane t
                if (lt >= 0) {
                    // ring half (lt & 1), dwords 4 m .. 4 m + 3 of lane q4 + t
                    const uint32_t *at = ringp + ((uint32_t)lt & 1u) * 1024u + m * 256u + q4 + t;
                    const u32x4 v = {at[0], at[64], at[128], at[192]};
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>(slots0 + (uint64_t)(q4 + t) * p.slot_bytes + (uint64_t)lt * kLaneLine +
                                                           16u * m) = v;
                }
            }
        };

        u32x4 cur[4], nxt[4];
        load_block(cur, nblocks - 1u);
        quad_transpose(cur[0], cur[1], cur[2], cur[3], lane);
        for (uint32_t b = nblocks; b-- > 0;) {
            if (b > 0)
                load_block(nxt, b - 1u);
#pragma unroll
            for (int g = 3; g >= 0; --g) {
                r64x2_encode_group<TRACK>(xA, xB, wk, worst, cur[g][3], cur[g][2], cur[g][1], cur[g][0], k4, m256, m1fff, ringv,
                                          kv);
                flush(pending() >= 64u);
            }
            if (b > 0) {
                quad_transpose(nxt[0], nxt[1], nxt[2], nxt[3], lane);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    cur[t] = nxt[t];
            }
        }
        // flush: state 1 first, state 0 ends up first in memory (main64.cpp:244-245; Rans64EncFlush: two dwords, low first)
        {
            auto emit = [&](uint32_t v) {
                wk = ringbase + ((wk - 256u) & 0x1fffu);
                *reinterpret_cast<uint32_t *>(smem + wk) = v;
            };
            emit((uint32_t)(xB >> 32));
            emit((uint32_t)xB);
            emit((uint32_t)(xA >> 32));
            emit((uint32_t)xA);
        }
        const uint32_t in_ring = pending(); // <= 63 + 16
        const uint32_t len = (uint32_t)p.slot_bytes - (flushed * kLaneLine - in_ring);
        flush(in_ring > 0u); // the line(s) that hold anything; what lies below the stream start in the lowest one is never read
        flush(in_ring > 64u);
        p.lengths[chunk0 + lane] = len;
        lanes_publish_slot(p, chunk0 + lane, len, ovf);
        if (fused)
            lanes_round_end(p, ctl, cs, wave, lane, batch, len);
    }
    if (__builtin_amdgcn_ballot_w64(worst >= (1u << p.scale_bits)) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

// ---------------------------------------------------------------------------
// k_encode_batch_r64_lanes -- the ragged form of k_encode_lanes_r64x2 (rans_amd_encode_batch[_ordered] under
// RANS_AMD_OPT_BATCH_ENCODE_LANES): a wave's sixty-four lanes hold sixty-four STREAMS of the reference's 2-way rans64 layout
// (main64.cpp:224-246), the mirror image of decode_lanes.hip's k_decode_batch_r64_lanes.  The unit of work is one wave-load
// of the hand-out order, claimed through the pooled counters: lane l of claim w holds the stream at position 64 w + l --
// stream order[64 w + l], or 64 w + l without an order; a position at or past nchunks has no stream.  The group of sixteen
// (E64_*, r64x2_encode_group), the 16-byte records at LDS address 0 and the ring (32 dwords per lane, dword d of lane l at
// ring + 256 d + 4 l, 8 KiB aligned) are k_encode_lanes_r64x2's as they are; the prologue that builds the records is that
// kernel's, written out again here (a shared helper would be one more thing the uniform kernel's code depends on).
//   * the coder runs from a stream's last symbol to its first: symbol i is state (i & 1)'s, an odd count's last symbol is
//     state 0's alone and is coded first (main64.cpp:232-236); Rans64EncFlush of state 1 comes first, then state 0, so
//     state 0's two dwords are the stream's lowest.  A stream of 0 symbols is the two flushed initial states, 16 bytes;
//   * the stream ends at its slot's end.  Ring dword d holds the bytes [4 d, 4 d + 4) of a 128-byte window whose end is the
//     slot's end (mod 128); LINES of 64 bytes are counted DOWN from the slot's end, line j (1, 2, ...) = the bytes
//     (64 (j - 1), 64 j] below it, in ring half j & 1.  `fl` lines have left; what the ring alone holds (pending) follows
//     from fl and the ring position, as in the uniform kernel -- bytes are never counted per symbol.  A group emits at most
//     64 bytes and a flush follows every group, so pending < 64 in front of a group and < 128 behind it;
//   * flushes by quads: a lane that has filled line j asks for it (req = j << 2 | first piece), its quad writes the line's
//     16-byte pieces, lane m the piece m at slot_end - 64 j + 16 m, with the asking lane's slot end and slot size through
//     DPP.  Slots are multiples of 16 bytes, not of 64: a piece that would start below the slot's first byte is never
//     stored (it is the neighbour's), and of the last line only the pieces that hold stream bytes are (the piece with the
//     stream's first byte whole, as the wave kernels store it).  All stores lie inside [slot_at, slot_end), which the
//     index check has put inside [0, out_cap);
//   * symbols, by the address of the stream's first symbol:
//       64-byte aligned (rans_amd_batch_layout with sym_align = 64, the fast layout): whole 64-symbol blocks are fetched by
//         the quad, instruction t the line of the quad's lane t, transposed in registers, the next block in flight during
//         the current one (k_encode_lanes_r64x2's loads, each under "lane t still has a block");
//       on the 4-byte grid: the same blocks, but the lane fetches its own four 16-byte pieces at the top of the block,
//         not ahead of it;
//       any other address: no blocks, every symbol goes through the rounds below.
//     The count - 64 blocks symbols behind the last whole block are the END of the stream, so they are coded FIRST, one
//     compiler-scheduled round (one symbol per lane, a byte load fetched a round ahead) at a time, lanes without a symbol
//     sitting out (r64x2_put_one: E64_FRONT / E64_BACK in C++, the same records, the same ring);
//   * whole blocks run under full exec on the asm sequence, four groups each, the lane's last block first.
// The 64 lanes START together and finish at different times.  A lane is FINALISED at the top of the iteration q ==
// blocks_l, right behind its last group: the two flushed states, its last line or two, lengths[s] and offsets[s] =
// slot_end - lengths[s].  From then on it is DEAD, and so is, from the start, a lane without a stream or with a rejected
// one.  A dead lane rides along under full exec (E64_FRONT sets exec = -1 itself) and is left to run free -- it is never
// resumed, so nothing is put back but `worst`:
//   * nothing of its own leaves the ring: flush() asks for a line under `live` only, which is cleared for good, and a
//     quad reads a member's column only for the line that member asked for; everything of its stream had left the ring
//     when it was finalised (the two final flushes);
//   * it still takes part in its quad-mates' flushes: flush() is called by the whole wave outside any divergent branch,
//     and the piece a lane stores is chosen by the ASKING lane's request alone;
//   * it writes only into its own column of the ring: the write position moves by -256 and is folded into the ring by
//     v_bfi (mask 0x1fff), which keeps its low eight bits, 4 l -- whatever its state becomes;
//   * it loads no symbol: the quad's load of lane t's line stands under q < that lane's blocks (0 for a lane that was dead
//     from the start), the lane's own loads under the same, the rounds' byte loads under k < tail; it codes zeros and
//     reads only the record of byte value 0;
//   * it cannot raise the model flag, even when byte value 0 has no record: `worst` is put back from a copy behind every
//     block for the lanes that did not run it, and the rounds track under `active` only;
//   * it cannot raise any other flag: bits 1 and 11 are set in the claim's set-up alone, bit 2 in the prologue.
// (k_encode_batch_byte_pairs needs a test with a dead pair at its ring's bound because a dead pair's CURSOR counts on without
// limit and is folded into the row at every write; here there is no cursor -- the write position IS the folded ring address,
// 13 bits of a register whose other bits v_bfi takes from the ring's base at every step, so there is no bound to run past.)
// Index entries are the caller's data and checked exactly as k_encode_batch_byte_pairs checks them, with need = align16(4 *
// count + 2 * 8) = rans_amd_chunk_bound(): a state emits at most one dword per symbol (rans64.h:83-88).  A slot that fails
// is not written, lengths[s] = 0, offsets[s] = the slot's end, bit 1 of the flags; an order entry that names no stream codes
// nothing, writes no index entry and sets bit 11.  Every lane addresses symbols and slots in 64 bits.
// No MFMA: integer, table-driven, serial per state.
// ---------------------------------------------------------------------------
typedef uint32_t lanes_enc_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes on the 4-byte grid

// one symbol on state x, compiler-scheduled: E64_FRONT and E64_BACK on the group sequence's record {rcp lo, rcp hi,
// bias << 6 | rcp_shift, cmpl} and ring (wk: the lane's folded write position); a lane that is not `active` does nothing
__device__ __forceinline__ void r64x2_put_one(uint64_t &x, uint32_t sym, bool active, uint8_t *smem, uint32_t &wk, uint32_t ringbase,
                                              uint32_t kv, uint32_t &worst)
{
    const uint4 rec = reinterpret_cast<const uint4 *>(smem)[sym];
    if (active) {
        worst = rec.w > worst ? rec.w : worst;
        if ((int32_t)((rec.w << kv) + (uint32_t)(x >> 32)) < 0) { // rans64.h:83-88 on the high dword (see the uniform kernel)
            wk = ringbase + ((wk - 256u) & 0x1fffu);
            *reinterpret_cast<uint32_t *>(smem + wk) = (uint32_t)x;
            x >>= 32;
        }
        const uint64_t rcp = (uint64_t)rec.x | ((uint64_t)rec.y << 32);
        const uint64_t qv = __umul64hi(x, rcp) >> (rec.z & 63u); // rans64.h:91
        x = x + (rec.z >> 6) + qv * rec.w;                       // rans64.h:92
    }
}

template <bool TRACK>
__global__ void __launch_bounds__(1024) k_encode_batch_r64_lanes(const EncParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    {   // (k_encode_lanes_r64x2's prologue, written out) EncRec {freq | rcp_shift << 24, bias, rcp lo, rcp hi} (model.h) ->
        // {rcp lo, rcp hi, bias << 6 | rcp_shift, cmpl}; a symbol without a frequency: cmpl = M, the largest value any record holds
        const uint4 *g = reinterpret_cast<const uint4 *>(p.enc_recs);
        uint4 *l = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) {
            uint4 r = i < p.nsyms ? g[i] : uint4{0u, 0u, 0u, 0u};
            const uint32_t freq = r.x & 0xffffffu;
            l[i] = freq ? uint4{r.z, r.w, (r.y << 6) | (r.x >> 24), (1u << p.scale_bits) - freq}
                        : uint4{0u, 0u, 0u, 1u << p.scale_bits};
        }
    }
    __syncthreads();
    if (!lds_starts_at_zero(smem)) { // the asm addresses the record table by raw LDS offsets
        if (threadIdx.x == 0)
            atomicOr(p.flags, 4u);
        return;
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t ringbase = kR64EncTable + wave * kR64EncRing; // LDS byte offset, 8 KiB aligned
    const uint32_t *ringp = reinterpret_cast<const uint32_t *>(smem + ringbase);
    uint32_t k4 = 4u, m256 = 0xffffff00u, m1fff = 0x1fffu, ringv = ringbase, kv = 31u - p.scale_bits;
    asm volatile("v_mov_b32 %0, %0" : "+v"(k4)); // VGPR copies: a VALU op with a literal or an SGPR operand issues slower
    asm volatile("v_mov_b32 %0, %0" : "+v"(m256));
    asm volatile("v_mov_b32 %0, %0" : "+v"(m1fff));
    asm volatile("v_mov_b32 %0, %0" : "+v"(ringv));
    asm volatile("v_mov_b32 %0, %0" : "+v"(kv));
    const uint32_t m = lane & 3u, q4 = lane & ~3u;
    const uint32_t loads = (uint32_t)(((uint64_t)p.nchunks + 63u) >> 6); // wave-loads, one per claim (the last one may hold fewer than 64
                                                                         // streams); stream indices are 32-bit
    uint32_t worst = 0;
    WorkClaims work;
    work.init(p.claims, wave, waves_per_block);
    for (;;) {
        const uint64_t load = work.take(lane);
        if ((load >> 32) != 0 || (uint32_t)load >= loads) // (scalar compares)
            break;
        // ---- this lane's stream: its index entries, all of them the caller's data
        const uint64_t pos = load * 64u + lane;
        const bool exists = pos < p.nchunks;
        uint32_t s = (uint32_t)pos; // (stream indices are 32-bit)
        if (exists && p.order)
            s = p.order[pos];
        const bool named = exists && s < p.nchunks;
        if (exists && !named) // an order entry that names no stream: nothing coded, no index entry
            atomicOr(p.flags, 2048u);
        uint64_t first = 0, slot_at = 0, slot_end = 0;
        uint32_t count = 0;
        if (named) {
            first = p.sym_offsets[s];
            count = p.sym_counts[s];
            slot_at = p.slot_offsets[s];
            slot_end = p.slot_offsets[(uint64_t)s + 1u];
        }
        // what rans_amd_chunk_bound() asks for this stream: a dword per symbol + the two flushed states
        const uint64_t need = ((uint64_t)count * 4u + 2u * 8u + 15u) & ~15ull;
        const uint64_t slot_size = slot_end - slot_at;
        const bool fits = ((slot_at | slot_end) & 15u) == 0 && slot_end >= slot_at && slot_end <= p.out_cap && slot_size >= need &&
                          slot_size <= 0xfffffff0ull;
        if (named && !fits) { // nothing of this stream is written
            atomicOr(p.flags, 2u);
            p.lengths[s] = 0u;
            p.offsets[s] = slot_end;
        }
        bool live = named && fits; // the lane holds a stream that is still being coded
        const uint32_t slot16 = live ? (uint32_t)(slot_size >> 4) : 0u; // the slot in 16-byte pieces
        const uint64_t out_end = reinterpret_cast<uint64_t>(p.scratch) + slot_end; // (live: 16-byte aligned, inside the container)
        const uint64_t src = reinterpret_cast<uint64_t>(p.syms) + first;
        const bool by_quad = (src & 63u) == 0, by_dwords = (src & 3u) == 0;
        const uint32_t blocks = (live && by_dwords) ? count >> 6 : 0u; // (count < 2^30 follows from the slot's size)
        const uint32_t tail = live ? count - (blocks << 6) : 0u;
        const uint32_t qblocks = by_quad ? blocks : 0u; // blocks that the quad fetches
        // (wave_max32 is the pair kernels': it takes a value that both lanes of a pair hold, so the pair's larger one goes in)
        const uint32_t blocks_o = quad_perm<0xB1>(blocks), tail_o = quad_perm<0xB1>(tail); // the lane ^ 1's
        const uint32_t max_blocks = wave_max32(blocks > blocks_o ? blocks : blocks_o), max_tail = wave_max32(tail > tail_o ? tail : tail_o);

        uint64_t xA = 1ull << 31, xB = 1ull << 31; // Rans64EncInit
        uint32_t wk = ringbase + lane * 4u;        // the window's end: the first dword goes to ring dword 31
        uint32_t fl = 0;                           // lines 1 .. fl of this lane's stream are in memory

        // bytes of this lane's stream that are in the ring only: below line fl, at most 127
        auto pending = [&]() { return (((fl & 1u) << 6) - ((wk >> 6) & 124u)) & 127u; };
        // The whole wave takes part, outside any divergent branch.  A lane that `wants` has its next line, fl + 1, written
        // by its quad: the pieces that hold any of the `have` stream bytes so far, and none that starts below the slot.
        auto flush = [&](bool wants, uint32_t have) {
            uint32_t req = 0; // line << 2 | first piece with stream bytes
            if (wants) {
                const uint64_t reach = 64ull * (fl + 1u);
                req = ((fl + 1u) << 2) | (reach > have ? (uint32_t)((reach - have) >> 4) : 0u);
                fl += 1u;
            }
            if (__builtin_amdgcn_ballot_w64(req != 0u) == 0)
                return;
            const uint32_t elo = (uint32_t)out_end, ehi = (uint32_t)(out_end >> 32);
            auto piece = [&](auto tc, uint32_t rt, uint32_t lo, uint32_t hi, uint32_t sl) { // rt: what the quad's lane t asked for
                constexpr uint32_t t = decltype(tc)::value;
                const uint32_t line = rt >> 2;
                const uint32_t below16 = 4u * line - m; // this lane's piece starts 16 * below16 bytes under the slot's end
                if (rt != 0u && m >= (rt & 3u) && below16 <= sl) {
                    // ring half (line & 1), dwords 4 m .. 4 m + 3 of lane q4 + t
                    const uint32_t *at = ringp + (line & 1u) * 1024u + m * 256u + q4 + t;
                    const u32x4 v = {at[0], at[64], at[128], at[192]};
                    *reinterpret_cast<u32x4 RANS_GLOBAL *>((((uint64_t)hi << 32) | lo) - 16ull * below16) = v;
                }
            };
            piece(std::integral_constant<uint32_t, 0>{}, quad_perm<0x00>(req), quad_perm<0x00>(elo), quad_perm<0x00>(ehi), quad_perm<0x00>(slot16));
            piece(std::integral_constant<uint32_t, 1>{}, quad_perm<0x55>(req), quad_perm<0x55>(elo), quad_perm<0x55>(ehi), quad_perm<0x55>(slot16));
            piece(std::integral_constant<uint32_t, 2>{}, quad_perm<0xAA>(req), quad_perm<0xAA>(elo), quad_perm<0xAA>(ehi), quad_perm<0xAA>(slot16));
            piece(std::integral_constant<uint32_t, 3>{}, quad_perm<0xFF>(req), quad_perm<0xFF>(elo), quad_perm<0xFF>(ehi), quad_perm<0xFF>(slot16));
        };

        // ---- the rounds: the symbols behind the last whole block, the stream's last symbol first
        {
            const uint8_t RANS_GLOBAL *tsrc = reinterpret_cast<const uint8_t RANS_GLOBAL *>(src);
            uint32_t sym_next = tail != 0u ? (uint32_t)tsrc[count - 1u] : 0u;
            for (uint32_t k = 0; k < max_tail; ++k) {
                const bool active = k < tail;
                const uint32_t i = count - 1u - k; // (active lanes: the symbol's index in the stream)
                const uint32_t sym = sym_next;
                sym_next = k + 1u < tail ? (uint32_t)tsrc[i - 1u] : 0u;
                const bool odd = (i & 1u) != 0u;
                uint64_t x = odd ? xB : xA;
                uint32_t w = 0;
                r64x2_put_one(x, sym, active, smem, wk, ringbase, kv, w);
                if (TRACK)
                    worst = w > worst ? w : worst;
                xA = active && !odd ? x : xA;
                xB = active && odd ? x : xB;
                if ((k & 15u) == 15u) // (sixteen rounds: at most 64 bytes)
                    flush(live && pending() >= 64u, ~0u);
            }
            flush(live && pending() >= 64u, ~0u);
        }

        // ---- whole blocks, the lane's last block first
        // symbol lines: instruction t = the line of the quad's lane t (while that lane has blocks left), this lane its piece m
        auto load_block = [&](u32x4 (&v)[4], uint32_t q) {
            const uint32_t slo = (uint32_t)src, shi = (uint32_t)(src >> 32);
            const uint32_t qbs[4] = {quad_perm<0x00>(qblocks), quad_perm<0x55>(qblocks), quad_perm<0xAA>(qblocks), quad_perm<0xFF>(qblocks)};
            const uint32_t los[4] = {quad_perm<0x00>(slo), quad_perm<0x55>(slo), quad_perm<0xAA>(slo), quad_perm<0xFF>(slo)};
            const uint32_t his[4] = {quad_perm<0x00>(shi), quad_perm<0x55>(shi), quad_perm<0xAA>(shi), quad_perm<0xFF>(shi)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[t] = u32x4{0u, 0u, 0u, 0u}; // (a lane without a block codes zeros)
                if (q < qbs[t]) // block qbs[t] - 1 - q of lane t's stream, my piece of it
                    v[t] = __builtin_nontemporal_load(reinterpret_cast<gvec_cptr>(
                        (((uint64_t)his[t] << 32) | los[t]) + ((uint64_t)(qbs[t] - 1u - q) << 6) + 16u * m));
            }
        };
        u32x4 cur[4], nxt[4];
        load_block(cur, 0u);
        quad_transpose(cur[0], cur[1], cur[2], cur[3], lane);
        for (uint32_t q = 0;; ++q) {
            // ---- finalise the lanes whose last group is behind them
            const bool fin = live && q == blocks;
            if (__builtin_amdgcn_ballot_w64(fin) != 0) {
                uint32_t len = 0, in_ring = 0;
                if (fin) {
                    // state 1 first, state 0 ends up first in memory (main64.cpp:244-245; Rans64EncFlush: two dwords, low first)
                    auto emit = [&](uint32_t v) {
                        wk = ringbase + ((wk - 256u) & 0x1fffu);
                        *reinterpret_cast<uint32_t *>(smem + wk) = v;
                    };
                    emit((uint32_t)(xB >> 32));
                    emit((uint32_t)xB);
                    emit((uint32_t)(xA >> 32));
                    emit((uint32_t)xA);
                    in_ring = pending(); // <= 63 + 16
                    len = fl * kLaneLine + in_ring;
                }
                flush(fin && in_ring > 0u, len); // the line(s) that hold anything
                flush(fin && in_ring > 64u, len);
                if (fin) {
                    p.lengths[s] = len;
                    p.offsets[s] = out_end - reinterpret_cast<uint64_t>(p.scratch) - len; // the slot's end - len
                }
                live = live && !fin; // dead: no line, no index store ever again
            }
            if (q == max_blocks)
                break;
            const bool run = q < blocks;
            if (q + 1u < max_blocks)
                load_block(nxt, q + 1u);
            if (run && !by_quad) { // a stream on the 4-byte grid: the lane's own 64 bytes
                const uint64_t a = src + ((uint64_t)(blocks - 1u - q) << 6);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    cur[g] = *reinterpret_cast<const lanes_enc_u32x4_a4 RANS_GLOBAL *>(a + 16u * g);
            }
            const uint32_t worst_keep = worst;
#pragma unroll
            for (int g = 3; g >= 0; --g) {
                r64x2_encode_group<TRACK>(xA, xB, wk, worst, cur[g][3], cur[g][2], cur[g][1], cur[g][0], k4, m256, m1fff, ringv,
                                          kv); // (under full exec: see the head)
                flush(live && pending() >= 64u, ~0u);
            }
            worst = run ? worst : worst_keep;
            if (q + 1u < max_blocks) {
                quad_transpose(nxt[0], nxt[1], nxt[2], nxt[3], lane);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    cur[t] = nxt[t];
            }
        }
    }
    if (TRACK && __builtin_amdgcn_ballot_w64(worst >= (1u << p.scale_bits)) != 0 && lane == 0)
        atomicOr(p.flags, 1u);
}

// Lane-per-stream encoder, second generation: symbols arrive as 16-byte per-lane loads
// (one scattered access per 16 symbols instead of per symbol), one group prefetched.
template <int FMT, int NW>
__global__ void __launch_bounds__(256) k_encode_lanes16(const EncParams p)
{
    using Tr = FmtTraits<FMT>;
    using state_t = typename Tr::state_t;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(p.enc_recs);
        uint4 *l = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < p.nsyms; i += blockDim.x)
            l[i] = g[i];
    }
    __syncthreads();
    const uint4 *recs = reinterpret_cast<const uint4 *>(smem);
    const bool wide_in = p.sym_bytes == 1 && ((reinterpret_cast<uintptr_t>(p.syms) | p.chunk_syms) & 15u) == 0;

    bool bad = false;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t chunk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; chunk < p.nchunks; chunk += stride) {
        const uint64_t first = chunk * p.chunk_syms;
        const uint32_t nsym = (uint32_t)((p.n - first) < p.chunk_syms ? (p.n - first) : p.chunk_syms);
        const uint8_t RANS_GLOBAL *src = (const uint8_t RANS_GLOBAL *)p.syms + first * p.sym_bytes;
        uint8_t RANS_GLOBAL *slot = (uint8_t RANS_GLOBAL *)p.scratch + chunk * p.slot_bytes;
        uint8_t RANS_GLOBAL *wp = slot + p.slot_bytes;

        state_t x[NW];
#pragma unroll
        for (int l = 0; l < NW; ++l)
            x[l] = Tr::kL;

        // symbol i belongs to state i mod NW; visit i = nsym-1 .. 0 (main.cpp:233-243).
        // [0, fast_end) is walked in 16-symbol groups; the ragged top part one by one.
        const uint32_t fast_end = wide_in ? (nsym & ~15u) : 0u;
        for (uint32_t i = nsym; i > fast_end; --i) {
            const uint32_t sym = p.sym_bytes == 1 ? (uint32_t)src[i - 1]
                                                  : (uint32_t) reinterpret_cast<const uint16_t RANS_GLOBAL *>(src)[i - 1];
            const uint32_t l = (i - 1) % NW;
#pragma unroll
            for (int ll = 0; ll < NW; ++ll) // static register indexing
                if ((uint32_t)ll == l)
                    lane_put<FMT>(x[ll], sym, recs, p, wp, bad);
        }
        if (fast_end) {
            const u32x4 RANS_GLOBAL *g16 = reinterpret_cast<const u32x4 RANS_GLOBAL *>(src);
            uint32_t g = fast_end >> 4;
            u32x4 cur = g16[g - 1], nxt = cur;
            while (g-- > 0) {
                if (g > 0)
                    nxt = g16[g - 1];
#pragma unroll
                for (int j = 15; j >= 0; --j) {
                    const uint32_t sym = (cur[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    lane_put<FMT>(x[j % NW], sym, recs, p, wp, bad);
                }
                cur = nxt;
            }
        }
        // flush states NW-1 .. 0 (lane 0's first in memory)
#pragma unroll
        for (int l = NW - 1; l >= 0; --l) {
            wp -= Tr::kStateBytes;
            if constexpr (FMT == FMT_R64) {
                reinterpret_cast<uint32_t RANS_GLOBAL *>(wp)[0] = (uint32_t)x[l];
                reinterpret_cast<uint32_t RANS_GLOBAL *>(wp)[1] = (uint32_t)(x[l] >> 32);
            } else if constexpr (FMT == FMT_WORD) {
                reinterpret_cast<uint16_t RANS_GLOBAL *>(wp)[0] = (uint16_t)x[l];
                reinterpret_cast<uint16_t RANS_GLOBAL *>(wp)[1] = (uint16_t)(x[l] >> 16);
            } else {
                wp[0] = (uint8_t)x[l];
                wp[1] = (uint8_t)(x[l] >> 8);
                wp[2] = (uint8_t)(x[l] >> 16);
                wp[3] = (uint8_t)(x[l] >> 24);
            }
        }
        p.lengths[chunk] = (uint32_t)((slot + p.slot_bytes) - wp);
        lanes_publish_slot(p, chunk, (uint32_t)((slot + p.slot_bytes) - wp));
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane_id() == 0)
        atomicOr(p.flags, 1u);
}

// The staged lane encoder (coalesced symbol loads, whole-line stream stores, fused placement) takes u8 symbols in
// 16-byte aligned chunks with slots made of whole lines, from six batches per CU on.  Everything else -- u16 symbols, chunk
// sizes that are not multiples of 16, unaligned buffers, a handful of batches -- is the NAMED FALLBACK's: the first generation's
// per-lane encoder k_encode_lanes16 (one chunk per lane, unit-by-unit stores).  Returns the waves per block the LDS allows, 0 = no.
static uint32_t encode_lanes_staged_waves(const EncParams &p, int num_cus, uint64_t min_batches_per_cu = 6)
{
    const size_t table_lds = (size_t)p.nsyms * sizeof(EncRec);
    // (room for the scanner wave and the control words of the fused placement, whether or not this launch uses them)
    const size_t fixed_lds = table_lds + 16 + kEncMailboxBytes;
    uint32_t sw = fixed_lds + kEncWaveLds <= 160 * 1024 ? (uint32_t)((160 * 1024 - fixed_lds) / kEncWaveLds) : 0;
    sw = sw > 16 - kLaneCopiers ? 16 - kLaneCopiers : sw;
    const bool staged = sw >= 1 && p.sym_bytes == 1 && (p.slot_bytes % kLaneLine) == 0 &&
                        ((reinterpret_cast<uintptr_t>(p.syms) | p.chunk_syms) & 15u) == 0 &&
                        (reinterpret_cast<uintptr_t>(p.scratch) & 15u) == 0 &&
                        // fewer, longer batches: the per-lane kernel's many small blocks hide latency better
                        (p.nchunks + 63) / 64 >= (uint64_t)num_cus * min_batches_per_cu;
    return staged ? sw : 0u;
}

// The shape the dedicated 2-way rans64 encoder k_encode_lanes_r64x2 takes (the reference's layout, config 2): whole batches
// of full chunks of a multiple of 64 symbols, at least one batch per CU.  launch_encode_lanes_t and encode_lanes_sized_ok
// both ask here, so that api.cpp is told what the launcher will do.
static bool encode_lanes_r64x2_shape(int format, const EncParams &p, int num_cus)
{
    return format == FMT_R64 && p.n_ways == 2 && (p.chunk_syms & 63u) == 0 && p.scale_bits >= 7 && p.scale_bits <= 16 &&
           p.nsyms <= 256 && (p.n / p.chunk_syms) / 64 >= (uint64_t)num_cus;
}

// Batches per CU from which the staged kernels are worth it.  (The dedicated 2-way rans64 encoder from one batch per CU
// on: 4096-symbol chunks, 1024 batches of config 2's 256 MiB, 0.78 ms with the per-lane kernel -- but not with the fused
// placement, where the answer must stay the one encode_lanes_fused() gave api.cpp.)
static uint64_t encode_lanes_min_batches(int format, const EncParams &p, int num_cus)
{
    return encode_lanes_r64x2_shape(format, p, num_cus) && !p.status ? 1 : 6;
}

template <int FMT, int NW> hipError_t launch_encode_lanes_t(const EncParams &p_in, int num_cus, hipStream_t stream, KernelId *name)
{
    EncParams p = p_in;
    const size_t table_lds = (size_t)p.nsyms * sizeof(EncRec);
    if (table_lds > 128 * 1024)
        return hipErrorInvalidValue;
    uint32_t sw = encode_lanes_staged_waves(p, num_cus, encode_lanes_min_batches(FMT, p, num_cus));
    const bool staged = sw >= 1;
    if (!staged && p.status)
        return hipErrorInvalidValue; // (api.cpp asks encode_lanes_fused() before it sets up the fused placement)
    if (staged) {
        // same split as the staged decoder: fewest rounds, batches spread evenly over them
        uint64_t batches = (p.nchunks + 63) / 64;
        p.batch_begin = 0;
        p.batch_end = batches;
        p.claim_slot = 0;
        p.unit_base = 0;
        if constexpr (FMT == FMT_R64 && NW == 2) {
            // the reference's 2-way rans64 layout (config 2) on its own kernel: whole batches of full chunks; what is
            // left (fewer than 64 chunks, the last one perhaps ragged) goes through the staged kernel below
            if (encode_lanes_r64x2_shape(FMT, p, num_cus)) {
                const uint64_t full_batches = (p.n / p.chunk_syms) / 64;
                // 8 KiB of table + 8 KiB of ring per coding wave (+ the scanner wave and its LDS words when it places the chunks)
                const uint32_t sw3 = lanes_even_waves(full_batches, num_cus, p.status ? 16 - kLaneCopiers : 16);
                // (a model in which every byte value has a frequency: the variant without the search for record-less symbols)
                auto kern3 = p.dense256 ? k_encode_lanes_r64x2<false> : k_encode_lanes_r64x2<true>;
                static std::atomic<uint64_t> lds_ok3[2] = {{0}, {0}};
                EncParams q = p;
                q.batch_end = full_batches;
                size_t lds3 = kR64EncTable + (size_t)sw3 * kR64EncRing;
                uint32_t waves3 = sw3;
                if (q.status) {
                    q.mailbox_off = (uint32_t)lds3;
                    lds3 += kEncMailboxBytes;
                    waves3 += kLaneCopiers;
                }
                if (name)
                    *name = KernelId::encode_lanes_r64x2;
                if (hipError_t e = launch_lanes(kern3, lds_ok3[p.dense256 ? 0 : 1], 160 * 1024,
                                                lanes_grid(full_batches, sw3, num_cus), 64 * waves3, lds3, stream, q);
                    e != hipSuccess)
                    return e;
                if (full_batches == batches)
                    return hipSuccess;
                p.batch_begin = full_batches; // the tail: its own claim counter, its units behind the ones of this launch
                p.claim_slot = 1;
                p.unit_base = (full_batches + sw3 - 1) / sw3;
                batches -= full_batches;
            }
        }
        sw = lanes_even_waves(batches, num_cus, sw);
        static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
        size_t lds = table_lds + (size_t)sw * kEncWaveLds;
        uint32_t waves = sw;
        if (p.status) { // fused placement: the block's scanner wave and its control words
            lds = (lds + 15) & ~(size_t)15;
            p.mailbox_off = (uint32_t)lds;
            lds += kEncMailboxBytes;
            waves += kLaneCopiers;
        }
        if (name && p.batch_begin == 0)
            *name = KernelId::encode_lanes_staged;
        return launch_lanes(k_encode_lanes_staged<FMT, NW>, lds_ok, 160 * 1024, lanes_grid(batches, sw, num_cus), 64 * waves, lds,
                            stream, p);
    }
    static std::atomic<uint64_t> lds_ok{0}; // per instantiation, one bit per device
    const uint64_t want = (p.nchunks + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus * 8;
    if (name)
        *name = KernelId::encode_lanes16;
    return launch_lanes(k_encode_lanes16<FMT, NW>, lds_ok, 128 * 1024, (uint32_t)(want < cap ? want : cap), 256, table_lds, stream,
                        p);
}

template <int FMT> hipError_t launch_encode_lanes_f(const EncParams &p, int num_cus, hipStream_t s, KernelId *name)
{
    switch (p.n_ways) {
    case 1: return launch_encode_lanes_t<FMT, 1>(p, num_cus, s, name);
    case 2: return launch_encode_lanes_t<FMT, 2>(p, num_cus, s, name);
    case 4: return launch_encode_lanes_t<FMT, 4>(p, num_cus, s, name);
    case 8: return launch_encode_lanes_t<FMT, 8>(p, num_cus, s, name);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

bool encode_lanes_fused(const EncParams &p, int num_cus) { return encode_lanes_staged_waves(p, num_cus) >= 1; }

// Sized slots: would launch_encode_lanes_t take one of its STAGED kernels (the 2-way rans64 one included) for this
// request?  Those flush whole lines and stop at their slot's first one; the per-lane kernel stores unit by unit and cannot
// tell that a chunk does not fit.  (The launcher's own question: encode_lanes_min_batches.)
bool encode_lanes_sized_ok(int format, const EncParams &p, int num_cus)
{
    if (format == FMT_WORD && encode_word_groups_applicable(p)) // (its block stores stop at the slot's first byte: encode_groups.hip)
        return true;
    return encode_lanes_staged_waves(p, num_cus, encode_lanes_min_batches(format, p, num_cus)) >= 1;
}

// The ragged form of the 2-way rans64 lane encoder: rans64 over u8 symbols at the scale_bits the group sequence takes (the
// caller has checked the format: the full-width variant is another kernel format), from 64 streams on; any symbol count, any
// symbol address.  The record table and at least one wave's ring inside the CU's 160 KiB of LDS (they always are: 16 KiB).
bool encode_batch_r64_lanes_applicable(const EncParams &p)
{
    return p.n_ways == 2 && p.sym_bytes == 1 && p.nsyms <= 256 && p.scale_bits >= 7 && p.scale_bits <= 16 && p.nchunks >= 64 &&
           (reinterpret_cast<uintptr_t>(p.scratch) & 15u) == 0 && kR64EncTable + kR64EncRing <= 160 * 1024;
}

hipError_t launch_encode_batch_r64_lanes(const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    if (!encode_batch_r64_lanes_applicable(p) || !p.enc_recs || !p.sym_offsets || !p.sym_counts || !p.slot_offsets || !p.lengths || !p.offsets ||
        !p.flags)
        return hipErrorInvalidValue;
    // one block per CU, as many waves as the table leaves rings for, sixteen at the most; a batch that does not fill them
    // spreads its wave-loads evenly (lanes_even_waves), as the lane decoder's launcher does
    const uint32_t room = (uint32_t)((160 * 1024 - kR64EncTable) / kR64EncRing);
    const uint32_t max_waves = room > 16 ? 16 : room;
    const uint64_t loads = (p.nchunks + 63) / 64;
    const uint32_t sw = loads >= (uint64_t)num_cus * max_waves ? max_waves : lanes_even_waves(loads, num_cus, max_waves);
    static std::atomic<uint64_t> lds_ok[2] = {{0}, {0}};
    if (name)
        *name = KernelId::encode_batch_r64_lanes;
    const size_t lds = kR64EncTable + (size_t)sw * kR64EncRing;
    // (a model in which every byte value has a frequency: the variant without the search for record-less symbols)
    return p.dense256 ? launch_lanes(k_encode_batch_r64_lanes<false>, lds_ok[0], 160 * 1024, lanes_grid(loads, sw, num_cus), 64 * sw, lds, stream, p)
                      : launch_lanes(k_encode_batch_r64_lanes<true>, lds_ok[1], 160 * 1024, lanes_grid(loads, sw, num_cus), 64 * sw, lds, stream, p);
}

hipError_t launch_encode_lanes(int format, const EncParams &p, int num_cus, hipStream_t stream, KernelId *name)
{
    switch (format) {
    case FMT_WORD: return launch_encode_lanes_f<FMT_WORD>(p, num_cus, stream, name);
    case FMT_BYTE: return launch_encode_lanes_f<FMT_BYTE>(p, num_cus, stream, name);
    case FMT_R64: return launch_encode_lanes_f<FMT_R64>(p, num_cus, stream, name);
    case FMT_ALIAS: return launch_encode_lanes_f<FMT_ALIAS>(p, num_cus, stream, name);
    default: return hipErrorInvalidValue;
    }
}

#undef E64_ZERO
#undef E64_SDWA
#undef E64_ADDR3
#undef E64_ADDR2
#undef E64_ADDR1
#undef E64_ADDR0
#undef E64_FRONT
#undef E64_BACK
#undef E64_BACK_A
#undef E64_BACK_B
#undef E64_PAIR0
#undef E64_PAIR1
#undef E64_READ0
#undef E64_READ1
#undef E64_CLOBBERS
#undef E64_GROUP_ASM

} // namespace rans_amd
