// lanes_common.hpp -- what both directions of the lane-per-stream kernels share (decode_lanes.hip, encode_lanes.hip).
#pragma once

#include "device_common.hpp"
#include "launchers.hpp"

namespace rans_amd {

namespace {

typedef __amdgpu_buffer_rsrc_t rsrc_t;

// ===========================================================================
// Lane-per-stream kernels for narrow interleaves (N = 1, 2, 4, 8; BASELINE config 2 is
// the reference's 2-way rans64 loop, main64.cpp:224-287).  An N-way stream with N << 64
// cannot feed a wavefront, so here every LANE owns a whole chunk: its N states live in
// registers, it walks its own stream with its own pointer (the renormalisation order
// inside a chunk is the sequential reference order, no cross-lane work at all), and a
// wave decodes 64 chunks at once.  Tables are shared through LDS as before.
// ===========================================================================

// A lane's stream is staged in LDS in a 128-byte ring of two 64-byte lines (decode_lanes.hip has the why); ring rows are
// 136 bytes apart, so that equal positions of the 64 lanes spread over 32 banks.
constexpr uint32_t kLaneLine = 64;
constexpr uint32_t kLaneRingStride = 2 * kLaneLine + 8;

// 4 x 4 transpose of 16-byte pieces inside every quad of lanes: lane 4k+m, piece t  <->  lane 4k+t, piece m.  A
// lane that stores its own 64-byte line issues four 16-byte requests, and 64 lanes 64 of them per instruction -- the
// vector-memory address path (TA) was 86 % busy in these kernels (profiles/r02_lanes_counters.md); after the
// transpose store instruction t writes the whole line of the quad's lane t: one 64-byte request per quad.
template <int CTRL> __device__ __forceinline__ uint32_t quad_perm(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ void quad_transpose(u32x4 &q0, u32x4 &q1, u32x4 &q2, u32x4 &q3, uint32_t lane)
{
    const bool b0 = (lane & 1u) != 0, b1 = (lane & 2u) != 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) { // lane bit 0 <-> piece bit 0
        const uint32_t a = q0[d], b = q1[d], c = q2[d], e = q3[d];
        const uint32_t fa = quad_perm<0xA0>(b), fb = quad_perm<0xF5>(a); // [0,0,2,2]: from lane - 1, [1,1,3,3]: from lane + 1
        const uint32_t fc = quad_perm<0xA0>(e), fe = quad_perm<0xF5>(c);
        q0[d] = b0 ? fa : a;
        q1[d] = b0 ? b : fb;
        q2[d] = b0 ? fc : c;
        q3[d] = b0 ? e : fe;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) { // lane bit 1 <-> piece bit 1
        const uint32_t a = q0[d], b = q1[d], c = q2[d], e = q3[d];
        const uint32_t fa = quad_perm<0x44>(c), fc = quad_perm<0xEE>(a); // [0,1,0,1]: from lane - 2, [2,3,2,3]: from lane + 2
        const uint32_t fb = quad_perm<0x44>(e), fe = quad_perm<0xEE>(b);
        q0[d] = b1 ? fa : a;
        q2[d] = b1 ? c : fc;
        q1[d] = b1 ? fb : b;
        q3[d] = b1 ? e : fe;
    }
}

// ---------------------------------------------------------------------------
// Launch geometry of the staged lane kernels.  A wave takes batches of 64 chunks; one batch is a long latency-bound job,
// so a last round with a few waves per CU costs as much as a full one: take the fewest rounds the wave limit allows and
// split the batches evenly over them (16 batches per CU: 16 waves x 1 round, or 8 x 2 -- never 14 + 2).
// Callers guarantee batches >= 1, num_cus >= 1 and max_waves >= 1 (lanes_applicable: 64 chunks and more).
// ---------------------------------------------------------------------------
inline uint32_t lanes_even_waves(uint64_t batches, int num_cus, uint32_t max_waves) // -> coding waves per block, 1..max_waves
{
    const uint64_t per_cu = (batches + (uint64_t)num_cus - 1) / (uint64_t)num_cus;
    const uint64_t rounds = (per_cu + max_waves - 1) / max_waves;
    return (uint32_t)((per_cu + rounds - 1) / rounds);
}
inline uint32_t lanes_grid(uint64_t batches, uint32_t waves, int num_cus) // one block per CU at the most
{
    const uint64_t blocks = (batches + waves - 1) / waves;
    return (uint32_t)(blocks < (uint64_t)num_cus ? blocks : (uint64_t)num_cus);
}

// The tail of every launch: raise the kernel's dynamic-LDS limit (once per device, `lds_ok` is the kernel's bit set),
// launch, report this launch's status.
template <typename Kernel, typename Params>
hipError_t launch_lanes(Kernel kern, std::atomic<uint64_t> &lds_ok, int lds_limit, uint32_t grid, uint32_t threads, size_t lds,
                        hipStream_t stream, const Params &p)
{
    if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), lds_limit, lds_ok); e != hipSuccess)
        return e;
    RANS_LAUNCH(kern, dim3(grid), dim3(threads), lds, stream, p);
    return hipGetLastError();
}

} // namespace

} // namespace rans_amd
