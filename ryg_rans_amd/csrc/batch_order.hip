// batch_order.hip -- rans_amd_batch_order: the streams of a ragged batch, longest first.
//
// The batch decoders hand their streams out dynamically (one claim per stream), so the order only matters at the end of a
// launch: a 64 Ki-symbol stream claimed last keeps one wave busy while the rest of the GPU idles.  What is wanted is not a
// sort but "long ones early": streams are binned by floor(log2(count + 1)) -- 33 buckets for 32-bit counts -- and written
// out bucket by bucket, the largest bucket first, in whatever order they arrive inside a bucket.  Three small kernels, no
// sort library:
//
//   k_order_hist     per-block histogram of the bucket keys in LDS, one global atomic per block and bucket
//   k_order_scan     33 totals -> where each bucket starts (descending keys), one wave
//   k_order_scatter  per block: ranks inside the block through LDS atomics, one global atomic per block and bucket reserves
//                    the block's piece of every bucket, then the indices are written
#include "launchers.hpp"

namespace rans_amd {

namespace {

constexpr uint32_t kOrderThreads = 256;
constexpr uint32_t kOrderItems = 8; // streams per thread: a block takes a tile of 2048
constexpr uint32_t kOrderTile = kOrderThreads * kOrderItems;

__device__ __forceinline__ uint32_t order_key(uint32_t count)
{
    return 63u - (uint32_t)__builtin_clzll((unsigned long long)count + 1ull); // floor(log2(count + 1)): 0 .. 32
}

__global__ void __launch_bounds__(kOrderThreads) k_order_hist(const uint32_t *counts, uint64_t n, uint32_t *hist)
{
    __shared__ uint32_t local[kOrderBuckets];
    if (threadIdx.x < kOrderBuckets)
        local[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kOrderTile;
#pragma unroll
    for (uint32_t j = 0; j < kOrderItems; ++j) {
        const uint64_t i = tile + (uint64_t)j * kOrderThreads + threadIdx.x;
        if (i < n)
            atomicAdd(&local[order_key(counts[i])], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kOrderBuckets && local[threadIdx.x])
        atomicAdd(hist + threadIdx.x, local[threadIdx.x]);
}

// hist[0 .. 33): totals per key; hist[33 .. 66) receives the first output position of every key, the largest key first
__global__ void __launch_bounds__(64) k_order_scan(uint32_t *hist)
{
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (int b = (int)kOrderBuckets - 1; b >= 0; --b) {
            hist[kOrderBuckets + b] = at;
            at += hist[b];
        }
    }
}

__global__ void __launch_bounds__(kOrderThreads) k_order_scatter(const uint32_t *counts, uint64_t n, uint32_t *cursor, uint32_t *order)
{
    __shared__ uint32_t local[kOrderBuckets], base[kOrderBuckets];
    if (threadIdx.x < kOrderBuckets)
        local[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kOrderTile;
    uint32_t key[kOrderItems], rank[kOrderItems];
#pragma unroll
    for (uint32_t j = 0; j < kOrderItems; ++j) {
        const uint64_t i = tile + (uint64_t)j * kOrderThreads + threadIdx.x;
        key[j] = 0u;
        rank[j] = 0u;
        if (i < n) {
            key[j] = order_key(counts[i]);
            rank[j] = atomicAdd(&local[key[j]], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kOrderBuckets)
        base[threadIdx.x] = local[threadIdx.x] ? atomicAdd(cursor + threadIdx.x, local[threadIdx.x]) : 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kOrderItems; ++j) {
        const uint64_t i = tile + (uint64_t)j * kOrderThreads + threadIdx.x;
        if (i < n) {
            const uint64_t at = (uint64_t)base[key[j]] + rank[j];
            if (at < n) // (always, unless the counts changed between the two passes: never write outside the permutation)
                order[at] = (uint32_t)i;
        }
    }
}

} // namespace

hipError_t launch_batch_order(const uint32_t *d_sym_counts, uint64_t n_streams, uint32_t *d_order, uint32_t *d_hist, int /*num_cus*/,
                              hipStream_t stream)
{
    if (n_streams == 0)
        return hipSuccess;
    if (n_streams > 0xffffffffull || !d_sym_counts || !d_order || !d_hist)
        return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)((n_streams + kOrderTile - 1) / kOrderTile);
    RANS_LAUNCH(k_order_hist, dim3(grid), dim3(kOrderThreads), 0, stream, d_sym_counts, n_streams, d_hist);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    RANS_LAUNCH(k_order_scan, dim3(1), dim3(64), 0, stream, d_hist);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    RANS_LAUNCH(k_order_scatter, dim3(grid), dim3(kOrderThreads), 0, stream, d_sym_counts, n_streams, d_hist + kOrderBuckets, d_order);
    return hipGetLastError();
}

} // namespace rans_amd
