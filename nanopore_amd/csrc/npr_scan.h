// npr_scan.h -- the one integer exclusive prefix sum of the analysis units ("counts -> offsets" on the device).  Included by .hip units
// only; the launchers are declared in npr_device.h and instantiated in npr_scan.hip, npr_pileup.hip builds its last pass from the pieces,
// and npr_seed.hip keeps a wider unchecked tile of its own on block_scan_exclusive (the reason is in its header).
//
// The contract, for In in {int32_t, uint32_t, int64_t} and Out in {int32_t, int64_t}:
//   out[i] = in[0] + ... + in[i - 1] for every i in 0 .. n, so out[n] is the total; in[n] is never read; n == 0 writes out[0] = 0;
//   in == out is allowed when the two types have the same width.
// Integer addition of a fixed width: the output does not depend on the order anything is summed in.
//   launch_scan_group  one workgroup, trips of SCAN_THREADS entries with a carry: one launch, for the thousands of entries of a per-read
//                      or per-tile table.
//   launch_scan_tiled  tiles of SCAN_TILE entries, SCAN_PER_THREAD consecutive ones per thread: the tiles' sums, their scan by the one
//                      workgroup in place, every tile on top of its offset.  `tile` is scratch of scan_tiles(n) entries.
#pragma once
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int SCAN_WAVE = 64;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_WAVES = SCAN_THREADS / SCAN_WAVE;
constexpr int SCAN_PER_THREAD = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD;

// One value per thread of a SCAN_THREADS workgroup -> the sum of the threads before it, and the workgroup's sum in *total; lds: SCAN_WAVES
// entries.  The first barrier keeps a second call from overwriting lds while a wavefront still reads the first call's sums.
template <typename T>
__device__ __forceinline__ T block_scan_exclusive(T v, T *lds, T *total) {
    const int lane = threadIdx.x & (SCAN_WAVE - 1), wv = threadIdx.x / SCAN_WAVE;
    T inc = v;  // inclusive, within the wavefront
#pragma unroll
    for (int o = 1; o < SCAN_WAVE; o <<= 1) {
        const T t = __shfl_up(inc, o, SCAN_WAVE);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == SCAN_WAVE - 1) lds[wv] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < SCAN_WAVES; ++q) {
        const T s = lds[q];
        if (q < wv) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// the thread's SCAN_PER_THREAD entries of its tile (0 from entry n on) and their sum
template <typename In, typename Out>
__device__ __forceinline__ Out scan_load(const In *in, int64_t n, int64_t j0, Out (&v)[SCAN_PER_THREAD]) {
    Out s = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) {
        v[q] = j0 + q < n ? static_cast<Out>(in[j0 + q]) : 0;
        s += v[q];
    }
    return s;
}
__device__ __forceinline__ int64_t scan_first_entry() { return static_cast<int64_t>(blockIdx.x) * SCAN_TILE + static_cast<int64_t>(threadIdx.x) * SCAN_PER_THREAD; }

// (a thread reads its entry of a trip before it writes it, and nobody else touches that entry: in place is safe)
template <typename In, typename Out>
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_group(const In *in, Out *out, int64_t n) {
    __shared__ Out lds[SCAN_WAVES];
    Out carry = 0;
    for (int64_t i0 = 0; i0 <= n; i0 += SCAN_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const Out v = i < n ? static_cast<Out>(in[i]) : 0;
        Out total;
        const Out ex = block_scan_exclusive(v, lds, &total);
        if (i <= n) out[i] = carry + ex;
        carry += total;
    }
}

template <typename In, typename Out>
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_tile_sums(const In *in, int64_t n, Out *tile) {
    __shared__ Out lds[SCAN_WAVES];
    Out v[SCAN_PER_THREAD], total;
    (void)block_scan_exclusive(scan_load(in, n, scan_first_entry(), v), lds, &total);
    if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// (a thread reads its entries before it writes them, and nobody else touches them: in place is safe)
template <typename In, typename Out>
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_tiles(const In *in, Out *out, int64_t n, const Out *tile) {
    __shared__ Out lds[SCAN_WAVES];
    const int64_t j0 = scan_first_entry();
    Out v[SCAN_PER_THREAD], total;
    Out run = block_scan_exclusive(scan_load(in, n, j0, v), lds, &total) + tile[blockIdx.x];
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) {
        if (j0 + q <= n) out[j0 + q] = run;
        run += v[q];
    }
}

}  // namespace

template <typename In, typename Out>
int launch_scan_group(const In *in, Out *out, int64_t n, void *stream) {
    if (n < 0) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL((k_scan_group<In, Out>), dim3(1), dim3(SCAN_THREADS), 0, static_cast<hipStream_t>(stream), in, out, n);
    return static_cast<int>(hipGetLastError());
}

template <typename In, typename Out>
int launch_scan_tiled(const In *in, Out *out, int64_t n, Out *tile, void *stream) {
    const int64_t tiles = scan_tiles(n);
    if (n < 0 || tiles >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((k_scan_tile_sums<In, Out>), dim3(static_cast<unsigned>(tiles)), dim3(SCAN_THREADS), 0, st, in, n, tile);
    hipLaunchKernelGGL((k_scan_group<Out, Out>), dim3(1), dim3(SCAN_THREADS), 0, st, tile, tile, tiles - 1);  // (tiles offsets: the last tile's sum is not read)
    hipLaunchKernelGGL((k_scan_tiles<In, Out>), dim3(static_cast<unsigned>(tiles)), dim3(SCAN_THREADS), 0, st, in, out, n, tile);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
