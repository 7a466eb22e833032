// npr_seedmap.hip -- two scans, k_map_sort, k_map_spans: what lies between k_seed_match (npr_seed.hip) and k_chain_dp (npr_seedchain.hip)
// when the rows stay on the device (npr_seed_map_create, npr_seedmap_api.cpp; the definition: include/nprealign.h, "reads to rows, chains
// and guides in one call").  npr_seed_matches and npr_seed_chains do the same three things on the host between their kernels: sum the
// reads' row counts, std::sort every read's rows (HitLess), walk them for the (read, reference) spans (for_each_span).
// The scans: launch_scan_group of npr_scan.h (one workgroup, one launch: this is one value per READ, 64 bits wide), counts -> their
// exclusive prefix as int64, the total behind it.  <uint32_t, int64_t> makes hit_off of what k_seed_match<false> counted, <int64_t, int64_t>
// in place makes chain_off of what k_map_spans<false> counted.
// k_map_sort: one workgroup per read sorts the read's rows by (strand, reference index, a, b) where k_seed_match<true> wrote them.  The
// network is the bitonic one in its one-direction form: merging blocks of k, the first step compares row i with its mirror image in the
// block (base + k - 1 - offset), the steps after it rows j apart, and EVERY exchange puts the smaller row at the lower index.  So rows
// past the end, thought of as larger than everything, would never move: a pair whose upper index is past the end is skipped and any
// number of rows is sorted with no padding -- which is what lets the same loop run on the rows in global memory, where there is no room
// to pad.  Rows of maximal matches are distinct: the order is total, the result does not depend on the network.
//   tier 1, at most NPR_SEED_MAP_LDS_ROWS rows: the rows are loaded into LDS (16 bytes each, 64 KB), sorted there, stored back.
//   tier 2, more rows: the same loop on the rows in global memory.  A step's exchanges touch disjoint pairs; between steps the
//   workgroup meets at a barrier, which at workgroup scope also orders the global stores of one wavefront before the loads of another
//   (one CU, one L1).  THAT HOLDS FOR THE BUILD AS IT IS: a workgroup's wavefronts share a CU unless the code object is compiled for
//   threadgroup-split mode (-mtgsplit), which the Makefile does not ask for; with it this tier (and k_chain_dp's tile hand-over) would
//   need agent-scope fences.  log2(n)^2 / 2 passes over the read's rows through L1 / L2: slow next to tier 1, and correct for any count.
//   A read with 0 or 1 rows returns after loading its two offsets.
// k_map_spans: one lane per read.  The rows are sorted, so the rows of strand 1 start at a lower bound, and inside a strand the rows of
// one reference end at an upper bound: the lane merges the two strands' lists of references in ascending index, stepping from run to
// run by binary search -- for_each_span of npr_seedchain_api.cpp without touching every row.  <false> counts the read's chains, <true>
// writes their spans (forward run, reverse run, read, reference; an empty run starts where it would lie, as on the host).
// Block shape (arithmetic, not measurement): k_map_sort 256 threads and 64 KB of static LDS, so two workgroups per CU (160 KB); the
// network for n rows has about log2(n)^2 / 2 steps of n / 2 exchanges, 78 steps of 8 exchanges per lane at 4096 rows.  A call has as
// many workgroups as reads; most reads have tens to hundreds of rows and finish in a few steps.
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int THREADS = 256;
static_assert(NPR_SEED_MAP_LDS_ROWS * 16 <= 64 * 1024, "tier 1 of k_map_sort holds a read's rows in the LDS of one workgroup");
static_assert(sizeof(SeedChainSpan) == 32, "a chain span is stored as one 32-byte struct");

// HitLess of npr_seed_api.cpp: (strand, reference index, a, b)
__device__ __forceinline__ bool row_less(const int4 &x, const int4 &y) {
    const uint32_t bx = static_cast<uint32_t>(x.z), by = static_cast<uint32_t>(y.z);
    if ((bx >> 31) != (by >> 31)) return (bx >> 31) < (by >> 31);
    if (x.x != y.x) return x.x < y.x;
    if (x.y != y.y) return x.y < y.y;
    return (bx & 0x7fffffffu) < (by & 0x7fffffffu);
}

// rows row[0 .. n) in ascending order, by the whole workgroup (every lane calls it: the barriers are the workgroup's)
__device__ __forceinline__ void sort_rows(int4 *row, int64_t n) {
    int64_t full = 1;  // the power of two the network is laid out for
    while (full < n) full <<= 1;
    const int64_t half = full >> 1;
    for (int64_t k = 2; k <= full; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);  // the first step of a merge
            for (int64_t t = threadIdx.x; t < half; t += THREADS) {
                const int64_t o = t & (j - 1), base = (t - o) << 1;  // exchange t of the step: offset o in a piece of 2 j rows at base
                const int64_t i = base + o, l = mirror ? base + 2 * j - 1 - o : i + j;
                if (l < n) {
                    const int4 x = row[i], y = row[l];
                    if (row_less(y, x)) row[i] = y, row[l] = x;
                }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_map_sort(SeedMapArgs a) {
    __shared__ int4 lds[NPR_SEED_MAP_LDS_ROWS];
    const int64_t lo = a.hit_off[blockIdx.x], n = a.hit_off[blockIdx.x + 1] - lo;
    if (n < 2) return;
    int4 *rows = reinterpret_cast<int4 *>(a.hits) + lo;
    if (n <= NPR_SEED_MAP_LDS_ROWS) {
        for (int64_t q = threadIdx.x; q < n; q += THREADS) lds[q] = rows[q];
        __syncthreads();
        sort_rows(lds, n);
        for (int64_t q = threadIdx.x; q < n; q += THREADS) rows[q] = lds[q];
    } else {
        sort_rows(rows, n);
    }
}

__device__ __forceinline__ uint32_t strand_at(const int32_t *hits, int64_t q) { return static_cast<uint32_t>(hits[4 * q + 2]) >> 31; }
// the first row of [lo, hi), rows of one strand, whose reference index is above r
__device__ __forceinline__ int64_t run_end(const int32_t *hits, int64_t lo, int64_t hi, int32_t r) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (hits[4 * mid] <= r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool WRITE>
__global__ void __launch_bounds__(THREADS) k_map_spans(SeedMapArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n_reads) return;
    const int64_t lo = a.hit_off[i], hi = a.hit_off[i + 1];
    int64_t mid = lo, top = hi;  // the first row of strand 1
    while (mid < top) {
        const int64_t m = (mid + top) >> 1;
        if (strand_at(a.hits, m) == 0) mid = m + 1; else top = m;
    }
    SeedChainSpan *s = WRITE ? a.span + a.chain_off[i] : nullptr;
    int64_t p = lo, q = mid, chains = 0;
    while (p < mid || q < hi) {
        const int32_t rp = p < mid ? a.hits[4 * p] : INT32_MAX, rq = q < hi ? a.hits[4 * q] : INT32_MAX, r = min(rp, rq);
        const int64_t p1 = rp == r ? run_end(a.hits, p, mid, r) : p, q1 = rq == r ? run_end(a.hits, q, hi, r) : q;
        if (WRITE) s[chains] = SeedChainSpan{{p, q}, {static_cast<int32_t>(p1 - p), static_cast<int32_t>(q1 - q)}, static_cast<int32_t>(i), r};
        ++chains, p = p1, q = q1;
    }
    if (!WRITE) a.chain_off[i] = chains;
}

inline unsigned blocks_for(int64_t threads) { return static_cast<unsigned>((threads + THREADS - 1) / THREADS); }

}  // namespace

int launch_seedmap_offsets(const SeedMapArgs &a, void *stream) {
    return launch_scan_group<uint32_t, int64_t>(a.count, a.hit_off, a.n_reads, stream);
}

int launch_seedmap_chains(const SeedMapArgs &a, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_map_sort, dim3(static_cast<unsigned>(a.n_reads)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_map_spans<false>, dim3(blocks_for(a.n_reads)), dim3(THREADS), 0, st, a);
    return launch_scan_group<int64_t, int64_t>(a.chain_off, a.chain_off, a.n_reads, stream);
}

int launch_seedmap_spans(const SeedMapArgs &a, void *stream) {
    hipLaunchKernelGGL(k_map_spans<true>, dim3(blocks_for(a.n_reads)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
