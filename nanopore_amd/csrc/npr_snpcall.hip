// npr_snpcall.hip -- the calling step of MarginAlignSnpCaller on the device (nanopore/analyses/marginAlignSnpCaller.py:18-23 and :163-197):
// k_snp_calls counts the calls into histograms (include/nprealign.h: npr_snp_calls_table, npr_batch_snp_calls, npr_pileup_snp_calls),
// k_snp_variants_count / a scan / k_snp_variants_emit return them (npr_snp_variants_table, npr_batch_snp_variants, npr_pileup_snp_variants).
//
// The host path copies a [positions][4] fp64 table over PCIe, computes the posterior of the four candidate bases at every position and
// appends one (probability, position) tuple per non-reference candidate to a Python list -- which is then reduced to two histograms of
// 101 bins over round(100 p) and one counter.  Here a thread takes a table row where it already lies (the fixed-point expectations
// k_base_expectations left, words 0-3 of a pileup, or an uploaded fp64 table: `source`, a template parameter -- no converted copy is
// made), computes the candidate posteriors in fp64 for up to four error models at once and adds its three calls per model to histograms
// in LDS.  A workgroup flushes its histograms once, after its grid-stride loop, with 64-bit atomics in global memory; counts are
// integers, so the result is the same from run to run.  Per row 35 bytes are read (two 16-byte loads and three bytes) against 4 exp per
// model: the kernel is memory-bound and nothing was spent on its arithmetic.  Not yet timed on hardware.
//
// The variant kernels share the per-row arithmetic (row_frequencies, candidate_weights) and work on one error model.  A workgroup owns
// tiles of SNP_VARIANT_TILE consecutive rows, one row per thread.  k_snp_variants_count reads the table once and writes three bytes per
// row -- the best base, its quality, and which candidates are calls -- and one count per tile; launch_scan_group (npr_scan.h), one workgroup, turns
// the counts into offsets and leaves the total for the host, which decides whether the calls fit; k_snp_variants_emit reads the mask
// bytes, skips a tile without calls, and lets only the rows that call recompute their posteriors.  A call's place is its tile's offset
// plus its rank in the tile (wavefront ballots, then the wavefronts before it): the arrays are in ascending (row, candidate) order
// whatever order the workgroups run in.  The whole call on a 4.6 Mb pileup: profiles/snp_variants_time.json (tools/snp_variants_time.py).
#include <hip/hip_runtime.h>

#include "npr_device.h"
#include "npr_snpmodel.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
// One workgroup per CU: a workgroup's flush is up to 4 x 204 atomics on the same few hundred words whatever it counted, so more workgroups
// buy memory parallelism with contention in L2.
constexpr int MAX_GRID = 256;
// A 32-bit LDS counter takes at most 3 x THREADS adds per trip of the loop: flushed every 2^20 trips it stays below 2^30.
constexpr int FLUSH_EVERY = 1 << 20;

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// the row's four weights and whether the row was seen at all
template <int SRC>
__device__ __forceinline__ bool load_row(const SnpCallArgs &a, int64_t r, double (&w)[4]) {
    if (SRC == SNP_SRC_FIXED) {
        const ulonglong2 *p = static_cast<const ulonglong2 *>(a.table) + 2 * r;
        const ulonglong2 u = p[0], v = p[1];
        constexpr double unit = 1.0 / static_cast<double>(EXPECT_FIXED_ONE);  // 2^-40: the product is the quotient npr_batch_base_expectations takes
        w[0] = static_cast<double>(u.x) * unit, w[1] = static_cast<double>(u.y) * unit;
        w[2] = static_cast<double>(v.x) * unit, w[3] = static_cast<double>(v.y) * unit;
        return a.seen[r] != 0;
    } else if (SRC == SNP_SRC_PILEUP) {
        const int32_t *row = static_cast<const int32_t *>(a.table) + r * NPR_PILEUP_WORDS;
        const int4 u = *reinterpret_cast<const int4 *>(row);
        const int other = row[4];
        w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
        return (static_cast<long long>(u.x) + u.y + u.z + u.w + other) != 0;
    } else {
        const double2 *p = static_cast<const double2 *>(a.table) + 2 * r;
        const double2 u = p[0], v = p[1];
        w[0] = u.x, w[1] = u.y, w[2] = v.x, w[3] = v.y;
        return a.seen[r] != 0;
    }
}

// What a table row is to a caller (include/nprealign.h: CALLABLE), and for a callable row the share of each observed base.
enum { ROW_UNSEEN = 0, ROW_SILENT = 1, ROW_CALLABLE = 2 };
template <int SRC>
__device__ __forceinline__ int row_frequencies(const SnpCallArgs &a, int64_t r, int ref, double (&f)[4]) {
    double w[4];
    const bool seen = load_row<SRC>(a, r, w);
    const double total = ((w[0] + w[1]) + w[2]) + w[3];
    if (!seen) return ROW_UNSEEN;
    if (!(total != 0.0 && ref <= 3)) return ROW_SILENT;
#pragma unroll
    for (int o = 0; o < 4; ++o) f[o] = w[o] / total;
    return ROW_CALLABLE;
}

// The four candidates of a callable row under one error model: lp[c] = log evolution[ref][c] + sum_o f[o] log error[c][o], e[c] =
// exp(lp[c] - the largest lp); returns ((e0 + e1) + e2) + e3: the posterior of candidate c is e[c] / that.  evo_row: the reference
// base's row of log_evolution.  Every kernel of this file takes its posteriors from here, in this order of operations.
__device__ __forceinline__ double candidate_weights(const double (&f)[4], const double *evo_row, const double (&log_error)[16], double (&lp)[4],
                                                    double (&e)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < 4; ++o) s += f[o] * log_error[4 * c + o];
        lp[c] = evo_row[c] + s;
    }
    const double top = fmax(fmax(lp[0], lp[1]), fmax(lp[2], lp[3]));  // finite: some candidate of every reference base is possible
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = exp(lp[c] - top);
    return ((e[0] + e[1]) + e[2]) + e[3];
}

template <int SRC>
__global__ void __launch_bounds__(THREADS) k_snp_calls(SnpCallArgs a) {
    __shared__ unsigned int hist[kSnpMaxModels * 2 * SNP_BINS];  // [model][true / false][bin]
    __shared__ unsigned int rows_of[2];                          // rows never seen, rows called
    __shared__ double evo[16];                                   // log_evolution: indexed by the row's reference base, per lane
    const int tid = threadIdx.x, nh = a.n_models * 2 * SNP_BINS;
    for (int i = tid; i < nh; i += THREADS) hist[i] = 0u;
    if (tid < 2) rows_of[tid] = 0u;
    if (tid < 16) evo[tid] = a.log_evolution[tid];
    __syncthreads();
    unsigned int unseen = 0u, called = 0u;
    // the workgroup's counts so far into the output, and its counters back to zero (every thread of the workgroup comes here together)
    auto flush = [&]() {
        unseen = wave_sum(unseen), called = wave_sum(called);
        if ((tid & (WAVE - 1)) == 0) {
            if (unseen) atomicAdd(&rows_of[0], unseen);
            if (called) atomicAdd(&rows_of[1], called);
        }
        unseen = called = 0u;
        __syncthreads();
        for (int i = tid; i < nh; i += THREADS) {
            const unsigned int v = hist[i];
            hist[i] = 0u;
            if (v) atomicAdd(a.out + i + 2 * (i / (2 * SNP_BINS)), static_cast<unsigned long long>(v));  // (SNP_OUT_WORDS = 2 SNP_BINS + 2 per model)
        }
        if (tid < 2 * a.n_models && rows_of[tid & 1])
            atomicAdd(a.out + (tid >> 1) * SNP_OUT_WORDS + 2 * SNP_BINS + (tid & 1), static_cast<unsigned long long>(rows_of[tid & 1]));
        __syncthreads();
        if (tid < 2) rows_of[tid] = 0u;
        __syncthreads();
    };
    int trips = 0;
    for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * THREADS; r0 < a.rows; r0 += static_cast<int64_t>(gridDim.x) * THREADS) {
        const int64_t r = r0 + tid;
        if (r < a.rows) {
            const int ref = a.ref_code[r];
            const int tru = a.true_code ? a.true_code[r] : ref;
            double f[4];
            const int state = row_frequencies<SRC>(a, r, ref, f);
            if (state == ROW_UNSEEN) {
                ++unseen;
            } else if (state == ROW_CALLABLE) {
                for (int m = 0; m < a.n_models; ++m) {
                    double lp[4], e[4];
                    const double sum = candidate_weights(f, evo + 4 * ref, a.log_error[m], lp, e);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c == ref) continue;
                        const int bin = static_cast<int>(fmin(fmax(rint(100.0 * (e[c] / sum)), 0.0), 100.0));  // round half to even, as numpy.rint
                        const bool is_true = tru != ref && tru == c;
                        atomicAdd(&hist[(2 * m + (is_true ? 0 : 1)) * SNP_BINS + bin], 1u);
                    }
                }
                ++called;
            }
        }
        if (++trips == FLUSH_EVERY) {
            flush();
            trips = 0;
        }
    }
    flush();
}

// ---- the calls themselves and a consensus: best base, quality and the list of calls (include/nprealign.h: npr_snp_variants_table) ----
constexpr int TILE = SNP_VARIANT_TILE;
constexpr int WAVES = THREADS / WAVE;
static_assert(TILE == THREADS, "a thread owns one row of its workgroup's tile");
// Eight workgroups a CU hide the table's latency; a workgroup takes tiles blockIdx.x, + gridDim.x, ... and loads the evolution rows once.
constexpr int VARIANT_GRID = 2048;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform(int64_t v) {
    const unsigned int lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned int>(v));
    const unsigned int hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned int>(static_cast<unsigned long long>(v) >> 32));
    return static_cast<int64_t>(static_cast<unsigned long long>(hi) << 32 | lo);
}

template <int SRC>
__global__ void __launch_bounds__(THREADS) k_snp_variants_count(SnpCallArgs a) {
    __shared__ double evo[16];
    __shared__ unsigned int wave_calls[WAVES];
    const int tid = threadIdx.x, wave = uniform(tid >> 6);
    if (tid < 16) evo[tid] = a.log_evolution[tid];
    __syncthreads();
    const int64_t tiles = snp_variant_tiles(a.rows);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * TILE + tid;
        unsigned int mask = 0u;
        if (r < a.rows) {
            const int ref = a.ref_code[r];
            int best = 4, qual = 0;
            double f[4];
            if (row_frequencies<SRC>(a, r, ref, f) == ROW_CALLABLE) {
                double lp[4], e[4];
                const double sum = candidate_weights(f, evo + 4 * ref, a.log_error[0], lp, e);
                const double top = fmax(fmax(lp[0], lp[1]), fmax(lp[2], lp[3]));
                // the candidate of largest lp; among equals the reference base, else the lowest code
                bool ref_on_top = false;
#pragma unroll
                for (int c = 3; c >= 0; --c) {
                    if (lp[c] == top) best = c;
                    ref_on_top = ref_on_top || (c == ref && lp[c] == top);
                }
                if (ref_on_top) best = ref;
                double others = 0.0;  // the three other e in ascending code (0.0 + x is x)
                int j = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c != best) others += e[c];
                    if (c != ref) {
                        if (e[c] / sum >= a.threshold) mask |= 1u << j;
                        ++j;
                    }
                }
                const double q = others / sum;
                qual = q == 0.0 ? 93 : static_cast<int>(fmin(floor(-10.0 * log10(q)), 93.0));  // (q <= 3/4: never negative)
            }
            a.best[r] = static_cast<uint8_t>(best), a.qual[r] = static_cast<uint8_t>(qual), a.mask[r] = static_cast<uint8_t>(mask);
        }
        const unsigned int in_wave = wave_sum(__popc(mask));
        if ((tid & (WAVE - 1)) == 0) wave_calls[wave] = in_wave;
        __syncthreads();
        if (tid == 0) a.tile_calls[tile] = (wave_calls[0] + wave_calls[1]) + (wave_calls[2] + wave_calls[3]);
        __syncthreads();
    }
}
static_assert(WAVES == 4, "k_snp_variants_count adds four wavefront counts");

template <int SRC>
__global__ void __launch_bounds__(THREADS) k_snp_variants_emit(SnpCallArgs a) {
    __shared__ double evo[16];
    __shared__ unsigned int wave_calls[WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uniform(tid >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (tid < 16) evo[tid] = a.log_evolution[tid];
    __syncthreads();
    const int64_t tiles = snp_variant_tiles(a.rows);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t first = uniform(a.tile_off[tile]), end = uniform(a.tile_off[tile + 1]);
        if (first == end) continue;  // (the whole workgroup: no barrier is skipped by some)
        const int64_t r = tile * TILE + tid;
        const unsigned int mask = r < a.rows ? a.mask[r] : 0u;
        // calls of the rows before this one: in the wavefront by ballots, then the wavefronts before
        unsigned int before = 0u, in_wave = 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned long long has = __ballot((mask >> j) & 1u);
            before += __popcll(has & below), in_wave += __popcll(has);
        }
        if (lane == 0) wave_calls[wave] = in_wave;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES - 1; ++w)
            if (w < wave) before += wave_calls[w];
        if (mask) {
            const int ref = a.ref_code[r];
            double f[4], lp[4], e[4];
            (void)row_frequencies<SRC>(a, r, ref, f);  // callable: the count kernel set a mask bit
            const double sum = candidate_weights(f, evo + 4 * ref, a.log_error[0], lp, e);
            int64_t at = first + before;
            int j = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c == ref) continue;
                if ((mask >> j) & 1u) {
                    if (at < a.n_calls) a.call_row[at] = r, a.call_alt[at] = static_cast<uint8_t>(c), a.call_p[at] = e[c] / sum;
                    ++at;
                }
                ++j;
            }
        }
        __syncthreads();
    }
}

}  // namespace

int launch_snp_calls(const SnpCallArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    if (a.n_models < 1 || a.n_models > kSnpMaxModels) return static_cast<int>(hipErrorInvalidValue);
    const int64_t groups = (a.rows + THREADS - 1) / THREADS;
    const int grid = static_cast<int>(groups < MAX_GRID ? groups : MAX_GRID);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.source == SNP_SRC_FIXED)
        hipLaunchKernelGGL(k_snp_calls<SNP_SRC_FIXED>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_PILEUP)
        hipLaunchKernelGGL(k_snp_calls<SNP_SRC_PILEUP>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_DOUBLE)
        hipLaunchKernelGGL(k_snp_calls<SNP_SRC_DOUBLE>, dim3(grid), dim3(THREADS), 0, s, a);
    else
        return static_cast<int>(hipErrorInvalidValue);
    return static_cast<int>(hipGetLastError());
}

namespace {
int variant_grid(int64_t rows) {
    const int64_t tiles = snp_variant_tiles(rows);
    return static_cast<int>(tiles < VARIANT_GRID ? tiles : VARIANT_GRID);
}
}  // namespace

int launch_snp_variants_count(const SnpCallArgs &a, void *stream) {
    if (a.rows <= 0) return static_cast<int>(hipErrorInvalidValue);
    const int grid = variant_grid(a.rows);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.source == SNP_SRC_FIXED)
        hipLaunchKernelGGL(k_snp_variants_count<SNP_SRC_FIXED>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_PILEUP)
        hipLaunchKernelGGL(k_snp_variants_count<SNP_SRC_PILEUP>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_DOUBLE)
        hipLaunchKernelGGL(k_snp_variants_count<SNP_SRC_DOUBLE>, dim3(grid), dim3(THREADS), 0, s, a);
    else
        return static_cast<int>(hipErrorInvalidValue);
    return launch_scan_group<uint32_t, int64_t>(a.tile_calls, a.tile_off, snp_variant_tiles(a.rows), stream);
}

int launch_snp_variants_emit(const SnpCallArgs &a, void *stream) {
    if (a.rows <= 0 || a.n_calls <= 0) return static_cast<int>(hipErrorInvalidValue);
    const int grid = variant_grid(a.rows);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.source == SNP_SRC_FIXED)
        hipLaunchKernelGGL(k_snp_variants_emit<SNP_SRC_FIXED>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_PILEUP)
        hipLaunchKernelGGL(k_snp_variants_emit<SNP_SRC_PILEUP>, dim3(grid), dim3(THREADS), 0, s, a);
    else if (a.source == SNP_SRC_DOUBLE)
        hipLaunchKernelGGL(k_snp_variants_emit<SNP_SRC_DOUBLE>, dim3(grid), dim3(THREADS), 0, s, a);
    else
        return static_cast<int>(hipErrorInvalidValue);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
