// npr_snpcall.hip -- k_snp_calls: the calling step of MarginAlignSnpCaller on the device (include/nprealign.h: npr_snp_calls_table,
// npr_batch_snp_calls, npr_pileup_snp_calls; nanopore/analyses/marginAlignSnpCaller.py:18-23 and :163-197).
//
// The host path copies a [positions][4] fp64 table over PCIe, computes the posterior of the four candidate bases at every position and
// appends one (probability, position) tuple per non-reference candidate to a Python list -- which is then reduced to two histograms of
// 101 bins over round(100 p) and one counter.  Here a thread takes a table row where it already lies (the fixed-point expectations
// k_base_expectations left, words 0-3 of a pileup, or an uploaded fp64 table: `source`, a template parameter -- no converted copy is
// made), computes the candidate posteriors in fp64 for up to four error models at once and adds its three calls per model to histograms
// in LDS.  A workgroup flushes its histograms once, after its grid-stride loop, with 64-bit atomics in global memory; counts are
// integers, so the result is the same from run to run.  Per row 35 bytes are read (two 16-byte loads and three bytes) against 4 exp per
// model: the kernel is memory-bound and nothing was spent on its arithmetic.  Not yet timed on hardware.
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
            double w[4];
            const bool seen = load_row<SRC>(a, r, w);
            const int ref = a.ref_code[r];
            const int tru = a.true_code ? a.true_code[r] : ref;
            const double total = ((w[0] + w[1]) + w[2]) + w[3];
            if (!seen) {
                ++unseen;
            } else if (total != 0.0 && ref <= 3) {
                const double f[4] = {w[0] / total, w[1] / total, w[2] / total, w[3] / total};
                for (int m = 0; m < a.n_models; ++m) {
                    double lp[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int o = 0; o < 4; ++o) s += f[o] * a.log_error[m][4 * c + o];
                        lp[c] = evo[4 * ref + c] + s;
                    }
                    const double top = fmax(fmax(lp[0], lp[1]), fmax(lp[2], lp[3]));  // finite: some candidate of every reference base is possible
                    double e[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) e[c] = exp(lp[c] - top);
                    const double sum = ((e[0] + e[1]) + e[2]) + e[3];
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

}  // namespace npr
