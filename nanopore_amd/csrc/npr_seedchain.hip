// npr_seedchain.hip -- k_chain_dp, k_chain_trace<false> / a scan / k_chain_trace<true>: the co-linear chains of seed rows and the guide
// alignments they stand for, all (read, reference) pairs of a call at once (the definition: include/nprealign.h, "chaining of seed rows";
// the host restatement of the same rule for one pair: npr_chain.cpp).
//
// A row (r, a, b | strand << 31, L) is a block of L aligned pairs; its last positions are e = a + L - 1 and f = b + L - 1.  Row j may
// precede row i when a_i > e_j, b_i > f_j, both on one strand, and (a_i - e_j) + (b_i - f_j) <= max_gap; best_i = L_i + the largest
// best_j, the first-sorting j among equals.  a_i > e_j >= a_j already says that j sorts before i, and the rows of one (read, strand,
// reference) -- a RUN -- are contiguous and in (a, b) order as npr_seed_matches sorts them, so inside a run "j sorts before i" is "j comes
// before i" and nothing has to be sorted here.  The two runs of a (read, reference) never chain with each other; they meet only when the
// chain's end is chosen.
// k_chain_dp: one wavefront per run, 64 rows (a TILE) at a time, lane t owns row i0 + t.  Candidates of earlier tiles come from the node
// scratch (e, f, best, pm: one 16-byte load each), where pm is the largest e of the run's rows up to that one: both gaps are at least 1, so
// a predecessor has e_j >= a_i - max_gap + 1, and since pm never decreases the first row whose pm reaches that bound (binary search) is
// where the lane's window starts -- a long block that starts far back and ends inside the window is still met, which a window by a_j would
// miss.  The lane walks its window in row order and takes a candidate only when it is strictly better, so the first-sorting one wins.
// Candidates of the lane's own tile: 64 steps, step t broadcasts lane t's (e, f, best); lane t's best is final by then because rows t and
// later fail a_i > e_j against it.  A wavefront that ran its window loop for a worst case (every row sees every earlier one) does the
// reference's quadratic scan, 64 rows at a time; no run length is refused.
// Between tiles the wavefront fences at workgroup scope: the node rows a tile stored are loaded by OTHER lanes of the same wavefront in
// the next tile, and only a fence orders one lane's store before another lane's load.  One CU, one L1: that scope is enough, and it costs
// a wait for the stores, not a cache write-back.
// k_chain_trace: one lane per (read, reference).  It picks the run whose best end is larger -- equal scores: the end that sorts last by
// (a, strand, b), so the reverse run wins unless the forward end starts later -- and walks the back pointers from that end.  Walking
// backwards it meets the guide's operations last to first: after the last block the read's rest (I) and the reference's rest (D), then per
// block its M and what lies before it (I, then D; forwards that is D then I as npr_chain_merge writes them); lengths of 0 dropped, equal
// neighbours merged in a register before anything is counted or stored.  <false> counts (rows in the chain, op pairs) and writes the chain
// row; launch_scan_group (npr_scan.h) turns the counts into offsets in place;
// <true> walks again and stores the pairs from the end of the chain's range backwards.  The walk is serial and its loads are dependent
// (row, back pointer, row ...): it is latency-bound by construction, and the lanes of a wavefront walk chains of different lengths.  That
// is accepted: a chain is tens of rows where the DP looked at thousands of pairs.
// Block shape (arithmetic, not measurement; nothing here has been profiled): 256 threads = four independent wavefronts of k_chain_dp, no
// LDS, no barrier; 48 VGPRs, so residency is bounded by the 32 waves of a CU only.
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;

struct Row {
    int32_t a, b, L;
};
__device__ __forceinline__ Row load_row(const int32_t *hits, int64_t row) {
    const int4 v = *reinterpret_cast<const int4 *>(hits + 4 * row);
    return Row{v.y, static_cast<int32_t>(static_cast<uint32_t>(v.z) & 0x7fffffffu), v.w};
}

// whether a block ending at (ce, cf) may precede the one starting at (a, b)
__device__ __forceinline__ bool may_precede(int32_t ce, int32_t cf, int32_t a, int32_t b, uint32_t max_gap) {
    return a > ce && b > cf && static_cast<uint32_t>(a - ce) + static_cast<uint32_t>(b - cf) <= max_gap;
}

__global__ void __launch_bounds__(THREADS) k_chain_dp(SeedChainArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t w = static_cast<int64_t>(blockIdx.x) * (THREADS / WAVE) + threadIdx.x / WAVE;  // run: strand w & 1 of chain span w >> 1
    if (w >= 2 * a.n_chains) return;
    const SeedChainSpan *sp = a.span + (w >> 1);
    const int64_t n = sp->n[w & 1];
    if (n == 0) {
        if (lane == 0) a.run_end[2 * w] = -1, a.run_end[2 * w + 1] = 0;
        return;
    }
    const int64_t first = sp->first[w & 1];
    int4 *node = reinterpret_cast<int4 *>(a.node) + first;
    int32_t *back = a.back + first;
    int32_t run_max = -1;                // largest e of the tiles before this one
    int32_t end_best = 0, end_idx = -1;  // the lane's own rows: the best chain end, the later one among equals
    for (int64_t i0 = 0; i0 < n; i0 += WAVE) {
        const int64_t i = i0 + lane;
        const bool live = i < n;
        Row r{0, 0, 0};
        int32_t e = INT32_MAX, f = INT32_MAX;  // (a lane without a row precedes nothing)
        if (live) {
            r = load_row(a.hits, first + i);
            e = r.a + r.L - 1, f = r.b + r.L - 1;
        }
        int32_t pm = live ? e : -1;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int32_t t = __shfl_up(pm, o, WAVE);
            if (lane >= o) pm = max(pm, t);
        }
        pm = max(pm, run_max);
        int32_t best = r.L, bk = -1;
        if (live && i0 > 0) {
            const int64_t need = static_cast<int64_t>(r.a) - static_cast<int64_t>(a.max_gap) + 1;  // e_j >= need
            int64_t lo = 0, hi = i0;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (node[mid].w < need) lo = mid + 1; else hi = mid;
            }
            for (int64_t j = lo; j < i0; ++j) {
                const int4 c = node[j];
                if (may_precede(c.x, c.y, r.a, r.b, a.max_gap) && r.L + c.z > best) best = r.L + c.z, bk = static_cast<int32_t>(j);
            }
        }
        const int rows_here = static_cast<int>(min(static_cast<int64_t>(WAVE), n - i0));
        for (int t = 0; t < rows_here; ++t) {
            const int32_t ce = __shfl(e, t, WAVE), cf = __shfl(f, t, WAVE), cb = __shfl(best, t, WAVE);
            if (may_precede(ce, cf, r.a, r.b, a.max_gap) && r.L + cb > best) best = r.L + cb, bk = static_cast<int32_t>(i0) + t;
        }
        if (live) {
            node[i] = make_int4(e, f, best, pm);
            back[i] = bk;
            if (best >= end_best) end_best = best, end_idx = static_cast<int32_t>(i);
        }
        run_max = __shfl(pm, WAVE - 1, WAVE);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const int32_t ob = __shfl_xor(end_best, o, WAVE), oi = __shfl_xor(end_idx, o, WAVE);
        if (ob > end_best || (ob == end_best && oi > end_idx)) end_best = ob, end_idx = oi;
    }
    if (lane == 0) a.run_end[2 * w] = end_idx, a.run_end[2 * w + 1] = end_best;
}

template <bool WRITE>
__global__ void __launch_bounds__(THREADS) k_chain_trace(SeedChainArgs a) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (c >= a.n_chains) return;
    const SeedChainSpan sp = a.span[c];
    const int32_t end0 = a.run_end[4 * c], best0 = a.run_end[4 * c + 1], end1 = a.run_end[4 * c + 2], best1 = a.run_end[4 * c + 3];
    int s;
    if (end0 < 0 || end1 < 0)
        s = end0 < 0;
    else if (best0 != best1)
        s = best1 > best0;
    else
        s = load_row(a.hits, sp.first[1] + end1).a >= load_row(a.hits, sp.first[0] + end0).a;  // equal a: strand 1 sorts later
    const int64_t first = sp.first[s];
    int32_t idx = s ? end1 : end0;
    int32_t x = a.ref_len[sp.ref], y = a.read_len[sp.read];  // what the blocks walked so far leave uncovered: reference [0, x), read [0, y)
    int32_t *wr = WRITE ? a.ops + 2 * a.n_ops[c + 1] : nullptr;
    int64_t pairs = 0;
    int32_t rows = 0, pend_op = -1, pend_len = 0;
    auto flush = [&] {
        if (pend_op < 0) return;
        ++pairs;
        if (WRITE) wr -= 2, *reinterpret_cast<int2 *>(wr) = make_int2(pend_op, pend_len);
    };
    auto emit = [&](int32_t op, int32_t len) {
        if (len <= 0) return;
        if (op == pend_op) {
            pend_len += len;
            return;
        }
        flush();
        pend_op = op, pend_len = len;
    };
    while (idx >= 0) {
        const Row r = load_row(a.hits, first + idx);
        emit(NPR_OP_I, y - (r.b + r.L));
        emit(NPR_OP_D, x - (r.a + r.L));
        emit(NPR_OP_M, r.L);
        x = r.a, y = r.b, ++rows;
        idx = a.back[first + idx];
    }
    emit(NPR_OP_I, y);
    emit(NPR_OP_D, x);
    flush();
    if (!WRITE) {
        *reinterpret_cast<int4 *>(a.chains + 4 * c) = make_int4(sp.ref, s, s ? best1 : best0, rows);
        a.n_ops[c] = pairs;
    }
}

inline unsigned blocks_for(int64_t threads) { return static_cast<unsigned>((threads + THREADS - 1) / THREADS); }

}  // namespace

int launch_seed_chain_dp(const SeedChainArgs &a, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_chain_dp, dim3(blocks_for(2 * a.n_chains * WAVE)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_chain_trace<false>, dim3(blocks_for(a.n_chains)), dim3(THREADS), 0, st, a);
    return launch_scan_group<int64_t, int64_t>(a.n_ops, a.n_ops, a.n_chains, stream);
}

int launch_seed_chain_write(const SeedChainArgs &a, void *stream) {
    hipLaunchKernelGGL(k_chain_trace<true>, dim3(blocks_for(a.n_chains)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
