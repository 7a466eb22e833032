// npr_alnqual.hip -- k_coverage_max, k_pileup_coverage, k_align_quality: the alignment-quality tables of the QualiMap analysis, counted on the device.
//
// nanopore/analyses/qualimap.py converts the SAM file to BAM, sorts it and hands it to the Java `qualimap bamqc`.  What this build reports instead is
// defined in exact integer terms in include/nprealign.h (npr_pileup_coverage, npr_align_quality): per window of the concatenated reference the depth
// sums, G + C, record starts, deletion columns and the MAPQ summed over M columns; histograms of depth, of record starts per position, of MAPQ, of
// the read bases and the soft clips by position in the read, of a record's G + C, and of the indel runs by homopolymer class and length.  All three
// kernels only add integers; the tests compare every table with a per-record, per-position restatement of the header's text.
//
// k_pileup_coverage: one pass over the pileup's table, 32 B per row (two 16-byte loads per lane) plus one reference byte -- memory-bound by construction.
//   A workgroup takes AQ_TILE = 2048 consecutive rows, each of its four wavefronts a quarter (512 rows, 64 at a time, neighbouring lanes neighbouring
//   rows).  Consecutive rows share a window, so the window words are a segmented reduction: a wavefront whose quarter lies in ONE window (two
//   divisions say so; at the default 400 windows of a 4.6 Mb contig that is 24 quarters in 25) adds into eight private 64-bit sums per lane and
//   reduces them once with shuffles; a quarter that holds a window boundary gives every lane its row's window and runs a segmented scan per 64 rows,
//   the last lane of each segment handing over the segment's sums.  What a wavefront hands over goes to an LDS table of the first AQ_SLOTS windows of
//   the tile and from there to the 64-bit table in global memory once per tile: one atomic per tile, window and word, not one per row (windows
//   further from the tile's first than AQ_SLOTS -- windows of fewer than 32 rows -- go to global memory directly).
//   The two histograms are 32-bit LDS counters in eight copies (a lane adds into copy lane & 7; a copy is 673 words long, odd, so the copies of a
//   counter lie in different banks): neighbouring rows have nearly equal depth, so same-address adds are the expected limiter and the copies cut the
//   lanes that can meet on one counter from 64 to 8.  Rows of depth 0 and rows that start no record -- most rows, for the start histogram -- are
//   counted in a register instead.  The histograms are flushed once, non-zero counters only.  A counter takes at most AQ_TILE: no overflow.
//   The largest depth is reduced first by k_coverage_max (the host refuses the call before the sum of depth^2 can leave int64); the table of a
//   4.6 Mb contig (147 MB) is then read a second time, largely from the memory-side cache.
// k_align_quality: one wavefront per record, as k_pileup_add works; the cost is a record's runs plus its read bases, never its reference span.
//   The whole cigar is summed first and compared with what the record has: a record that runs past its read or its sequence adds nothing and sets *bad.
//   The per-workgroup histograms (mapq_hist, pos_base, clip_hist, gc_hist, indel, indel_len, totals: 3 064 counters of 64 bits, 24.5 KB, so six
//   workgroups fit a CU's LDS) are flushed once at the end of the grid-stride loop, non-zero counters only.  The read bases an M or I run consumes
//   are the bases [start, start + consumed) of the read: 64 at a time, one byte per lane; far from the read's start the 64 positions share a bin,
//   and then the five base counts are five ballots and ONE LDS add by five lanes instead of 64 same-address adds.  The clips are a range add: lanes
//   take the bins the range overlaps.  The lane that holds an I or D run classifies it: it reads the run's bases until one differs (a run of three
//   equal bases is a homopolymer by itself) and at most three reference bases on either side, inside the record's sequence.
//   The M columns per window: the wavefront keeps the window it is in and that window's rows; while the M runs of a chunk of 64 operations lie
//   inside it their lengths are summed across the wavefront into a running count, handed over with two 64-bit global atomics (columns, columns x
//   MAPQ) when the window changes or the record ends -- one pair per record and window.  A chunk that reaches past the window is taken by the lanes
//   themselves: each splits its run at the window boundaries.
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int PART = AQ_TILE / WAVES;   // rows of a tile one wavefront takes
constexpr int STEPS = PART / WAVE;
static_assert(STEPS * WAVE * WAVES == AQ_TILE, "a tile is dealt to the wavefronts in whole steps");
constexpr int AQ_SLOTS = 64;            // windows of a tile, from its first on, that are summed in LDS
constexpr int COPIES = 8;
constexpr int HIST_WORDS = 2 * RQ_POS_BINS;
constexpr int COPY_STRIDE = HIST_WORDS + 1;  // odd: the copies of a counter lie in different banks
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t code_of(uint32_t c) {
    c &= 0xdfu;  // upper case
    return c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u)));
}

__device__ __forceinline__ uint32_t pos_bin(int64_t p) {
    if (p < 16) return static_cast<uint32_t>(p);
    if (p >= (int64_t(1) << 24)) return RQ_POS_BINS - 1;
    const uint32_t q = static_cast<uint32_t>(p);
    const int e = 31 - __clz(static_cast<int>(q));
    return 16u * static_cast<uint32_t>(e - 3) + ((q >> (e - 4)) & 15u);
}
// [lo, hi) of bin b; the last bin has no end
__device__ __forceinline__ int64_t bin_lo(uint32_t b) { return b < 16 ? static_cast<int64_t>(b) : static_cast<int64_t>(16 + (b & 15u)) << (b / 16 - 1); }
__device__ __forceinline__ int64_t bin_hi(uint32_t b) {
    if (b >= RQ_POS_BINS - 1) return INT64_MAX;
    return b < 16 ? static_cast<int64_t>(b) + 1 : bin_lo(b) + (int64_t(1) << (b / 16 - 1));
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const T t = __shfl_xor(v, o, WAVE);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int wave_scan(int v, int lane) {  // inclusive
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

// the window of row r (0 <= r < T)
__device__ __forceinline__ int64_t window_of(int64_t r, int64_t W, int64_t T) { return ((r + 1) * W - 1) / T; }

struct Row {
    int64_t depth;
    int32_t del, ins, starts;
};
__device__ __forceinline__ Row load_row(const int32_t *tab, int64_t r) {
    const int4 *p = reinterpret_cast<const int4 *>(tab + r * NPR_PILEUP_WORDS);
    const int4 u = p[0], v = p[1];
    return Row{static_cast<int64_t>(u.x) + u.y + u.z + u.w + v.x, v.y, v.z, v.w};
}

__global__ void __launch_bounds__(THREADS) k_coverage_max(CoverageArgs a) {
    int64_t m = 0;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x; r < a.rows; r += static_cast<int64_t>(gridDim.x) * THREADS) {
        const int64_t d = load_row(a.tab, r).depth;
        m = d > m ? d : m;
    }
    m = wave_max(m);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m > 0) atomicMax(a.max_depth, static_cast<u64>(m));
}

// a window's eight sums from a wavefront: into the tile's LDS table when the window is one of its first AQ_SLOTS, else to global memory
__device__ __forceinline__ void hand_over(u64 *slots, int64_t w_tile, const CoverageArgs &a, int64_t w, const u64 *v) {
    const int64_t s = w - w_tile;
#pragma unroll
    for (int q = 0; q < AQ_WIN_WORDS; ++q) {
        if (!v[q]) continue;
        if (s < AQ_SLOTS) atomicAdd(&slots[s * AQ_WIN_WORDS + q], v[q]);
        else atomicAdd(a.win + w * AQ_WIN_WORDS + q, v[q]);
    }
}

__global__ void __launch_bounds__(THREADS) k_pileup_coverage(CoverageArgs a) {
    __shared__ uint32_t h[COPIES * COPY_STRIDE];
    __shared__ u64 slots[AQ_SLOTS * AQ_WIN_WORDS];
    __shared__ u64 tot[AQ_TOTALS];
    for (int q = threadIdx.x; q < COPIES * COPY_STRIDE; q += THREADS) h[q] = 0;
    for (int q = threadIdx.x; q < AQ_SLOTS * AQ_WIN_WORDS; q += THREADS) slots[q] = 0;
    if (threadIdx.x < AQ_TOTALS) tot[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int64_t T = a.rows, W = a.n_windows;
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * AQ_TILE;  // (< T: the grid has ceil(T / AQ_TILE) workgroups)
    const int64_t w_tile = window_of(tile0, W, T);
    const int64_t p0 = tile0 + static_cast<int64_t>(wv) * PART, p1 = p0 + PART < T ? p0 + PART : T;  // the wavefront's rows [p0, p1)
    uint32_t *hw = h + (lane & (COPIES - 1)) * COPY_STRIDE;
    u64 zero_depth = 0, zero_starts = 0, t_ins = 0;
    int64_t max_starts = 0;
    if (p0 < p1) {
        const int64_t w_first = window_of(p0, W, T), w_last = window_of(p1 - 1, W, T);
        const bool one_window = w_first == w_last;
        u64 acc[AQ_WIN_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
        for (int step = 0; step < STEPS; ++step) {
            const int64_t r = p0 + step * WAVE + lane;
            const bool have = r < p1;
            u64 v[AQ_WIN_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (have) {
                const Row row = load_row(a.tab, r);
                const uint32_t c = code_of(a.ref[r]);
                const u64 d = static_cast<u64>(row.depth);
                v[0] = 1, v[1] = d, v[2] = d * d, v[3] = d != 0, v[4] = c == 1u || c == 2u, v[5] = c < 4u;
                v[6] = static_cast<u64>(row.starts), v[7] = static_cast<u64>(row.del);
                t_ins += static_cast<u64>(row.ins);
                max_starts = row.starts > max_starts ? row.starts : max_starts;
                if (d) atomicAdd(&hw[pos_bin(row.depth)], 1u); else ++zero_depth;
                if (row.starts) atomicAdd(&hw[RQ_POS_BINS + pos_bin(row.starts)], 1u); else ++zero_starts;
            }
            if (one_window) {
#pragma unroll
                for (int q = 0; q < AQ_WIN_WORDS; ++q) acc[q] += v[q];
                continue;
            }
            if (p0 + step * WAVE >= p1) continue;  // (the whole wavefront: nothing left)
            // every lane its row's window (rows past the end: one no row has), a segmented running sum, and the last lane of a segment hands over
            const int64_t w = have ? window_of(r, W, T) : W;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const int64_t wo = __shfl_up(w, o, WAVE);
                const bool same = lane >= o && wo == w;
#pragma unroll
                for (int q = 0; q < AQ_WIN_WORDS; ++q) {
                    const u64 t = __shfl_up(v[q], o, WAVE);
                    if (same) v[q] += t;
                }
            }
            const int64_t w_next = __shfl_down(w, 1, WAVE);
            if (have && (lane == WAVE - 1 || w_next != w)) hand_over(slots, w_tile, a, w, v);
        }
        if (one_window) {
#pragma unroll
            for (int q = 0; q < AQ_WIN_WORDS; ++q) acc[q] = wave_sum(acc[q]);
            if (lane == 0) hand_over(slots, w_tile, a, w_first, acc);
        }
    }
    zero_depth = wave_sum(zero_depth), zero_starts = wave_sum(zero_starts), t_ins = wave_sum(t_ins), max_starts = wave_max(max_starts);
    if (lane == 0) {
        if (zero_depth) atomicAdd(&h[0], static_cast<uint32_t>(zero_depth));
        if (zero_starts) atomicAdd(&h[RQ_POS_BINS], static_cast<uint32_t>(zero_starts));
        if (t_ins) atomicAdd(&tot[7], t_ins);
        if (max_starts) atomicMax(&tot[4], static_cast<u64>(max_starts));
    }
    __syncthreads();
    // the flush: the tile's windows (their sums give the totals too), then the histograms
    for (int q = threadIdx.x; q < AQ_SLOTS * AQ_WIN_WORDS; q += THREADS) {
        const u64 v = slots[q];
        if (v) atomicAdd(a.win + (w_tile + q / AQ_WIN_WORDS) * AQ_WIN_WORDS + q % AQ_WIN_WORDS, v);
    }
    for (int q = threadIdx.x; q < HIST_WORDS; q += THREADS) {
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < COPIES; ++c) v += h[c * COPY_STRIDE + q];
        if (v) atomicAdd((q < RQ_POS_BINS ? a.depth_hist : a.start_hist - RQ_POS_BINS) + q, static_cast<u64>(v));
    }
    if (threadIdx.x == 4 && tot[4]) atomicMax(a.totals + 4, tot[4]);
    if (threadIdx.x == 7 && tot[7]) atomicAdd(a.totals + 7, tot[7]);
}

// ---- k_align_quality ----
constexpr int T_MAPQ = 0, T_POS_BASE = T_MAPQ + AQ_MAPQ_COLS, T_CLIP = T_POS_BASE + RQ_POS_BINS * RQ_BASE_COLS, T_GC = T_CLIP + RQ_POS_BINS,
              T_INDEL = T_GC + RQ_GC_COLS, T_INDEL_LEN = T_INDEL + 2 * AQ_CLASSES, T_TOTALS = T_INDEL_LEN + 2 * RQ_POS_BINS;
static_assert(T_TOTALS + AQ_TOTALS == AQ_TABLE_WORDS, "the workgroup's tables are the ones the host unpacks");
static_assert(AQ_TABLE_WORDS * 8 * 6 <= 160 * 1024, "six workgroups per CU");

// the positions [lo, hi) of a read into clip_hist: lanes take the bins the range overlaps
__device__ __forceinline__ void clip_range(u64 *t, int64_t lo, int64_t hi, int lane) {
    if (hi <= lo) return;
    const uint32_t b0 = pos_bin(lo), b1 = pos_bin(hi - 1);
    for (uint32_t b = b0 + lane; b <= b1; b += WAVE) {
        const int64_t x = bin_lo(b) > lo ? bin_lo(b) : lo, y = bin_hi(b) < hi ? bin_hi(b) : hi;
        if (y > x) atomicAdd(&t[T_CLIP + b], static_cast<u64>(y - x));
    }
}

// the M columns [x, x + len) of rows with one MAPQ into win_mapq, split at the window boundaries (one lane)
__device__ __forceinline__ void columns_by_window(const AlnQualArgs &a, int64_t x, int64_t len, u64 mapq) {
    const int64_t T = a.rows, W = a.n_windows, end = x + len;
    int64_t w = window_of(x, W, T);
    while (x < end) {
        const int64_t stop = (w + 1) * T / W, upto = stop < end ? stop : end;
        if (upto > x) {
            atomicAdd(a.win_mapq + 2 * w, static_cast<u64>(upto - x));
            if (mapq) atomicAdd(a.win_mapq + 2 * w + 1, static_cast<u64>(upto - x) * mapq);
            x = upto;
        }
        ++w;
    }
}

// class of an indel run at row x of a sequence [s0, s1): b = the code all its bases share (4: none)
__device__ __forceinline__ int indel_class(const uint8_t *ref, int64_t s0, int64_t s1, int64_t x, int64_t right_from, int64_t own, uint32_t b) {
    if (b >= 4u) return 4;
    int64_t have = own;
    for (int64_t q = x - 1, n = 0; have < AQ_HOMOPOLYMER && n < AQ_HOMOPOLYMER && q >= s0 && code_of(ref[q]) == b; --q, ++n) ++have;
    for (int64_t q = right_from, n = 0; have < AQ_HOMOPOLYMER && n < AQ_HOMOPOLYMER && q < s1 && code_of(ref[q]) == b; ++q, ++n) ++have;
    return have >= AQ_HOMOPOLYMER ? static_cast<int>(b) : 4;
}

__global__ void __launch_bounds__(THREADS) k_align_quality(AlnQualArgs a) {
    __shared__ u64 t[AQ_TABLE_WORDS];
    for (int q = threadIdx.x; q < static_cast<int>(AQ_TABLE_WORDS); q += THREADS) t[q] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int64_t T = a.rows, W = a.n_windows;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * WAVES + wv; r < a.n; r += static_cast<int64_t>(gridDim.x) * WAVES) {
        const AlnQualRec rec = a.recs[r];
        if (rec.xlen < 0) continue;  // not selected
        const int64_t o0 = a.ops_off[r], nops = a.ops_off[r + 1] - o0;
        // the cigar against what the record has, before the first add
        long long sx = 0, sy = 0;
        int other = 0;
        for (int64_t i = lane; i < nops; i += WAVE) {
            const uint32_t w = a.ops[o0 + i];
            const long long len = w >> 2;
            const uint32_t op = w & 3u;
            other |= op == 3u;
            if (op != NPR_OP_I) sx += len;
            if (op != NPR_OP_D) sy += len;
        }
        sx = wave_sum(sx), sy = wave_sum(sy), other = wave_sum(other);
        if (other || sx > rec.xlen || sy > rec.span - rec.sy) {
            if (lane == 0) *a.bad = 1;
            continue;
        }
        const u64 mapq = static_cast<u64>(rec.mapq);
        const uint8_t *seq = a.seq + rec.y_off;
        // per record: MAPQ, the clips, G + C of the whole read span
        if (lane == 0) {
            atomicAdd(&t[T_MAPQ + rec.mapq], 1ull);
            atomicAdd(&t[T_TOTALS + 0], 1ull);
            if (rec.clip0 + rec.clip1) atomicAdd(&t[T_TOTALS + 6], static_cast<u64>(rec.clip0 + rec.clip1)), atomicAdd(&t[T_TOTALS + 7], 1ull);
        }
        clip_range(t, 0, rec.clip0, lane);
        clip_range(t, rec.clip0 + rec.span, rec.clip0 + rec.span + rec.clip1, lane);
        if (rec.span > 0) {
            uint32_t gc = 0, acgt = 0;
            for (int64_t y = lane; y < rec.span; y += WAVE) {
                const uint32_t c = code_of(seq[y]);
                gc += c == 1u || c == 2u, acgt += c < 4u;
            }
            const u64 both = wave_sum((static_cast<u64>(gc) << 32) | acgt);
            const u64 g = both >> 32, n = both & 0xffffffffull;
            if (lane == 0) atomicAdd(&t[T_GC + (n ? (200ull * g + n) / (2ull * n) : static_cast<u64>(RQ_GC_COLS - 1))], 1ull);
        }
        // the read bases the cigar consumes, by position in the read
        const int64_t pbase = rec.clip0 + rec.sy;
        for (long long y0 = 0; y0 < sy; y0 += WAVE) {
            const long long y = y0 + lane;
            const bool have = y < sy;
            const uint32_t c = have ? code_of(seq[rec.sy + y]) : 5u;
            const long long y_last = y0 + WAVE - 1 < sy - 1 ? y0 + WAVE - 1 : sy - 1;
            const uint32_t b_first = pos_bin(pbase + y0), b_last = pos_bin(pbase + y_last);
            if (b_first == b_last) {
                u64 mine = 0;
#pragma unroll
                for (uint32_t q = 0; q < RQ_BASE_COLS; ++q) {
                    const u64 m = __ballot(c == q);
                    if (static_cast<uint32_t>(lane) == q) mine = static_cast<u64>(__popcll(m));
                }
                if (lane < RQ_BASE_COLS && mine) atomicAdd(&t[T_POS_BASE + b_first * RQ_BASE_COLS + lane], mine);
            } else if (have) {
                atomicAdd(&t[T_POS_BASE + pos_bin(pbase + y) * RQ_BASE_COLS + c], 1ull);
            }
        }
        // the runs
        long long X0 = 0, Y0 = 0;  // reference / read bases consumed before the chunk
        int64_t cw = -1, cw_lo = 0, cw_hi = 0;  // the window the M columns are being summed for, its rows [cw_lo, cw_hi)
        u64 cw_cols = 0;
        u64 n_m = 0, n_i = 0, n_ib = 0, n_d = 0, n_db = 0;
        for (int64_t base = 0; base < nops; base += WAVE) {
            const uint32_t w = base + lane < nops ? a.ops[o0 + base + lane] : 0u;
            const int len = static_cast<int>(w >> 2), op = static_cast<int>(w & 3u);
            const int dx = op != NPR_OP_I ? len : 0, dy = op != NPR_OP_D ? len : 0;
            const int ix = wave_scan(dx, lane), iy = wave_scan(dy, lane);
            const int64_t x = rec.row0 + X0 + ix - dx;     // the row of the next column at the run
            const long long yb = rec.sy + Y0 + iy - dy;    // the read base at the run, from read_begin
            const bool is_m = len > 0 && op == NPR_OP_M;
            if (len > 0 && op != NPR_OP_M) {
                const bool ins = op == NPR_OP_I;
                uint32_t b;
                int64_t own = 0;  // the run's own bases when they all share b (a D run's count towards the homopolymer), up to the threshold
                if (ins) {
                    b = code_of(seq[yb]);
                    for (int q = 1; q < len && b < 4u; ++q)
                        if (code_of(seq[yb + q]) != b) b = 4u;
                } else {
                    b = code_of(a.ref[x]);
                    int q = 1;
                    for (; q < len && b < 4u; ++q)
                        if (code_of(a.ref[x + q]) != b) b = 4u;
                    own = len < AQ_HOMOPOLYMER ? len : AQ_HOMOPOLYMER;
                }
                const int cls = indel_class(a.ref, rec.s0, rec.s1, x, ins ? x : x + len, own, b);
                atomicAdd(&t[T_INDEL + (ins ? 0 : AQ_CLASSES) + cls], 1ull);
                atomicAdd(&t[T_INDEL_LEN + (ins ? 0 : RQ_POS_BINS) + pos_bin(len)], 1ull);
                if (ins) ++n_i, n_ib += static_cast<u64>(len); else ++n_d, n_db += static_cast<u64>(len);
            }
            // the chunk's M columns by window
            const u64 m_lanes = __ballot(is_m);
            if (m_lanes) {
                const int first = __ffsll(static_cast<long long>(m_lanes)) - 1, last = 63 - __builtin_clzll(m_lanes);
                const int64_t x_first = __shfl(x, first, WAVE), x_end = __shfl(x, last, WAVE) + __shfl(len, last, WAVE);
                const u64 cols = wave_sum(static_cast<u64>(is_m ? len : 0));
                n_m += cols;
                if (cw < 0 || x_first < cw_lo || x_first >= cw_hi) {  // the chunk begins in another window
                    if (cw >= 0 && cw_cols && lane == 0) {
                        atomicAdd(a.win_mapq + 2 * cw, cw_cols);
                        if (mapq) atomicAdd(a.win_mapq + 2 * cw + 1, cw_cols * mapq);
                    }
                    cw = window_of(x_first, W, T), cw_lo = cw * T / W, cw_hi = (cw + 1) * T / W, cw_cols = 0;
                }
                if (x_end <= cw_hi) cw_cols += cols;
                else if (is_m) columns_by_window(a, x, len, mapq);
            }
            X0 += __shfl(ix, WAVE - 1, WAVE), Y0 += __shfl(iy, WAVE - 1, WAVE);
        }
        if (cw >= 0 && cw_cols && lane == 0) {
            atomicAdd(a.win_mapq + 2 * cw, cw_cols);
            if (mapq) atomicAdd(a.win_mapq + 2 * cw + 1, cw_cols * mapq);
        }
        n_i = wave_sum(n_i), n_ib = wave_sum(n_ib), n_d = wave_sum(n_d), n_db = wave_sum(n_db);
        if (lane == 0) {
            if (n_m) atomicAdd(&t[T_TOTALS + 1], n_m);
            if (n_i) atomicAdd(&t[T_TOTALS + 2], n_i), atomicAdd(&t[T_TOTALS + 3], n_ib);
            if (n_d) atomicAdd(&t[T_TOTALS + 4], n_d), atomicAdd(&t[T_TOTALS + 5], n_db);
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < static_cast<int>(AQ_TABLE_WORDS); q += THREADS) {
        const u64 v = t[q];
        if (v) atomicAdd(a.tab + q, v);
    }
}

}  // namespace

int launch_coverage_max(const CoverageArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    const int64_t blocks = (a.rows + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_coverage_max, dim3(static_cast<int>(blocks < 2048 ? blocks : 2048)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_pileup_coverage(const CoverageArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    const int64_t tiles = (a.rows + AQ_TILE - 1) / AQ_TILE;
    if (tiles >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(k_pileup_coverage, dim3(static_cast<unsigned>(tiles)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_align_quality(const AlnQualArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int64_t groups = (a.n + WAVES - 1) / WAVES;
    const int grid = static_cast<int>(groups < 1536 ? groups : 1536);  // 256 CUs x 6 resident workgroups
    hipLaunchKernelGGL(k_align_quality, dim3(grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
