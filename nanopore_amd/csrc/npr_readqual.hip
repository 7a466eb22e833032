// npr_readqual.hip -- k_read_quality, k_read_quality_reads: the read-quality tables of the FastQC analysis, counted on the device.
//
// nanopore/analyses/fastqc.py hands the FASTQ file to the Java FastQC.  What this build reports instead is defined in exact integer terms in
// include/nprealign.h (npr_read_quality): per position bin (sixteen bins per octave, 336 in all) a histogram of the quality bytes and of the
// base codes, and per read its length bin, its mean quality, its G + C percentage, and the totals of a group.  Both kernels only add integers;
// the tests compare every table with np.add.at over the same definitions.
//
// Block shape (chosen before any measurement; the reasons are arithmetic):
//   The unit of work is a (read, tile) pair: RQ_TILE = 2048 consecutive positions of one read, eight per lane of a 256-thread workgroup, read
//   with one aligned 8-byte load of the bases and one of the quality bytes.  A 200 kb read is a hundred items spread over the grid and a
//   100-base read is one item.  The host lays the items out by one counting sort (a histogram over (group, tile index), ONE prefix sum, one
//   scatter) so that the items of one key lie together, and a workgroup takes one contiguous stretch of the list: it meets a new key, and
//   flushes, about once or twice in its life and not once per read -- ten thousand 100-base reads are ten thousand items of the key
//   (group, tile 0) and share one flush per workgroup.
//   Histograms are 32-bit LDS counters addressed relative to the tile's first bin, 100 columns per bin (95 quality columns, 5 base columns).
//   Tile 0 (positions 0 .. 2047) touches bins 0 .. 127: one table of 128 x 100 counters = 51 200 B.  A later tile starts at a multiple of 2048
//   >= 2048, where a bin is 128 positions wide or wider and bin edges and octave edges are multiples of the bin width, so it touches at most 16
//   bins (the issue's bound of 17 allows for an unaligned tile, which does not occur); the same LDS then holds EIGHT copies of a 16 x 100 table,
//   a lane adding into copy lane & 7.  Far from the read's start all 64 lanes of a wavefront fall into one bin and quality values cluster, so
//   same-address adds are the expected limiter (as npr_kmer.hip's header found for its hot bins): the copies cut the lanes that can meet on
//   one counter from 64 to 8, a copy is 1601 words long so that the eight copies of a counter lie in eight different banks, and a lane first
//   combines what its own eight positions add to one counter (equal neighbouring quality bytes; the five base counters of its bin) into one
//   add.  All of this is integer adds into counters that are summed at the flush: the counts stay exact.
//   LDS per workgroup: 8 x 1601 x 4 = 51 232 B, so three workgroups (twelve wavefronts) fit the 160 KB of a CU; the issue asks for two.  A
//   whole-table layout (336 x 100 x 4 = 134 KB) would leave one.
//   A flush adds only the non-zero counters to the 64-bit tables (one global atomic each, as npr_kmer.hip's flush); no global atomic is issued
//   per base.  A counter takes at most 2048 per item and a workgroup flushes after 2^20 items at the latest: no counter can reach 2^32.
//   The per-read sums (quality sum, G + C, A + C + G + T, bad quality bytes, smallest and largest quality byte) are reduced per wavefront with
//   shuffles and added into the read's scratch row by lane 0: six 64-bit atomics per wavefront and item at most.
//   k_read_quality_reads, one thread per read, turns the rows into len_hist, meanq_hist, gc_hist and totals, again through LDS counters
//   (32-bit for the histograms, 64-bit for the totals) and one flush per workgroup.  No floating point anywhere.
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int RUN = 8;  // positions per lane and item
static_assert(THREADS * RUN == RQ_TILE, "a workgroup takes one tile per item");
static_assert(RUN <= RQ_ALIGN, "a lane's load stays inside the padding of its read");
constexpr int COLS = RQ_QUAL_COLS + RQ_BASE_COLS;        // counters per position bin in LDS
constexpr int NEAR_BINS = 128, FAR_BINS = 16, COPIES = 8;
constexpr int FAR_STRIDE = FAR_BINS * COLS + 1;          // words from one copy to the next: odd, so the copies of a counter lie in different banks
constexpr int LDS_WORDS = COPIES * FAR_STRIDE > NEAR_BINS * COLS ? COPIES * FAR_STRIDE : NEAR_BINS * COLS;
static_assert(LDS_WORDS * 4 * 3 <= 160 * 1024, "three workgroups per CU");
constexpr int FLUSH_ITEMS = 1 << 20;                     // x RQ_TILE adds at most = 2^31 per counter
constexpr int READ_WORDS = RQ_POS_BINS + RQ_QUAL_COLS + RQ_GC_COLS;  // the per-read histograms of one group in k_read_quality_reads

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

// the table a workgroup holds: tile 0 or a later tile of one group, LDS bin 0 = table bin b0
struct Held {
    int group;
    uint32_t b0;
    bool far;
};

__device__ __forceinline__ void flush(uint32_t *h, const Held &t, const ReadQualArgs &a) {
    __syncthreads();
    const int words = (t.far ? FAR_BINS : NEAR_BINS) * COLS;
    for (int q = threadIdx.x; q < words; q += THREADS) {
        uint32_t v = 0;
        if (t.far) {
#pragma unroll
            for (int c = 0; c < COPIES; ++c) v += h[c * FAR_STRIDE + q], h[c * FAR_STRIDE + q] = 0;
        } else {
            v = h[q], h[q] = 0;
        }
        const uint32_t bin = t.b0 + static_cast<uint32_t>(q / COLS), col = static_cast<uint32_t>(q % COLS);
        if (v && bin < RQ_POS_BINS) {
            const size_t row = static_cast<size_t>(t.group) * RQ_POS_BINS + bin;
            if (col < RQ_QUAL_COLS) atomicAdd(a.pos_qual + row * RQ_QUAL_COLS + col, static_cast<unsigned long long>(v));
            else atomicAdd(a.pos_base + row * RQ_BASE_COLS + (col - RQ_QUAL_COLS), static_cast<unsigned long long>(v));
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(THREADS) k_read_quality(ReadQualArgs a) {
    __shared__ uint32_t h[LDS_WORDS];
    for (int q = threadIdx.x; q < LDS_WORDS; q += THREADS) h[q] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t per = (a.n_items + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * per, i1 = i0 + per < a.n_items ? i0 + per : a.n_items;
    Held held{-1, 0, false};
    int since_flush = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const unsigned long long item = a.items[i];
        const int64_t r = static_cast<int64_t>(item >> 32), p0 = static_cast<int64_t>(item & 0xffffffffull) * RQ_TILE;
        const int g = a.group[r];
        const int64_t len = a.len[r];
        const bool far = p0 != 0;
        const uint32_t b0 = far ? pos_bin(p0) : 0u;
        if (g != held.group || b0 != held.b0 || since_flush == FLUSH_ITEMS) {  // (b0 = 0 for tile 0 only: the key says which layout)
            if (held.group >= 0) flush(h, held, a);
            held = Held{g, b0, far}, since_flush = 0;
        }
        ++since_flush;
        if (p0 + static_cast<int64_t>(threadIdx.x - lane) * RUN >= len) continue;  // the whole wavefront lies past the read's end
        const int64_t p = p0 + static_cast<int64_t>(threadIdx.x) * RUN;
        uint32_t qsum = 0, bad = 0, inv_min = 0, qmax = 0;
        unsigned long long bases = 0;  // five 12-bit fields: the lane's (then the wavefront's: 512 at most) positions per base code
        if (p < len) {
            const int nv = len - p < RUN ? static_cast<int>(len - p) : RUN;
            const int64_t at = a.start[r] + p;  // a multiple of 8: start is one of RQ_ALIGN, p of RUN
            const uint2 sw = *reinterpret_cast<const uint2 *>(a.seq + at), qw = *reinterpret_cast<const uint2 *>(a.qual + at);
            uint32_t *hw = far ? h + (lane & (COPIES - 1)) * FAR_STRIDE : h;
            const uint32_t top = far ? FAR_BINS - 1 : NEAR_BINS - 1;  // (the bound a wrong bin could not pass; a right one never meets it)
            const bool one_bin = p >= 128;  // bins are 8 positions wide from 128 on and p is a multiple of 8
            const uint32_t rel0 = min(pos_bin(p) - b0, top);
            uint32_t prev = 0, cnt = 0;
#pragma unroll
            for (int j = 0; j < RUN; ++j) {
                if (j < nv) {
                    const uint32_t c = ((j < 4 ? qw.x : qw.y) >> (8 * (j & 3))) & 0xffu, s = code_of(((j < 4 ? sw.x : sw.y) >> (8 * (j & 3))) & 0xffu);
                    const bool ok = c - 33u <= 93u;
                    qsum += ok ? c - 33u : 0u, bad += ok ? 0u : 1u;
                    inv_min = max(inv_min, 255u - c), qmax = max(qmax, c);
                    bases += 1ull << (12 * s);
                    const uint32_t rel = one_bin ? rel0 : min(pos_bin(p + j) - b0, top);
                    const uint32_t key = rel * COLS + (ok ? c - 33u : static_cast<uint32_t>(RQ_QUAL_COLS - 1));
                    if (cnt && key == prev) {
                        ++cnt;
                    } else {
                        if (cnt) atomicAdd(&hw[prev], cnt);
                        prev = key, cnt = 1;
                    }
                    if (!one_bin) atomicAdd(&hw[rel * COLS + RQ_QUAL_COLS + s], 1u);
                }
            }
            if (cnt) atomicAdd(&hw[prev], cnt);
            if (one_bin) {
#pragma unroll
                for (int s = 0; s < RQ_BASE_COLS; ++s) {
                    const uint32_t v = static_cast<uint32_t>(bases >> (12 * s)) & 0xfffu;
                    if (v) atomicAdd(&hw[rel0 * COLS + RQ_QUAL_COLS + s], v);
                }
            }
        }
        uint32_t sums = qsum | (bad << 16);  // a wavefront's quality sum is at most 64 x 8 x 93 < 2^16
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            sums += __shfl_xor(sums, o, WAVE);
            bases += __shfl_xor(bases, o, WAVE);
            inv_min = max(inv_min, __shfl_xor(inv_min, o, WAVE));
            qmax = max(qmax, __shfl_xor(qmax, o, WAVE));
        }
        if (lane == 0) {
            unsigned long long *row = a.rows + r * RQ_ROW;
            const unsigned long long nA = bases & 0xfffu, nC = (bases >> 12) & 0xfffu, nG = (bases >> 24) & 0xfffu, nT = (bases >> 36) & 0xfffu;
            if (sums & 0xffffu) atomicAdd(row + 0, static_cast<unsigned long long>(sums & 0xffffu));
            if (nC + nG) atomicAdd(row + 1, nC + nG);
            if (nA + nC + nG + nT) atomicAdd(row + 2, nA + nC + nG + nT);
            if (sums >> 16) atomicAdd(row + 3, static_cast<unsigned long long>(sums >> 16));
            atomicMax(row + 4, static_cast<unsigned long long>(inv_min));
            atomicMax(row + 5, static_cast<unsigned long long>(qmax));
        }
    }
    if (held.group >= 0) flush(h, held, a);
}

// one thread per read: its length bin, and from its scratch row its mean quality, its G + C percentage and its part of the group's totals
__global__ void __launch_bounds__(THREADS) k_read_quality_reads(ReadQualArgs a) {
    __shared__ uint32_t h[RQ_MAX_GROUPS * READ_WORDS];
    __shared__ unsigned long long tot[RQ_MAX_GROUPS * RQ_TOTALS];
    const int hist_words = a.n_groups * READ_WORDS, tot_words = a.n_groups * RQ_TOTALS;
    for (int q = threadIdx.x; q < hist_words; q += THREADS) h[q] = 0;
    for (int q = threadIdx.x; q < tot_words; q += THREADS) tot[q] = 0;
    __syncthreads();
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x; r < a.n; r += static_cast<int64_t>(gridDim.x) * THREADS) {
        const int g = a.group[r];
        const unsigned long long len = static_cast<unsigned long long>(a.len[r]);
        uint32_t *hg = h + g * READ_WORDS;
        unsigned long long *tg = tot + g * RQ_TOTALS;
        atomicAdd(&hg[pos_bin(static_cast<int64_t>(len))], 1u);
        atomicAdd(tg + 0, 1ull);
        atomicAdd(tg + 1, len);
        atomicMax(tg + 2, RQ_LEN_TOP - len);
        atomicMax(tg + 3, len);
        if (len == 0) {
            atomicAdd(tg + 6, 1ull);
            continue;
        }
        const unsigned long long *row = a.rows + r * RQ_ROW;
        const unsigned long long qsum = row[0], gc = row[1], n = row[2], bad = row[3];
        const uint32_t mean = bad ? static_cast<uint32_t>(RQ_QUAL_COLS - 1) : min(static_cast<uint32_t>(qsum / len), static_cast<uint32_t>(RQ_QUAL_COLS - 2));
        const uint32_t pct = n ? min(static_cast<uint32_t>((200ull * gc + n) / (2ull * n)), 100u) : static_cast<uint32_t>(RQ_GC_COLS - 1);
        atomicAdd(&hg[RQ_POS_BINS + mean], 1u);
        atomicAdd(&hg[RQ_POS_BINS + RQ_QUAL_COLS + pct], 1u);
        atomicMax(tg + 4, row[4]);
        atomicMax(tg + 5, row[5]);
        if (bad) atomicAdd(tg + 7, 1ull);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < hist_words; q += THREADS) {
        const uint32_t v = h[q];
        if (!v) continue;
        const int g = q / READ_WORDS, w = q % READ_WORDS;
        unsigned long long *out = w < RQ_POS_BINS ? a.len_hist + static_cast<size_t>(g) * RQ_POS_BINS + w
                                  : w < RQ_POS_BINS + RQ_QUAL_COLS ? a.meanq_hist + static_cast<size_t>(g) * RQ_QUAL_COLS + (w - RQ_POS_BINS)
                                                                   : a.gc_hist + static_cast<size_t>(g) * RQ_GC_COLS + (w - RQ_POS_BINS - RQ_QUAL_COLS);
        atomicAdd(out, static_cast<unsigned long long>(v));
    }
    for (int q = threadIdx.x; q < tot_words; q += THREADS) {
        const unsigned long long v = tot[q];
        const int w = q % RQ_TOTALS;
        if (!v) continue;
        if (w >= 2 && w <= 5) atomicMax(a.totals + q, v); else atomicAdd(a.totals + q, v);
    }
}

}  // namespace

int launch_read_quality(const ReadQualArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    if (a.n_items > 0) {
        const int grid = static_cast<int>(a.n_items < 768 ? a.n_items : 768);  // 256 CUs x 3 resident workgroups
        hipLaunchKernelGGL(k_read_quality, dim3(grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
        const int rc = static_cast<int>(hipGetLastError());
        if (rc != 0) return rc;
    }
    const int64_t blocks = (a.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_read_quality_reads, dim3(static_cast<int>(blocks < 1024 ? blocks : 1024)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
