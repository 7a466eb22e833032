// npr_kmer.hip -- k_kmer_spectrum, k_kmer_spectrum_groups, k_indel_kmers: the k-mer tables of the reference's KmerAnalysis, UnmappedKmerAnalysis and
// IndelKmerAnalysis, counted on the device.
//
// nanopore/analyses/kmerAnalysis.py:15-28 slices every window of every reference and read sequence in Python, and
// indelKmerAnalysis.py:11-19, :29-40 walks every alignment column of every SAM record through an ordered set to find the k-mers that
// straddle a gap.  Both are integer histograms over base codes; here each is one kernel that adds into a table of 4^k + 1 bins (a k-mer's bin
// is its base-4 number, first base most significant, A C G T = 0..3; the last bin takes the k-mers that hold any other base), k = 1 .. 6.
// The reverse complements (kmerAnalysis.py:20, :28) and reversals (indelKmerAnalysis.py:36, :40) the reference adds are permutations of the
// bins and are left to the host.  Counts are exact integers: the tests compare them with Counters over Python slices and with a literal
// restatement of the reference's column walk.
//
// First numbers (rocprofv3 --kernel-trace --stats, tools/kmer_time.py: 50 000 reads of ~8 kb, k = 5, one MI355X): k_kmer_spectrum 0.67 ms for
// 394 MB of bases (0.59 TB/s: the LDS adds, not HBM, set the pace); k_indel_kmers 10.5 ms for 98.8 M cigar words read twice (0.79 GB) and
// 160 M k-mers counted -- the wave-uniform walk over the operations is what it waits for.  Neither shape has been tuned.
// k_kmer_spectrum_groups (the same windows into one table per group, below), same bases dealt round-robin into groups, same box and session
// (tools/kmer_groups_time.py, medians of seven launches, range in brackets; profiles/kmer_groups_time.json): k_kmer_spectrum 0.667 ms
// (0.666 - 0.668; the parent commit's build 0.666, 0.665 - 0.667), two groups 0.688 ms (0.687 - 0.690: + 3.3 %), eight groups 0.706 ms
// (0.702 - 0.706: + 5.9 %) -- outside the 0.3 % the launches scatter by.  What it does more: a flush per group a workgroup meets (each
// of the 2304 workgroups strides over the whole text and so meets every group: G x 1025 64-bit atomics per workgroup instead of 1 x), and per
// tile four dependent loads from the group tables (tile0, seq_first twice, the group's end) before the tile's own search can start; the
// step from one table to two groups (one more flush) costs more than each further group, which points at the per-tile loads.  Keeping
// them in registers until the group changes is the obvious next step and has not been measured.  The whole call (stage the spans into
// the pinned buffer ordered by group, one H2D, kernel, D2H): 13.6 ms (12.6 - 26.8) for two groups and 12.6 ms (11.9 - 13.1) for eight,
// against 8.2 / 9.9 ms for npr_kmer_counts once per group on bases that ALREADY lie contiguous per group (all bases as one table: 8.1 ms)
// and ~1 000 ms when numpy has to gather each group first: the staging copy of 394 MB on the host is the difference, and it is serial
// with the H2D it feeds.
// Block shape (chosen before any measurement; the reasons are arithmetic):
//   Both kernels keep their histogram in LDS as 32-bit counters (4 bytes x 4097 bins = 16 KB per table at k = 6) and flush it to the 64-bit
//   table in global memory with one atomic per non-empty bin and workgroup -- the per-base traffic never leaves the CU.  256 threads per
//   workgroup: four wavefronts share one histogram, so a CU's 160 KB of LDS holds 9 workgroups of k_kmer_spectrum (16 KB) or 4 of
//   k_indel_kmers (two tables, 32 KB) -- 32 / 16 wavefronts per CU, enough to cover the latency of an LDS atomic that waits on a bank;
//   one wavefront per workgroup would leave 9 / 4 wavefronts per CU, 64 lanes adding into one table from 1024 threads would make the
//   flush rarer but serialise more adds on hot bins (poly-A).  A 32-bit counter cannot overflow: k_kmer_spectrum flushes after 2^18 tiles
//   (at most 2^13 adds each), k_indel_kmers before the records at hand could add 2^32 (a record adds at most one k-mer per position).
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int RUN = 32;               // window starts per lane and tile of k_kmer_spectrum: two 16-byte loads, the halo in a third
constexpr int TILE = THREADS * RUN;
static_assert(TILE == NPR_KMER_TILE, "the host lays the groups of k_kmer_spectrum_groups out in tiles of this size");
static_assert(RUN + 16 <= NPR_KMER_PAD, "a lane whose run starts at the last base reads RUN + 16 bytes");

__device__ __forceinline__ uint32_t code_of(uint32_t c) {
    c &= 0xdfu;  // upper case
    return c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u)));
}

__device__ __forceinline__ void flush(uint32_t *h, int nb, unsigned long long *out) {
    __syncthreads();
    for (int q = threadIdx.x; q < nb; q += blockDim.x) {
        const uint32_t v = h[q];
        h[q] = 0;
        if (v) atomicAdd(out + q, static_cast<unsigned long long>(v));
    }
    __syncthreads();
}

// Every window s[j .. j + k) of every sequence with j + k < len(s): kmerAnalysis.py:16-17's `xrange(kmerSize, len(seq))` stops one window
// short of the end, and so does this.  The bases of all sequences lie back to back; a lane owns RUN consecutive window starts, reads its
// run and a halo of k - 1 bases, keeps the code of the last k bases and the number of bases since the last one outside ACGT, and adds a
// window when it lies inside one sequence (the sequence of a lane's first start: a search per wavefront, then a walk along seq_off).
// One tile of one lane: the window starts j0 .. j0 + RUN of bases that end at n, which seq_off[0 .. n_seqs] cuts into sequences
// (seq_off[0] <= the tile's first base, seq_off[n_seqs] = n).
__device__ __forceinline__ void count_run(uint32_t *hist, const uint8_t *seq, int64_t tile0, int64_t n, const int64_t *seq_off, int64_t n_seqs, int k, int nb,
                                          uint32_t mask) {
    const int64_t j0 = tile0 + static_cast<int64_t>(threadIdx.x) * RUN;
    if (j0 < n) {
        // last sequence that starts at or before the wavefront's first base
        const int64_t jw = tile0 + static_cast<int64_t>(threadIdx.x & ~(WAVE - 1)) * RUN;
        int64_t lo = 0, hi = n_seqs - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (seq_off[mid] <= jw) lo = mid; else hi = mid - 1;
        }
        int64_t si = lo, end = seq_off[si + 1];
        const uint4 *p = reinterpret_cast<const uint4 *>(seq + j0);
        const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
        const uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        uint32_t code = 0;
        int good = 0;
#pragma unroll
        for (int i = 0; i < RUN + NPR_KMER_MAX_K - 1; ++i) {
            if (i < RUN + k - 1) {
                const uint32_t c = code_of((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
                code = ((code << 2) | (c & 3u)) & mask;
                good = c < 4u ? good + 1 : 0;
                const int64_t j = j0 + i - (k - 1);  // start of the window that ends with this base
                if (i >= k - 1 && j < n) {
                    while (j >= end) end = seq_off[++si + 1];  // (seq_off[n_seqs] = n > j: the walk ends)
                    if (j + k < end) atomicAdd(&hist[good >= k ? code : static_cast<uint32_t>(nb - 1)], 1u);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_kmer_spectrum(KmerArgs a) {
    extern __shared__ uint32_t hist[];
    const int k = a.k, nb = kmer_bins(k);
    const uint32_t mask = static_cast<uint32_t>(nb - 2);
    for (int q = threadIdx.x; q < nb; q += THREADS) hist[q] = 0;
    __syncthreads();
    const int64_t tiles = (a.n + TILE - 1) / TILE;
    int since_flush = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        count_run(hist, a.seq, tile * TILE, a.n, a.seq_off, a.n_seqs, k, nb, mask);
        if (++since_flush == (1 << 18)) flush(hist, nb, a.counts), since_flush = 0;
    }
    flush(hist, nb, a.counts);
}

// The same windows into one table per group (the unmapped-read meta-analyses: read type x mapped / unmapped).  The host has laid the
// sequences out ordered by group, every group's bases from a tile boundary on (KmerGroupArgs), so a tile belongs to one group and is
// counted exactly as k_kmer_spectrum counts it, with the group's own end and its own stretch of seq_off.  A workgroup still keeps ONE
// histogram: its tiles come in ascending order, so their groups do too, and it flushes to the table of the group it leaves -- at most one
// flush per group a workgroup touches (4 atomics per thread at k = 5), the LDS budget above unchanged for any number of groups.
__global__ void __launch_bounds__(THREADS) k_kmer_spectrum_groups(KmerGroupArgs a) {
    extern __shared__ uint32_t hist[];
    const int k = a.k, nb = kmer_bins(k);
    const uint32_t mask = static_cast<uint32_t>(nb - 2);
    for (int q = threadIdx.x; q < nb; q += THREADS) hist[q] = 0;
    __syncthreads();
    const int64_t tiles = a.tile0[a.n_groups];
    int since_flush = 0, g = 0, cur = -1;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        while (tile >= a.tile0[g + 1]) ++g;  // (tile < tile0[n_groups]: the walk ends; a group without bases has no tile)
        if (g != cur) {
            if (cur >= 0) flush(hist, nb, a.counts + static_cast<int64_t>(cur) * nb), since_flush = 0;
            cur = g;
        }
        const int64_t first = a.seq_first[g], n_seqs = a.seq_first[g + 1] - first - 1;
        const int64_t *seq_off = a.seq_off + first;
        count_run(hist, a.seq, tile * TILE, seq_off[n_seqs], seq_off, n_seqs, k, nb, mask);
        if (++since_flush == (1 << 18)) flush(hist, nb, a.counts + static_cast<int64_t>(cur) * nb), since_flush = 0;
    }
    if (cur >= 0) flush(hist, nb, a.counts + static_cast<int64_t>(cur) * nb);
}

// ---- k_indel_kmers ----
// The reference walks a record's alignment columns on each side -- the read side holds a read position for an M or I column and None for a D
// column, the reference side a reference position for M or D and None for I -- through an ordered set r of at most k + 1 distinct elements
// (None is in it at most once): add the element; if r[0] is None, or r is full and its last element is None, or r is full without None:
// drop r[0]; else if r is full: count the k-mer seq[r[0] .. r[k]] (k consecutive bases, the gap point somewhere inside) and drop r[0].
// In runs instead of columns, per side (tests/test_kmer_host.py pins this against the literal walk on random cigars):
//   r is either b <= k positions without None, or "live": None with c <= k - 1 positions after it.
//   positions, m of them: not live: b = min(b + m, k); live: c += m while that stays <= k - 1, else None has left: not live, b = k.
//   a gap of g columns: live and c < k - 1: nothing at all (the gap is swallowed); live and c = k - 1: its first column drops the old None
//   (not live, b = k - 1) and the rest is a gap of g - 1 columns; not live, g > 0 and b >= 1: the gap goes live with b0 = min(b, k - 1)
//   positions before it and c = 0, and will count the k-mers that start at pos - b0 .. pos - b0 + E - 1, E = min(F, k - 1) - (k - b0) + 1
//   clamped to [0, b0], F = positions of this side still to come in the record -- later gaps cannot interrupt it, they are swallowed.
// So a long M run costs nothing and a gap is O(1) for the walk; its at most k - 1 k-mers are read by the lane that holds the gap's operation.
// One wavefront per record, 64 operations at a time: the walk over the chunk's operations is wave-uniform (both sides at once: an I is a gap
// of the reference side, a D of the read side, so an operation opens at most one gap), the k-mers of the chunk's gaps are counted in parallel.
// Positions are window coordinates (the aligned part of the read).  The reference indexes record.query with positions that count from the
// start of SEQ, which differ for a soft-clipped record; for records without soft clips (every chained or realigned record) the two agree.
struct Side {
    int live, b, c, pos;
    int total;  // positions of this side in the whole record
};
__device__ __forceinline__ int side_gap(Side &s, int g, int k, int &first) {
    if (s.live) {
        if (s.c != k - 1) return 0;
        s.live = 0, s.b = k - 1, --g;
    }
    if (g <= 0 || s.b < 1) return 0;
    const int b0 = min(s.b, k - 1);
    first = s.pos - b0;
    s.live = 1, s.c = 0;
    return max(0, min(min(s.total - s.pos, k - 1) - (k - b0) + 1, b0));
}
__device__ __forceinline__ void side_positions(Side &s, int m, int k) {
    if (s.live) {
        if (m <= k - 1 - s.c) s.c += m; else s.live = 0, s.b = k;
    } else {
        s.b = m >= k ? k : min(s.b + m, k);
    }
    s.pos += m;
}

__global__ void __launch_bounds__(THREADS) k_indel_kmers(IndelKmerArgs a) {
    extern __shared__ uint32_t hist[];  // read-side table, reference-side table, one bound per wavefront
    const int k = a.k, nb = kmer_bins(k);
    const uint32_t mask = static_cast<uint32_t>(nb - 2);
    uint32_t *bound = hist + 2 * nb;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    constexpr int WAVES = THREADS / WAVE;
    for (int q = threadIdx.x; q < 2 * nb; q += THREADS) hist[q] = 0;
    __syncthreads();
    unsigned long long pending = 0;  // adds a bin may have taken since the last flush, at most
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * WAVES; first < a.s.n_reads; first += static_cast<int64_t>(gridDim.x) * WAVES) {
        const int64_t r = first + wv;
        bool ok = false;
        int64_t o0 = 0;
        int nops = 0, tx = 0, ty = 0;
        StatsSeg g{};
        if (r < a.s.n_reads && a.s.seg_off[r + 1] > a.s.seg_off[r]) {
            o0 = a.s.ops_off[r];
            nops = static_cast<int>(a.s.ops_off[r + 1] - o0);
            g = a.s.segs[a.s.seg_off[r]];
            long long sx = 0, sy = 0;
            for (int i = lane; i < nops; i += WAVE) {
                const uint32_t w = a.s.ops[o0 + i];
                const long long len = w >> 2;
                if ((w & 3u) != NPR_OP_I) sx += len;
                if ((w & 3u) != NPR_OP_D) sy += len;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sx += __shfl_xor(sx, o, WAVE), sy += __shfl_xor(sy, o, WAVE);
            ok = sx <= g.xe - g.xs && sy <= g.ye - g.ys;
            if (!ok && lane == 0) *a.bad = 1;
            tx = static_cast<int>(sx), ty = static_cast<int>(sy);
        }
        if (lane == 0) bound[wv] = ok ? static_cast<uint32_t>(max(tx, ty)) : 0u;
        __syncthreads();
        unsigned long long sum = 0;
        for (int q = 0; q < WAVES; ++q) sum += bound[q];
        if (pending + sum >= (1ull << 32)) {
            flush(hist, nb, a.read_counts);
            flush(hist + nb, nb, a.ref_counts);
            pending = 0;
        }
        pending += sum;
        if (ok && k > 1) {
            const uint8_t *seq_y = a.s.seq + g.y_off, *seq_x = a.s.seq + g.x_off;
            Side sy{0, 0, 0, 0, ty}, sx{0, 0, 0, 0, tx};
            for (int base = 0; base < nops; base += WAVE) {
                const int cnt = min(WAVE, nops - base);
                const uint32_t w = lane < cnt ? a.s.ops[o0 + base + lane] : 0u;
                int my_first = 0, my_count = 0, my_side = 0;
                for (int i = 0; i < cnt; ++i) {
                    const uint32_t wi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(w), i));
                    const int op = static_cast<int>(wi & 3u), len = static_cast<int>(wi >> 2);
                    if (len == 0) continue;
                    int f = 0, e = 0;
                    if (op == NPR_OP_D) e = side_gap(sy, len, k, f); else side_positions(sy, len, k);
                    if (op == NPR_OP_I) e = side_gap(sx, len, k, f); else side_positions(sx, len, k);
                    if (lane == i && e > 0) my_first = f, my_count = e, my_side = op == NPR_OP_I;
                }
                if (my_count > 0) {
                    const uint8_t *p = (my_side ? seq_x : seq_y) + my_first;
                    uint32_t *h = hist + (my_side ? nb : 0);
                    uint32_t code = 0;
                    int good = 0;
                    for (int t = 0; t < k - 1 + my_count; ++t) {
                        const uint32_t c = p[t];
                        code = ((code << 2) | (c & 3u)) & mask;
                        good = c < 4u ? good + 1 : 0;
                        if (t >= k - 1) atomicAdd(&h[good >= k ? code : static_cast<uint32_t>(nb - 1)], 1u);
                    }
                }
            }
        }
        __syncthreads();
    }
    flush(hist, nb, a.read_counts);
    flush(hist + nb, nb, a.ref_counts);
}

}  // namespace

int launch_kmer_spectrum(const KmerArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int64_t tiles = (a.n + TILE - 1) / TILE;
    const int grid = static_cast<int>(tiles < 2304 ? tiles : 2304);  // 256 CUs x 9 resident workgroups
    hipLaunchKernelGGL(k_kmer_spectrum, dim3(grid), dim3(THREADS), sizeof(uint32_t) * kmer_bins(a.k), static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_kmer_spectrum_groups(const KmerGroupArgs &a, int64_t tiles, void *stream) {
    if (tiles <= 0) return 0;
    const int grid = static_cast<int>(tiles < 2304 ? tiles : 2304);  // as k_kmer_spectrum
    hipLaunchKernelGGL(k_kmer_spectrum_groups, dim3(grid), dim3(THREADS), sizeof(uint32_t) * kmer_bins(a.k), static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_indel_kmers(const IndelKmerArgs &a, void *stream) {
    if (a.s.n_reads <= 0) return 0;
    const int64_t groups = (static_cast<int64_t>(a.s.n_reads) + THREADS / WAVE - 1) / (THREADS / WAVE);
    const int grid = static_cast<int>(groups < 2048 ? groups : 2048);
    hipLaunchKernelGGL(k_indel_kmers, dim3(grid), dim3(THREADS), sizeof(uint32_t) * (2 * kmer_bins(a.k) + THREADS / WAVE), static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
