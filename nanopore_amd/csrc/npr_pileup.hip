// npr_pileup.hip -- k_pileup_add, k_pileup_scan (on the tile offsets of npr_scan.h), k_pileup_depth: the per-position table of a set of
// alignments (include/nprealign.h: npr_pileup_*), what the reference gets from `samtools depth` / `samtools mpileup` after writing, converting,
// sorting and indexing the realigned SAM (nanopore/metaAnalyses/coverageDepth.py:49-65, analyses/consensus.py).
//
// Table: NPR_PILEUP_WORDS = 8 int32 per reference position (32 bytes, one row), rows in the order of the caller's reference sequences:
//   0-3 M columns by read base A C G T, 4 M columns with another read base, 5 deletion columns, 6 insertion runs attached to the position,
//   7 records whose first column is the position.
// A record costs O(its cigar runs + its M columns), never O(its reference span): a chained / realigned record is a global alignment whose leading
// and trailing D runs span the contig (4.6 * 10^6 columns per record, 2 * 10^11 per 50 000 records against 4 * 10^8 M columns).  So word 5 is
// not counted per column: a D run adds +1 at its first position and -1 one past its last to a DIFFERENCE ARRAY (two atomics per run), and the
// running sum of that array, taken when the counts are asked for, is the number of D runs that cover a position.  The difference array has one
// slot more than positions per reference sequence (sequence k's slots start at its first row + k): the -1 of a run that ends with its sequence
// lands in that sequence's spare slot, every sequence's slots sum to zero, and one plain running sum over all slots restarts from zero at every
// sequence's first row by itself.
// k_pileup_add: one wavefront per record, 64 cigar operations at a time.  First the whole cigar is summed (reference and read bases it consumes)
// and compared with what the record has: a record that runs past its read or its reference, or holds an operation outside M I D, adds nothing and
// sets *bad.  Then, per chunk: three wave prefix sums give every operation its first reference position, read position and M column; the lane
// that holds a D or I operation makes its one or two adds; the chunk's M columns are dealt to the lanes 64 at a time (column c of the chunk
// belongs to the last operation whose first M column is <= c: a 6-step search through ds_bpermute), so neighbouring lanes read neighbouring read
// bases and add to neighbouring rows whatever the run lengths are.  The adds are atomicAdd on int32 in global memory (they resolve in L2); counts
// are integers, so the table does not depend on the order.
// First numbers (tools/pileup_time.py, one MI355X, median of seven): 24 576 finished reads of ~10 kb, 227 M M columns, added where their cigars lie in
// 7.9 ms (the whole call); the running sum + depth of a 4.6 M position table 2.2 ms.  The window-owned LDS histogram has not been tried.
#include <hip/hip_runtime.h>

#include "npr_device.h"
#include "npr_scan.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;

__device__ __forceinline__ uint32_t code_of(uint32_t c) {
    c &= 0xdfu;  // upper case
    return c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u)));
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
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

__global__ void __launch_bounds__(THREADS) k_pileup_add(PileupArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * WAVES + wv; r < a.n; r += static_cast<int64_t>(gridDim.x) * WAVES) {
        const PileupRec rec = a.recs[r];
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
        if (other || sx > rec.xlen || sy > rec.ylen) {
            if (lane == 0) *a.bad = 1;
            continue;
        }
        if (sx > 0 && lane == 0) atomicAdd(a.tab + rec.row0 * NPR_PILEUP_WORDS + 7, 1);
        const uint8_t *seq = a.seq + rec.y_off;
        int X0 = 0, Y0 = 0;   // reference / read bases consumed before the chunk
        bool prev_i = false;  // the last operation of non-zero length before the chunk is an I
        for (int64_t base = 0; base < nops; base += WAVE) {
            const uint32_t w = base + lane < nops ? a.ops[o0 + base + lane] : 0u;
            const int len = static_cast<int>(w >> 2), op = static_cast<int>(w & 3u);
            const int dx = op != NPR_OP_I ? len : 0, dy = op != NPR_OP_D ? len : 0, dm = op == NPR_OP_M ? len : 0;
            const int ix = wave_scan(dx, lane), iy = wave_scan(dy, lane), im = wave_scan(dm, lane);
            const int xb = X0 + ix - dx, yb = Y0 + iy - dy, mb = im - dm;
            const unsigned long long some = __ballot(len > 0), ins = __ballot(len > 0 && op == NPR_OP_I);
            if (len > 0 && op == NPR_OP_D) {
                atomicAdd(a.diff + rec.d0 + xb, 1);
                atomicAdd(a.diff + rec.d0 + xb + len, -1);
            } else if (len > 0 && op == NPR_OP_I) {
                // attached to the last column before it; no column yet: to nothing; the operation before it is an I too: counted there
                const unsigned long long below = some & ((1ull << lane) - 1ull);
                const bool after_i = below ? ((ins >> (63 - __builtin_clzll(below))) & 1ull) != 0 : prev_i;
                if (!after_i && xb > 0) atomicAdd(a.tab + (rec.row0 + xb - 1) * NPR_PILEUP_WORDS + 6, 1);
            }
            // the chunk's M columns, 64 at a time
            const int total = __shfl(im, WAVE - 1, WAVE);
            for (int c0 = 0; c0 < total; c0 += WAVE) {
                const int c = min(c0 + lane, total - 1);
                int at = 0;
#pragma unroll
                for (int step = WAVE / 2; step >= 1; step >>= 1) {
                    const int m = __shfl(mb, at + step, WAVE);  // (at + step <= 63)
                    if (m <= c) at += step;
                }
                const int d = c - __shfl(mb, at, WAVE);
                const int x = __shfl(xb, at, WAVE) + d, y = __shfl(yb, at, WAVE) + d;
                if (c0 + lane < total) {
                    const uint32_t b = seq[y];
                    const uint32_t code = a.ascii ? code_of(b) : min(b, 4u);
                    atomicAdd(a.tab + (rec.row0 + x) * NPR_PILEUP_WORDS + code, 1);
                }
            }
            X0 += __shfl(ix, WAVE - 1, WAVE), Y0 += __shfl(iy, WAVE - 1, WAVE);
            if (some) prev_i = ((ins >> (63 - __builtin_clzll(some))) & 1ull) != 0;
        }
    }
}

// ---- the running sum of the difference array into word 5 of the table ----
// The tiled scan of npr_scan.h with a last pass of its own: the tiles' sums, their exclusive running sum (k_scan_tile_sums, k_scan_group), then
// every tile's INCLUSIVE running sum on top of its offset, written to word 5 of the slot's row.  Slot j of sequence k (dbase[k] <= j < dbase[k + 1],
// dbase[k] = first row of k + k) is row j - k; the last slot of a sequence is the spare one and has no row.
__global__ void __launch_bounds__(SCAN_THREADS) k_pileup_scan(PileupScanArgs a) {
    __shared__ int32_t lds[SCAN_WAVES];
    const int64_t j0 = scan_first_entry();
    int32_t v[SCAN_PER_THREAD], total;
    int32_t run = a.tile[blockIdx.x] + block_scan_exclusive(scan_load(a.diff, a.n_slots, j0, v), lds, &total);
    if (j0 >= a.n_slots) return;
    // the sequence of the thread's first slot: the last k with dbase[k] <= j0
    int64_t lo = 0, hi = a.n_refs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.dbase[mid] <= j0) lo = mid; else hi = mid - 1;
    }
    int64_t k = lo, end = a.dbase[k + 1];
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) {
        const int64_t j = j0 + q;
        if (j >= a.n_slots) break;
        while (j >= end) end = a.dbase[++k + 1];  // (dbase[n_refs] = n_slots > j: the walk ends)
        run += v[q];
        if (j != end - 1) a.tab[(j - k) * NPR_PILEUP_WORDS + 5] = run;
    }
}

// depth as `samtools depth` prints it (words 0-4) and whether the position gets a line (words 0-5): 5 bytes per position leave the device
__global__ void __launch_bounds__(THREADS) k_pileup_depth(const int32_t *tab, int64_t rows, int32_t *depth, uint8_t *covered) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (r >= rows) return;
    const int4 *p = reinterpret_cast<const int4 *>(tab + r * NPR_PILEUP_WORDS);
    const int4 u = p[0], v = p[1];
    const int d = u.x + u.y + u.z + u.w + v.x;
    depth[r] = d;
    covered[r] = (d + v.y) != 0;
}

}  // namespace

int launch_pileup_add(const PileupArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int64_t groups = (a.n + WAVES - 1) / WAVES;
    const int grid = static_cast<int>(groups < 4096 ? groups : 4096);  // 256 CUs x 4 workgroups x 4 wavefronts: half of every SIMD's slots
    hipLaunchKernelGGL(k_pileup_add, dim3(grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_pileup_scan(const PileupScanArgs &a, void *stream) {
    if (a.n_slots <= 0 || a.n_refs <= 0) return 0;
    const int64_t tiles = scan_tiles(a.n_slots);
    if (tiles >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((k_scan_tile_sums<int32_t, int32_t>), dim3(static_cast<unsigned>(tiles)), dim3(SCAN_THREADS), 0, st, a.diff, a.n_slots, a.tile);
    hipLaunchKernelGGL((k_scan_group<int32_t, int32_t>), dim3(1), dim3(SCAN_THREADS), 0, st, a.tile, a.tile, tiles - 1);
    hipLaunchKernelGGL(k_pileup_scan, dim3(static_cast<unsigned>(tiles)), dim3(SCAN_THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_pileup_depth(const int32_t *tab, int64_t rows, int32_t *depth, uint8_t *covered, void *stream) {
    if (rows <= 0) return 0;
    const int64_t grid = (rows + THREADS - 1) / THREADS;
    if (grid >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(k_pileup_depth, dim3(static_cast<unsigned>(grid)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), tab, rows, depth, covered);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
