// npr_bampile.hip -- k_bampile_check, k_bampile_add: the records of an uncompressed BAM stream (what npr_inflate.hip leaves on the device, walked
// by k_bam_head / k_bam_walk of npr_bamread.hip) into the table of a pileup (npr_pileup.hip) where they lie: no SAM text, no cigar rebuilt on
// the host, no base uploaded again (the ABI: include/nprealign.h, npr_bam_open and npr_pileup_add_bam; the host side: npr_bam_api.cpp).
//   k_bampile_check  a thread a record runs bamrec_check (npr_bamrec.h, the body the host program of tests/native/bamrec_check.cpp runs too):
//                    selected or not, the stored cigar or -- under the placeholder <l_seq>S<n>N, the only records whose auxiliary bytes are
//                    walked -- the elements of the first CG:B:I field, the reference and read bases the cigar consumes in 64 bits, the verdict.
//                    It writes the verdict, where the cigar words and the packed bases lie, the row of POS and its slot in the difference array,
//                    and counts the selected, added and refused records.  Every cigar is checked here, before the first add of any record.
//   k_bampile_add    one wavefront per record with the verdict BR_ADD, 64 operations at a time, the structure of k_pileup_add: three wave prefix
//                    sums give every operation its first reference position, read position and column (M = X); the lane of a D run makes its two
//                    adds to the difference array; the lane of an I run looks for the last run of non-zero length before it that is a column run
//                    (M D = X) or an I run -- in the chunk by two ballots, before the chunk by what the last chunk left -- and adds to word 6 of
//                    that column run's last row, or not at all after an I run or before the first column; the first column run's lane adds to
//                    word 7; the chunk's columns are dealt to the lanes 64 at a time (the 6-step search of k_pileup_add), so neighbouring lanes
//                    read neighbouring nibbles and add to neighbouring rows.  What differs from k_pileup_add: the operations are BAM words
//                    (length << 4 | code, nine codes) at any alignment in the stream, read bytewise; the bases are nibbles, high one first (1 2 4
//                    8 are A C G T, words 0-3; every other code word 4); the read position advances over S too, the reference position over N.
// The adds are atomicAdd on int32 in global memory; counts are integers, so the table does not depend on the order.  The six lines of the wave
// prefix sum are this unit's own, as in npr_pileup.hip, npr_alnqual.hip and npr_cigtext.hip.
// First numbers (tools/bam_pileup_time.py, profiles/bam_pileup_time.json; one MI355X, medians of seven after a warm-up).  They are WHOLE CALLS from
// the file on disk to the depth arrays on the host (read, block scan, H2D, inflate, walk, these two kernels, the running sum, depth, D2H); the
// kernels were not timed alone (a compressed file's time is mostly its inflate: tools/bam_read_time.py had the whole npr_bgzf_inflate call on that
// file, the stream's copy back included, at 470 ms).  50 000 records of ~8 kb, 355 M
// M columns on a 4.6 Mb contig: pileup_of_bam + depth() 185 ms from the stored 988 MB file and 539 ms from the compressed 272 MB one, against 682
// and 1 023 ms through bam_to_sam + pileup_of_sam + depth() (607 MB of SAM text); the eighth-size files 30 and 78 ms against 106 and 155 ms.
#include <hip/hip_runtime.h>

#include "npr_bamrec.h"
#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;

__device__ __forceinline__ int wave_scan(int v, int lane) {  // inclusive
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ void __launch_bounds__(THREADS) k_bampile_check(BamPileArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int64_t at = a.rec_off[i];
    BamRecVerdict v;
    bamrec_check(a.stream + at, a.len - at, a.ref_len, a.n_ref, a.flag_mask, v);
    BamPileRec rec;
    rec.ops_at = at + v.ops_at, rec.n_ops = v.n_ops, rec.seq_at = at + v.seq_at, rec.row0 = 0, rec.d0 = 0, rec.verdict = v.verdict, rec.pad = 0;
    if (v.verdict == BR_ADD) {
        rec.d0 = a.dbase[v.tid] + v.pos;
        rec.row0 = rec.d0 - v.tid;
    }
    a.recs[i] = rec;
    if (v.verdict == BR_SKIP) return;
    atomicAdd(a.counts + 1, 1ull);
    atomicAdd(a.counts + (v.verdict == BR_ADD ? 2 : 3), 1ull);
}

__global__ void __launch_bounds__(THREADS) k_bampile_add(BamPileArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * WAVES + wv; r < a.n; r += static_cast<int64_t>(gridDim.x) * WAVES) {
        const BamPileRec rec = a.recs[r];
        if (rec.verdict != BR_ADD) continue;
        // (k_bampile_check: POS >= 0, POS + the reference bases <= l_ref < 2^31, the read bases = l_seq < 2^31: positions fit an int)
        const uint8_t *ops = a.stream + rec.ops_at, *seq = a.stream + rec.seq_at;
        int X0 = 0, Y0 = 0;   // reference / read bases consumed before the chunk
        int prev_kind = 0;    // the last run of non-zero length before the chunk that is a column run (1) or an I run (2); 0: none yet
        int prev_end = 0;     // ... a column run: the reference position one past its last column
        bool started = false; // a column run lies before the chunk
        for (int64_t base = 0; base < rec.n_ops; base += WAVE) {
            const uint32_t w = base + lane < rec.n_ops ? br_ld32(ops + 4 * (base + lane)) : 0u;
            const int len = static_cast<int>(w >> 4);
            const uint32_t op = w & 15u;
            const bool is_m = op == 0u || op == 7u || op == 8u;
            const int dx = (is_m || op == 2u || op == 3u) ? len : 0, dy = (is_m || op == 1u || op == 4u) ? len : 0, dm = is_m ? len : 0;
            const int ix = wave_scan(dx, lane), iy = wave_scan(dy, lane), im = wave_scan(dm, lane);
            const int xb = X0 + ix - dx, yb = Y0 + iy - dy, mb = im - dm;
            const bool is_col = len > 0 && (is_m || op == 2u), is_ins = len > 0 && op == 1u;
            const unsigned long long cols = __ballot(is_col), ins = __ballot(is_ins), both = cols | ins;
            if (!started && cols) {
                if (lane == __builtin_ctzll(cols)) atomicAdd(a.tab + (rec.row0 + xb) * NPR_PILEUP_WORDS + 7, 1);
                started = true;
            }
            if (len > 0 && op == 2u) {
                atomicAdd(a.diff + rec.d0 + xb, 1);
                atomicAdd(a.diff + rec.d0 + xb + len, -1);
            }
            // an I run: attached to the last column before it; no column yet: to nothing; an I run since that column: counted there
            const unsigned long long below = both & ((1ull << lane) - 1ull);
            const int src = below ? 63 - __builtin_clzll(below) : 0;
            const int src_end = __shfl(xb + dx, src, WAVE);
            if (is_ins) {
                const int kind = below ? (((ins >> src) & 1ull) ? 2 : 1) : prev_kind;
                const int end = below ? src_end : prev_end;
                if (kind == 1) atomicAdd(a.tab + (rec.row0 + end - 1) * NPR_PILEUP_WORDS + 6, 1);
            }
            // the chunk's M = X columns, 64 at a time
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
                    const uint32_t b = seq[y >> 1];
                    const uint32_t nib = (y & 1) ? (b & 15u) : (b >> 4);
                    const uint32_t code = nib == 1u ? 0u : (nib == 2u ? 1u : (nib == 4u ? 2u : (nib == 8u ? 3u : 4u)));
                    atomicAdd(a.tab + (rec.row0 + x) * NPR_PILEUP_WORDS + code, 1);
                }
            }
            if (both) {
                const int last = 63 - __builtin_clzll(both);
                prev_kind = ((ins >> last) & 1ull) ? 2 : 1;
                prev_end = __shfl(xb + dx, last, WAVE);
            }
            X0 += __shfl(ix, WAVE - 1, WAVE), Y0 += __shfl(iy, WAVE - 1, WAVE);
        }
    }
}

}  // namespace

int launch_bampile_check(const BamPileArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int64_t grid = (a.n + THREADS - 1) / THREADS;
    if (grid >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(k_bampile_check, dim3(static_cast<unsigned>(grid)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_bampile_add(const BamPileArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int64_t groups = (a.n + WAVES - 1) / WAVES;
    const int grid = static_cast<int>(groups < 4096 ? groups : 4096);  // as launch_pileup_add: half of every SIMD's slots
    hipLaunchKernelGGL(k_bampile_add, dim3(grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
