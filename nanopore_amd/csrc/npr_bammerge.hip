// npr_bammerge.hip -- the records of BAM streams that lie on the device (npr_bam_open) to one BAM stream there, without SAM text (the ABI:
// include/nprealign.h, "BAM streams to BAM files": npr_bam_streams_bam, npr_bam_index; the host side: npr_bammerge_api.cpp).  The sort, the
// frame and the index are npr_bam.hip's, the compressed frame npr_deflate.hip's.  Integers and bytes only: every output is exact.
//   k_merge_sources  a thread per record of one stream: where the record lies (the stream's base + its table entry), so that the records
//                    of several streams are one list.
//   k_merge_measure  a thread per record: bamrec_measure (npr_bamrec.h, one body for host and device: the cigar walk is bamrec_interval's)
//                    gives the sort key's parts, the size, end and bin; a refused record raises a.bad (atomicMax: the word does not depend on the order).
//   k_merge_ordered  (npr_bam_index) a thread per pair of neighbours: (refID, pos) never decreases, refID -1 last; else a.bad = -1.
//   k_merge_place    a thread per place j: the size, the source and the bin of the record that goes there; launch_scan_tiled (npr_scan.h)
//                    turns the sizes into offsets.
//   k_merge_gather   the copy.  The output stream behind the header is cut by DESTINATION into pieces of MERGE_PIECE bytes at multiples of
//                    MERGE_PIECE, a wavefront a piece, four to a workgroup; a lane takes every 64th chunk of 16 bytes of its piece.  The
//                    wavefront finds the records of its piece's first and last byte by binary search in the scanned sizes (a record of 300 KB
//                    is shared by 75 wavefronts and the search ends there; a piece of a hundred 40-byte records costs one wavefront), a lane the
//                    record of its chunk by a search between the two.  A chunk that lies in one record is one 16-byte store at a 16-byte-
//                    aligned address: the source, which agrees with it in no alignment, is read as the two aligned 16-byte words around it
//                    (the second only when the source is not aligned itself) and shifted together, whole words by selects, bytes by
//                    v_alignbyte.  Every aligned word read holds a byte of the record, so no read leaves the 16-byte-aligned extent of the
//                    source stream's allocation (hipMalloc: 256-byte aligned, whole pages).  Only a chunk that a record boundary, the
//                    header's end or the stream's end cuts goes a byte at a time.  The two bytes of `bin` (14, 15 of a record) are set on
//                    the way.  No LDS.  Timed alone: tools/bam_merge_time.py (profiles/bam_merge_time.json).
#include <hip/hip_runtime.h>

#include "npr_bamrec.h"
#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
static_assert(MERGE_PIECE % (16 * WAVE) == 0, "a piece is whole rounds of a wavefront's 16-byte chunks");

__global__ void __launch_bounds__(THREADS) k_merge_sources(const uint8_t *stream, const int64_t *rec_off, int64_t n, const uint8_t **src) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i < n) src[i] = stream + rec_off[i];
}

__global__ void __launch_bounds__(THREADS) k_merge_measure(MergeArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    BamRecMeasure m;
    bamrec_measure(a.src[i], m);
    if (m.refused != BR_WHY_NONE) atomicMax(a.bad, m.refused);  // (BR_WHY_OP above BR_WHY_AUX: the same word whichever thread comes first)
    BamRec r{};
    r.tid = m.tid, r.pos = m.pos, r.flag = m.flag;
    a.recs[i] = r;
    BamMeasure out{};
    out.size = m.size, out.bin = m.bin;
    out.end = static_cast<int32_t>(m.end < 0x7fffffff ? m.end : 0x7fffffff);  // (the index clamps an end to its reference's last window)
    a.meas[i] = out;
    a.tid[i] = m.tid, a.pos[i] = m.pos < -1 ? -1 : m.pos, a.flag[i] = m.flag;  // (the key takes pos + 1 as unsigned: a pos below -1 sorts with -1)
}

__global__ void __launch_bounds__(THREADS) k_merge_ordered(MergeArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x + 1;
    if (j >= a.n) return;
    const unsigned long long before = static_cast<unsigned long long>(static_cast<uint32_t>(a.tid[j - 1])) << 32 | static_cast<uint32_t>(a.pos[j - 1] + 1);
    const unsigned long long here = static_cast<unsigned long long>(static_cast<uint32_t>(a.tid[j])) << 32 | static_cast<uint32_t>(a.pos[j] + 1);
    if (here < before) atomicCAS(a.bad, 0, -1);  // (a refused record of k_merge_measure, which ran before, keeps its word)  // (refID -1 is the largest unsigned refID; pos + 1 is 0 .. 2^31 - 1)
}

__global__ void __launch_bounds__(THREADS) k_merge_place(MergeArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (j >= a.n) return;
    const int64_t i = a.order ? a.order[j] : j;
    a.size_sorted[j] = a.meas[i].size;
    a.place_src[j] = a.src[i];
    a.place_bin[j] = a.meas[i].bin;
}

// the largest j in [lo, hi] with off[j] <= e, given off[lo] <= e
__device__ __forceinline__ int64_t last_at_or_before(const int64_t *off, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t set_byte(uint32_t w, int k, uint32_t v) { return (w & ~(0xffu << (8 * k))) | v << (8 * k); }

__global__ void __launch_bounds__(THREADS) k_merge_gather(MergeArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t piece = a.header_len / MERGE_PIECE + static_cast<int64_t>(blockIdx.x) * WAVES + threadIdx.x / WAVE;
    const int64_t d0 = piece * MERGE_PIECE < a.header_len ? a.header_len : piece * MERGE_PIECE;
    const int64_t d1 = (piece + 1) * MERGE_PIECE < a.stream_len ? (piece + 1) * MERGE_PIECE : a.stream_len;
    if (d0 >= d1) return;
    const int64_t *const off = a.size_sorted;  // off[j] = first byte of place j's record behind the header, off[n] = their end; off[0] = 0
    const int64_t j_first = last_at_or_before(off, 0, a.n - 1, d0 - a.header_len);
    const int64_t j_last = last_at_or_before(off, j_first, a.n - 1, d1 - 1 - a.header_len);
    for (int64_t c = piece * MERGE_PIECE + 16 * lane; c < d1; c += 16 * WAVE) {
        const int64_t lo = c < d0 ? d0 : c, hi = c + 16 < d1 ? c + 16 : d1;
        if (lo >= hi) continue;
        int64_t j = last_at_or_before(off, j_first, j_last, lo - a.header_len);
        int64_t begin = a.header_len + off[j], end = a.header_len + off[j + 1];
        if (hi - lo == 16 && end >= hi) {
            const int64_t at = c - begin;  // the chunk is the record's bytes [at, at + 16)
            const uintptr_t s = reinterpret_cast<uintptr_t>(a.place_src[j]) + static_cast<uintptr_t>(at);
            const int shift = static_cast<int>(s & 15);
            const uint4 *const p = reinterpret_cast<const uint4 *>(s - shift);
            const uint4 w0 = p[0], w1 = shift ? p[1] : make_uint4(0, 0, 0, 0);
            uint32_t v[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            if (shift & 4) {
#pragma unroll
                for (int k = 0; k < 7; ++k) v[k] = v[k + 1];
            }
            if (shift & 8) {
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] = v[k + 2];
            }
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = __builtin_amdgcn_alignbyte(v[k + 1], v[k], static_cast<uint32_t>(shift & 3));
            if (at < 16) {  // bytes 14 and 15 of the record are its bin
                const uint32_t bin = a.place_bin[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t b = at + 4 * k;  // the record's bytes [b, b + 4)
                    if (b <= 14 && 14 < b + 4) o[k] = set_byte(o[k], static_cast<int>(14 - b), bin & 0xffu);
                    if (b <= 15 && 15 < b + 4) o[k] = set_byte(o[k], static_cast<int>(15 - b), (bin >> 8) & 0xffu);
                }
            }
            *reinterpret_cast<uint4 *>(a.raw + c) = make_uint4(o[0], o[1], o[2], o[3]);
            continue;
        }
        for (int64_t d = lo; d < hi; ++d) {  // a chunk that a record boundary or an end of the records cuts: at most 15 bytes of every such cut
            while (d >= end) ++j, begin = end, end = a.header_len + off[j + 1];  // (d < stream_len = header_len + off[n]: j stays below n)
            const int64_t at = d - begin;
            a.raw[d] = at == 14 ? static_cast<uint8_t>(a.place_bin[j] & 0xffu) : (at == 15 ? static_cast<uint8_t>(a.place_bin[j] >> 8) : a.place_src[j][at]);
        }
    }
}

template <typename K, typename... A>
int launch(K kernel, int64_t grid, void *stream, A... args) {
    if (grid <= 0) return 0;
    if (grid >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), args...);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

int launch_merge_sources(const uint8_t *stream, const int64_t *rec_off, int64_t n, const uint8_t **src, void *hip_stream) {
    return launch(k_merge_sources, (n + THREADS - 1) / THREADS, hip_stream, stream, rec_off, n, src);
}
int launch_merge_measure(const MergeArgs &a, void *stream) { return launch(k_merge_measure, (a.n + THREADS - 1) / THREADS, stream, a); }
int launch_merge_ordered(const MergeArgs &a, void *stream) { return launch(k_merge_ordered, (a.n - 1 + THREADS - 1) / THREADS, stream, a); }
int launch_merge_place(const MergeArgs &a, void *stream) { return launch(k_merge_place, (a.n + THREADS - 1) / THREADS, stream, a); }
int launch_merge_gather(const MergeArgs &a, void *stream) {
    if (a.n <= 0 || a.stream_len <= a.header_len) return 0;
    const int64_t pieces = (a.stream_len + MERGE_PIECE - 1) / MERGE_PIECE - a.header_len / MERGE_PIECE;
    return launch(k_merge_gather, (pieces + WAVES - 1) / WAVES, stream, a);
}

}  // namespace npr
