// npr_bamregion.hip -- a region query on an indexed BAM file (the ABI: include/nprealign.h, "region queries": npr_bam_open_region,
// npr_bam_stream_restrict; the host side: npr_bam_api.cpp; the chunks: npr_bai_chunks, npr_bam_host.cpp).  The stream is the COMPACT one: the
// payloads of the blocks the index names, inflated back to back by k_bgzf_inflate (npr_inflate.hip), a chunk of the index a span of it.
//   k_bam_chunk_walk<false>  one wavefront per chunk (its first lane: the block_size chain is a chain of dependent loads) follows the chain from
//                    the chunk's first byte until the record offset reaches the chunk's end, with the per-record checks of k_bam_walk
//                    (bam_walk_step, npr_bamrec.h: one body), and counts the records.  A record that ends past the chunk's end: WALK_CHUNK.
//                    Every load is checked against the stream's length before it happens; a step moves on by at least 37 bytes, so the loop
//                    is bounded by the chunk's length.
//   (launch_scan_tiled of npr_scan.h places the chunks' records: the table is in file order and no atomic decides a position)
//   k_bam_chunk_walk<true>   the same walk again, now writing every record's offset at its place.
//   k_bam_overlap    a thread per record: refID, then the record's interval by bamrec_interval (npr_bamrec.h; under the placeholder
//                    <l_seq>S<n>N the auxiliary fields are walked by bamrec_aux_walk, the body k_bampile_check runs) and 1 for a record that
//                    overlaps [beg, end).  Only records of the query's refID with FLAG 4 clear are looked at further than their fixed fields.
//   (the scan again)
//   k_bam_gather     the offsets of the kept records, order preserved.
// The kernels were not timed alone; whole calls: tools/bam_region_time.py (profiles/bam_region_time.json; README quotes them).
#include <hip/hip_runtime.h>

#include "npr_bamrec.h"
#include "npr_device.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;

template <bool WRITE>
__global__ void __launch_bounds__(THREADS) k_bam_chunk_walk(BamChunkArgs a) {
    if ((threadIdx.x & (WAVE - 1)) != 0) return;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + threadIdx.x / WAVE;
    if (c >= a.n_chunks) return;
    const int64_t end = a.chunk_end[c] < a.len ? a.chunk_end[c] : a.len;
    int64_t at = a.chunk_beg[c], n = 0;
    int status = WALK_OK;
    int64_t *const to = WRITE ? a.table + a.count[c] : nullptr;
    const int64_t room = WRITE ? a.count[c + 1] - a.count[c] : 0;
    while (at >= 0 && at < end) {
        int64_t next = at;
        status = bam_walk_step(a.stream, a.len, at, a.n_ref, &next);
        if (status == WALK_OK && next > end) status = WALK_CHUNK;
        if (status != WALK_OK) break;
        if (WRITE) {
            if (n >= room) break;  // (the count pass found `room` records: the stream has not changed)
            to[n] = at;
        }
        ++n, at = next;
    }
    if (!WRITE) a.count[c] = n, a.stop[c] = at, a.status[c] = status;
}

__global__ void __launch_bounds__(THREADS) k_bam_overlap(BamOverlapArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t *r = a.stream + a.rec_off[i];
    int64_t keep = 0;
    if (static_cast<int32_t>(br_ld32(r + 4)) == a.tid) {
        int64_t rb, re;
        if (!bamrec_interval(r, &rb, &re)) *a.bad = 1;
        else keep = rb < a.end && re > a.beg;
    }
    a.keep[i] = keep;
}

__global__ void __launch_bounds__(THREADS) k_bam_gather(BamOverlapArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    if (a.keep[i + 1] != a.keep[i]) a.kept[a.keep[i]] = a.rec_off[i];
}

template <typename K, typename A>
int launch(K kernel, int64_t grid, const A &a, void *stream) {
    if (grid <= 0) return 0;
    if (grid >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

int launch_bam_chunk_count(const BamChunkArgs &a, void *stream) { return launch(k_bam_chunk_walk<false>, (a.n_chunks + WAVES - 1) / WAVES, a, stream); }
int launch_bam_chunk_write(const BamChunkArgs &a, void *stream) { return launch(k_bam_chunk_walk<true>, (a.n_chunks + WAVES - 1) / WAVES, a, stream); }
int launch_bam_overlap_flags(const BamOverlapArgs &a, void *stream) { return launch(k_bam_overlap, (a.n + THREADS - 1) / THREADS, a, stream); }
int launch_bam_overlap_gather(const BamOverlapArgs &a, void *stream) { return launch(k_bam_gather, (a.n + THREADS - 1) / THREADS, a, stream); }

}  // namespace npr
