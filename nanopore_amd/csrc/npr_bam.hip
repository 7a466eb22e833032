// npr_bam.hip -- SAM records to a coordinate-sorted BAM image and the tables of its BAI index, on the device (the definitions:
// include/nprealign.h, "coordinate-sorted BAM"; the host side of the entry points: npr_bam_api.cpp).  Integers only: every output is exact
// and the same from run to run.
//   the sort     k_sort_keys, then per 8-bit pass k_sort_hist (digit counts of every workgroup, digit-major), launch_scan_tiled over them,
//                k_sort_scatter.  The scatter is STABLE by construction: a workgroup walks its tile in rounds of 256 consecutive keys; in a
//                round a key's place is (keys of its digit in earlier rounds) + (in earlier wavefronts of the round) + (in lower lanes of
//                its wavefront).  The last comes from eight ballots (v_mbcnt over the lanes whose digit agrees in every bit), the middle
//                from counts the lowest such lane of every wavefront stores, the first from a running table: no rank depends on the order
//                in which an atomic lands.  (The histogram counts with LDS atomics: a count does not depend on their order.)
//   the frame    k_bgzf_frame, one workgroup per block of 65 280 = 256 x 255 payload bytes: the header, the payload copied, and its CRC-32
//                (below), ISIZE; one more workgroup writes the end-of-file block.
//   the records  k_bam_measure (one thread a record: the cigar's operations, reference bases, bin, size), k_bam_gather_sizes + the scan +
//                k_bam_place (offsets in output order), k_bam_cigar (one thread a record) and k_bam_encode (one workgroup per (record, tile
//                of NPR_BAM_TILE bases); tile 0 also writes the fixed fields, the name and the tags).
//   the index    k_bam_index_heads (run heads, linear windows by atomicMin, per-reference counts), the scan, k_bam_index_runs,
//                the sort again over (tid, bin), k_bam_gather_runs.
// CRC-32 (zlib's: polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF).  With R(M, s) the register after the bytes M
// from state s, R(A || B, s) = R(B, 0) ^ R(A, s) * x^(8 |B|) modulo the polynomial (the register is linear in its state).  Thread t
// takes the slice [255 t, 255 t + 255) of the payload with the byte table in LDS (thread 0 from state 0xFFFFFFFF, the others from 0); a
// tree of eight levels combines neighbours (crc, bytes): level k multiplies the left crc by x^(8 * bytes of the right half), which is the
// constant x^(8 * 255 * 2^k) when the right half is full and comes from square-and-multiply over x^(2^j) otherwise (the short last
// block).  LDS: 1 KiB table + 256 x 8 bytes of tree = 3 KiB a workgroup.
#include <hip/hip_runtime.h>

#include "npr_bamrec.h"
#include "npr_bgzf.h"
#include "npr_device.h"

namespace npr {
namespace {

constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;

// ------------------------------------------------------------------ the sort
__global__ void __launch_bounds__(THREADS) k_sort_keys(int64_t n, const int32_t *tid, const int64_t *pos, const int32_t *flag, int32_t no_tid,
                                                       unsigned long long *keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long t = static_cast<unsigned long long>(tid[i] < 0 ? no_tid : tid[i]);
    keys[i] = t << 33 | static_cast<unsigned long long>(pos[i] + 1) << 1 | static_cast<unsigned long long>((flag[i] >> 4) & 1);
}

__global__ void __launch_bounds__(THREADS) k_sort_hist(BamSortArgs a) {
    __shared__ uint32_t cnt[BAM_SORT_DIGITS];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = static_cast<int64_t>(blockIdx.x) * BAM_SORT_TILE;
    for (int r = 0; r < BAM_SORT_ROUNDS; ++r) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        if (i < a.n) atomicAdd(&cnt[(a.keys_in[i] >> a.shift) & (BAM_SORT_DIGITS - 1)], 1u);
    }
    __syncthreads();
    a.hist[static_cast<int64_t>(threadIdx.x) * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(THREADS) k_sort_scatter(BamSortArgs a) {
    __shared__ uint32_t run[BAM_SORT_DIGITS];          // where the next key of a digit goes
    __shared__ uint32_t wcnt[WAVES][BAM_SORT_DIGITS];  // keys of a digit per wavefront of the round
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    run[threadIdx.x] = a.hist[static_cast<int64_t>(threadIdx.x) * gridDim.x + blockIdx.x];
    for (int w = 0; w < WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = static_cast<int64_t>(blockIdx.x) * BAM_SORT_TILE;
    for (int r = 0; r < BAM_SORT_ROUNDS; ++r) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        const bool have = i < a.n;
        const unsigned long long key = have ? a.keys_in[i] : 0;
        const uint32_t d = static_cast<uint32_t>(key >> a.shift) & (BAM_SORT_DIGITS - 1);
        // the lanes of this wavefront that hold a key of the same digit
        unsigned long long peers = __ballot(have);
#pragma unroll
        for (int b = 0; b < BAM_SORT_BITS; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? m : ~m;
        }
        const uint32_t below = __popcll(peers & ((1ull << lane) - 1));
        if (have && below == 0) wcnt[wv][d] = __popcll(peers);
        __syncthreads();
        if (have) {
            uint32_t at = run[d] + below;
            for (int w = 0; w < wv; ++w) at += wcnt[w][d];
            a.keys_out[at] = key;
            a.vals_out[at] = a.vals_in ? a.vals_in[i] : static_cast<uint32_t>(i);
        }
        __syncthreads();
        {
            uint32_t s = 0;
            for (int w = 0; w < WAVES; ++w) s += wcnt[w][threadIdx.x], wcnt[w][threadIdx.x] = 0;
            run[threadIdx.x] += s;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ BGZF
__global__ void __launch_bounds__(THREADS) k_bgzf_frame(BgzfArgs a) {
    __shared__ uint32_t table[256];
    __shared__ uint32_t t_crc[THREADS], t_len[THREADS];
    const int64_t blocks = (a.len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    const int64_t b = blockIdx.x;
    uint8_t *const out = a.out + b * (BGZF_PAYLOAD + BGZF_OVERHEAD);
    if (b >= blocks) {  // the end-of-file block, behind the last block (which may be short)
        bgzf_put_eof(a.out + a.len + blocks * BGZF_OVERHEAD, threadIdx.x);
        return;
    }
    const uint8_t *const in = a.data + b * BGZF_PAYLOAD;
    const uint32_t L = static_cast<uint32_t>(a.len - b * BGZF_PAYLOAD < BGZF_PAYLOAD ? a.len - b * BGZF_PAYLOAD : BGZF_PAYLOAD);
    if (threadIdx.x == 0) {
        bgzf_put_header(out, L + BGZF_OVERHEAD);
        out[18] = 1;
        put16(out + 19, L), put16(out + 21, ~L & 0xffffu);
    }
    for (uint32_t k = threadIdx.x; k < L; k += THREADS) out[23 + k] = in[k];
    const uint32_t crc = bgzf_crc(in, L, a, table, t_crc, t_len);
    if (threadIdx.x == 0) put32(out + 23 + L, crc), put32(out + 27 + L, L);
}

// ------------------------------------------------------------------ the records
__device__ __forceinline__ int cigar_op(uint8_t c) {
    switch (c) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return -1;
    }
}

// the cigar text [p, e): its operations counted (and, WRITE, stored as words at `out`, byte by byte: a record starts anywhere), the
// reference bases it consumes; false: malformed
template <bool WRITE>
__device__ bool walk_cigar(const uint8_t *p, const uint8_t *e, uint32_t *n_ops, uint32_t *consumed, uint8_t *out) {
    uint32_t ops = 0;
    unsigned long long ref = 0;
    if (e - p == 1 && *p == '*') {
        *n_ops = 0, *consumed = 0;
        return true;
    }
    if (p >= e) return false;
    while (p < e) {
        uint32_t v = 0;
        int digits = 0;
        while (p < e && *p >= '0' && *p <= '9' && digits < 10) v = v * 10 + (*p - '0'), ++p, ++digits;
        if (digits == 0 || digits > 9 || p >= e || v >= (1u << 28)) return false;
        const int op = cigar_op(*p++);
        if (op < 0) return false;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref += v;
        if (WRITE) put32(out + 4 * static_cast<int64_t>(ops), v << 4 | static_cast<uint32_t>(op));
        ++ops;
    }
    if (ref >= (1ull << 30)) return false;
    *n_ops = ops, *consumed = static_cast<uint32_t>(ref);
    return true;
}

__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return static_cast<uint32_t>(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return static_cast<uint32_t>(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return static_cast<uint32_t>(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return static_cast<uint32_t>(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return static_cast<uint32_t>(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

__global__ void __launch_bounds__(THREADS) k_bam_measure(BamArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    const BamRec r = a.recs[i];
    BamMeasure m{};
    if (!walk_cigar<false>(a.text + r.cigar_lo, a.text + r.cigar_hi, &m.n_ops, &m.consumed, nullptr) || m.consumed >= (1u << 30)) {
        *a.bad = 1;
        m.n_ops = m.consumed = 0;
    }
    const int64_t beg = r.pos < 0 ? 0 : r.pos;
    const int64_t end = (m.consumed == 0 || (r.flag & 4)) ? static_cast<int64_t>(r.pos) + 1 : static_cast<int64_t>(r.pos) + m.consumed;
    m.end = static_cast<int32_t>(end);
    m.bin = r.tid < 0 ? 4680u : reg2bin(beg, end < beg + 1 ? beg + 1 : end);
    const bool big = m.n_ops > 65535u;
    m.size = 36 + r.l_name + 1 + 4 * static_cast<int64_t>(big ? 2 : m.n_ops) + (r.l_seq + 1) / 2 + r.l_seq + r.tag_len +
             (big ? 8 + 4 * static_cast<int64_t>(m.n_ops) : 0);
    a.meas[i] = m;
}

__global__ void __launch_bounds__(THREADS) k_bam_gather_sizes(BamArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (j < a.n) a.size_sorted[j] = a.meas[a.order ? a.order[j] : j].size;
}
__global__ void __launch_bounds__(THREADS) k_bam_place(BamArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (j < a.n) a.rec_off[a.order ? a.order[j] : j] = a.header_len + a.size_sorted[j];
}

__global__ void __launch_bounds__(WAVE) k_bam_cigar(BamArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * WAVE + threadIdx.x;
    if (i >= a.n) return;
    const BamRec r = a.recs[i];
    const BamMeasure m = a.meas[i];
    uint8_t *const rec = a.raw + a.rec_off[i];
    uint8_t *const cig = rec + 36 + r.l_name + 1;
    uint32_t n_ops, consumed;
    if (m.n_ops <= 65535u) {
        (void)walk_cigar<true>(a.text + r.cigar_lo, a.text + r.cigar_hi, &n_ops, &consumed, cig);
        return;
    }
    put32(cig, static_cast<uint32_t>(r.l_seq) << 4 | 4u), put32(cig + 4, m.consumed << 4 | 3u);
    uint8_t *const cg = cig + 8 + (r.l_seq + 1) / 2 + r.l_seq + r.tag_len;
    cg[0] = 'C', cg[1] = 'G', cg[2] = 'B', cg[3] = 'I';
    put32(cg + 4, m.n_ops);
    (void)walk_cigar<true>(a.text + r.cigar_lo, a.text + r.cigar_hi, &n_ops, &consumed, cg + 8);
}

__device__ __forceinline__ uint32_t base_code(uint8_t c) {
    switch (c & 0xdf) {  // letters in either case; '=' is looked at before
        case 'A': return 1;
        case 'C': return 2;
        case 'M': return 3;
        case 'G': return 4;
        case 'R': return 5;
        case 'S': return 6;
        case 'V': return 7;
        case 'T': return 8;
        case 'W': return 9;
        case 'Y': return 10;
        case 'H': return 11;
        case 'K': return 12;
        case 'D': return 13;
        case 'B': return 14;
        default: return 15;
    }
}
__device__ __forceinline__ uint32_t nibble(uint8_t c) {
    if (c == '=') return 0;
    return ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) ? base_code(c) : 15u;
}

__global__ void __launch_bounds__(THREADS) k_bam_encode(BamArgs a) {
    const unsigned long long item = a.items[blockIdx.x];
    const int64_t i = static_cast<int64_t>(item >> 32);
    const int64_t tile = static_cast<int64_t>(item & 0xffffffffu);
    const BamRec r = a.recs[i];
    const BamMeasure m = a.meas[i];
    uint8_t *const rec = a.raw + a.rec_off[i];
    const int64_t n_cig = m.n_ops > 65535u ? 2 : m.n_ops;
    uint8_t *const seq = rec + 36 + r.l_name + 1 + 4 * n_cig;
    uint8_t *const qual = seq + (r.l_seq + 1) / 2;
    if (tile == 0) {
        if (threadIdx.x == 0) {
            put32(rec, static_cast<uint32_t>(m.size - 4));
            put32(rec + 4, static_cast<uint32_t>(r.tid)), put32(rec + 8, static_cast<uint32_t>(r.pos));
            rec[12] = static_cast<uint8_t>(r.l_name + 1), rec[13] = static_cast<uint8_t>(r.mapq);
            put16(rec + 14, m.bin), put16(rec + 16, static_cast<uint32_t>(n_cig)), put16(rec + 18, static_cast<uint32_t>(r.flag));
            put32(rec + 20, static_cast<uint32_t>(r.l_seq)), put32(rec + 24, static_cast<uint32_t>(r.next_tid));
            put32(rec + 28, static_cast<uint32_t>(r.next_pos)), put32(rec + 32, static_cast<uint32_t>(r.tlen));
        }
        for (int k = threadIdx.x; k <= r.l_name; k += THREADS) rec[36 + k] = k < r.l_name ? a.text[r.name + k] : 0;
        uint8_t *const tag = qual + r.l_seq;
        for (int k = threadIdx.x; k < r.tag_len; k += THREADS) tag[k] = a.tags[r.tag_off + k];
    }
    const int64_t b0 = tile * BAM_TILE, b1 = min(static_cast<int64_t>(r.l_seq), b0 + BAM_TILE);
    const uint8_t *const s = a.text + r.seq;
    for (int64_t k = b0 / 2 + threadIdx.x; 2 * k < b1; k += THREADS) {
        const uint32_t hi = nibble(s[2 * k]), lo = 2 * k + 1 < r.l_seq ? nibble(s[2 * k + 1]) : 0u;
        seq[k] = static_cast<uint8_t>(hi << 4 | lo);
    }
    if (r.qual < 0) {
        for (int64_t k = b0 + threadIdx.x; k < b1; k += THREADS) qual[k] = 0xff;
    } else {
        const uint8_t *const q = a.text + r.qual;
        for (int64_t k = b0 + threadIdx.x; k < b1; k += THREADS) qual[k] = static_cast<uint8_t>(q[k] - 33);
    }
}

// ------------------------------------------------------------------ the index
// the virtual offset of stream byte u: in blocks of BGZF_PAYLOAD bytes the file offset of its block from the table of a compressed file, in
// closed form without one; in the blocks of any writer (a.stream_off) by a search in the scan's tables (bgzf_voffset_search, npr_bamrec.h)
__device__ __forceinline__ unsigned long long voffset(const BamArgs &a, int64_t u) {
    if (a.stream_off) return bgzf_voffset_search(a.stream_off, a.block_off, a.n_blocks, u);
    const int64_t at = a.block_off ? a.block_off[u / BGZF_PAYLOAD] : u / BGZF_PAYLOAD * (BGZF_PAYLOAD + BGZF_OVERHEAD);
    return static_cast<unsigned long long>(at) << 16 | static_cast<unsigned long long>(u % BGZF_PAYLOAD);
}

// size_sorted holds the scan: place j's record is the stream bytes [header_len + size_sorted[j], header_len + size_sorted[j + 1]); without
// an order the records lie in their places (npr_bam_index)
__global__ void __launch_bounds__(THREADS) k_bam_index_heads(BamArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (j >= a.n) return;
    const int64_t i = a.order ? a.order[j] : j;
    const BamRec r = a.recs[i];
    const BamMeasure m = a.meas[i];
    bool head = j == 0;
    if (!head) {
        const int64_t ip = a.order ? a.order[j - 1] : j - 1;
        head = a.recs[ip].tid != r.tid || a.meas[ip].bin != m.bin;
    }
    a.head[j] = head;
    if (r.tid < 0) {
        atomicAdd(a.no_coor, 1ull);
        return;
    }
    const unsigned long long v0 = voffset(a, a.header_len + a.size_sorted[j]), v1 = voffset(a, a.header_len + a.size_sorted[j + 1]);
    unsigned long long *const mt = a.meta + 4 * static_cast<int64_t>(r.tid);
    atomicMin(mt, v0), atomicMax(mt + 1, v1), atomicAdd(mt + ((r.flag & 4) ? 3 : 2), 1ull);
    const int64_t w_first = a.lin_off[r.tid], windows = a.lin_off[r.tid + 1] - w_first;
    const int64_t beg = r.pos < 0 ? 0 : r.pos, end = m.end < beg + 1 ? beg + 1 : m.end;
    const int64_t w1 = min((end - 1) >> 14, windows - 1);
    for (int64_t w = min(beg >> 14, windows - 1); w <= w1; ++w) atomicMin(a.linear + w_first + w, v0);
}

// head holds the scan: run number of place j
__global__ void __launch_bounds__(THREADS) k_bam_index_runs(BamArgs a) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (j >= a.n) return;
    const int32_t *const run = reinterpret_cast<const int32_t *>(a.head);
    const int32_t q = run[j];
    if (run[j + 1] == q) return;  // no head
    const int64_t i = a.order ? a.order[j] : j;
    const unsigned long long t = a.recs[i].tid < 0 ? static_cast<unsigned long long>(a.n_refs) : static_cast<unsigned long long>(a.recs[i].tid);
    const unsigned long long v0 = voffset(a, a.header_len + a.size_sorted[j]);
    a.run_key[q] = t << 16 | a.meas[i].bin;
    a.run_beg[q] = v0;
    if (q > 0) a.run_end[q - 1] = v0;
    if (q == run[a.n] - 1) a.run_end[q] = voffset(a, a.header_len + a.size_sorted[a.n]);
}

__global__ void __launch_bounds__(THREADS) k_bam_gather_runs(BamGatherArgs a) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (q >= a.n_runs) return;
    const uint32_t from = a.perm[q];
    const unsigned long long key = a.key[from];
    const int32_t t = static_cast<int32_t>(key >> 16);
    a.run_tid[q] = t == a.no_tid ? -1 : t;
    a.run_bin[q] = static_cast<uint32_t>(key & 0xffffu);
    a.out_beg[q] = a.beg[from], a.out_end[q] = a.end[from];
}

inline unsigned grid_of(int64_t n, int threads) { return static_cast<unsigned>((n + threads - 1) / threads); }

}  // namespace

int launch_bam_sort_keys(int64_t n, const int32_t *tid, const int64_t *pos, const int32_t *flag, int32_t no_tid, unsigned long long *keys, void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_sort_keys, dim3(grid_of(n, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), n, tid, pos, flag, no_tid, keys);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_sort_pass(const BamSortArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = bam_sort_blocks(a.n);
    hipLaunchKernelGGL(k_sort_hist, dim3(static_cast<unsigned>(blocks)), dim3(THREADS), 0, st, a);
    const int rc = launch_scan_tiled<uint32_t, int32_t>(a.hist, reinterpret_cast<int32_t *>(a.hist), BAM_SORT_DIGITS * blocks, a.tile, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sort_scatter, dim3(static_cast<unsigned>(blocks)), dim3(THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_bgzf_frame(const BgzfArgs &a, void *stream) {
    const int64_t blocks = (a.len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    hipLaunchKernelGGL(k_bgzf_frame, dim3(static_cast<unsigned>(blocks + 1)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_measure(const BamArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k_bam_measure, dim3(grid_of(a.n, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_offsets(const BamArgs &a, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.n > 0) hipLaunchKernelGGL(k_bam_gather_sizes, dim3(grid_of(a.n, THREADS)), dim3(THREADS), 0, st, a);
    const int rc = launch_scan_tiled<int64_t, int64_t>(a.size_sorted, a.size_sorted, a.n, a.tile, stream);
    if (rc) return rc;
    if (a.n > 0) hipLaunchKernelGGL(k_bam_place, dim3(grid_of(a.n, THREADS)), dim3(THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_encode(const BamArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_bam_cigar, dim3(grid_of(a.n, WAVE)), dim3(WAVE), 0, st, a);
    hipLaunchKernelGGL(k_bam_encode, dim3(static_cast<unsigned>(a.n_items)), dim3(THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_index_heads(const BamArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k_bam_index_heads, dim3(grid_of(a.n, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launch_scan_tiled<uint32_t, int32_t>(a.head, reinterpret_cast<int32_t *>(a.head), a.n, a.head_tile, stream);
}

int launch_bam_index_runs(const BamArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k_bam_index_runs, dim3(grid_of(a.n, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_bam_gather_runs(const BamGatherArgs &a, void *stream) {
    if (a.n_runs <= 0) return 0;
    hipLaunchKernelGGL(k_bam_gather_runs, dim3(grid_of(a.n_runs, THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
