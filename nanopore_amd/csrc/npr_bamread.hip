// npr_bamread.hip -- the records of an uncompressed BAM stream (what npr_inflate.hip leaves on the device) as SAM text (the ABI:
// include/nprealign.h, npr_bam_sam; the host side: npr_bam_api.cpp; the auxiliary fields' text: npr_bam_aux_text, npr_bam_host.cpp).
//   k_bam_head     one wavefront (its first lane: the walk is a chain of dependent loads) checks "BAM\1", l_text, n_ref and every l_name / l_ref
//                  against the stream's length and returns the header's end.
//   k_bam_walk     one wavefront follows the block_size chain from there and writes record offsets into a table of fixed size; the host calls
//                  it in rounds, resuming where the last one stopped.  One dependent load a record: serial by the format.  Per record:
//                  block_size at least 33, the record inside the stream, l_read_name at least 1 with a NUL at its end, the fixed parts (32
//                  bytes, name, cigar, SEQ, QUAL) inside block_size, refID and next_refID in -1 .. n_ref - 1, pos and next_pos at most
//                  2^31 - 2 (SAM's POS and PNEXT end at 2^31 - 1; pos + 1 stays an int32 in the kernels below).
//   k_bam_measure  a thread a record: the text length of the eleven mandatory columns (the stored cigar's apart), the span of the auxiliary
//                  bytes, whether the stored cigar is the placeholder <l_seq>S<n>N.
//   k_bam_gather_aux  the auxiliary bytes of all records packed back to back: they go to the host once.
//   (the host turns them to text, finds a CG:B:I tag, makes the lines' lengths; launch_scan_tiled of npr_scan.h makes their offsets)
//   k_bam_emit     a workgroup per (record, tile of BAM_TILE bases): every tile writes its bases and qualities, tile 0 also the other columns --
//                  the cigar by all threads, 256 operations a trip, placed by a prefix sum of their digits (npr_devtext.h, block_scan_exclusive).
// THE LINE: QNAME; FLAG; RNAME, "*" for refID -1; POS + 1; MAPQ; CIGAR: "*" for no operation, else <length><MIDNSHP=X> per operation -- when the
// stored cigar is the placeholder <l_seq>S<n>N and the record has a CG:B:I tag, the tag's operations instead, and the tag is dropped from the
// line --; RNEXT: "*" for next_refID -1, "=" when it equals refID (which is then at least 0), else the name; PNEXT + 1; TLEN; SEQ through
// "=ACMGRSVTWYHKDBN", "*" for l_seq 0; QUAL + 33, "*" when l_seq is 0 or the first byte is 0xFF; then, each after a tab, the auxiliary fields
// as TAG:TYPE:VALUE (npr_bam_aux_text); "\n".  Columns are separated by one tab.
#include <hip/hip_runtime.h>

#include "npr_bamrec.h"
#include "npr_device.h"
#include "npr_devtext.h"
#include "npr_scan.h"

namespace npr {
namespace {

constexpr int THREADS = SCAN_THREADS;

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}
__device__ __forceinline__ int32_t ld32s(const uint8_t *p) { return static_cast<int32_t>(ld32(p)); }

enum { HEAD_OK = 0, HEAD_MAGIC = 1, HEAD_TEXT = 2, HEAD_REFS = 3 };

__global__ void __launch_bounds__(64) k_bam_head(const uint8_t *s, int64_t len, int64_t *out) {
    if (threadIdx.x != 0) return;
    out[0] = HEAD_MAGIC, out[1] = 0, out[2] = 0, out[3] = 0;
    if (len < 12 || s[0] != 'B' || s[1] != 'A' || s[2] != 'M' || s[3] != 1) return;
    out[0] = HEAD_TEXT;
    const int64_t l_text = ld32s(s + 4);
    if (l_text < 0 || 8 + l_text + 4 > len) return;
    out[0] = HEAD_REFS;
    int64_t at = 8 + l_text;
    const int64_t n_ref = ld32s(s + at);
    at += 4;
    if (n_ref < 0) return;
    for (int64_t k = 0; k < n_ref; ++k) {
        if (at + 4 > len) return;
        const int64_t l_name = ld32s(s + at);
        if (l_name < 1 || at + 4 + l_name + 4 > len || s[at + 4 + l_name - 1] != 0) return;
        at += 8 + l_name;
    }
    out[0] = HEAD_OK, out[1] = at, out[2] = l_text, out[3] = n_ref;
}

__global__ void __launch_bounds__(64) k_bam_walk(const uint8_t *s, int64_t len, int64_t start, int32_t n_ref, int64_t *table, int64_t cap, int64_t *out) {
    if (threadIdx.x != 0) return;
    int64_t at = start, n = 0;
    int status = WALK_OK;
    while (at < len && n < cap) {
        int64_t next = at;
        status = bam_walk_step(s, len, at, n_ref, &next);  // (npr_bamrec.h: the checks named above)
        if (status != WALK_OK) break;
        table[n++] = at;
        at = next;
    }
    out[0] = n, out[1] = at, out[2] = status;
}

// what both the measure and the emit kernel read of a record
struct Rec {
    const uint8_t *r;
    int32_t tid, pos, l_name, mapq, n_cig, flag, l_seq, ntid, npos, tlen;
    int64_t size;
    __device__ __forceinline__ void load(const uint8_t *p) {
        r = p, size = ld32s(p), tid = ld32s(p + 4), pos = ld32s(p + 8), l_name = p[12], mapq = p[13], n_cig = p[16] | p[17] << 8, flag = p[18] | p[19] << 8;
        l_seq = ld32s(p + 20), ntid = ld32s(p + 24), npos = ld32s(p + 28), tlen = ld32s(p + 32);
    }
    __device__ __forceinline__ const uint8_t *cigar() const { return r + 36 + l_name; }
    __device__ __forceinline__ const uint8_t *seq() const { return cigar() + 4 * static_cast<int64_t>(n_cig); }
    __device__ __forceinline__ const uint8_t *qual() const { return seq() + (l_seq + 1) / 2; }
    __device__ __forceinline__ const uint8_t *aux() const { return qual() + l_seq; }
    __device__ __forceinline__ bool no_qual() const { return l_seq == 0 || qual()[0] == 0xff; }
};
__device__ __forceinline__ int name_len(const BamReadArgs &a, int32_t tid) { return tid < 0 ? 1 : static_cast<int>(a.name_off[tid + 1] - a.name_off[tid]); }

__global__ void __launch_bounds__(THREADS) k_bam_measure(BamReadArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= a.n) return;
    Rec c;
    c.load(a.stream + a.rec_off[i]);
    int64_t cig = 0;
    const uint8_t *ops = c.cigar();
    for (int q = 0; q < c.n_cig; ++q) {
        const uint32_t v = ld32(ops + 4 * q);
        if ((v & 15u) > 8u) *a.bad = 1;
        cig += digits30(v >> 4) + 1;
    }
    if (c.n_cig == 0) cig = 1;
    const bool same = c.ntid >= 0 && c.ntid == c.tid;
    const int64_t fixed = (c.l_name - 1) + digits32(static_cast<uint32_t>(c.flag)) + name_len(a, c.tid) + signed_len(c.pos + 1) + digits32(static_cast<uint32_t>(c.mapq)) + cig +
                          (same ? 1 : name_len(a, c.ntid)) + signed_len(c.npos + 1) + signed_len(c.tlen) + (c.l_seq ? c.l_seq : 1) + (c.no_qual() ? 1 : c.l_seq) + 10;
    BamReadRec m;
    m.aux_off = c.aux() - a.stream, m.aux_len = static_cast<int32_t>(a.rec_off[i] + 4 + c.size - m.aux_off), m.l_seq = c.l_seq;
    m.fixed_len = static_cast<int32_t>(fixed), m.cig_len = static_cast<int32_t>(cig);
    m.placeholder = c.n_cig == 2 && ld32(ops) == (static_cast<uint32_t>(c.l_seq) << 4 | 4u) && (ld32(ops + 4) & 15u) == 3u;
    m.pad = 0;
    a.meas[i] = m;
}

__global__ void __launch_bounds__(THREADS) k_bam_gather_aux(BamReadArgs a) {
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint8_t *from = a.stream + a.meas[i].aux_off;
        uint8_t *to = a.aux_pack + a.aux_pack_off[i];
        const int64_t n = a.aux_pack_off[i + 1] - a.aux_pack_off[i];
        for (int64_t k = threadIdx.x; k < n; k += THREADS) to[k] = from[k];
    }
}

__global__ void __launch_bounds__(THREADS) k_bam_emit(BamReadArgs a) {
    __shared__ int lds[SCAN_WAVES];
    const int t = threadIdx.x;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t i = static_cast<int64_t>(a.items[item] >> 32), tile = static_cast<int64_t>(a.items[item] & 0xffffffffu);
        Rec c;
        c.load(a.stream + a.rec_off[i]);
        const BamReadRec m = a.meas[i];
        uint8_t *const line = a.out + a.line_off[i];
        const int64_t L = a.line_off[i + 1] - a.line_off[i];
        const int64_t aux_n = a.aux_text_off[i + 1] - a.aux_text_off[i], tail = (aux_n ? 1 + aux_n : 0) + 1;
        const int64_t cig_len = L - tail - (m.fixed_len - m.cig_len);   // (the host made L of these terms and the real cigar's length)
        const bool same = c.ntid >= 0 && c.ntid == c.tid;
        // where the columns begin
        const int64_t p_flag = c.l_name, p_rname = p_flag + digits32(static_cast<uint32_t>(c.flag)) + 1, p_pos = p_rname + name_len(a, c.tid) + 1;
        const int64_t p_mapq = p_pos + signed_len(c.pos + 1) + 1, p_cig = p_mapq + digits32(static_cast<uint32_t>(c.mapq)) + 1, p_rnext = p_cig + cig_len + 1;
        const int64_t p_pnext = p_rnext + (same ? 1 : name_len(a, c.ntid)) + 1, p_tlen = p_pnext + signed_len(c.npos + 1) + 1, p_seq = p_tlen + signed_len(c.tlen) + 1;
        const int64_t p_qual = p_seq + (c.l_seq ? c.l_seq : 1) + 1, p_aux = p_qual + (c.no_qual() ? 1 : c.l_seq);
        if (cig_len < 1 || p_aux + tail != L) {  // a defect: nothing is written from lengths that disagree
            if (t == 0) *a.bad = 2;
            continue;
        }
        // the tile's bases and qualities
        const int64_t lo = tile * BAM_TILE, hi = min(static_cast<int64_t>(c.l_seq), lo + BAM_TILE);
        const uint8_t *seq = c.seq(), *qual = c.qual();
        const bool with_qual = !c.no_qual();
        for (int64_t k = lo + t; k < hi; k += THREADS) {
            const uint8_t b = seq[k >> 1];
            line[p_seq + k] = "=ACMGRSVTWYHKDBN"[(k & 1) ? (b & 15) : (b >> 4)];
            if (with_qual) line[p_qual + k] = static_cast<uint8_t>(qual[k] + 33);
        }
        if (tile != 0) continue;
        // the other columns
        for (int k = t; k < c.l_name - 1; k += THREADS) line[k] = c.r[36 + k];
        if (t == 0) {
            line[c.l_name - 1] = '\t';
            put_digits(line + p_flag, static_cast<uint32_t>(c.flag), digits32(static_cast<uint32_t>(c.flag))), line[p_rname - 1] = '\t';
            if (c.tid < 0) line[p_rname] = '*';
            else for (int64_t k = a.name_off[c.tid]; k < a.name_off[c.tid + 1]; ++k) line[p_rname + k - a.name_off[c.tid]] = a.names[k];
            line[p_pos - 1] = '\t', put_signed(line + p_pos, c.pos + 1), line[p_mapq - 1] = '\t';
            put_digits(line + p_mapq, static_cast<uint32_t>(c.mapq), digits32(static_cast<uint32_t>(c.mapq))), line[p_cig - 1] = '\t';
            line[p_rnext - 1] = '\t';
            if (c.ntid < 0) line[p_rnext] = '*';
            else if (same) line[p_rnext] = '=';
            else for (int64_t k = a.name_off[c.ntid]; k < a.name_off[c.ntid + 1]; ++k) line[p_rnext + k - a.name_off[c.ntid]] = a.names[k];
            line[p_pnext - 1] = '\t', put_signed(line + p_pnext, c.npos + 1), line[p_tlen - 1] = '\t', put_signed(line + p_tlen, c.tlen), line[p_seq - 1] = '\t';
            if (c.l_seq == 0) line[p_seq] = '*';
            line[p_qual - 1] = '\t';
            if (!with_qual) line[p_qual] = '*';
            if (aux_n) line[p_aux] = '\t';
            line[L - 1] = '\n';
        }
        for (int64_t k = t; k < aux_n; k += THREADS) line[p_aux + 1 + k] = a.aux_text[a.aux_text_off[i] + k];
        // the cigar: the stored operations, or the CG tag's
        const bool folded = a.cg[2 * i] >= 0;
        const uint8_t *ops = folded ? c.aux() + a.cg[2 * i] : c.cigar();
        const int64_t n_ops = folded ? a.cg[2 * i + 1] : c.n_cig;
        if (n_ops == 0) {
            if (t == 0) line[p_cig] = '*';
            continue;
        }
        int64_t run = 0;
        for (int64_t base = 0; base < n_ops; base += THREADS) {
            const int64_t q = base + t;
            const uint32_t v = q < n_ops ? ld32(ops + 4 * q) : 0u;
            const int k = q < n_ops ? digits30(v >> 4) + 1 : 0;
            int total;
            const int ex = block_scan_exclusive<int>(k, lds, &total);
            if (k && run + ex + k <= cig_len) {
                uint8_t *p = line + p_cig + run + ex;
                put_digits(p, v >> 4, k - 1);
                p[k - 1] = "MIDNSHP=X??????"[v & 15u];
            }
            run += total;
        }
        if (run != cig_len && t == 0) *a.bad = 2;
    }
}

}  // namespace

int launch_bam_head(const uint8_t *stream, int64_t len, int64_t *out4, void *hip_stream) {
    hipLaunchKernelGGL(k_bam_head, dim3(1), dim3(64), 0, static_cast<hipStream_t>(hip_stream), stream, len, out4);
    return static_cast<int>(hipGetLastError());
}
int launch_bam_walk(const uint8_t *stream, int64_t len, int64_t start, int32_t n_ref, int64_t *table, int64_t cap, int64_t *out3, void *hip_stream) {
    hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(64), 0, static_cast<hipStream_t>(hip_stream), stream, len, start, n_ref, table, cap, out3);
    return static_cast<int>(hipGetLastError());
}
int launch_bam_read_measure(const BamReadArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k_bam_measure, dim3(static_cast<unsigned>((a.n + THREADS - 1) / THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}
int launch_bam_gather_aux(const BamReadArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k_bam_gather_aux, dim3(static_cast<unsigned>(a.n < 65536 ? a.n : 65536)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}
int launch_bam_emit(const BamReadArgs &a, void *stream) {
    if (a.n_items <= 0) return 0;
    hipLaunchKernelGGL(k_bam_emit, dim3(static_cast<unsigned>(a.n_items < (1 << 20) ? a.n_items : (1 << 20))), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
