// npr_bamrec.h -- the checks of ONE BAM record before it may be added to a pileup (include/nprealign.h, npr_pileup_add_bam): whether it is
// selected, which cigar applies, what that cigar consumes, the verdict.  Plain C++ on a byte pointer and lengths, one body for host and device
// (the kernel: k_bampile_check, npr_bampile.hip; the host program under AddressSanitizer: tests/native/bamrec_check.cpp).  No intrinsics.
// r points at the record's block_size, `avail` bytes of the stream lie from there on.  In this order:
//   the parts      block_size at least 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq with l_read_name at least 1 and l_seq at least 0,
//                  the record inside `avail`, refID below n_ref: else BR_REFUSED / BR_WHY_PARTS (k_bam_walk has refused such a file already)
//   selection      refID >= 0, (flag & flag_mask) == 0, l_seq > 0, n_cigar_op > 0: else BR_SKIP
//   the cigar      the stored operations -- unless they are exactly <l_seq>S<n>N: then the auxiliary fields are walked (types A c C s S i I f Z H B,
//                  every step checked against the record's end; a field cut by the end, an unknown type or array subtype, a Z or H without NUL, an
//                  array past the end: BR_REFUSED / BR_WHY_AUX) and the elements of the FIRST CG:B:I field are the operations, when there is one;
//                  such a field of no element: BR_SKIP
//   the sums       in 64 bits over all operations: reference bases (M D N = X), read bases (M I S = X); a code above 8: BR_REFUSED / BR_WHY_OP
//   the verdict    pos < 0: BR_WHY_POS; pos + reference bases > l_ref: BR_WHY_REF; read bases != l_seq: BR_WHY_READ; else BR_ADD
// Every read index is checked against the record's end, which lies inside `avail`, before it happens.
// Also here, for the same reason (one body wherever a record is looked at): bam_walk_step, a step of the block_size chain with the checks of
// npr_bam_sam (k_bam_walk, k_bam_chunk_walk), bamrec_interval, the reference interval of a record for a region query (k_bam_overlap), bamrec_measure,
// what a writer of sorted BAM needs of a record (k_merge_measure, npr_bammerge.hip), and bgzf_voffset_search, a virtual offset in any writer's blocks
// (the index kernels of npr_bam.hip; both under AddressSanitizer: tests/native/bammerge_check.cpp).
#ifndef NPR_BAMREC_H
#define NPR_BAMREC_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NPR_BR_FN __host__ __device__ inline
#else
#define NPR_BR_FN inline
#endif

namespace npr {

enum { BR_SKIP = 0, BR_ADD = 1, BR_REFUSED = 2 };
enum { BR_WHY_NONE = 0, BR_WHY_PARTS, BR_WHY_AUX, BR_WHY_OP, BR_WHY_POS, BR_WHY_REF, BR_WHY_READ };

struct BamRecVerdict {
    int32_t verdict, why;
    int32_t from_cg;           // the operations are a CG:B:I field's elements
    int32_t tid, pos, l_seq;
    int64_t ops_at, n_ops;     // the operations: 4-byte words from r + ops_at on (any alignment)
    int64_t seq_at;            // the packed bases from r + seq_at on
    int64_t ref_sum, read_sum;
};

NPR_BR_FN uint32_t br_ld32(const uint8_t *p) {
    return p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}
NPR_BR_FN int br_width(uint8_t t) { return (t == 'c' || t == 'C') ? 1 : ((t == 's' || t == 'S') ? 2 : ((t == 'i' || t == 'I' || t == 'f') ? 4 : 0)); }

// The auxiliary fields r[at, end): false when one is malformed.  *cg_at / *cg_n: where the elements of the first CG:B:I field lie (from r) and
// how many; -1 / 0 without one.
NPR_BR_FN bool bamrec_aux_walk(const uint8_t *r, int64_t at, int64_t end, int64_t *cg_at, int64_t *cg_n) {
    *cg_at = -1, *cg_n = 0;
    while (at < end) {
        if (end - at < 3) return false;
        const uint8_t t0 = r[at], t1 = r[at + 1], type = r[at + 2];
        at += 3;
        const int w = br_width(type);
        if (type == 'A') {
            if (end - at < 1) return false;
            at += 1;
        } else if (w) {
            if (end - at < w) return false;
            at += w;
        } else if (type == 'Z' || type == 'H') {
            while (at < end && r[at] != 0) ++at;
            if (at >= end) return false;
            at += 1;
        } else if (type == 'B') {
            if (end - at < 5) return false;
            const uint8_t sub = r[at];
            const int sw = br_width(sub);
            const int64_t count = br_ld32(r + at + 1);
            if (!sw || sw * count > end - (at + 5)) return false;
            if (*cg_at < 0 && t0 == 'C' && t1 == 'G' && sub == 'I') *cg_at = at + 5, *cg_n = count;
            at += 5 + sw * count;
        } else {
            return false;
        }
    }
    return true;
}

// One step of the block_size chain (k_bam_walk, npr_bamread.hip; k_bam_chunk_walk, npr_bamregion.hip): the record at s + at of a stream of
// len bytes, at < len.  In this order: block_size inside the stream (WALK_PAST) and at least 33 (WALK_SIZE), the record inside the stream
// (WALK_PAST), l_read_name at least 1 (WALK_NAME), l_seq at least 0 and the fixed parts inside block_size (WALK_PARTS), a NUL at the name's end
// (WALK_NAME), refID and next_refID in -1 .. n_ref - 1 (WALK_REF), pos and next_pos at most 2^31 - 2 (WALK_POS: POS / PNEXT = pos + 1 would
// not fit SAM's 2^31 - 1, nor an int32).  WALK_OK: *next = where the next record begins.  WALK_CHUNK is the chunk walk's: a chunk of an
// index that does not end on a record boundary.
enum { WALK_OK = 0, WALK_SIZE = 1, WALK_PAST = 2, WALK_NAME = 3, WALK_PARTS = 4, WALK_REF = 5, WALK_POS = 6, WALK_CHUNK = 7 };

NPR_BR_FN int bam_walk_step(const uint8_t *s, int64_t len, int64_t at, int32_t n_ref, int64_t *next) {
    if (at + 4 > len) return WALK_PAST;
    const int64_t size = static_cast<int32_t>(br_ld32(s + at));
    if (size < 33) return WALK_SIZE;
    if (at + 4 + size > len) return WALK_PAST;
    const uint8_t *r = s + at;
    const int32_t tid = static_cast<int32_t>(br_ld32(r + 4)), ntid = static_cast<int32_t>(br_ld32(r + 24));
    const int64_t l_name = r[12], n_cig = r[16] | static_cast<int64_t>(r[17]) << 8, l_seq = static_cast<int32_t>(br_ld32(r + 20));
    if (l_name < 1) return WALK_NAME;
    if (l_seq < 0 || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > size) return WALK_PARTS;
    if (r[36 + l_name - 1] != 0) return WALK_NAME;  // (inside the record: the parts fit)
    if (tid < -1 || tid >= n_ref || ntid < -1 || ntid >= n_ref) return WALK_REF;
    if (static_cast<int32_t>(br_ld32(r + 8)) > 0x7ffffffe || static_cast<int32_t>(br_ld32(r + 28)) > 0x7ffffffe) return WALK_POS;
    *next = at + 4 + size;
    return WALK_OK;
}

// The interval of a record the walk has accepted, for a region query (include/nprealign.h, "region queries"): rb = max(pos, 0), re = max(pos +
// the reference bases of its cigar, rb + 1), re = rb + 1 with FLAG 4 or without a cigar; under the placeholder <l_seq>S<n>N the operations of
// the first CG:B:I field, when there is one.  r points at block_size; the record lies inside the stream and its parts inside block_size
// (bam_walk_step).  false: malformed auxiliary fields under a placeholder cigar (the interval is then [rb, rb + 1)).
NPR_BR_FN bool bamrec_ref_bases(const uint8_t *r, int64_t *ref_sum, bool *op_above_8);
NPR_BR_FN bool bamrec_interval(const uint8_t *r, int64_t *rb, int64_t *re) {
    const int64_t pos = static_cast<int32_t>(br_ld32(r + 8)), n_cig = r[16] | static_cast<int64_t>(r[17]) << 8;
    const int32_t flag = r[18] | r[19] << 8;
    *rb = pos > 0 ? pos : 0, *re = *rb + 1;
    if ((flag & 4) != 0 || n_cig == 0) return true;
    int64_t ref_sum = 0;
    bool other = false;
    if (!bamrec_ref_bases(r, &ref_sum, &other)) return false;
    if (pos + ref_sum > *re) *re = pos + ref_sum;
    return true;
}

// THE cigar walk of a record the block_size chain has accepted: the reference bases (M D N = X) of the operations that apply -- the stored
// ones, or, under the placeholder <l_seq>S<n>N, those of the first CG:B:I field when there is one -- and whether one of them has a code
// above 8.  false: malformed auxiliary fields under a placeholder cigar (the sums are then the stored operations').
NPR_BR_FN bool bamrec_ref_bases(const uint8_t *r, int64_t *ref_sum, bool *op_above_8) {
    const int64_t size = static_cast<int32_t>(br_ld32(r));
    const int64_t l_name = r[12], n_cig = r[16] | static_cast<int64_t>(r[17]) << 8, l_seq = static_cast<int32_t>(br_ld32(r + 20));
    const int64_t end = 4 + size, cigar_at = 36 + l_name, aux_at = cigar_at + 4 * n_cig + (l_seq + 1) / 2 + l_seq;
    int64_t ops_at = cigar_at, n_ops = n_cig;
    bool fine = true;
    if (n_cig == 2 && br_ld32(r + cigar_at) == (static_cast<uint32_t>(l_seq) << 4 | 4u) && (br_ld32(r + cigar_at + 4) & 15u) == 3u) {
        int64_t cg_at, cg_n;
        fine = bamrec_aux_walk(r, aux_at, end, &cg_at, &cg_n);
        if (fine && cg_at >= 0) ops_at = cg_at, n_ops = cg_n;
    }
    int64_t sum = 0;
    bool other = false;
    for (int64_t q = 0; q < n_ops; ++q) {  // (the stored words lie inside the parts, a CG field's inside the record: bamrec_aux_walk)
        const uint32_t w = br_ld32(r + ops_at + 4 * q), op = w & 15u;
        other |= op > 8u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) sum += w >> 4;
    }
    *ref_sum = sum, *op_above_8 = other;
    return fine;
}

// What a writer of sorted BAM needs of a record the walk has accepted (include/nprealign.h, "BAM streams to BAM files", MEASURE): the sort
// key's parts, the record's bytes with block_size, end = pos + the reference bases of its cigar (pos + 1 without any, or with FLAG 4), its
// bin = reg2bin(max(pos, 0), max(end, max(pos, 0) + 1)) (4680 for refID -1), and why it is refused: BR_WHY_OP for an operation above 8,
// BR_WHY_AUX for malformed auxiliary fields under a placeholder cigar on a record with refID >= 0 and FLAG 4 clear, else BR_WHY_NONE.
struct BamRecMeasure {
    int32_t tid, pos, flag, refused;
    int64_t size, end;
    uint32_t bin;
};
NPR_BR_FN uint32_t bamrec_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return static_cast<uint32_t>(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return static_cast<uint32_t>(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return static_cast<uint32_t>(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return static_cast<uint32_t>(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return static_cast<uint32_t>(1 + (beg >> 26));
    return 0;
}
NPR_BR_FN void bamrec_measure(const uint8_t *r, BamRecMeasure &m) {
    m.tid = static_cast<int32_t>(br_ld32(r + 4)), m.pos = static_cast<int32_t>(br_ld32(r + 8)), m.flag = r[18] | r[19] << 8;
    m.size = 4 + static_cast<int64_t>(static_cast<int32_t>(br_ld32(r)));
    int64_t ref_sum = 0;
    bool other = false;
    const bool fine = bamrec_ref_bases(r, &ref_sum, &other);
    m.refused = other ? BR_WHY_OP : ((!fine && m.tid >= 0 && (m.flag & 4) == 0) ? BR_WHY_AUX : BR_WHY_NONE);
    m.end = static_cast<int64_t>(m.pos) + ((ref_sum == 0 || (m.flag & 4) != 0) ? 1 : ref_sum);
    const int64_t beg = m.pos > 0 ? m.pos : 0;
    m.bin = m.tid < 0 ? 4680u : bamrec_reg2bin(beg, m.end < beg + 1 ? beg + 1 : m.end);
}

// The virtual offset of byte u of a stream of `blocks` BGZF blocks (npr_bgzf_scan's tables: block b holds the stream bytes [stream_off[b],
// stream_off[b + 1]) and begins at file byte block_off[b]; entry `blocks` is the stream's length and the end-of-file block's offset): the
// LAST block whose first byte is at or before u -- a block of ISIZE 0 holds no byte and is passed over -- and u's place in it.  u == the
// stream's length lies one past the payload of a short last block, and at the end-of-file block after a full one (65 280 bytes).
NPR_BR_FN unsigned long long bgzf_voffset_search(const int64_t *stream_off, const int64_t *block_off, int64_t blocks, int64_t u) {
    if (blocks <= 0) return 0;
    if (u >= stream_off[blocks]) {
        const int64_t ln = stream_off[blocks] - stream_off[blocks - 1];
        return ln < 65280 ? static_cast<unsigned long long>(block_off[blocks - 1]) << 16 | static_cast<unsigned long long>(ln)
                          : static_cast<unsigned long long>(block_off[blocks]) << 16;
    }
    int64_t lo = 0, hi = blocks;  // the first block that begins after u lies in (lo, hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (stream_off[mid] <= u) lo = mid;
        else hi = mid;
    }
    return static_cast<unsigned long long>(block_off[lo]) << 16 | static_cast<unsigned long long>(u - stream_off[lo]);
}

NPR_BR_FN void bamrec_check(const uint8_t *r, int64_t avail, const int64_t *ref_len, int64_t n_ref, int32_t flag_mask, BamRecVerdict &v) {
    v.verdict = BR_REFUSED, v.why = BR_WHY_PARTS, v.from_cg = 0, v.tid = -1, v.pos = 0, v.l_seq = 0;
    v.ops_at = 0, v.n_ops = 0, v.seq_at = 0, v.ref_sum = 0, v.read_sum = 0;
    if (avail < 36) return;
    const int64_t size = static_cast<int32_t>(br_ld32(r));
    const int64_t l_name = r[12], n_cig = r[16] | static_cast<int64_t>(r[17]) << 8, l_seq = static_cast<int32_t>(br_ld32(r + 20));
    const int32_t tid = static_cast<int32_t>(br_ld32(r + 4)), pos = static_cast<int32_t>(br_ld32(r + 8)), flag = r[18] | r[19] << 8;
    if (size < 32 || 4 + size > avail || l_name < 1 || l_seq < 0 || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > size || tid >= n_ref) return;
    const int64_t end = 4 + size, cigar_at = 36 + l_name, seq_at = cigar_at + 4 * n_cig, aux_at = seq_at + (l_seq + 1) / 2 + l_seq;
    v.tid = tid, v.pos = pos, v.l_seq = static_cast<int32_t>(l_seq), v.seq_at = seq_at;
    v.verdict = BR_SKIP, v.why = BR_WHY_NONE;
    if (tid < 0 || (flag & flag_mask) != 0 || l_seq <= 0 || n_cig == 0) return;
    v.ops_at = cigar_at, v.n_ops = n_cig;
    if (n_cig == 2 && br_ld32(r + cigar_at) == (static_cast<uint32_t>(l_seq) << 4 | 4u) && (br_ld32(r + cigar_at + 4) & 15u) == 3u) {
        int64_t cg_at, cg_n;
        if (!bamrec_aux_walk(r, aux_at, end, &cg_at, &cg_n)) {
            v.verdict = BR_REFUSED, v.why = BR_WHY_AUX;
            return;
        }
        if (cg_at >= 0) {
            v.from_cg = 1, v.ops_at = cg_at, v.n_ops = cg_n;
            if (cg_n == 0) return;
        }
    }
    int64_t ref_sum = 0, read_sum = 0;
    bool other = false;
    for (int64_t q = 0; q < v.n_ops; ++q) {
        const uint32_t w = br_ld32(r + v.ops_at + 4 * q), op = w & 15u;
        const int64_t len = w >> 4;
        other |= op > 8u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ref_sum += len;
        if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) read_sum += len;
    }
    v.ref_sum = ref_sum, v.read_sum = read_sum;
    v.verdict = BR_REFUSED;
    if (other) v.why = BR_WHY_OP;
    else if (pos < 0) v.why = BR_WHY_POS;
    else if (pos + ref_sum > ref_len[tid]) v.why = BR_WHY_REF;
    else if (read_sum != l_seq) v.why = BR_WHY_READ;
    else v.verdict = BR_ADD;
}

}  // namespace npr
#endif
