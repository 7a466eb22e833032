// npr_huff.h -- the parts of a DEFLATE encoder (RFC 1951) that one thread runs: the code lengths of a Huffman code from sorted counts, their
// limit to 15 (7) bits, the canonical codes, and the symbols of a match's length and distance.  Plain integer code for host and device (the
// kernel: npr_deflate.hip).  Every loop is bounded by the alphabet's size.
#ifndef NPR_HUFF_H
#define NPR_HUFF_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NPR_HUFF_FN __host__ __device__ inline
#else
#define NPR_HUFF_FN inline
#endif

namespace npr {

constexpr int DEFLATE_LL = 286, DEFLATE_D = 30, DEFLATE_CL = 19;
constexpr int DEFLATE_MIN_MATCH = 3, DEFLATE_MAX_MATCH = 258, DEFLATE_WINDOW = 32768;
constexpr int HUFF_MAX_DEPTH = 32;  // a count below 2^17 in total keeps every depth below this (the Fibonacci bound: 23)

// A[0 .. n) are the counts of the used symbols in ascending order, n >= 2: on return A[i] is the code length of the i-th of them, in place
// (Moffat and Katajainen, "In-place calculation of minimum-redundancy codes", 1995): the lengths of a Huffman code.
NPR_HUFF_FN void huff_lengths(uint32_t *A, int n) {
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root], A[root++] = static_cast<uint32_t>(next);
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root], A[root++] = static_cast<uint32_t>(next);
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    int next = n - 1;
    while (avbl > 0 && dpth <= n) {
        while (root >= 0 && static_cast<int>(A[root]) == dpth) ++used, --root;
        while (avbl > used && next >= 0) A[next--] = static_cast<uint32_t>(dpth), --avbl;
        avbl = 2 * used, ++dpth, used = 0;
    }
}

// cnt[0 .. n): the used symbols (count > 0) ordered by (count, symbol) into A (counts) and S (symbols), by one thread; returns how many
NPR_HUFF_FN int huff_sort_serial(const uint32_t *cnt, int n, uint32_t *A, uint16_t *S) {
    int used = 0;
    for (int s = 0; s < n; ++s) {
        const uint32_t c = cnt[s];
        if (!c) continue;
        int r = 0;
        for (int s2 = 0; s2 < n; ++s2) {
            const uint32_t c2 = cnt[s2];
            r += (c2 && (c2 < c || (c2 == c && s2 < s))) ? 1 : 0;
        }
        A[r] = c, S[r] = static_cast<uint16_t>(s);
        ++used;
    }
    return used;
}

// The code lengths len[0 .. n) of an alphabet whose `used` symbols of count > 0 stand in S ordered by (count, symbol), their counts in A
// (overwritten).  No symbol: all zero.  One symbol: one code of one bit.  Else the lengths of a Huffman code; when one of them exceeds
// max_bits, the number of codes per length is folded to max_bits and, while the Kraft sum exceeds one, a code of the largest length below
// max_bits that has one moves a bit down and takes a max_bits code beside it (fewer steps than codes were folded): a complete prefix code
// again.  The lengths go to the symbols in S's order, the longest first, so of two symbols the rarer (then the lower) never has the shorter code.
NPR_HUFF_FN void huff_build(uint32_t *A, const uint16_t *S, int used, int n, int max_bits, uint8_t *len) {
    for (int s = 0; s < n; ++s) len[s] = 0;
    if (used == 0) return;
    if (used == 1) {
        len[S[0]] = 1;
        return;
    }
    huff_lengths(A, used);
    int per[HUFF_MAX_DEPTH + 1];
    for (int k = 0; k <= HUFF_MAX_DEPTH; ++k) per[k] = 0;
    for (int k = 0; k < used; ++k) ++per[A[k] > static_cast<uint32_t>(max_bits) ? max_bits : static_cast<int>(A[k])];
    uint32_t total = 0;
    for (int k = max_bits; k > 0; --k) total += static_cast<uint32_t>(per[k]) << (max_bits - k);
    for (int step = 0; total > (1u << max_bits) && step < n; ++step) {
        --per[max_bits];
        for (int k = max_bits - 1; k > 0; --k)
            if (per[k]) {
                --per[k], per[k + 1] += 2;
                break;
            }
        --total;
    }
    int j = used;
    for (int k = 1; k <= max_bits; ++k)
        for (int c = per[k]; c > 0 && j > 0; --c) len[S[--j]] = static_cast<uint8_t>(k);
}

// the canonical codes of RFC 1951 3.2.2 for len[0 .. n), every code with its bits reversed: DEFLATE packs a Huffman code from its most
// significant bit, everything else from the least
NPR_HUFF_FN void huff_codes(const uint8_t *len, int n, int max_bits, uint16_t *code) {
    uint32_t next[16];
    uint32_t per[16];
    for (int k = 0; k < 16; ++k) per[k] = 0, next[k] = 0;
    for (int s = 0; s < n; ++s) ++per[len[s]];
    per[0] = 0;
    uint32_t c = 0;
    for (int k = 1; k <= max_bits; ++k) c = (c + per[k - 1]) << 1, next[k] = c;
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        uint32_t v = l ? next[l]++ : 0, r = 0;
        for (int k = 0; k < l; ++k) r = r << 1 | (v & 1), v >>= 1;
        code[s] = static_cast<uint16_t>(r);
    }
}

struct DeflateSym {
    uint32_t sym, extra_bits, extra;
};
NPR_HUFF_FN DeflateSym deflate_length_sym(uint32_t len) {  // 3 .. 258
    const uint32_t l = len - 3;
    if (l < 8) return {257 + l, 0, 0};
    if (len == 258) return {285, 0, 0};
    const uint32_t eb = 31 - __builtin_clz(l) - 2;
    return {261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1u << eb) - 1)};
}
NPR_HUFF_FN DeflateSym deflate_dist_sym(uint32_t dist) {  // 1 .. 32768
    const uint32_t d = dist - 1;
    if (d < 4) return {d, 0, 0};
    const uint32_t k = 31 - __builtin_clz(d), eb = k - 1;
    return {2 * k + ((d >> eb) & 1), eb, d & ((1u << eb) - 1)};
}

// the order in which a dynamic block's header stores the code-length alphabet's lengths
NPR_HUFF_FN int deflate_cl_order(int k) {
    const uint8_t order[DEFLATE_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[k];
}

}  // namespace npr
#endif
