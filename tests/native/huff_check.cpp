// huff_check.cpp -- csrc/npr_huff.h on the host (tests/test_huff_host.py builds this with AddressSanitizer and UBSan and runs it): the code
// lengths against a Huffman tree built with a priority queue, the 15- and 7-bit limits on counts that need them (Fibonacci numbers), the
// canonical codes as a prefix code, and the length and distance symbols against the tables of RFC 1951 3.2.5.
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <vector>

#include "npr_huff.h"

using namespace npr;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("huff_check: line %d: %s\n", __LINE__, #c);      \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// the cost and the largest depth of a Huffman tree over the counts above zero
static void reference(const std::vector<uint32_t> &cnt, unsigned long long *cost, int *depth) {
    struct Node {
        unsigned long long w;
        int depth;
    };
    auto cmp = [](const Node &a, const Node &b) { return a.w > b.w || (a.w == b.w && a.depth > b.depth); };
    std::priority_queue<Node, std::vector<Node>, decltype(cmp)> q(cmp);
    for (uint32_t c : cnt)
        if (c) q.push({c, 0});
    *cost = 0, *depth = 0;
    while (q.size() > 1) {
        Node a = q.top();
        q.pop();
        Node b = q.top();
        q.pop();
        *cost += a.w + b.w;
        q.push({a.w + b.w, (a.depth > b.depth ? a.depth : b.depth) + 1});
    }
    if (!q.empty()) *depth = q.top().depth;
}

// builds the code of cnt as the kernel does; returns true when no length had to be limited
static bool build_and_check(const std::vector<uint32_t> &cnt, int max_bits) {
    const int n = static_cast<int>(cnt.size());
    std::vector<uint32_t> A(n + 2);
    std::vector<uint16_t> S(n + 2), code(n);
    std::vector<uint8_t> len(n, 0xee);
    const int used = huff_sort_serial(cnt.data(), n, A.data(), S.data());
    for (int k = 1; k < used; ++k) CHECK(A[k - 1] < A[k] || (A[k - 1] == A[k] && S[k - 1] < S[k]));
    huff_build(A.data(), S.data(), used, n, max_bits, len.data());
    unsigned long long kraft = 0, cost = 0, want = 0;
    int depth = 0;
    for (int s = 0; s < n; ++s) {
        CHECK((len[s] == 0) == (cnt[s] == 0) && len[s] <= max_bits);
        if (len[s]) kraft += 1ull << (max_bits - len[s]);
        cost += static_cast<unsigned long long>(cnt[s]) * len[s];
        for (int s2 = 0; s2 < n; ++s2)   // the rarer of two symbols (then the lower) never has the shorter code
            if (cnt[s] && cnt[s2] && (cnt[s] < cnt[s2] || (cnt[s] == cnt[s2] && s < s2))) CHECK(len[s] >= len[s2]);
    }
    if (used == 0) CHECK(kraft == 0);
    if (used == 1) CHECK(kraft == 1ull << (max_bits - 1));
    if (used >= 2) CHECK(kraft == 1ull << max_bits);   // a complete prefix code
    reference(cnt, &want, &depth);
    if (used >= 2 && depth <= max_bits) CHECK(cost == want);   // optimal whenever nothing needs limiting
    if (used >= 2) CHECK(cost >= want);
    // the canonical codes: no code is the beginning of another (the codes are stored with their bits reversed)
    huff_codes(len.data(), n, max_bits, code.data());
    for (int s = 0; s < n; ++s)
        for (int s2 = 0; s2 < n; ++s2)
            if (s != s2 && len[s] && len[s2] && len[s] <= len[s2]) CHECK((code[s2] & ((1u << len[s]) - 1)) != code[s]);
    return depth <= max_bits;
}

int main() {
    // Fibonacci counts make the deepest tree: 30 of them reach depth 29, 19 of them depth 18
    int limited = 0;
    for (int max_bits : {15, 7}) {
        for (int n = 2; n <= (max_bits == 15 ? 24 : 19); ++n) {   // (the counts of one block sum to at most 65 281: fib(24) = 46 368)
            std::vector<uint32_t> fib(max_bits == 15 ? DEFLATE_LL : DEFLATE_CL, 0);
            uint32_t a = 1, b = 1;
            for (int k = 0; k < n; ++k) {
                fib[(k * 7) % fib.size()] = a;
                const uint32_t c = a + b;
                a = b, b = c;
            }
            limited += build_and_check(fib, max_bits) ? 0 : 1;
        }
    }
    CHECK(limited >= 15);
    std::mt19937 rng(5);
    for (int trial = 0; trial < 4000; ++trial) {
        const int max_bits = trial & 1 ? 15 : 7;
        std::vector<uint32_t> cnt(trial & 1 ? (trial & 2 ? DEFLATE_LL : DEFLATE_D) : DEFLATE_CL, 0);
        const int used = rng() % (cnt.size() + 1), shape = rng() % 4;
        for (int k = 0; k < used; ++k) {
            const uint32_t r = rng();
            cnt[rng() % cnt.size()] = shape == 0 ? 1 + r % 3 : shape == 1 ? 1 + r % 200 : shape == 2 ? 1u << (r % 16) : 1 + (r % 65000) / (1 + (r >> 20) % 4000);
        }
        limited += build_and_check(cnt, max_bits) ? 0 : 1;
    }
    // RFC 1951 3.2.5
    const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int len = 3; len <= 258; ++len) {
        const DeflateSym s = deflate_length_sym(len);
        CHECK(s.sym >= 257 && s.sym <= 285);
        const int k = s.sym - 257;
        CHECK(static_cast<int>(s.extra_bits) == lext[k] && lbase[k] + static_cast<int>(s.extra) == len && s.extra < (1u << s.extra_bits));
    }
    for (int dist = 1; dist <= 32768; ++dist) {
        const DeflateSym s = deflate_dist_sym(dist);
        CHECK(s.sym < 30);
        const int ext = s.sym < 4 ? 0 : static_cast<int>(s.sym) / 2 - 1;
        const int base = s.sym < 4 ? static_cast<int>(s.sym) + 1 : (1 << (ext + 1)) + (s.sym & 1) * (1 << ext) + 1;
        CHECK(static_cast<int>(s.extra_bits) == ext && base + static_cast<int>(s.extra) == dist && s.extra < (1u << s.extra_bits));
    }
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int k = 0; k < 19; ++k) CHECK(deflate_cl_order(k) == order[k]);
    std::printf("huff_check ok: %d codes limited\n", limited);
    return 0;
}
