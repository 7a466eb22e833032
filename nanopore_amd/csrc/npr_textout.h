// npr_textout.h -- the one writer of the host-side text formatters (npr_text.cpp, npr_io.cpp, npr_seed_api.cpp, npr_seedchain_api.cpp): a
// formatter says what a record consists of ONCE, as emit(i, sink), and format_records runs it twice -- over a sink that counts, which gives the
// offsets, and over a sink that writes.  A record's length is whatever its emit says to the counting sink: there is no length formula to keep
// in step with a writer.  Standard library and npr_threads.h only, so that a host program without HIP can use it.  Not installed.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "npr_threads.h"

namespace npr {

// NPR_ERR_INVALID / NPR_ERR_CAPACITY of include/nprealign.h, which this header does without (npr_text.cpp asserts that they agree)
constexpr int64_t kTextErrInvalid = -1, kTextErrCapacity = -3;

// cigar letters by operation code: the realigner's own three, and SAM's nine in pysam's numbering (the chains of npr_seedchain_api.cpp)
constexpr char kOpsMID[] = "MID";
constexpr char kOpsSam[] = "MIDNSHP=X";

// decimal digits of v >= 0, without a division below 10^10 (a job formats 10^8 cigar lengths of 30 bits)
inline int digits(int64_t v) {
    int k = 0;
    while (v >= INT64_C(10000000000)) v /= INT64_C(10000000000), k += 10;
    return k + (v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8 : v < 1000000000 ? 9 : 10);
}
template <typename T>
inline void put(char *&w, T v) {  // (the divisions by ten in the width of T)
    const int k = digits(static_cast<int64_t>(v));
    for (int j = k - 1; j >= 0; --j) w[j] = static_cast<char>('0' + v % 10), v /= 10;
    w += k;
}
inline char complement(char c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        case 'a': return 't';
        case 'c': return 'g';
        case 'g': return 'c';
        case 't': return 'a';
        default: return c;
    }
}

// The two sinks have the same members.  The cigar members say whether every operation was one of the table's and no length negative; the
// writing sink takes that for granted (it runs only after the counting sink has looked) and says true.
struct CountSink {
    int64_t n = 0;
    void bytes(const void *, int64_t k) { n += k; }
    void ch(char) { ++n; }
    template <size_t N>
    void lit(const char (&)[N]) { n += static_cast<int64_t>(N) - 1; }
    void num(int64_t v) { n += digits(v); }
    // packed operations, length << 2 | code with the codes of kOpsMID; no operation: "*"
    bool cigar_words(const uint32_t *words, int64_t m) {
        if (m <= 0) return ch('*'), true;
        bool ok = true;
        int64_t k = 0;
        for (int64_t q = 0; q < m; ++q) {
            if ((words[q] & 3u) > 2u) ok = false;
            k += digits(words[q] >> 2) + 1;
        }
        n += k;
        return ok;
    }
    // (code, length) pairs; no pair: "*"
    template <size_t N>
    bool cigar_pairs(const int32_t *ops, int64_t m, const char (&)[N]) {
        if (m <= 0) return ch('*'), true;
        bool ok = true;
        for (int64_t q = 0; q < m; ++q) {
            if (ops[2 * q] < 0 || ops[2 * q] >= static_cast<int32_t>(N) - 1 || ops[2 * q + 1] < 0) ok = false;
            n += digits(ops[2 * q + 1]) + 1;
        }
        return ok;
    }
    void revcomp(const uint8_t *, int64_t k) { n += k; }
};

struct WriteSink {
    char *w;
    void bytes(const void *p, int64_t k) {
        if (k) std::memcpy(w, p, static_cast<size_t>(k));
        w += k;
    }
    void ch(char c) { *w++ = c; }
    template <size_t N>
    void lit(const char (&s)[N]) { std::memcpy(w, s, N - 1), w += N - 1; }
    void num(int64_t v) { put(w, v); }
    bool cigar_words(const uint32_t *words, int64_t m) {
        if (m <= 0) return ch('*'), true;
        char *p = w;
        for (int64_t q = 0; q < m; ++q) {
            const uint32_t v = words[q] >> 2;
            if (v < 10u) {  // (most operations of a realigned nanopore read)
                p[0] = static_cast<char>('0' + v), p[1] = kOpsMID[words[q] & 3u], p += 2;
                continue;
            }
            put(p, v);
            *p++ = kOpsMID[words[q] & 3u];
        }
        w = p;
        return true;
    }
    template <size_t N>
    bool cigar_pairs(const int32_t *ops, int64_t m, const char (&table)[N]) {
        if (m <= 0) return ch('*'), true;
        char *p = w;  // (a local: a store through a char pointer may be a store to `w` itself, as far as the compiler knows)
        for (int64_t q = 0; q < m; ++q) put(p, ops[2 * q + 1]), *p++ = table[ops[2 * q]];
        w = p;
        return true;
    }
    // the reverse complement of seq[0 .. k): A <-> T, C <-> G in either case, everything else kept
    void revcomp(const uint8_t *seq, int64_t k) {
        char *p = w;
        for (int64_t u = 0; u < k; ++u) p[u] = complement(static_cast<char>(seq[k - 1 - u]));
        w = p + k;
    }
};

// n records, record i = what emit(i, sink) gives the sink; emit says false for a record that is invalid (and may stop there).  rec_off[n + 1]
// receives the offsets and record i lands at out[rec_off[i] .. rec_off[i + 1]); out == nullptr: only the offsets.  Returns the total length,
// kTextErrInvalid when a record was invalid (rec_off and out untouched), kTextErrCapacity when cap is smaller (out untouched).  Both passes are
// spread over `threads` threads, in pieces of 256 and 64 records (the second pass has the memory traffic).
template <typename Emit>
int64_t format_records(int64_t n, int threads, int64_t *rec_off, char *out, int64_t cap, Emit emit) {
    std::vector<int64_t> len(static_cast<size_t>(n));
    std::atomic<int> bad{0};
    parallel_for((n + 255) / 256, threads, [&](int64_t c) {
        for (int64_t i = c * 256, hi = std::min(n, (c + 1) * 256); i < hi; ++i) {
            CountSink s;
            if (!emit(i, s)) bad = 1;
            len[i] = s.n;
        }
    });
    if (bad) return kTextErrInvalid;
    rec_off[0] = 0;
    for (int64_t i = 0; i < n; ++i) rec_off[i + 1] = rec_off[i] + len[i];
    if (!out) return rec_off[n];
    if (cap < rec_off[n]) return kTextErrCapacity;
    parallel_for((n + 63) / 64, threads, [&](int64_t c) {
        for (int64_t i = c * 64, hi = std::min(n, (c + 1) * 64); i < hi; ++i) {
            WriteSink s{out + rec_off[i]};
            emit(i, s);
        }
    });
    return rec_off[n];
}

}  // namespace npr
