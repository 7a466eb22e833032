// npr_bam_host.cpp -- the host side of the SAM -> sorted BAM + BAI conversion (include/nprealign.h, "coordinate-sorted BAM"): the columns
// npr_sam_parse leaves aside (npr_sam_parse_tail), the optional fields as BAM auxiliary bytes (npr_bam_tags), the bytes before the first
// record (npr_bam_header) and the index file from the tables the device made (npr_bai_write); and, for the way back, the block table of a
// BGZF file (npr_bgzf_scan; "reading BGZF") and the chunks of a region from a BAI file (npr_bai_chunks; "region queries").  Host code,
// threaded, no HIP.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "nprealign.h"
#include "npr_threads.h"

using npr::parallel_for;
using npr::usable_cpus;

namespace {

inline const char *find(const char *p, const char *end, char c) {
    const void *q = p < end ? std::memchr(p, c, static_cast<size_t>(end - p)) : nullptr;
    return q ? static_cast<const char *>(q) : end;
}

// decimal integer spanning the whole field (an optional leading '-' or '+'); false when anything else is in it
inline bool parse_int(const char *p, const char *end, int64_t &v) {
    if (p >= end) return false;
    bool neg = false;
    if (*p == '-' || *p == '+') neg = *p == '-', ++p;
    if (p >= end || end - p > 18) return false;
    int64_t x = 0;
    for (; p < end; ++p) {
        if (*p < '0' || *p > '9') return false;
        x = x * 10 + (*p - '0');
    }
    v = neg ? -x : x;
    return true;
}

inline bool parse_float(const char *p, const char *end, float &v) {
    if (p >= end || end - p > 63 || *p == ' ' || *p == '\t') return false;
    char buf[64];
    std::memcpy(buf, p, static_cast<size_t>(end - p));
    buf[end - p] = 0;
    char *stop = nullptr;
    v = std::strtof(buf, &stop);
    return stop == buf + (end - p);
}

// a sink that counts, or writes little-endian bytes
struct Sink {
    uint8_t *p;  // nullptr: count only
    int64_t n = 0;
    void byte(uint8_t b) {
        if (p) p[n] = b;
        ++n;
    }
    void bytes(const void *src, int64_t k) {
        if (p && k) std::memcpy(p + n, src, static_cast<size_t>(k));
        n += k;
    }
    template <typename T>
    void le(T v, int width) {
        for (int k = 0; k < width; ++k) byte(static_cast<uint8_t>(static_cast<uint64_t>(v) >> (8 * k)));
    }
};

inline int width_of(char t) { return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0; }
inline bool fits(char t, int64_t v) {
    switch (t) {
        case 'c': return v >= -128 && v <= 127;
        case 'C': return v >= 0 && v <= 255;
        case 's': return v >= -32768 && v <= 32767;
        case 'S': return v >= 0 && v <= 65535;
        case 'i': return v >= -(int64_t(1) << 31) && v < (int64_t(1) << 31);
        case 'I': return v >= 0 && v < (int64_t(1) << 32);
        default: return false;
    }
}

// one TAG:TYPE:VALUE field [p, e) into the sink; false: malformed
bool aux_field(const char *p, const char *e, Sink &s) {
    if (e - p < 5 || p[2] != ':' || p[4] != ':') return false;
    const char type = p[3];
    const char *v = p + 5;
    s.byte(static_cast<uint8_t>(p[0])), s.byte(static_cast<uint8_t>(p[1]));
    switch (type) {
        case 'A':
            if (e - v != 1 || *v < '!' || *v > '~') return false;
            s.byte('A'), s.byte(static_cast<uint8_t>(*v));
            return true;
        case 'i': {
            int64_t x;
            if (!parse_int(v, e, x) || x < -(int64_t(1) << 31) || x >= (int64_t(1) << 32)) return false;
            const char t = x >= 0 ? (x <= 255 ? 'C' : x <= 65535 ? 'S' : 'I') : (x >= -128 ? 'c' : x >= -32768 ? 's' : 'i');
            s.byte(static_cast<uint8_t>(t)), s.le(x, width_of(t));
            return true;
        }
        case 'f': {
            float f;
            if (!parse_float(v, e, f)) return false;
            uint32_t bits;
            std::memcpy(&bits, &f, 4);
            s.byte('f'), s.le(bits, 4);
            return true;
        }
        case 'Z':
            s.byte('Z'), s.bytes(v, e - v), s.byte(0);
            return true;
        case 'H':
            if ((e - v) & 1) return false;
            for (const char *q = v; q < e; ++q)
                if (!((*q >= '0' && *q <= '9') || (*q >= 'a' && *q <= 'f') || (*q >= 'A' && *q <= 'F'))) return false;
            s.byte('H'), s.bytes(v, e - v), s.byte(0);
            return true;
        case 'B': {
            if (v >= e) return false;
            const char sub = *v++;
            const int w = width_of(sub);
            if (!w) return false;
            uint32_t count = 0;
            for (const char *q = v; q < e; ++q) count += *q == ',';
            if (v < e && *v != ',') return false;
            s.byte('B'), s.byte(static_cast<uint8_t>(sub)), s.le(count, 4);
            while (v < e) {
                const char *a = v + 1, *b = find(a, e, ',');
                if (sub == 'f') {
                    float f;
                    if (!parse_float(a, b, f)) return false;
                    uint32_t bits;
                    std::memcpy(&bits, &f, 4);
                    s.le(bits, 4);
                } else {
                    int64_t x;
                    if (!parse_int(a, b, x) || !fits(sub, x)) return false;
                    s.le(x, w);
                }
                v = b;
            }
            return true;
        }
        default: return false;
    }
}

// the optional fields [p, e) of one line; -1: malformed
int64_t aux_line(const char *p, const char *e, uint8_t *out) {
    Sink s{out};
    while (p < e) {
        const char *t = find(p, e, '\t');
        if (!aux_field(p, t, s)) return -1;
        if (t < e && t + 1 == e) return -1;  // a tab at the end: an empty field
        p = t < e ? t + 1 : e;
    }
    return s.n;
}

// the way back: the auxiliary bytes [p, e) of one record as tab-separated TAG:TYPE:VALUE text into the sink; false: malformed.  With
// `placeholder` a CG:B:I field is left out of the text and cg[0 .. 1] say where its elements lie (offset from p) and how many they are.
bool aux_text_line(const uint8_t *p, const uint8_t *e, bool placeholder, Sink &s, int64_t *cg) {
    const uint8_t *const p0 = p;
    char num[48];
    bool first = true;
    cg[0] = cg[1] = -1;
    auto number = [&](const char *fmt, auto v) { s.bytes(num, std::snprintf(num, sizeof(num), fmt, v)); };
    auto element = [&](char t, const uint8_t *q) {  // one value of an integer type or 'f' at q
        uint32_t u = 0;
        for (int k = 0; k < width_of(t); ++k) u |= static_cast<uint32_t>(q[k]) << (8 * k);
        if (t == 'f') {
            float f;
            std::memcpy(&f, &u, 4);
            number("%g", static_cast<double>(f));
        } else if (t == 'c') number("%d", static_cast<int>(static_cast<int8_t>(u)));
        else if (t == 's') number("%d", static_cast<int>(static_cast<int16_t>(u)));
        else if (t == 'i') number("%d", static_cast<int>(static_cast<int32_t>(u)));
        else number("%u", u);
    };
    while (p < e) {
        if (e - p < 3) return false;
        const uint8_t t0 = p[0], t1 = p[1];
        const char type = static_cast<char>(p[2]);
        p += 3;
        if (placeholder && cg[0] < 0 && t0 == 'C' && t1 == 'G' && type == 'B' && e - p >= 5 && p[0] == 'I') {
            const int64_t count = p[1] | static_cast<int64_t>(p[2]) << 8 | static_cast<int64_t>(p[3]) << 16 | static_cast<int64_t>(p[4]) << 24;
            if (count >= (int64_t(1) << 31) || 4 * count > e - (p + 5)) return false;
            for (int64_t k = 0; k < count; ++k)
                if ((p[5 + 4 * k] & 15) > 8) return false;
            cg[0] = p + 5 - p0, cg[1] = count;
            p += 5 + 4 * count;
            continue;
        }
        if (!first) s.byte('\t');
        first = false;
        s.byte(t0), s.byte(t1), s.byte(':');
        const int w = width_of(type);
        if (type == 'A') {
            if (e - p < 1) return false;
            s.byte('A'), s.byte(':'), s.byte(*p++);
        } else if (w) {
            if (e - p < w) return false;
            s.byte(type == 'f' ? 'f' : 'i'), s.byte(':'), element(type, p);
            p += w;
        } else if (type == 'Z' || type == 'H') {
            const void *nul = std::memchr(p, 0, static_cast<size_t>(e - p));
            if (!nul) return false;
            const uint8_t *z = static_cast<const uint8_t *>(nul);
            s.byte(static_cast<uint8_t>(type)), s.byte(':'), s.bytes(p, z - p);
            p = z + 1;
        } else if (type == 'B') {
            if (e - p < 5) return false;
            const char sub = static_cast<char>(p[0]);
            const int sw = width_of(sub);
            const int64_t count = p[1] | static_cast<int64_t>(p[2]) << 8 | static_cast<int64_t>(p[3]) << 16 | static_cast<int64_t>(p[4]) << 24;
            if (!sw || sw * count > e - (p + 5)) return false;
            s.byte('B'), s.byte(':'), s.byte(static_cast<uint8_t>(sub));
            for (int64_t k = 0; k < count; ++k) s.byte(','), element(sub, p + 5 + sw * k);
            p += 5 + sw * count;
        } else {
            return false;
        }
    }
    return true;
}

// the value of FIELD: in a tab-separated header line [p, e): its span, or (e, e)
std::string_view header_field(const char *p, const char *e, const char *key) {
    for (const char *q = find(p, e, '\t'); q < e;) {
        const char *f = q + 1, *t = find(f, e, '\t');
        if (t - f >= 3 && f[0] == key[0] && f[1] == key[1] && f[2] == ':') return std::string_view(f + 3, static_cast<size_t>(t - f - 3));
        q = t;
    }
    return std::string_view(e, 0);
}

}  // namespace

extern "C" {

int32_t npr_sam_parse_tail(const char *text, const int64_t *span, const int64_t *fields, int64_t n, const char *rnames, const int64_t *rname_off,
                           int64_t n_refs, int64_t *tail) {
    if (n < 0 || n_refs < 0 || (n && (!text || !span || !fields || !tail)) || (n_refs && (!rnames || !rname_off))) return NPR_ERR_INVALID;
    try {
        std::unordered_map<std::string_view, int64_t> tid;
        tid.reserve(static_cast<size_t>(n_refs) * 2);
        for (int64_t k = 0; k < n_refs; ++k) tid.emplace(std::string_view(rnames + rname_off[k], static_cast<size_t>(rname_off[k + 1] - rname_off[k])), k);
        parallel_for((n + 127) / 128, usable_cpus(), [&](int64_t c) {
            for (int64_t i = c * 128, hi = std::min(n, (c + 1) * 128); i < hi; ++i) {
                int64_t *t = tail + i * NPR_SAM_TAIL_COLS;
                const char *const ls = text + span[2 * i], *const le = text + span[2 * i + 1];
                std::fill(t, t + NPR_SAM_TAIL_COLS, int64_t(0));
                t[0] = -1, t[3] = t[4] = t[5] = t[6] = le - text, t[7] = NPR_ERR_INVALID;
                const char *col[11], *col_end[11];
                col[0] = ls;
                int got = 1;
                for (const char *q = ls; got < 11;) {
                    const char *tb = find(q, le, '\t');
                    if (tb >= le) break;
                    col[got++] = tb + 1, q = tb + 1;
                }
                if (got < 11) continue;
                for (int k = 0; k < 10; ++k) col_end[k] = col[k + 1] - 1;
                col_end[10] = find(col[10], le, '\t');
                t[3] = col[10] - text, t[4] = col_end[10] - text;
                t[5] = col_end[10] < le ? col_end[10] + 1 - text : le - text, t[6] = le - text;
                int64_t flag, pos, mapq, pnext, tlen;
                if (*col[1] == '+' || *col[3] == '+' || *col[4] == '+' || *col[7] == '+' || *col[8] == '+') continue;  // (npr_sam_parse takes no sign but '-')
                if (!parse_int(col[1], col_end[1], flag) || !parse_int(col[3], col_end[3], pos) || !parse_int(col[4], col_end[4], mapq) ||
                    !parse_int(col[7], col_end[7], pnext) || !parse_int(col[8], col_end[8], tlen))
                    continue;
                t[1] = pnext - 1, t[2] = tlen;
                const std::string_view rn(col[6], static_cast<size_t>(col_end[6] - col[6]));
                if (rn.size() == 1 && rn[0] == '=') {
                    t[0] = fields[i * NPR_SAM_COLS + 10];
                } else {
                    const auto it = tid.find(rn);
                    t[0] = it == tid.end() ? -1 : it->second;
                }
                const int64_t limit = int64_t(1) << 29;
                if (flag < 0 || flag > 65535 || mapq < 0 || mapq > 255 || pos < 0 || pos > limit || pnext < 0 || pnext > limit ||
                    tlen <= -(int64_t(1) << 31) || tlen >= (int64_t(1) << 31) || col_end[0] == col[0] || col_end[0] - col[0] > 254)
                    continue;
                const bool no_seq = col_end[9] - col[9] == 1 && *col[9] == '*', no_qual = col_end[10] - col[10] == 1 && *col[10] == '*';
                if (!no_qual && (no_seq || col_end[10] - col[10] != col_end[9] - col[9])) continue;
                t[7] = NPR_OK;
            }
        });
        return NPR_OK;
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_bgzf_scan(const uint8_t *file, int64_t len, int64_t *block_off, int64_t *stream_off, int64_t cap_blocks, int64_t *n_blocks) {
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!file || len < 28 || cap_blocks < 0 || !n_blocks || std::memcmp(file + len - 28, eof, 28) != 0) return NPR_ERR_INVALID;
    const int64_t end = len - 28;  // the blocks fill [0, end) exactly
    int64_t at = 0, stream = 0, n = 0;
    while (at < end) {
        if (end - at < 12 + 6 + 8) return NPR_ERR_INVALID;
        const uint8_t *b = file + at;
        if (b[0] != 0x1f || b[1] != 0x8b || b[2] != 8 || !(b[3] & 4)) return NPR_ERR_INVALID;
        const int64_t xlen = b[10] | static_cast<int64_t>(b[11]) << 8;
        if (12 + xlen + 8 > end - at) return NPR_ERR_INVALID;
        int64_t size = -1;
        for (int64_t x = 12; x < 12 + xlen;) {  // the extra subfields: SI1, SI2, SLEN, the data; BC may stand anywhere among them
            if (x + 4 > 12 + xlen) return NPR_ERR_INVALID;
            const int64_t slen = b[x + 2] | static_cast<int64_t>(b[x + 3]) << 8;
            if (x + 4 + slen > 12 + xlen) return NPR_ERR_INVALID;
            if (b[x] == 'B' && b[x + 1] == 'C' && slen == 2 && size < 0) size = (b[x + 4] | static_cast<int64_t>(b[x + 5]) << 8) + 1;
            x += 4 + slen;
        }
        if (size < 12 + xlen + 8 || size > end - at) return NPR_ERR_INVALID;
        const int64_t isize = b[size - 4] | static_cast<int64_t>(b[size - 3]) << 8 | static_cast<int64_t>(b[size - 2]) << 16 | static_cast<int64_t>(b[size - 1]) << 24;
        if (isize > 65536) return NPR_ERR_INVALID;
        if (n < cap_blocks) {
            if (block_off) block_off[n] = at;
            if (stream_off) stream_off[n] = stream;
        }
        ++n, at += size, stream += isize;
    }
    *n_blocks = n;
    if (block_off || stream_off) {
        if (n + 1 > cap_blocks) return NPR_ERR_CAPACITY;
        if (block_off) block_off[n] = end;
        if (stream_off) stream_off[n] = stream;
    }
    return stream;
}

int64_t npr_bai_chunks(const uint8_t *bai, int64_t bai_len, int32_t tid, int64_t beg, int64_t end, uint64_t *chunk_beg, uint64_t *chunk_end, int64_t cap,
                       int64_t *n_ref) {
    if (!bai || bai_len < 8 || cap < 0 || !n_ref || (chunk_beg && !chunk_end)) return NPR_ERR_INVALID;
    try {
        int64_t at = 0;
        // a little-endian value of `width` bytes at `at`, which moves on; false: it runs past the image
        auto take = [&](int width, uint64_t &v) {
            if (bai_len - at < width) return false;
            v = 0;
            for (int k = 0; k < width; ++k) v |= static_cast<uint64_t>(bai[at + k]) << (8 * k);
            at += width;
            return true;
        };
        auto count = [&](int64_t &v) {  // an int32 count: not negative
            uint64_t u;
            if (!take(4, u)) return false;
            v = static_cast<int32_t>(static_cast<uint32_t>(u));
            return v >= 0;
        };
        if (std::memcmp(bai, "BAI\1", 4) != 0) return NPR_ERR_INVALID;
        at = 4;
        int64_t refs = 0;
        if (!count(refs)) return NPR_ERR_INVALID;
        *n_ref = refs;
        if (tid < 0 || tid >= refs || beg < 0 || beg >= end || end > (int64_t(1) << 29)) return NPR_ERR_INVALID;
        // reg2bins(beg, end): bin 0 and, per level, the bins of beg >> shift .. (end - 1) >> shift
        auto wanted = [&](uint64_t bin) {
            if (bin == 0) return true;
            static const int shift[5] = {26, 23, 20, 17, 14};
            static const int64_t first[5] = {1, 9, 73, 585, 4681};
            for (int lv = 0; lv < 5; ++lv) {
                const int64_t b = static_cast<int64_t>(bin) - first[lv];
                if (b >= (beg >> shift[lv]) && b <= ((end - 1) >> shift[lv]) && static_cast<int64_t>(bin) < (lv < 4 ? first[lv + 1] : 37449)) return true;
            }
            return false;
        };
        std::vector<std::pair<uint64_t, uint64_t>> found;
        uint64_t low = 0;
        for (int64_t k = 0; k < refs; ++k) {
            int64_t n_bin = 0, n_intv = 0;
            if (!count(n_bin)) return NPR_ERR_INVALID;
            for (int64_t b = 0; b < n_bin; ++b) {
                uint64_t bin;
                int64_t n_chunk = 0;
                if (!take(4, bin) || !count(n_chunk) || n_chunk > (bai_len - at) / 16) return NPR_ERR_INVALID;
                const bool use = k == tid && bin != 37450 && wanted(bin);
                for (int64_t c = 0; c < n_chunk; ++c) {
                    uint64_t cb, ce;
                    (void)take(8, cb), (void)take(8, ce);  // (n_chunk was checked against what is left)
                    if (bin == 37450) continue;            // (the pseudo-bin's pairs are an interval and two counts)
                    if (ce < cb) return NPR_ERR_INVALID;
                    if (use) found.emplace_back(cb, ce);
                }
            }
            if (!count(n_intv) || n_intv > (bai_len - at) / 8) return NPR_ERR_INVALID;
            if (k == tid && n_intv) {
                int64_t keep = at;
                at += 8 * std::min<int64_t>(beg >> 14, n_intv - 1);
                (void)take(8, low);
                at = keep;
            }
            at += 8 * n_intv;
        }
        if (bai_len - at != 0 && bai_len - at != 8) return NPR_ERR_INVALID;  // n_no_coor, or nothing
        found.erase(std::remove_if(found.begin(), found.end(), [&](const std::pair<uint64_t, uint64_t> &c) { return c.second <= low; }), found.end());
        std::sort(found.begin(), found.end());
        size_t n = 0;
        for (size_t i = 0; i < found.size(); ++i) {
            if (n && found[i].first <= found[n - 1].second) found[n - 1].second = std::max(found[n - 1].second, found[i].second);
            else found[n++] = found[i];
        }
        if (!chunk_beg) return static_cast<int64_t>(n);
        if (cap < static_cast<int64_t>(n)) return NPR_ERR_CAPACITY;
        for (size_t i = 0; i < n; ++i) chunk_beg[i] = found[i].first, chunk_end[i] = found[i].second;
        return static_cast<int64_t>(n);
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_bam_aux_text(const uint8_t *aux, const int64_t *aux_off, int64_t n, const uint8_t *placeholder, int64_t *text_off, int64_t *cg, uint8_t *out,
                         int64_t cap) {
    if (n < 0 || !aux_off || !text_off || !cg || cap < 0 || (n && aux_off[n] > aux_off[0] && !aux)) return NPR_ERR_INVALID;
    try {
        std::atomic<bool> bad{false};
        const int64_t chunks = (n + 127) / 128;
        parallel_for(chunks, usable_cpus(), [&](int64_t c) {
            for (int64_t i = c * 128, hi = std::min(n, (c + 1) * 128); i < hi; ++i) {
                Sink s{nullptr};
                if (aux_off[i + 1] < aux_off[i] || !aux_text_line(aux + aux_off[i], aux + aux_off[i + 1], placeholder && placeholder[i], s, cg + 2 * i)) bad = true;
                text_off[i + 1] = s.n;
            }
        });
        if (bad) return NPR_ERR_INVALID;
        text_off[0] = 0;
        for (int64_t i = 0; i < n; ++i) text_off[i + 1] += text_off[i];
        const int64_t total = text_off[n];
        if (!out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        parallel_for(chunks, usable_cpus(), [&](int64_t c) {
            for (int64_t i = c * 128, hi = std::min(n, (c + 1) * 128); i < hi; ++i) {
                Sink s{out + text_off[i]};
                (void)aux_text_line(aux + aux_off[i], aux + aux_off[i + 1], placeholder && placeholder[i], s, cg + 2 * i);
            }
        });
        return total;
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_bam_tags(const char *text, const int64_t *tail, int64_t n, int64_t *tag_off, uint8_t *out, int64_t cap) {
    if (n < 0 || !tag_off || (n && (!text || !tail)) || cap < 0) return NPR_ERR_INVALID;
    try {
        std::atomic<bool> bad{false};
        const int64_t chunks = (n + 127) / 128;
        auto span_of = [&](int64_t i, const char *&p, const char *&e) {
            const int64_t *t = tail + i * NPR_SAM_TAIL_COLS;
            p = text + t[5], e = t[7] == NPR_OK ? text + t[6] : p;
        };
        parallel_for(chunks, usable_cpus(), [&](int64_t c) {
            for (int64_t i = c * 128, hi = std::min(n, (c + 1) * 128); i < hi; ++i) {
                const char *p, *e;
                span_of(i, p, e);
                const int64_t len = aux_line(p, e, nullptr);
                if (len < 0) bad = true;
                tag_off[i + 1] = std::max<int64_t>(len, 0);
            }
        });
        if (bad) return NPR_ERR_INVALID;
        tag_off[0] = 0;
        for (int64_t i = 0; i < n; ++i) tag_off[i + 1] += tag_off[i];
        const int64_t total = tag_off[n];
        if (!out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        parallel_for(chunks, usable_cpus(), [&](int64_t c) {
            for (int64_t i = c * 128, hi = std::min(n, (c + 1) * 128); i < hi; ++i) {
                const char *p, *e;
                span_of(i, p, e);
                (void)aux_line(p, e, out + tag_off[i]);
            }
        });
        return total;
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_bam_header(const char *sam_header, int64_t len, int32_t sorted, uint8_t *out, int64_t cap, int64_t *n_refs, int64_t *ref_len, int64_t cap_refs) {
    if (len < 0 || (len && !sam_header) || cap < 0 || !n_refs) return NPR_ERR_INVALID;
    try {
        const char *const end = sam_header + len;
        const std::string so = sorted ? "coordinate" : "unsorted";
        std::string text;
        std::vector<std::pair<std::string_view, int64_t>> refs;
        bool have_hd = false;
        for (const char *p = sam_header; p < end;) {
            const char *nl = find(p, end, '\n');
            const char *e = nl;
            if (e > p && e[-1] == '\r') --e;
            if (e - p >= 3 && p[0] == '@' && p[1] == 'H' && p[2] == 'D' && !have_hd) {
                have_hd = true;
                const std::string_view v = header_field(p, e, "SO");
                if (v.data() == e) {
                    text.append(p, e), text += "\tSO:" + so;
                } else {
                    text.append(p, v.data()), text += so, text.append(v.data() + v.size(), e);
                }
                text.append(e, nl < end ? nl + 1 : end);
                if (nl >= end) text += '\n';
            } else {
                if (e - p >= 3 && p[0] == '@' && p[1] == 'S' && p[2] == 'Q') {
                    const std::string_view sn = header_field(p, e, "SN"), ln = header_field(p, e, "LN");
                    int64_t l = 0;
                    if (sn.data() == e || sn.empty() || sn.size() > 254 || !parse_int(ln.data(), ln.data() + ln.size(), l) || l < 1 || l >= (int64_t(1) << 31)) return NPR_ERR_INVALID;
                    refs.emplace_back(sn, l);
                }
                text.append(p, nl < end ? nl + 1 : end);
                if (nl >= end && nl > p) text += '\n';
            }
            p = nl < end ? nl + 1 : end;
        }
        if (refs.empty()) return NPR_ERR_INVALID;
        if (!have_hd) text = "@HD\tVN:1.0\tSO:" + so + "\n" + text;
        *n_refs = static_cast<int64_t>(refs.size());
        if (ref_len) {
            if (cap_refs < *n_refs) return NPR_ERR_CAPACITY;
            for (size_t k = 0; k < refs.size(); ++k) ref_len[k] = refs[k].second;
        }
        Sink s{nullptr};
        for (int pass = 0; pass < 2; ++pass) {
            s.n = 0;
            s.bytes("BAM\1", 4), s.le(text.size(), 4), s.bytes(text.data(), static_cast<int64_t>(text.size())), s.le(refs.size(), 4);
            for (const auto &r : refs) s.le(r.first.size() + 1, 4), s.bytes(r.first.data(), static_cast<int64_t>(r.first.size())), s.byte(0), s.le(r.second, 4);
            if (!out) return s.n;
            if (cap < s.n) return NPR_ERR_CAPACITY;
            s.p = out;
        }
        return s.n;
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_bai_write(int64_t n_refs, const int64_t *ref_len, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg,
                      const uint64_t *run_end, const uint64_t *linear, const uint64_t *meta, int64_t n_no_coor, uint8_t *out, int64_t cap) {
    if (n_refs < 0 || n_runs < 0 || cap < 0 || n_no_coor < 0 || (n_refs && (!ref_len || !linear || !meta)) || (n_runs && (!run_tid || !run_bin || !run_beg || !run_end)))
        return NPR_ERR_INVALID;
    try {
        const uint64_t none = ~uint64_t(0);
        for (int64_t r = 0; r < n_runs; ++r) {
            if (run_tid[r] < -1 || run_tid[r] >= n_refs) return NPR_ERR_INVALID;
            if (r == 0) continue;
            const uint64_t a = run_tid[r - 1] < 0 ? uint64_t(n_refs) : uint64_t(run_tid[r - 1]), b = run_tid[r] < 0 ? uint64_t(n_refs) : uint64_t(run_tid[r]);
            if (a > b || (a == b && run_bin[r - 1] > run_bin[r])) return NPR_ERR_INVALID;
        }
        for (int64_t k = 0; k < n_refs; ++k)
            if (ref_len[k] < 1) return NPR_ERR_INVALID;
        Sink s{nullptr};
        std::vector<uint64_t> win;
        for (int pass = 0; pass < 2; ++pass) {
            s.n = 0;
            s.bytes("BAI\1", 4), s.le(n_refs, 4);
            int64_t r = 0, w0 = 0;
            for (int64_t k = 0; k < n_refs; ++k) {
                while (r < n_runs && run_tid[r] >= 0 && run_tid[r] < k) ++r;
                int64_t r1 = r, bins = 0;
                for (; r1 < n_runs && run_tid[r1] == k; ++r1) bins += r1 == r || run_bin[r1] != run_bin[r1 - 1];
                const uint64_t *m = meta + 4 * k;
                const bool any = m[0] != none;
                s.le(bins + (any ? 1 : 0), 4);
                for (int64_t a = r; a < r1;) {
                    int64_t b = a;
                    while (b < r1 && run_bin[b] == run_bin[a]) ++b;
                    s.le(run_bin[a], 4), s.le(b - a, 4);
                    for (int64_t q = a; q < b; ++q) s.le(run_beg[q], 8), s.le(run_end[q], 8);
                    a = b;
                }
                if (any) {
                    s.le(37450, 4), s.le(2, 4);
                    for (int q = 0; q < 4; ++q) s.le(m[q], 8);
                }
                r = r1;
                const int64_t nwin = ((ref_len[k] - 1) >> 14) + 1;
                int64_t used = nwin;
                while (used > 0 && linear[w0 + used - 1] == none) --used;
                win.assign(linear + w0, linear + w0 + used);
                for (int64_t q = used - 2; q >= 0; --q)
                    if (win[q] == none) win[q] = win[q + 1];
                s.le(used, 4);
                for (int64_t q = 0; q < used; ++q) s.le(win[q], 8);
                w0 += nwin;
            }
            s.le(n_no_coor, 8);
            if (!out) return s.n;
            if (cap < s.n) return NPR_ERR_CAPACITY;
            s.p = out;
        }
        return s.n;
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

}  // extern "C"
