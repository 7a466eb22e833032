// npr_inflate.h -- the inflate core: the deflate data of ONE BGZF block, body[0, n), into at most isize bytes (RFC 1951 in full: any number
// of blocks up to the one with BFINAL, BTYPE 0 / 1 / 2, code-length symbols 16 / 17 / 18, lengths 3 .. 258, distances 1 .. 32768, matches
// that overlap their own output).  Plain C++ on a byte pointer and lengths, one body for host and device (the kernel: npr_inflate.hip; the
// host program under AddressSanitizer: tests/native/inflate_check.cpp).  No intrinsics.
// It accepts what a fresh raw inflater of zlib (no history, window 32768) accepts and ends on, and refuses the rest with a status:
//   INF_BTYPE           BTYPE 3
//   INF_STORED_LEN      a stored block whose LEN is not ~NLEN
//   INF_OVERSUBSCRIBED  code lengths whose Kraft sum exceeds one
//   INF_INCOMPLETE      code lengths whose Kraft sum is below one -- except, as zlib's inflate_table rules, a literal/length or distance
//                       code whose longest length is 1 (one code of one bit: its other bit pattern is no symbol), and a distance code
//                       without any length (then a match is no symbol); the code-length code must be complete
//   INF_REPEAT          symbol 16 with no length before it, or a repeat running past HLIT + HDIST
//   INF_NO_EOB          no code for symbol 256
//   INF_SYMBOL          HLIT above 286 or HDIST above 30, literal/length symbols 286 / 287, distance symbols 30 / 31, bits that are no code
//   INF_DISTANCE        a distance that reaches before the block's first byte
//   INF_OUTPUT          output past isize
//   INF_INPUT           input past n
//   INF_TRAILING        whole bytes of deflate data left after the final block
//   INF_ISIZE           a produced length that is not isize (the caller adds: ISIZE above 65536 or not what the block table says)
//   INF_CRC             (the caller's: the CRC-32 of the output is not the trailer's)
//   INF_BOUND           the step bound ran out (unreachable: every step consumes a bit, emits a byte or moves a phase on)
// At the data's end the statuses are not exact: a code is looked for bit by bit, and when the data runs out before the bits are shown to be no
// code the status is INF_INPUT where more data would have given INF_SYMBOL.  The data is refused either way, as zlib does not end on it.
// Every read index is checked against the window, which ends at n at the latest, and every write against isize, before it happens.
//
// The work is cut into PHASES so that a workgroup can share it: inflate_member(...) runs the loop below with `lanes` callers that meet at
// sync() -- 256 threads and __syncthreads() on the device, one caller and nothing on the host.  Lane 0 alone decodes; all lanes
//   refill   copy body[lo, lo + window) into the window (LDS on the device) whenever fewer than INF_MARGIN bytes lie ahead in it,
//   HEADER   (lane 0) BFINAL, BTYPE; stored: LEN / NLEN; dynamic: HLIT, HDIST, HCLEN, the code-length code, the lengths; fixed: the lengths
//            of RFC 1951 3.2.6; then per code the counts per length, the Kraft check and the symbols in canonical order,
//   STORED   all lanes copy the LEN bytes from body to the output,
//   CLEAR    all lanes zero the two look-up tables, FILL all lanes enter the codes of at most INF_FAST bits (a symbol a lane: its code
//            from its place in the canonical order, every table entry whose low bits are the reversed code),
//   SYMBOLS  (lane 0) literals, matches, the end of block: a table look-up for codes of at most INF_FAST bits, else bit by bit through
//            the counts per length; it hands back to the loop when the window runs low,
//   FINISH   (lane 0) trailing bytes, the produced length.
#ifndef NPR_INFLATE_H
#define NPR_INFLATE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NPR_INF_FN __host__ __device__ inline
#else
#define NPR_INF_FN inline
#endif

namespace npr {

enum {
    INF_OK = 0, INF_BTYPE, INF_STORED_LEN, INF_OVERSUBSCRIBED, INF_INCOMPLETE, INF_REPEAT, INF_NO_EOB, INF_SYMBOL, INF_DISTANCE, INF_OUTPUT,
    INF_INPUT, INF_TRAILING, INF_ISIZE, INF_CRC, INF_BOUND
};
enum { INF_PH_HEADER = 0, INF_PH_STORED, INF_PH_CLEAR, INF_PH_FILL, INF_PH_SYMBOLS, INF_PH_FINISH, INF_PH_DONE };
enum { INF_KIND_CODES = 0, INF_KIND_LENS, INF_KIND_DISTS };

constexpr int INF_FAST = 10;              // bits of the look-up tables
constexpr uint32_t INF_MARGIN = 1024;     // window bytes a phase may need: a dynamic header is at most 17 + 57 + 316 * 14 bits = 563 bytes
constexpr uint32_t INF_SYMBOL_BYTES = 16; // ... and one literal or match: 15 + 5 + 15 + 13 bits, beside the 8 bytes the bit buffer holds
constexpr uint32_t INF_MAX_ISIZE = 65536;
constexpr int INF_LL = 288, INF_D = 32;   // symbols a code can be given (the fixed codes have 288 and 32; 286 / 287 and 30 / 31 are refused when met)

struct InflateCode {
    uint16_t count[16];          // codes per length
    uint16_t first[16];          // the first canonical code of a length
    uint16_t offs[17];           // place of a length's first symbol in `symbol`; offs[16] = the used symbols
    uint16_t symbol[INF_LL];     // the used symbols in canonical order
    uint16_t fast[1 << INF_FAST];  // symbol << 4 | length at every index whose low bits are a code of at most INF_FAST bits, reversed; 0: none
};

struct Inflate {
    // the bit reader (lane 0): bits [0, nacc) of acc are the next of the data; pos = the next byte of body to enter acc
    uint64_t acc;
    uint32_t nacc, pos;
    uint32_t win_lo, win_hi;     // the window holds body[win_lo, win_hi)
    uint32_t produced;
    int32_t status;
    uint32_t phase, final_block;
    uint32_t steps;              // what is left of the step bound
    uint32_t stored_src, stored_len;
    uint32_t nlen, ndist;
    uint8_t lens[INF_LL + INF_D];
    InflateCode ll, d;
};

// ---- the bit reader (lane 0) ----
NPR_INF_FN void inf_refill(Inflate &s, const uint8_t *win) {
    while (s.nacc <= 56 && s.pos < s.win_hi) {   // (pos >= win_lo by the loop's refill rule; win_hi <= n)
        s.acc |= static_cast<uint64_t>(win[s.pos - s.win_lo]) << s.nacc;
        ++s.pos, s.nacc += 8;
    }
}
// k <= 32 bits, or false: input past n
NPR_INF_FN bool inf_bits(Inflate &s, const uint8_t *win, uint32_t k, uint32_t *v) {
    if (s.nacc < k) inf_refill(s, win);
    if (s.nacc < k) return false;
    *v = static_cast<uint32_t>(s.acc & ((uint64_t(1) << k) - 1));
    s.acc >>= k, s.nacc -= k;
    return true;
}

// one symbol bit by bit through the counts per length (canonical codes, most significant bit first): the symbol, -INF_INPUT or -INF_SYMBOL
NPR_INF_FN int inf_decode_slow(Inflate &s, const uint8_t *win, const uint16_t *count, const uint16_t *symbol, int max_bits) {
    inf_refill(s, win);
    uint32_t code = 0, first = 0, index = 0;
    for (int len = 1; len <= max_bits; ++len) {
        if (s.nacc < static_cast<uint32_t>(len)) return -INF_INPUT;
        code |= static_cast<uint32_t>(s.acc >> (len - 1)) & 1u;
        const uint32_t c = count[len];
        if (code < first + c) {
            s.acc >>= len, s.nacc -= len;
            return symbol[index + (code - first)];
        }
        index += c, first = (first + c) << 1, code <<= 1;
    }
    return -INF_SYMBOL;
}
NPR_INF_FN int inf_decode(Inflate &s, const uint8_t *win, const InflateCode &c) {
    inf_refill(s, win);
    const uint32_t e = c.fast[s.acc & ((1u << INF_FAST) - 1)];
    if (e) {
        const uint32_t len = e & 15;
        if (len > s.nacc) return -INF_INPUT;
        s.acc >>= len, s.nacc -= len;
        return static_cast<int>(e >> 4);
    }
    return inf_decode_slow(s, win, c.count, c.symbol, 15);
}

// counts per length, the Kraft check of zlib's inflate_table, the first codes, the symbols in canonical order: INF_OK or the refusal
NPR_INF_FN int inf_code_prepare(InflateCode &c, const uint8_t *lens, int n, int kind) {
    for (int k = 0; k < 16; ++k) c.count[k] = 0;
    for (int s = 0; s < n; ++s) ++c.count[lens[s] & 15];
    c.count[0] = 0;
    int left = 1, max_len = 0;
    for (int k = 1; k < 16; ++k) {
        left = (left << 1) - c.count[k];
        if (left < 0) return INF_OVERSUBSCRIBED;
        if (c.count[k]) max_len = k;
    }
    if (max_len == 0) {
        if (kind == INF_KIND_CODES) return INF_INCOMPLETE;   // (zlib reads on and then misses symbol 256: refused either way)
    } else if (left > 0 && (kind == INF_KIND_CODES || max_len != 1)) {
        return INF_INCOMPLETE;
    }
    uint32_t code = 0, at = 0;
    for (int k = 1; k < 16; ++k) {
        code = (code + c.count[k - 1]) << 1;
        c.first[k] = static_cast<uint16_t>(code), c.offs[k] = static_cast<uint16_t>(at);
        at += c.count[k];
    }
    c.first[0] = 0, c.offs[0] = 0, c.offs[16] = static_cast<uint16_t>(at);
    uint16_t next[16];
    for (int k = 0; k < 16; ++k) next[k] = c.offs[k];
    for (int s = 0; s < n; ++s)
        if (lens[s] & 15) c.symbol[next[lens[s] & 15]++] = static_cast<uint16_t>(s);   // (next[k] < offs[k + 1] <= n <= INF_LL)
    return INF_OK;
}

NPR_INF_FN void inf_code_clear(InflateCode &c, uint32_t lane, uint32_t lanes) {
    for (uint32_t k = lane; k < (1u << INF_FAST); k += lanes) c.fast[k] = 0;
}
// (the code is a prefix code -- the Kraft check passed --, so no two symbols write one entry)
NPR_INF_FN void inf_code_fill(InflateCode &c, uint32_t lane, uint32_t lanes) {
    const uint32_t used = c.offs[16];
    for (uint32_t i = lane; i < used && i < static_cast<uint32_t>(INF_LL); i += lanes) {
        uint32_t len = 1;
        while (len < 15 && i >= c.offs[len + 1]) ++len;
        if (len > static_cast<uint32_t>(INF_FAST)) continue;
        uint32_t v = c.first[len] + (i - c.offs[len]), r = 0;
        for (uint32_t k = 0; k < len; ++k) r = r << 1 | (v & 1), v >>= 1;
        const uint16_t e = static_cast<uint16_t>(c.symbol[i] << 4 | len);
        for (uint32_t k = r; k < (1u << INF_FAST); k += 1u << len) c.fast[k] = e;
    }
}

NPR_INF_FN void inf_fail(Inflate &s, int status) { s.status = status, s.phase = INF_PH_DONE; }

// ---- HEADER (lane 0) ----
NPR_INF_FN void inf_header(Inflate &s, const uint8_t *win, uint32_t n, uint32_t isize) {
    uint32_t v = 0;
    if (!inf_bits(s, win, 3, &v)) return inf_fail(s, INF_INPUT);
    s.final_block = v & 1;
    const uint32_t type = v >> 1;
    if (type == 3) return inf_fail(s, INF_BTYPE);
    if (type == 0) {
        s.acc >>= s.nacc & 7, s.nacc -= s.nacc & 7;   // to the byte's end
        uint32_t len = 0, nlen = 0;
        if (!inf_bits(s, win, 16, &len) || !inf_bits(s, win, 16, &nlen)) return inf_fail(s, INF_INPUT);
        if (len != (~nlen & 0xffffu)) return inf_fail(s, INF_STORED_LEN);
        const uint32_t at = s.pos - s.nacc / 8;   // (nacc is whole bytes now: the bytes in acc go back)
        if (len > n - at) return inf_fail(s, INF_INPUT);           // (at <= pos <= n)
        if (len > isize - s.produced) return inf_fail(s, INF_OUTPUT);   // (produced <= isize)
        s.acc = 0, s.nacc = 0, s.pos = at;
        s.stored_src = at, s.stored_len = len, s.phase = INF_PH_STORED;
        return;
    }
    if (type == 1) {
        for (int k = 0; k < 144; ++k) s.lens[k] = 8;
        for (int k = 144; k < 256; ++k) s.lens[k] = 9;
        for (int k = 256; k < 280; ++k) s.lens[k] = 7;
        for (int k = 280; k < 288; ++k) s.lens[k] = 8;
        for (int k = 0; k < 32; ++k) s.lens[288 + k] = 5;
        s.nlen = 288, s.ndist = 32;
    } else {
        uint32_t hlit = 0, hdist = 0, hclen = 0;
        if (!inf_bits(s, win, 5, &hlit) || !inf_bits(s, win, 5, &hdist) || !inf_bits(s, win, 4, &hclen)) return inf_fail(s, INF_INPUT);
        s.nlen = hlit + 257, s.ndist = hdist + 1;
        if (s.nlen > 286 || s.ndist > 30) return inf_fail(s, INF_SYMBOL);
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint8_t cl[19];
        for (int k = 0; k < 19; ++k) cl[k] = 0;
        for (uint32_t k = 0; k < hclen + 4; ++k) {
            if (!inf_bits(s, win, 3, &v)) return inf_fail(s, INF_INPUT);
            cl[order[k]] = static_cast<uint8_t>(v);
        }
        // the code-length code borrows the distance code's arrays: they are made after it has served
        const int rc = inf_code_prepare(s.d, cl, 19, INF_KIND_CODES);
        if (rc != INF_OK) return inf_fail(s, rc);
        const uint32_t total = s.nlen + s.ndist;   // <= 316
        uint32_t have = 0;
        while (have < total) {
            const int sym = inf_decode_slow(s, win, s.d.count, s.d.symbol, 7);
            if (sym < 0) return inf_fail(s, -sym);
            if (sym < 16) {
                s.lens[have++] = static_cast<uint8_t>(sym);
                continue;
            }
            uint32_t rep = 0, val = 0;
            if (sym == 16) {
                if (have == 0) return inf_fail(s, INF_REPEAT);
                if (!inf_bits(s, win, 2, &rep)) return inf_fail(s, INF_INPUT);
                val = s.lens[have - 1], rep += 3;
            } else if (sym == 17) {
                if (!inf_bits(s, win, 3, &rep)) return inf_fail(s, INF_INPUT);
                rep += 3;
            } else {
                if (!inf_bits(s, win, 7, &rep)) return inf_fail(s, INF_INPUT);
                rep += 11;
            }
            if (rep > total - have) return inf_fail(s, INF_REPEAT);
            for (; rep; --rep) s.lens[have++] = static_cast<uint8_t>(val);
        }
        if (s.lens[256] == 0) return inf_fail(s, INF_NO_EOB);
        // the distance lengths to their place behind 288 literal/length lengths (from the top: the ranges may overlap)
        for (uint32_t k = s.ndist; k-- > 0;) s.lens[288 + k] = s.lens[s.nlen + k];
    }
    int rc = inf_code_prepare(s.ll, s.lens, static_cast<int>(s.nlen), INF_KIND_LENS);
    if (rc == INF_OK) rc = inf_code_prepare(s.d, s.lens + 288, static_cast<int>(s.ndist), INF_KIND_DISTS);
    if (rc != INF_OK) return inf_fail(s, rc);
    s.phase = INF_PH_CLEAR;
}

// ---- SYMBOLS (lane 0) ----
NPR_INF_FN void inf_symbols(Inflate &s, const uint8_t *win, uint32_t n, uint8_t *out, uint32_t isize) {
    for (;;) {
        if (s.steps == 0) return inf_fail(s, INF_BOUND);
        --s.steps;
        if (s.win_hi < n && s.pos + INF_SYMBOL_BYTES > s.win_hi) return;   // the window runs low: the loop refills it
        const int sym = inf_decode(s, win, s.ll);
        if (sym < 0) return inf_fail(s, -sym);
        if (sym < 256) {
            if (s.produced >= isize) return inf_fail(s, INF_OUTPUT);
            out[s.produced++] = static_cast<uint8_t>(sym);
            continue;
        }
        if (sym == 256) {
            s.phase = s.final_block ? INF_PH_FINISH : INF_PH_HEADER;
            return;
        }
        if (sym >= 286) return inf_fail(s, INF_SYMBOL);
        uint32_t len, extra = 0, k = static_cast<uint32_t>(sym) - 257;   // RFC 1951 3.2.5
        if (k < 8) {
            len = 3 + k;
        } else if (k == 28) {
            len = 258;
        } else {
            const uint32_t eb = k / 4 - 1;
            if (!inf_bits(s, win, eb, &extra)) return inf_fail(s, INF_INPUT);
            len = 3 + ((4 + (k & 3)) << eb) + extra;
        }
        const int dsym = inf_decode(s, win, s.d);
        if (dsym < 0) return inf_fail(s, -dsym);
        if (dsym >= 30) return inf_fail(s, INF_SYMBOL);
        uint32_t dist;
        if (dsym < 4) {
            dist = 1 + static_cast<uint32_t>(dsym);
        } else {
            const uint32_t eb = static_cast<uint32_t>(dsym) / 2 - 1;
            if (!inf_bits(s, win, eb, &extra)) return inf_fail(s, INF_INPUT);
            dist = 1 + ((2 + (static_cast<uint32_t>(dsym) & 1)) << eb) + extra;
        }
        if (dist > s.produced) return inf_fail(s, INF_DISTANCE);
        if (len > isize - s.produced) return inf_fail(s, INF_OUTPUT);
        for (uint32_t j = 0; j < len; ++j, ++s.produced) out[s.produced] = out[s.produced - dist];   // (byte by byte: a match may overlap its output)
    }
}

NPR_INF_FN void inf_finish(Inflate &s, uint32_t n, uint32_t isize) {
    const uint32_t used = s.pos - s.nacc / 8;   // whole bytes in the bit buffer were not used
    if (used != n) return inf_fail(s, INF_TRAILING);
    if (s.produced != isize) return inf_fail(s, INF_ISIZE);
    s.status = INF_OK, s.phase = INF_PH_DONE;
}

// The deflate data body[0, n) into out[0, isize), by `lanes` callers with lane = 0 .. lanes - 1 that all call with the same arguments and
// meet at sync().  s, win[0, win_cap) and out are shared by them (LDS on the device); win_cap >= 2 * INF_MARGIN.  On return (after a last
// sync) s.status and s.produced are final: INF_OK means the data ended exactly at n with exactly isize bytes produced.
template <typename Sync>
NPR_INF_FN void inflate_member(Inflate &s, const uint8_t *body, uint32_t n, uint8_t *out, uint32_t isize, uint8_t *win, uint32_t win_cap, uint32_t lane,
                               uint32_t lanes, Sync sync) {
    if (lane == 0) {
        s.acc = 0, s.nacc = 0, s.pos = 0, s.win_lo = 0, s.win_hi = 0, s.produced = 0, s.status = INF_OK, s.phase = INF_PH_HEADER, s.final_block = 0;
        s.steps = 8 * n + isize + 64;   // a step of SYMBOLS consumes a bit or ends the phase
        s.stored_src = 0, s.stored_len = 0, s.nlen = 0, s.ndist = 0;
        if (isize > INF_MAX_ISIZE) inf_fail(s, INF_ISIZE);
    }
    // a block of deflate data takes at least 10 bits and at most four phases, a refill comes after INF_MARGIN - INF_SYMBOL_BYTES bytes at the earliest
    const uint32_t rounds = 4 * n + 64;
    for (uint32_t round = 0;; ++round) {
        sync();
        const uint32_t phase = s.phase, pos = s.pos, win_hi = s.win_hi, src = s.stored_src, len = s.stored_len, produced = s.produced;
        sync();   // every lane has read the state: lane 0 may change it
        if (phase == INF_PH_DONE) break;
        if (round >= rounds) {
            if (lane == 0) inf_fail(s, INF_BOUND);
            continue;
        }
        if (phase != INF_PH_STORED && win_hi < n && pos + INF_MARGIN > win_hi) {
            const uint32_t hi = n - pos < win_cap ? n : pos + win_cap;   // (pos <= win_hi < n)
            for (uint32_t k = pos + lane; k < hi; k += lanes) win[k - pos] = body[k];
            if (lane == 0) s.win_lo = pos, s.win_hi = hi;
            sync();
        }
        switch (phase) {
        case INF_PH_HEADER:
            if (lane == 0) inf_header(s, win, n, isize);
            break;
        case INF_PH_STORED:   // (src + len <= n and produced + len <= isize: inf_header)
            for (uint32_t k = lane; k < len; k += lanes) out[produced + k] = body[src + k];
            if (lane == 0) {
                s.produced = produced + len, s.pos = src + len;
                s.win_lo = s.pos, s.win_hi = s.pos;   // an empty window at the data's next byte
                s.phase = s.final_block ? INF_PH_FINISH : INF_PH_HEADER;
            }
            break;
        case INF_PH_CLEAR:
            inf_code_clear(s.ll, lane, lanes), inf_code_clear(s.d, lane, lanes);
            if (lane == 0) s.phase = INF_PH_FILL;
            break;
        case INF_PH_FILL:
            inf_code_fill(s.ll, lane, lanes), inf_code_fill(s.d, lane, lanes);
            if (lane == 0) s.phase = INF_PH_SYMBOLS;
            break;
        case INF_PH_SYMBOLS:
            if (lane == 0) inf_symbols(s, win, n, out, isize);
            break;
        default:
            if (lane == 0) inf_finish(s, n, isize);
            break;
        }
    }
}

}  // namespace npr
#endif
