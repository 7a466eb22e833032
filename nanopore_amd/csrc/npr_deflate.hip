// npr_deflate.hip -- BGZF blocks whose deflate data is compressed, on the device (the layout, the choice rule and the virtual offsets:
// include/nprealign.h, npr_bgzf_deflate; the host side: npr_bam_api.cpp).  Integers only; nothing depends on the order in which threads or
// atomics land, so the output is the same bytes from run to run.
//   k_bgzf_deflate   one workgroup of 256 threads compresses one BGZF block (block b = the payload bytes [b P, min(len, (b + 1) P)), as in the
//                    stored layout) into its slot of DEFLATE_SLOT bytes, as one final block of raw DEFLATE (RFC 1951), in these steps:
//     payload        into LDS; its CRC-32 (bgzf_crc, shared with k_bgzf_frame).
//     matches        in rounds of 256 consecutive positions, one a thread.  A position p with three bytes left reads the table entry of the
//                    hash of its three bytes, then -- after a barrier -- enters itself with atomicMax(p + 1): what a round reads is what the
//                    rounds before it left, the largest position of that hash, whatever order the atomics took.  The candidates of p are that
//                    position and p - 1 (which finds a run at its second byte); the longer match wins, on a tie the nearer; a match is 3 ..
//                    258 bytes, at most 32 768 back, lies in the block and ends with it at the latest.
//     parse          greedy from position 0 by one thread: a match where the position has one, else a literal (a bit per token start).
//     counts         literal/length and distance symbols of that parse, and of the literals alone, with LDS atomics (a count does not depend
//                    on their order).
//     codes          per alphabet the used symbols ordered by (count, symbol) by all threads (a rank each), then one thread an alphabet:
//                    huff_build, huff_codes (npr_huff.h).  The code-length alphabet of each of the two candidates the same way; the code
//                    lengths are sent one by one (no symbols 16 / 17 / 18).
//     choice         the exact bits of (a) dynamic Huffman over matches and literals, (b) dynamic Huffman over the literals alone, (c) stored;
//                    the smallest is emitted, on a tie the later.  So a block never exceeds L + 31 bytes.
//     emission       thread t takes the positions [255 t, 255 t + 255); thread 0 also the block's header, thread 255 the end-of-block code.  A
//                    prefix sum of the threads' bits gives each its first bit; a thread stores the bytes whose first bit is its own, hands
//                    the bits it has in a byte begun by another to that byte's owner through LDS, and the owner stores the byte once.
//   the scan         launch_scan_tiled over the blocks' lengths: block_off[0 .. blocks]
//   k_bgzf_pack      block b from its slot to block_off[b]; one more workgroup writes the end-of-file block at block_off[blocks].
// LDS of k_bgzf_deflate (one workgroup a CU): payload 65 280 + match lengths 65 280 + match bits 8 160 + a region of 24 KiB that holds, in turn,
// the CRC's tables, the hash table (4 096 entries), and the token bits, counts, codes and hand-over bytes.
#include <hip/hip_runtime.h>

#include "npr_bgzf.h"
#include "npr_device.h"
#include "npr_huff.h"

namespace npr {
namespace {

constexpr int THREADS = BGZF_THREADS;
constexpr int HASH_BITS = 12, HASH_SIZE = 1 << HASH_BITS;
constexpr int BIT_WORDS = BGZF_PAYLOAD / 32;  // 2040: BGZF_PAYLOAD is a multiple of 32
static_assert(BGZF_PAYLOAD % 32 == 0 && BGZF_SLICE * THREADS == BGZF_PAYLOAD, "slices and bit words tile the payload");

// byte offsets in LDS
constexpr int O_PAY = 0, O_LENB = O_PAY + BGZF_PAYLOAD, O_HASM = O_LENB + BGZF_PAYLOAD, O_REGION = O_HASM + 4 * BIT_WORDS;
constexpr int REGION = 24576;
constexpr int LDS_BYTES = O_REGION + REGION;
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup's LDS");
// the region while the codes are made and the block is emitted
constexpr int R_TOK = 0;                                   // uint32 [BIT_WORDS] token starts
constexpr int R_CNT_A = R_TOK + 4 * BIT_WORDS;             // uint32 [286] literal/length counts of (a)
constexpr int R_CNT_B = R_CNT_A + 4 * DEFLATE_LL;          // uint32 [286] of (b)
constexpr int R_CNT_D = R_CNT_B + 4 * DEFLATE_LL;          // uint32 [32] distance counts
constexpr int R_CNT_CL = R_CNT_D + 4 * 32;                 // uint32 [2][32] code-length counts of (a), (b)
constexpr int R_WORK_A = R_CNT_CL + 4 * 64;                // uint32 [3][288] sorted counts
constexpr int R_WORK_S = R_WORK_A + 4 * 3 * 288;           // uint16 [3][288] sorted symbols
constexpr int R_LEN = R_WORK_S + 2 * 3 * 288;              // uint8: ll (a) [288], ll (b) [288], d [32], cl (a) [32], cl (b) [32]
constexpr int R_CODE = R_LEN + 288 + 288 + 32 + 32 + 32;   // uint16, the same order
constexpr int R_SCAN = R_CODE + 2 * (288 + 288 + 32 + 32 + 32);  // uint32 [256]
constexpr int R_LEAD = R_SCAN + 4 * THREADS;               // uint32 [256] hand-over bytes
constexpr int R_MISC = R_LEAD + 4 * THREADS;               // uint32 [16]
constexpr int R_END = R_MISC + 4 * 16;
static_assert(R_END <= REGION && 4 * HASH_SIZE <= REGION && R_CNT_A % 4 == 0 && R_CODE % 2 == 0 && R_SCAN % 4 == 0, "the region's layout");
enum { M_EXTRA = 0, M_BITS_A, M_BITS_B, M_HDR_A, M_HDR_B, M_HLIT_A, M_HLIT_B, M_HDIST_A, M_HCLEN_A, M_HCLEN_B, M_USED0, M_USED1, M_USED2 };
constexpr uint32_t LEAD_NONE = 0xFFFFFFFFu, LEAD_EMPTY = 0xFFFFFFFEu;

__device__ __forceinline__ uint32_t hash3(const uint8_t *p) {
    const uint32_t v = p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16;
    return (v * 0x9E3779B1u) >> (32 - HASH_BITS);
}

__device__ __forceinline__ uint32_t match_len(const uint8_t *pay, uint32_t q, uint32_t p, uint32_t max_len) {
    uint32_t n = 0;
    while (n < max_len && pay[q + n] == pay[p + n]) ++n;
    return n;
}

// the used symbols of cnt[0 .. n) ordered by (count, symbol), a rank a thread (all threads call)
__device__ __forceinline__ void rank_sort(const uint32_t *cnt, int n, uint32_t *A, uint16_t *S) {
    for (int s = threadIdx.x; s < n; s += THREADS) {
        const uint32_t c = cnt[s];
        if (!c) continue;
        int r = 0;
        for (int s2 = 0; s2 < n; ++s2) {
            const uint32_t c2 = cnt[s2];
            r += (c2 && (c2 < c || (c2 == c && s2 < s))) ? 1 : 0;
        }
        A[r] = c, S[r] = static_cast<uint16_t>(s);
    }
}
__device__ __forceinline__ int count_used(const uint32_t *cnt, int n) {
    int used = 0;
    for (int s = 0; s < n; ++s) used += cnt[s] ? 1 : 0;
    return used;
}

// a thread's part of the deflate data: bits [first, ...) of the block; bytes begun by this thread are stored, the bits in a byte begun by
// another are kept in `lead`, and the byte the thread leaves unfinished in `tail`
struct BitWriter {
    uint8_t *out;
    unsigned long long acc;
    uint32_t byte, n_bits;
    bool owns;      // the byte being filled began with this thread's bits
    uint32_t lead;  // index << 8 | bits, or LEAD_NONE
    __device__ __forceinline__ void begin(uint8_t *o, uint32_t first) {
        out = o, acc = 0, byte = first >> 3, n_bits = first & 7, owns = (first & 7) == 0, lead = LEAD_NONE;
    }
    __device__ __forceinline__ void put(uint32_t bits, uint32_t n) {
        acc |= static_cast<unsigned long long>(bits) << n_bits;
        n_bits += n;
        while (n_bits >= 8) {
            const uint32_t v = static_cast<uint32_t>(acc & 0xff);
            if (owns) out[byte] = static_cast<uint8_t>(v);
            else lead = byte << 8 | v;
            owns = true, ++byte, acc >>= 8, n_bits -= 8;
        }
    }
};

__global__ void __launch_bounds__(THREADS) k_bgzf_deflate(DeflateArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    uint8_t *const pay = lds + O_PAY;
    uint8_t *const lenb = lds + O_LENB;
    uint32_t *const hasm = reinterpret_cast<uint32_t *>(lds + O_HASM);
    uint8_t *const reg = lds + O_REGION;
    uint32_t *const hash = reinterpret_cast<uint32_t *>(reg);
    uint32_t *const tok = reinterpret_cast<uint32_t *>(reg + R_TOK);
    uint32_t *const cnt_a = reinterpret_cast<uint32_t *>(reg + R_CNT_A);
    uint32_t *const cnt_b = reinterpret_cast<uint32_t *>(reg + R_CNT_B);
    uint32_t *const cnt_d = reinterpret_cast<uint32_t *>(reg + R_CNT_D);
    uint32_t *const cnt_cl = reinterpret_cast<uint32_t *>(reg + R_CNT_CL);
    uint32_t *const work_a = reinterpret_cast<uint32_t *>(reg + R_WORK_A);
    uint16_t *const work_s = reinterpret_cast<uint16_t *>(reg + R_WORK_S);
    uint8_t *const len_a = reg + R_LEN, *const len_b = len_a + 288, *const len_d = len_b + 288, *const len_cla = len_d + 32, *const len_clb = len_cla + 32;
    uint16_t *const code_a = reinterpret_cast<uint16_t *>(reg + R_CODE);
    uint16_t *const code_b = code_a + 288, *const code_d = code_b + 288, *const code_cla = code_d + 32, *const code_clb = code_cla + 32;
    uint32_t *const scan = reinterpret_cast<uint32_t *>(reg + R_SCAN);
    uint32_t *const lead = reinterpret_cast<uint32_t *>(reg + R_LEAD);
    uint32_t *const misc = reinterpret_cast<uint32_t *>(reg + R_MISC);

    const uint32_t t = threadIdx.x;
    const int64_t blocks = (a.z.len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    uint16_t *const dist = a.dist + static_cast<int64_t>(blockIdx.x) * BGZF_PAYLOAD;
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint8_t *const in = a.z.data + b * BGZF_PAYLOAD;
        uint8_t *const out = a.z.out + b * DEFLATE_SLOT;
        const uint32_t L = static_cast<uint32_t>(a.z.len - b * BGZF_PAYLOAD < BGZF_PAYLOAD ? a.z.len - b * BGZF_PAYLOAD : BGZF_PAYLOAD);
        __syncthreads();  // the block before is done with the LDS
        for (uint32_t k = t; k < L; k += THREADS) pay[k] = in[k];
        for (uint32_t k = t; k < BIT_WORDS; k += THREADS) hasm[k] = 0;
        __syncthreads();
        const uint32_t crc = bgzf_crc(pay, L, a.z, hash, hash + 256, hash + 512);

        // ---- matches
        for (uint32_t k = t; k < HASH_SIZE; k += THREADS) hash[k] = 0;
        __syncthreads();
        const uint32_t rounds = (L + THREADS - 1) / THREADS;
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t p = r * THREADS + t;
            const bool can = p + DEFLATE_MIN_MATCH <= L;
            uint32_t h = 0, cand = 0;
            if (can) h = hash3(pay + p), cand = hash[h];
            __syncthreads();
            if (can) {
                atomicMax(&hash[h], p + 1);
                const uint32_t max_len = min(static_cast<uint32_t>(DEFLATE_MAX_MATCH), L - p);
                uint32_t best = 0, best_d = 0;
                if (p >= 1) {
                    best = match_len(pay, p - 1, p, max_len), best_d = 1;
                }
                if (cand) {
                    const uint32_t d = p - (cand - 1);
                    if (d > 1 && d <= DEFLATE_WINDOW) {
                        const uint32_t n = match_len(pay, p - d, p, max_len);
                        if (n > best) best = n, best_d = d;
                    }
                }
                if (best >= DEFLATE_MIN_MATCH) {
                    lenb[p] = static_cast<uint8_t>(best - DEFLATE_MIN_MATCH);
                    atomicOr(&hasm[p >> 5], 1u << (p & 31));
                    dist[p] = static_cast<uint16_t>(best_d - 1);
                }
            }
            __syncthreads();
        }

        // ---- the parse; the counts
        for (uint32_t k = t; k < (R_END - R_TOK) / 4; k += THREADS) tok[k] = 0;  // token bits, counts, lengths, codes, misc
        __syncthreads();
        if (t == 0) {
            uint32_t p = 0;
            while (p < L) {
                tok[p >> 5] |= 1u << (p & 31);
                p += ((hasm[p >> 5] >> (p & 31)) & 1) ? lenb[p] + DEFLATE_MIN_MATCH : 1u;
            }
        }
        __syncthreads();
        {
            uint32_t extra = 0;
            for (uint32_t p = t; p < L; p += THREADS) {
                const uint32_t c = pay[p];
                atomicAdd(&cnt_b[c], 1u);
                if (!((tok[p >> 5] >> (p & 31)) & 1)) continue;
                if ((hasm[p >> 5] >> (p & 31)) & 1) {
                    const DeflateSym ls = deflate_length_sym(lenb[p] + DEFLATE_MIN_MATCH), ds = deflate_dist_sym(dist[p] + 1u);
                    atomicAdd(&cnt_a[ls.sym], 1u), atomicAdd(&cnt_d[ds.sym], 1u);
                    extra += ls.extra_bits + ds.extra_bits;
                } else {
                    atomicAdd(&cnt_a[c], 1u);
                }
            }
            if (t == 0) atomicAdd(&cnt_a[256], 1u), atomicAdd(&cnt_b[256], 1u);
            if (extra) atomicAdd(&misc[M_EXTRA], extra);
        }
        __syncthreads();

        // ---- the codes
        rank_sort(cnt_a, DEFLATE_LL, work_a, work_s);
        rank_sort(cnt_b, DEFLATE_LL, work_a + 288, work_s + 288);
        rank_sort(cnt_d, DEFLATE_D, work_a + 576, work_s + 576);
        __syncthreads();
        if (t == 0) {
            huff_build(work_a, work_s, count_used(cnt_a, DEFLATE_LL), DEFLATE_LL, 15, len_a);
            huff_codes(len_a, DEFLATE_LL, 15, code_a);
        } else if (t == 64) {
            huff_build(work_a + 288, work_s + 288, count_used(cnt_b, DEFLATE_LL), DEFLATE_LL, 15, len_b);
            huff_codes(len_b, DEFLATE_LL, 15, code_b);
        } else if (t == 128) {
            huff_build(work_a + 576, work_s + 576, count_used(cnt_d, DEFLATE_D), DEFLATE_D, 15, len_d);
            huff_codes(len_d, DEFLATE_D, 15, code_d);
        }
        __syncthreads();
        if (t == 0 || t == 64) {  // the header of (a) and of (b): HLIT, HDIST, the code-length code, HCLEN; the candidate's bits
            const bool is_a = t == 0;
            const uint8_t *const ll = is_a ? len_a : len_b;
            const uint32_t *const cnt = is_a ? cnt_a : cnt_b;
            uint32_t *const ccl = cnt_cl + (is_a ? 0 : 32);
            uint8_t *const lcl = is_a ? len_cla : len_clb;
            uint32_t *const wa = work_a + (is_a ? 0 : 288);
            uint16_t *const ws = work_s + (is_a ? 0 : 288);
            int hlit = DEFLATE_LL, hdist = 1;
            while (hlit > 257 && ll[hlit - 1] == 0) --hlit;
            if (is_a) {
                hdist = DEFLATE_D;
                while (hdist > 1 && len_d[hdist - 1] == 0) --hdist;
            }
            for (int s = 0; s < hlit; ++s) ++ccl[ll[s]];
            for (int s = 0; s < hdist; ++s) ++ccl[is_a ? len_d[s] : 0];
            const int used = huff_sort_serial(ccl, DEFLATE_CL, wa, ws);
            huff_build(wa, ws, used, DEFLATE_CL, 7, lcl);
            huff_codes(lcl, DEFLATE_CL, 7, is_a ? code_cla : code_clb);
            int hclen = DEFLATE_CL;
            while (hclen > 4 && lcl[deflate_cl_order(hclen - 1)] == 0) --hclen;
            uint32_t hdr = 3 + 5 + 5 + 4 + 3 * hclen, bits = 0;
            for (int s = 0; s < DEFLATE_CL; ++s) hdr += ccl[s] * lcl[s];
            for (int s = 0; s < DEFLATE_LL; ++s) bits += cnt[s] * ll[s];
            if (is_a) {
                for (int s = 0; s < DEFLATE_D; ++s) bits += cnt_d[s] * len_d[s];
                bits += misc[M_EXTRA];
            }
            misc[is_a ? M_HDR_A : M_HDR_B] = hdr, misc[is_a ? M_BITS_A : M_BITS_B] = hdr + bits;
            misc[is_a ? M_HLIT_A : M_HLIT_B] = hlit, misc[is_a ? M_HCLEN_A : M_HCLEN_B] = hclen;
            if (is_a) misc[M_HDIST_A] = hdist;
        }
        __syncthreads();

        // ---- the choice
        const uint32_t bits_c = 8 * L + 40;  // 3 bits, the rest of their byte, LEN and its complement, the payload
        int mode = 0;
        uint32_t bits = misc[M_BITS_A];
        if (misc[M_BITS_B] <= bits) mode = 1, bits = misc[M_BITS_B];
        if (bits_c <= bits) mode = 2, bits = bits_c;

        // ---- the emission
        uint8_t *const z = out + 18;
        uint32_t total = bits;
        if (mode < 2) {
            const bool is_a = mode == 0;
            const uint8_t *const ll = is_a ? len_a : len_b, *const lcl = is_a ? len_cla : len_clb;
            const uint16_t *const cll = is_a ? code_a : code_b, *const ccl = is_a ? code_cla : code_clb;
            const uint32_t lo = min(L, t * BGZF_SLICE), hi = min(L, lo + BGZF_SLICE);
            uint32_t mine = 0;
            for (uint32_t p = lo; p < hi; ++p) {
                if (!is_a) {
                    mine += ll[pay[p]];
                } else if ((tok[p >> 5] >> (p & 31)) & 1) {
                    if ((hasm[p >> 5] >> (p & 31)) & 1) {
                        const DeflateSym ls = deflate_length_sym(lenb[p] + DEFLATE_MIN_MATCH), ds = deflate_dist_sym(dist[p] + 1u);
                        mine += ll[ls.sym] + ls.extra_bits + len_d[ds.sym] + ds.extra_bits;
                    } else {
                        mine += ll[pay[p]];
                    }
                }
            }
            if (t == 0) mine += misc[is_a ? M_HDR_A : M_HDR_B];
            if (t == THREADS - 1) mine += ll[256];
            scan[t] = mine;
            __syncthreads();
            for (uint32_t step = 1; step < THREADS; step <<= 1) {  // inclusive prefix sum
                const uint32_t v = t >= step ? scan[t - step] : 0;
                __syncthreads();
                scan[t] += v;
                __syncthreads();
            }
            total = scan[THREADS - 1];
            const uint32_t first = scan[t] - mine;
            if (total == bits) {  // (else a defect: nothing is written from a count that disagrees; below)
                BitWriter w;
                w.begin(z, first);
                if (t == 0) {
                    const int hlit = misc[is_a ? M_HLIT_A : M_HLIT_B], hdist = is_a ? misc[M_HDIST_A] : 1, hclen = misc[is_a ? M_HCLEN_A : M_HCLEN_B];
                    w.put(5, 3);  // BFINAL 1, BTYPE 10
                    w.put(hlit - 257, 5), w.put(hdist - 1, 5), w.put(hclen - 4, 4);
                    for (int k = 0; k < hclen; ++k) w.put(lcl[deflate_cl_order(k)], 3);
                    for (int s = 0; s < hlit; ++s) w.put(ccl[ll[s]], lcl[ll[s]]);
                    for (int s = 0; s < hdist; ++s) {
                        const int l = is_a ? len_d[s] : 0;
                        w.put(ccl[l], lcl[l]);
                    }
                }
                for (uint32_t p = lo; p < hi; ++p) {
                    if (!is_a) {
                        w.put(cll[pay[p]], ll[pay[p]]);
                    } else if ((tok[p >> 5] >> (p & 31)) & 1) {
                        if ((hasm[p >> 5] >> (p & 31)) & 1) {
                            const DeflateSym ls = deflate_length_sym(lenb[p] + DEFLATE_MIN_MATCH), ds = deflate_dist_sym(dist[p] + 1u);
                            w.put(cll[ls.sym], ll[ls.sym]), w.put(ls.extra, ls.extra_bits);
                            w.put(code_d[ds.sym], len_d[ds.sym]), w.put(ds.extra, ds.extra_bits);
                        } else {
                            w.put(cll[pay[p]], ll[pay[p]]);
                        }
                    }
                }
                if (t == THREADS - 1) w.put(cll[256], ll[256]);
                // the unfinished byte: this thread's to store when it began it, else all its bits lie in a byte of another's
                const uint32_t rest = static_cast<uint32_t>(w.acc & 0xff);
                const bool tail = w.n_bits > 0 && w.owns;
                if (w.n_bits > 0 && !w.owns) w.lead = w.byte << 8 | rest;
                lead[t] = mine ? w.lead : LEAD_EMPTY;
                __syncthreads();
                if (tail) {
                    uint32_t v = rest;
                    for (uint32_t u = t + 1; u < THREADS; ++u) {
                        const uint32_t ld = lead[u];
                        if (ld == LEAD_EMPTY) continue;
                        if (ld == LEAD_NONE || (ld >> 8) != w.byte) break;
                        v |= ld & 0xff;
                    }
                    z[w.byte] = static_cast<uint8_t>(v);
                }
            } else {
                mode = 3;
            }
        }
        if (mode >= 2) {  // stored
            total = bits_c;
            if (t == 0) z[0] = 1, put16(z + 1, L), put16(z + 3, ~L & 0xffffu);
            for (uint32_t k = t; k < L; k += THREADS) z[5 + k] = pay[k];
        }
        if (t == 0) {
            const uint32_t n = (total + 7) / 8;
            bgzf_put_header(out, n + 26);
            put32(z + n, crc), put32(z + n + 4, L);
            a.block_len[b] = n + 26;
            atomicAdd(&a.chosen[mode], 1u);
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_bgzf_pack(DeflateArgs a) {
    const int64_t blocks = (a.z.len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    const int64_t b = blockIdx.x;
    uint8_t *const to = a.packed + a.block_len[b];  // (the scan has made offsets of the lengths)
    if (b >= blocks) {
        bgzf_put_eof(to, threadIdx.x);
        return;
    }
    const uint8_t *const from = a.z.out + b * DEFLATE_SLOT;
    const int64_t n = a.block_len[b + 1] - a.block_len[b];
    for (int64_t k = threadIdx.x; k < n; k += THREADS) to[k] = from[k];
}

}  // namespace

int launch_bgzf_deflate(const DeflateArgs &a, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = (a.z.len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
    if (blocks > 0) hipLaunchKernelGGL(k_bgzf_deflate, dim3(static_cast<unsigned>(deflate_groups(blocks))), dim3(THREADS), 0, st, a);
    const int rc = launch_scan_tiled<int64_t, int64_t>(a.block_len, a.block_len, blocks, a.tile, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bgzf_pack, dim3(static_cast<unsigned>(blocks + 1)), dim3(THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
