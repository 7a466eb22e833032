// npr_seed.hip -- k_seed_encode, k_seed_bucket_count / k_seed_tile_sums / k_seed_scan_tiles / k_seed_scan_apply / k_seed_bucket_fill, k_seed_match:
// the maximal exact matches of reads against a set of reference sequences, the local hits a base mapper hands to chainSamFile
// (nanopore_amd/mappers/seedMapper.py; the definition: include/nprealign.h, "exact-match seeding").
//
// A match is (a, b, L): reference bases a .. a + L equal read bases b .. b + L, not extendable to either side, L >= min_len >= k; a base
// outside ACGT equals nothing.  Position pair (i, j) starts a match exactly when the bases before it differ (or one sequence starts there)
// and the bases from it on agree for min_len or more -- so every match is found once, at its left end, and nothing needs a second look.
// Both sides lie in code buffers (npr_device.h, SeedEncodeArgs): bases 0..3, every other byte a value only its own side has and a
// separator around every sequence, so "the bytes are equal" is "the bases match", an extension compares eight bytes at a time (xor, count
// the trailing zero bits) and stops at a separator at the latest without a length in sight, and the base before a sequence's first one is
// a separator that differs from everything.  k_seed_encode makes the buffers from ASCII, the reads' reverse complements included (a
// reverse-strand match is a match of the same kernel against that second buffer; b counts in its orientation, as a FLAG 16 record's does).
// The index: every reference position whose k bases are all ACGT, bucketed by its first kb = min(k, 12) bases (4^kb + 1 int32 counters:
// 64 MB at kb = 12): count, exclusive scan in place, fill -- the fill's atomic adds turn the table of bucket starts into the table of
// bucket ENDS, and bucket `key` begins where bucket key - 1 ends: one table, no copy.  The order inside a bucket is whatever the atomics
// gave; it decides the order matches are found in, not which, and the caller sorts a read's matches.
// k_seed_match: a lane owns a read position, forms its bucket's key, and walks the bucket: left check (one byte each side), extension
// from the position itself (which re-checks the kb bases the bucket promises and the other k - kb), keep if L >= min_len.  It runs twice
// over the same work: counting (one atomic add per lane with matches into its read's counter) and, after the host has summed the counters
// into the reads' ranges, emitting (one atomic add per match for its row, one 16-byte store).
// A LONG BUCKET MAKES ONE LANE SLOW: a homopolymer run of the reference puts hundreds of positions into one bucket and a read position
// with that key walks all of them while its 63 neighbours wait.  That is accepted here; there is no cap on a bucket's occurrences, because
// one would change the result set.
// Block shape (chosen before any measurement; the reasons are arithmetic; no kernel here has been timed on hardware):
//   256 threads, no LDS but the scan's four wave sums, a handful of registers: nothing limits residency but the 32 waves of a CU.
//   k_seed_match starts one lane per byte of the read buffer and no grid-stride loop: the work of a lane is between nothing (no window, an
//   empty bucket: at 16.7 M buckets a megabase reference fills 6 % of them) and a bucket walk, so many short workgroups let the
//   dispatcher even out what a fixed assignment would not.  The loads of a walk are scattered (pos[s], then 8-byte pieces of the reference
//   around it): the reference and its table are read-only and stay in L2 / the Infinity Cache for any reference this project has met
//   (a 4.6 Mb contig: 4.6 MB of codes, 18 MB of positions, 64 MB of table).
//   k_seed_encode gives a lane 16 consecutive bytes of the buffer (one search for the first one's sequence, one 16-byte store); the bytes
//   of the reverse complement leave one by one (they run backwards).
//   The scan: 4096 entries per workgroup (16 per lane as four 16-byte loads), tile sums, one workgroup over the at most 4097 tile sums,
//   then the tiles again.  Three launches over 64 MB: a few tens of microseconds at the HBM rate, once per reference.  The unit keeps these
//   kernels of its own on npr_scan.h's block_scan_exclusive: launch_scan_tiled (8 bounds-checked entries per lane) made npr_seed_index_create
//   0.07 ms slower on a 4.6 Mb reference (profiles/scan_refactor_time.json), and the whole-tile padding of the table stays with them.
#include <hip/hip_runtime.h>

#include "npr_device.h"
#include "npr_scan.h"

namespace npr {
namespace {

constexpr int THREADS = 256;
constexpr int RUN = 16;  // bytes of the code buffer per lane of k_seed_encode
static_assert(NPR_SEED_SCAN_TILE == THREADS * 16 && THREADS == SCAN_THREADS, "a lane of the scan holds four 16-byte pieces of the table");
static_assert(NPR_SEED_PAD >= 32 + 8, "a window load reads 32 bytes from a position, an extension step 8 bytes from a separator");

__device__ __forceinline__ uint64_t load8(const uint8_t *p) {  // (any alignment)
    uint64_t v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

// first position of sequence s in a code buffer
__device__ __forceinline__ int64_t seq_start(const int64_t *off, int64_t s) { return off[s] + s + 1; }
// the last sequence that starts at or before position d >= 1 (n_seqs: d lies in the padding)
__device__ __forceinline__ int64_t seq_of(const int64_t *off, int64_t n_seqs, int64_t d) {
    int64_t lo = 0, hi = n_seqs;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (seq_start(off, mid) <= d) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(THREADS) k_seed_encode(SeedEncodeArgs a) {
    const int64_t d0 = (static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x) * RUN;
    if (d0 >= a.bytes) return;
    int64_t s = seq_of(a.off, a.n_seqs, d0 > 0 ? d0 : 1);
    uint32_t w[RUN / 4] = {};
#pragma unroll
    for (int e = 0; e < RUN; ++e) {
        const int64_t d = d0 + e;
        while (s < a.n_seqs && d >= seq_start(a.off, s + 1)) ++s;
        uint32_t c = a.sep;
        int64_t mirror = d;  // where the byte goes in the buffer of the reverse complements
        if (d > 0 && s < a.n_seqs) {
            const int64_t t = d - seq_start(a.off, s), len = a.off[s + 1] - a.off[s];
            if (t < len) {
                const uint32_t ch = a.ascii[a.off[s] + t] & 0xdfu;  // upper case
                c = ch == 'A' ? 0u : (ch == 'C' ? 1u : (ch == 'G' ? 2u : (ch == 'T' ? 3u : a.other)));
                mirror = d + (len - 1 - 2 * t);
            }
        }
        w[e >> 2] |= c << (8 * (e & 3));
        if (a.rc) a.rc[mirror] = static_cast<uint8_t>(c < 4u ? 3u - c : c);
    }
    *reinterpret_cast<uint4 *>(a.codes + d0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// eight bases 0..3, one per byte, as 16 bits (the first base lowest)
__device__ __forceinline__ uint32_t squeeze(uint64_t w) {
    w &= 0x0303030303030303ull;
    w = (w | (w >> 6)) & 0x000f000f000f000full;
    w = (w | (w >> 12)) & 0x000000ff000000ffull;
    return static_cast<uint32_t>(w | (w >> 24)) & 0xffffu;
}
// the window of k bytes at s: whether all of them are bases, and the bucket of its first kb (32 readable bytes at s)
__device__ __forceinline__ bool window_key(const uint8_t *s, int k, int kb, uint32_t &key) {
    constexpr uint64_t kNoBase = 0xfcfcfcfcfcfcfcfcull;
    const uint64_t w0 = load8(s), w1 = load8(s + 8);
    const int n1 = k >= 16 ? 8 : k - 8;  // (k >= 8: the first word counts whole)
    uint64_t bad = (w0 & kNoBase) | (w1 & kNoBase & (n1 == 8 ? ~0ull : (1ull << (8 * n1)) - 1));
    if (k > 16) {
        const int n2 = k >= 24 ? 8 : k - 16;
        bad |= load8(s + 16) & kNoBase & (n2 == 8 ? ~0ull : (1ull << (8 * n2)) - 1);
    }
    if (k > 24) {
        const int n3 = k - 24;
        bad |= load8(s + 24) & kNoBase & (n3 == 8 ? ~0ull : (1ull << (8 * n3)) - 1);
    }
    key = (squeeze(w0) | (squeeze(w1) << 16)) & ((1u << (2 * kb)) - 1u);
    return bad == 0;
}

template <bool FILL>
__global__ void __launch_bounds__(THREADS) k_seed_bucket(SeedIndexArgs a) {  // FILL = false: k_seed_bucket_count, true: k_seed_bucket_fill
    const int64_t p = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (p >= a.bytes - 32) return;
    uint32_t key;
    if (!window_key(a.codes + p, a.k, a.kb, key)) return;
    const int32_t slot = atomicAdd(&a.table[key], 1);
    if (FILL) a.pos[slot] = static_cast<int32_t>(p);  // (slot < window starts <= bytes: the counts are those of the first pass)
}

__device__ __forceinline__ int32_t load_run(const int32_t *table, int32_t v[16]) {
    const uint4 *p = reinterpret_cast<const uint4 *>(table + (static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x) * 16);
    int32_t sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 u = p[q];
        v[4 * q] = static_cast<int32_t>(u.x), v[4 * q + 1] = static_cast<int32_t>(u.y), v[4 * q + 2] = static_cast<int32_t>(u.z), v[4 * q + 3] = static_cast<int32_t>(u.w);
        sum += v[4 * q] + v[4 * q + 1] + v[4 * q + 2] + v[4 * q + 3];
    }
    return sum;
}

__global__ void __launch_bounds__(THREADS) k_seed_tile_sums(const int32_t *table, int32_t *tile) {
    __shared__ int32_t wave_sum[SCAN_WAVES];
    int32_t v[16], total;
    (void)block_scan_exclusive(load_run(table, v), wave_sum, &total);
    if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

__global__ void __launch_bounds__(THREADS) k_seed_scan_tiles(int32_t *tile, int32_t n_tiles) {  // one workgroup
    __shared__ int32_t wave_sum[SCAN_WAVES];
    const int32_t per = (n_tiles + THREADS - 1) / THREADS;
    const int32_t lo = min(static_cast<int32_t>(threadIdx.x) * per, n_tiles), hi = min(lo + per, n_tiles);
    int32_t sum = 0, total;
    for (int32_t q = lo; q < hi; ++q) sum += tile[q];
    int32_t run = block_scan_exclusive(sum, wave_sum, &total);
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t t = tile[q];
        tile[q] = run;
        run += t;
    }
}

__global__ void __launch_bounds__(THREADS) k_seed_scan_apply(int32_t *table, const int32_t *tile) {
    __shared__ int32_t wave_sum[SCAN_WAVES];
    int32_t v[16], total;
    int32_t run = block_scan_exclusive(load_run(table, v), wave_sum, &total) + tile[blockIdx.x];
    uint4 *p = reinterpret_cast<uint4 *>(table + (static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint4 u;
        u.x = static_cast<uint32_t>(run), run += v[4 * q];
        u.y = static_cast<uint32_t>(run), run += v[4 * q + 1];
        u.z = static_cast<uint32_t>(run), run += v[4 * q + 2];
        u.w = static_cast<uint32_t>(run), run += v[4 * q + 3];
        p[q] = u;
    }
}

template <bool EMIT>
__global__ void __launch_bounds__(THREADS) k_seed_match(SeedMatchArgs a) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
    if (q >= a.bytes - 32) return;
    uint32_t key;
    if (!window_key(a.read + q, a.k, a.kb, key)) return;  // (position 0 is a separator: q >= 1 from here on)
    int32_t s = key ? a.table[key - 1] : 0;
    const int32_t end = a.table[key];
    if (s >= end) return;
    const int64_t r = seq_of(a.read_off, a.n_reads, q);
    if (r >= a.n_reads) return;  // (a window of bases lies inside a read)
    const uint8_t before = a.read[q - 1];
    uint32_t found = 0;
    for (; s < end; ++s) {
        const int64_t p = a.pos[s];
        if (a.ref[p - 1] == before) continue;  // not the left end of its match (a separator or another base: equal to nothing here)
        int64_t len = 0;
        for (;;) {  // (ends at the separator behind either sequence at the latest)
            const uint64_t x = load8(a.ref + p + len) ^ load8(a.read + q + len);
            if (x) {
                len += __builtin_ctzll(x) >> 3;
                break;
            }
            len += 8;
        }
        if (len < a.min_len) continue;
        if (!EMIT) {
            ++found;
        } else {
            const int64_t k = seq_of(a.ref_off, a.n_refs, p);
            const int64_t row = a.hit_off[r] + atomicAdd(&a.count[r], 1u);
            if (row < a.hit_off[r + 1])  // (always: the counting pass saw the same matches)
                *reinterpret_cast<int4 *>(a.hits + 4 * row) =
                    make_int4(static_cast<int32_t>(k), static_cast<int32_t>(p - seq_start(a.ref_off, k)),
                              static_cast<int32_t>(static_cast<uint32_t>(q - seq_start(a.read_off, r)) | (a.strand << 31)), static_cast<int32_t>(len));
        }
    }
    if (!EMIT && found) atomicAdd(&a.count[r], found);
}

inline unsigned blocks_for(int64_t threads) { return static_cast<unsigned>((threads + THREADS - 1) / THREADS); }

}  // namespace

int launch_seed_encode(const SeedEncodeArgs &a, void *stream) {
    hipLaunchKernelGGL(k_seed_encode, dim3(blocks_for(a.bytes / RUN)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_seed_index(const SeedIndexArgs &a, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned tiles = static_cast<unsigned>(seed_table_entries(a.kb) / NPR_SEED_SCAN_TILE);
    hipLaunchKernelGGL(k_seed_bucket<false>, dim3(blocks_for(a.bytes - 32)), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_seed_tile_sums, dim3(tiles), dim3(THREADS), 0, st, a.table, a.tile);
    hipLaunchKernelGGL(k_seed_scan_tiles, dim3(1), dim3(THREADS), 0, st, a.tile, static_cast<int32_t>(tiles));
    hipLaunchKernelGGL(k_seed_scan_apply, dim3(tiles), dim3(THREADS), 0, st, a.table, a.tile);
    hipLaunchKernelGGL(k_seed_bucket<true>, dim3(blocks_for(a.bytes - 32)), dim3(THREADS), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_seed_match(const SeedMatchArgs &a, bool emit, void *stream) {
    if (emit)
        hipLaunchKernelGGL(k_seed_match<true>, dim3(blocks_for(a.bytes - 32)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(k_seed_match<false>, dim3(blocks_for(a.bytes - 32)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
