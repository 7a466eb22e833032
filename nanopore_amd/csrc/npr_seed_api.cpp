// npr_seed_api.cpp -- exact-match seeding: the index of a reference set and the maximal exact matches of reads against it on the device
// (npr_seed.hip), and the matches as the SAM records of a base mapper (host code)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"
#include "npr_textout.h"

#include <array>

namespace npr_impl {

// n ASCII sequences lying back to back on the host (`bases` bytes at `ascii`, offsets off[n + 1] from 0) -> their code buffer on the device, and
// the buffer of their reverse complements when rc is given; d_off receives the offsets
void encode_on_device(const Call &dev, const uint8_t *ascii, const std::vector<int64_t> &off, uint8_t other, uint8_t sep, DevBuf<uint8_t> &codes, DevBuf<uint8_t> *rc,
                      DevBuf<int64_t> &d_off) {
    const int64_t n = static_cast<int64_t>(off.size()) - 1, bases = off[n], bytes = seed_code_bytes(bases, n);
    DevBuf<uint8_t> d_ascii;
    dev.upload(d_ascii, ascii, static_cast<size_t>(bases));
    dev.alloc(codes, static_cast<size_t>(bytes));
    if (rc) dev.alloc(*rc, static_cast<size_t>(bytes));
    dev.upload(d_off, off);
    const SeedEncodeArgs a{d_ascii.p, d_off.p, n, bytes, other, sep, codes.p, rc ? rc->p : nullptr};
    dev.launched(launch_seed_encode(a, dev.ctx->stream), "k_seed_encode");
    dev.sync();  // (the ASCII copy on the device goes when this returns)
}

// what npr_seed_matches and npr_seed_map_create (npr_seedmap_api.cpp) do alike: the reads' spans looked at and summed into off[n_reads + 1]
// (nothing is launched when they are refused) ...
void seed_check_reads(const Call &dev, int64_t n_reads, const uint8_t *text, const int64_t *begin, const int64_t *end, std::vector<int64_t> &off) {
    off.assign(static_cast<size_t>(n_reads) + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) {
        if (end[i] < begin[i] || begin[i] < 0) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": a span that ends before it begins").c_str());
        off[i + 1] = off[i] + (end[i] - begin[i]);
    }
    if (off[n_reads] && !text) dev.refuse(NPR_ERR_INVALID);
    if (seed_code_bytes(off[n_reads], n_reads) >= (int64_t(1) << 31))
        dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": 2^31 read positions and more in one call (give the reads in several)").c_str());
}

// ... the reads back to back in the pinned staging, then as code buffers on the device (both orientations when the reverse strand is asked for) ...
void seed_stage_reads(const Call &dev, int32_t strands, int64_t n_reads, const uint8_t *text, const int64_t *begin, const int64_t *end, const std::vector<int64_t> &off,
                      DevBuf<uint8_t> &fwd, DevBuf<uint8_t> &rev, DevBuf<int64_t> &d_off) {
    dev.passed(grow_pin_stage(dev.ctx, static_cast<size_t>(off[n_reads]), (std::string(dev.entry) + ": hipHostMalloc").c_str()));
    uint8_t *const h_ascii = static_cast<uint8_t *>(dev.ctx->pin_stage);
    parallel_for((n_reads + 255) / 256, dev.ctx->host_threads, [&](int64_t c) {
        for (int64_t i = c * 256, hi = std::min(n_reads, (c + 1) * 256); i < hi; ++i)
            std::memcpy(h_ascii + off[i], text + begin[i], static_cast<size_t>(end[i] - begin[i]));
    });
    encode_on_device(dev, h_ascii, off, NPR_SEED_READ_OTHER, NPR_SEED_READ_SEP, fwd, (strands & 2) ? &rev : nullptr, d_off);
}

// ... the arguments of k_seed_match for them (the orientation, and the rows once they have a buffer, are filled in later) ...
SeedMatchArgs seed_match_args(const npr_seed_index *ix, int64_t min_len, const std::vector<int64_t> &off, const int64_t *d_off, uint32_t *d_count, const int64_t *d_hit_off) {
    const int64_t n_reads = static_cast<int64_t>(off.size()) - 1;
    return SeedMatchArgs{ix->codes.p, ix->table.p, ix->pos.p, ix->off.p, ix->n_refs, ix->k, ix->kb, static_cast<int32_t>(min_len), nullptr, seed_code_bytes(off[n_reads], n_reads),
                         d_off, n_reads, 0u, d_count, d_hit_off, nullptr};
}

// ... and one pass of it, counting or emitting, over the orientations asked for
void seed_match_pass(const Call &dev, SeedMatchArgs &a, int32_t strands, const uint8_t *fwd, const uint8_t *rev, bool emit) {
    dev.zero(a.count, static_cast<size_t>(a.n_reads) * sizeof(uint32_t));
    for (uint32_t strand = 0; strand < 2; ++strand) {
        if (!(strands & (1 << strand))) continue;
        a.read = strand ? rev : fwd, a.strand = strand;
        dev.launched(launch_seed_match(a, emit, dev.ctx->stream), "k_seed_match");
    }
}

}  // namespace npr_impl

namespace {

struct HitLess {  // (strand, reference index, a, b)
    bool operator()(const std::array<int32_t, 4> &x, const std::array<int32_t, 4> &y) const {
        const uint32_t bx = static_cast<uint32_t>(x[2]), by = static_cast<uint32_t>(y[2]);
        if ((bx >> 31) != (by >> 31)) return (bx >> 31) < (by >> 31);
        if (x[0] != y[0]) return x[0] < y[0];
        if (x[1] != y[1]) return x[1] < y[1];
        return (bx & 0x7fffffffu) < (by & 0x7fffffffu);
    }
};

}  // namespace

extern "C" {

int32_t npr_seed_index_create(npr_ctx *ctx, int32_t k, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, npr_seed_index **out) {
    if (!ctx || !out) return NPR_ERR_INVALID;
    *out = nullptr;
    if (k < NPR_SEED_MIN_K || k > NPR_SEED_MAX_K) return fail(ctx, NPR_ERR_INVALID, "npr_seed_index_create: k outside 8 .. 32");
    if (n_refs < 0 || (n_refs && !ref_off)) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_seed_index_create", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> off(n_refs + 1, 0);
        for (int64_t i = 1; i <= n_refs; ++i) {
            off[i] = ref_off[i] - ref_off[0];
            if (off[i] < off[i - 1]) return fail(ctx, NPR_ERR_INVALID, "npr_seed_index_create: sequence offsets decrease");
        }
        if (off[n_refs] && !ref) return NPR_ERR_INVALID;
        if (seed_code_bytes(off[n_refs], n_refs) >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_seed_index_create: 2^31 reference positions and more");
        std::unique_ptr<npr_seed_index> ix(new npr_seed_index);
        ix->ctx = ctx, ix->k = k, ix->kb = std::min<int32_t>(k, NPR_SEED_MAX_KB), ix->n_refs = n_refs;
        ix->bytes = seed_code_bytes(off[n_refs], n_refs);
        ix->ref_len.resize(static_cast<size_t>(n_refs));
        for (int64_t i = 0; i < n_refs; ++i) ix->ref_len[i] = static_cast<int32_t>(off[i + 1] - off[i]);
        encode_on_device(dev, n_refs ? ref + ref_off[0] : nullptr, off, NPR_SEED_REF_OTHER, NPR_SEED_REF_SEP, ix->codes, nullptr, ix->off);
        const size_t entries = static_cast<size_t>(seed_table_entries(ix->kb));
        DevBuf<int32_t> tile;
        dev.alloc(ix->table, entries);
        dev.alloc(ix->pos, static_cast<size_t>(ix->bytes));
        dev.alloc(tile, entries / NPR_SEED_SCAN_TILE);
        dev.zero(ix->table);
        const SeedIndexArgs a{ix->codes.p, ix->bytes, ix->k, ix->kb, ix->table.p, tile.p, ix->pos.p};
        dev.launched(launch_seed_index(a, ctx->stream), "k_seed_bucket");
        dev.sync();
        *out = ix.release();
        return NPR_OK;
    });
}

void npr_seed_index_destroy(npr_seed_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    delete ix;
}

int64_t npr_seed_matches(npr_seed_index *ix, int64_t min_len, int32_t strands, int64_t n_reads, const uint8_t *text, const int64_t *begin, const int64_t *end,
                         int64_t *hit_off, int32_t *hits, int64_t cap) {
    if (!ix) return NPR_ERR_INVALID;
    npr_ctx *ctx = ix->ctx;
    if (min_len < ix->k || min_len >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_seed_matches: min_len outside k .. 2^31 - 1");
    if (strands < 1 || strands > 3) return fail(ctx, NPR_ERR_INVALID, "npr_seed_matches: strands outside 1 .. 3");
    if (n_reads < 0 || cap < 0 || !hit_off || (n_reads && (!begin || !end))) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_seed_matches", [&](const Call &dev) -> int64_t {
        std::vector<int64_t> off;
        seed_check_reads(dev, n_reads, text, begin, end, off);
        std::fill(hit_off, hit_off + n_reads + 1, int64_t(0));
        if (off[n_reads] == 0) return 0;
        DevBuf<uint8_t> fwd, rev;
        DevBuf<int64_t> d_off, d_hit_off;
        DevBuf<uint32_t> d_count;
        DevBuf<int32_t> d_hits;
        seed_stage_reads(dev, strands, n_reads, text, begin, end, off, fwd, rev, d_off);
        dev.alloc(d_count, static_cast<size_t>(n_reads));
        dev.alloc(d_hit_off, static_cast<size_t>(n_reads) + 1);
        SeedMatchArgs a = seed_match_args(ix, min_len, off, d_off.p, d_count.p, d_hit_off.p);
        seed_match_pass(dev, a, strands, fwd.p, rev.p, false);
        std::vector<uint32_t> count(n_reads);
        dev.fetch(count.data(), d_count.p, d_count.bytes());
        dev.sync();
        for (int64_t i = 0; i < n_reads; ++i) hit_off[i + 1] = hit_off[i] + count[i];
        const int64_t total = hit_off[n_reads];
        if (total == 0) return 0;
        if (!hits || total > cap) return fail(ctx, NPR_ERR_CAPACITY, "npr_seed_matches: more matches than the buffer holds (hit_off says how many)");
        dev.alloc(d_hits, static_cast<size_t>(total) * 4);
        dev.copy_up(d_hit_off.p, hit_off, d_hit_off.bytes());
        a.hits = d_hits.p;
        seed_match_pass(dev, a, strands, fwd.p, rev.p, true);
        dev.fetch(hits, d_hits.p, d_hits.bytes());
        dev.sync();
        // a read's matches arrive in the order the lanes found them: sorted here, the result is the same from run to run
        static_assert(sizeof(std::array<int32_t, 4>) == 4 * sizeof(int32_t), "a match is four int32");
        parallel_for((n_reads + 63) / 64, ctx->host_threads, [&](int64_t c) {
            std::vector<std::array<int32_t, 4>> rows;
            for (int64_t i = c * 64, hi = std::min(n_reads, (c + 1) * 64); i < hi; ++i) {
                const int64_t m = hit_off[i + 1] - hit_off[i];
                if (m < 2) continue;
                rows.resize(static_cast<size_t>(m));
                std::memcpy(rows.data(), hits + 4 * hit_off[i], static_cast<size_t>(m) * 16);
                std::sort(rows.begin(), rows.end(), HitLess());
                std::memcpy(hits + 4 * hit_off[i], rows.data(), static_cast<size_t>(m) * 16);
            }
        });
        return total;
    });
}

int64_t npr_seed_sam_text(int64_t n_reads, const uint8_t *text, const int64_t *name_span, const int64_t *begin, const int64_t *end, const char *rnames,
                          const int64_t *rname_off, int64_t n_refs, const int64_t *hit_off, const int32_t *hits, int64_t *rec_off, char *out, int64_t cap) {
    if (n_reads < 0 || n_refs < 0 || !hit_off || !rec_off || (n_reads && (!text || !name_span || !begin || !end))) return NPR_ERR_INVALID;
    const int64_t total = hit_off[n_reads];
    if (hit_off[0] != 0 || total < 0 || (total && (!hits || !rnames || !rname_off))) return NPR_ERR_INVALID;
    return guarded(nullptr, "npr_seed_sam_text", [&](const Call &) -> int64_t {  // (host code)
        for (int64_t i = 0; i < n_reads; ++i)
            if (hit_off[i + 1] < hit_off[i] || end[i] < begin[i] || name_span[2 * i + 1] < name_span[2 * i]) return NPR_ERR_INVALID;
        // qname, flag, rname, pos, "255", cigar, "*", "0", "0", seq, "*"
        return format_records(total, usable_cpus(), rec_off, out, cap, [&](int64_t q, auto &s) {
            const int64_t i = std::upper_bound(hit_off, hit_off + n_reads + 1, q) - hit_off - 1;  // the row's read: hit_off[i] <= q < hit_off[i + 1]
            const int64_t len = end[i] - begin[i];
            const int32_t *h = hits + 4 * q;
            const int64_t r = h[0], a = h[1], b = static_cast<uint32_t>(h[2]) & 0x7fffffffu, L = h[3], rest = len - b - L;
            const bool reverse = static_cast<uint32_t>(h[2]) >> 31;
            if (r < 0 || r >= n_refs || a < 0 || L < 1 || rest < 0) return false;
            s.bytes(text + name_span[2 * i], name_span[2 * i + 1] - name_span[2 * i]);
            s.ch('\t');
            s.num(reverse ? 16 : 0);
            s.ch('\t');
            s.bytes(rnames + rname_off[r], rname_off[r + 1] - rname_off[r]);
            s.ch('\t');
            s.num(a + 1);
            s.lit("\t255\t");
            if (b) s.num(b), s.ch('H');
            s.num(L), s.ch('M');
            if (rest) s.num(rest), s.ch('H');
            s.lit("\t*\t0\t0\t");
            if (!reverse) {
                s.bytes(text + begin[i] + b, L);
            } else {  // base u of the match is base b + u of the reverse complement: the complement of read base len - 1 - (b + u)
                s.revcomp(text + begin[i] + rest, L);
            }
            s.lit("\t*\n");
            return true;
        });
    });
}

}  // extern "C"
