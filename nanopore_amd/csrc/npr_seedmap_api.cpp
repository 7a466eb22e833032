// npr_seedmap_api.cpp -- reads to rows, chains and guides in one call: npr_seed_matches and npr_seed_chains with the rows never leaving the
// device.  The encode and the two match passes are npr_seed_api.cpp's, the chain kernels npr_seedchain_api.cpp's; what those two calls do on
// the host in between -- the reads' row offsets, the sort of every read's rows, the chain spans -- is npr_seedmap.hip's.  The host reads
// back three totals, to size the three buffers that depend on them.
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace {

// one int64 from the device, waited for
int64_t fetch_total(const Call &dev, const int64_t *d) {
    int64_t v = 0;
    dev.fetch(&v, d, sizeof(v));
    dev.sync();
    return v;
}

void fill_map(const Call &dev, npr_seed_map *m, npr_seed_index *ix, int64_t min_len, int32_t strands, int64_t max_gap, const uint8_t *text, const int64_t *begin,
              const int64_t *end, const std::vector<int64_t> &off) {
    const hipStream_t stream = dev.ctx->stream;
    const int64_t n_reads = m->n_reads;
    DevBuf<uint8_t> fwd, rev;
    DevBuf<int64_t> d_off;
    DevBuf<uint32_t> d_count;
    seed_stage_reads(dev, strands, n_reads, text, begin, end, off, fwd, rev, d_off);
    dev.alloc(d_count, static_cast<size_t>(n_reads));
    dev.alloc(m->hit_off, static_cast<size_t>(n_reads) + 1);
    // count, offsets by a scan on the device, emit
    SeedMatchArgs match = seed_match_args(ix, min_len, off, d_off.p, d_count.p, m->hit_off.p);
    SeedMapArgs a{n_reads, d_count.p, m->hit_off.p, nullptr, nullptr, nullptr};
    seed_match_pass(dev, match, strands, fwd.p, rev.p, false);
    dev.launched(launch_seedmap_offsets(a, stream), "k_map_scan");
    m->rows = fetch_total(dev, m->hit_off.p + n_reads);
    if (m->rows == 0) return;
    dev.alloc(m->hits, static_cast<size_t>(m->rows) * 4);
    dev.alloc(m->chain_off, static_cast<size_t>(n_reads) + 1);
    match.hits = m->hits.p;
    seed_match_pass(dev, match, strands, fwd.p, rev.p, true);
    // every read's rows sorted where they lie, its chains counted and the counts scanned
    a.hits = m->hits.p, a.chain_off = m->chain_off.p;
    dev.launched(launch_seedmap_chains(a, stream), "k_map_sort");
    m->chains = fetch_total(dev, m->chain_off.p + n_reads);
    fwd.release(), rev.release();  // (the reads' codes have served; the kernels that read them have finished)
    // the chain spans, then the chain kernels on the rows where they lie
    DevBuf<SeedChainSpan> d_span;
    DevBuf<int32_t> d_len;
    std::vector<int32_t> len32(ix->ref_len);  // reference lengths, then read lengths
    len32.resize(static_cast<size_t>(ix->n_refs + n_reads));
    for (int64_t i = 0; i < n_reads; ++i) len32[static_cast<size_t>(ix->n_refs + i)] = static_cast<int32_t>(off[i + 1] - off[i]);
    dev.alloc(d_span, static_cast<size_t>(m->chains));
    dev.upload(d_len, len32);
    a.span = d_span.p;
    dev.launched(launch_seedmap_spans(a, stream), "k_map_spans");
    SeedChainRun run;
    run.count(dev, m->hits.p, m->rows, d_span.p, m->chains, max_gap, d_len.p, d_len.p + ix->n_refs);
    run.write(dev);
    dev.sync();  // (the scratch of the chain kernels and the spans go when this returns)
    m->pairs = run.pairs;
    m->chain_rows.take(run.chains), m->ops_off.take(run.n_ops), m->ops.take(run.ops);
}

}  // namespace

extern "C" {

int32_t npr_seed_map_create(npr_seed_index *ix, int64_t min_len, int32_t strands, int64_t max_gap, int64_t n_reads, const uint8_t *text, const int64_t *begin,
                            const int64_t *end, npr_seed_map **out) {
    if (!ix || !out) return NPR_ERR_INVALID;
    *out = nullptr;
    npr_ctx *ctx = ix->ctx;
    if (min_len < ix->k || min_len >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_seed_map_create: min_len outside k .. 2^31 - 1");
    if (strands < 1 || strands > 3) return fail(ctx, NPR_ERR_INVALID, "npr_seed_map_create: strands outside 1 .. 3");
    if (max_gap < 0) return fail(ctx, NPR_ERR_INVALID, "npr_seed_map_create: a negative max_gap");
    if (n_reads < 0 || (n_reads && (!begin || !end))) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_seed_map_create", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> off;
        seed_check_reads(dev, n_reads, text, begin, end, off);
        std::unique_ptr<npr_seed_map> m(new npr_seed_map);
        m->ctx = ctx, m->n_reads = n_reads;
        if (off[n_reads] != 0) fill_map(dev, m.get(), ix, min_len, strands, max_gap, text, begin, end, off);  // (without a base there is no row: nothing to launch)
        *out = m.release();
        return NPR_OK;
    });
}

int32_t npr_seed_map_counts(const npr_seed_map *m, int64_t counts[3]) {
    if (!m || !counts) return NPR_ERR_INVALID;
    counts[0] = m->rows, counts[1] = m->chains, counts[2] = m->pairs;
    return NPR_OK;
}

int32_t npr_seed_map_fetch(npr_seed_map *m, int64_t *hit_off, int32_t *hits, int64_t *chain_off, int32_t *chains, int64_t *ops_off, int32_t *ops) {
    if (!m) return NPR_ERR_INVALID;
    if (m->rows == 0) {  // no buffer on the device: the empty, well-formed result
        if (hit_off) std::fill(hit_off, hit_off + m->n_reads + 1, int64_t(0));
        if (chain_off) std::fill(chain_off, chain_off + m->n_reads + 1, int64_t(0));
        if (ops_off) ops_off[0] = 0;
        return NPR_OK;
    }
    return guarded(m->ctx, "npr_seed_map_fetch", [&](const Call &dev) -> int32_t {
        auto fetch = [&](void *dst, const void *src, size_t bytes) {
            if (dst) dev.fetch(dst, src, bytes);
        };
        fetch(hit_off, m->hit_off.p, m->hit_off.bytes());
        fetch(hits, m->hits.p, m->hits.bytes());
        fetch(chain_off, m->chain_off.p, m->chain_off.bytes());
        fetch(chains, m->chain_rows.p, m->chain_rows.bytes());
        fetch(ops_off, m->ops_off.p, m->ops_off.bytes());
        fetch(ops, m->ops.p, m->ops.bytes());
        dev.sync();
        return NPR_OK;
    });
}

void npr_seed_map_destroy(npr_seed_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    delete m;
}

}  // extern "C"
