// npr_seedmap_api.cpp -- reads to rows, chains and guides in one call: npr_seed_matches and npr_seed_chains with the rows never leaving the
// device.  The encode and the two match passes are npr_seed_api.cpp's, the chain kernels npr_seedchain_api.cpp's; what those two calls do on
// the host in between -- the reads' row offsets, the sort of every read's rows, the chain spans -- is npr_seedmap.hip's.  The host reads
// back three totals, to size the three buffers that depend on them.
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace {

// one int64 from the device, waited for
int32_t fetch_total(npr_ctx *ctx, const int64_t *d, int64_t &v) {
    HIP_TRY(ctx, hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

int32_t fill_map(npr_seed_map *m, npr_seed_index *ix, int64_t min_len, int32_t strands, int64_t max_gap, const uint8_t *text, const int64_t *begin, const int64_t *end,
                 const std::vector<int64_t> &off) {
    npr_ctx *ctx = m->ctx;
    const int64_t n_reads = m->n_reads;
    const char *const what = "npr_seed_map_create: hipMalloc";
    DevBuf<uint8_t> fwd, rev;
    DevBuf<int64_t> d_off;
    DevBuf<uint32_t> d_count;
    int32_t rc = seed_stage_reads(ctx, "npr_seed_map_create", strands, n_reads, text, begin, end, off, fwd, rev, d_off);
    if (rc != NPR_OK) return rc;
    hipError_t e;
    if ((e = d_count.alloc(static_cast<size_t>(n_reads))) != hipSuccess || (e = m->hit_off.alloc(static_cast<size_t>(n_reads) + 1)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, what, e);
    // count, offsets by a scan on the device, emit
    SeedMatchArgs match = seed_match_args(ix, min_len, off, d_off.p, d_count.p, m->hit_off.p);
    SeedMapArgs a{n_reads, d_count.p, m->hit_off.p, nullptr, nullptr, nullptr};
    if ((rc = seed_match_pass(ctx, match, strands, fwd.p, rev.p, false)) != NPR_OK) return rc;
    int r = launch_seedmap_offsets(a, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_map_scan launch", static_cast<hipError_t>(r));
    if ((rc = fetch_total(ctx, m->hit_off.p + n_reads, m->rows)) != NPR_OK) return rc;
    if (m->rows == 0) return NPR_OK;
    if ((e = m->hits.alloc(static_cast<size_t>(m->rows) * 4)) != hipSuccess || (e = m->chain_off.alloc(static_cast<size_t>(n_reads) + 1)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, what, e);
    match.hits = m->hits.p;
    if ((rc = seed_match_pass(ctx, match, strands, fwd.p, rev.p, true)) != NPR_OK) return rc;
    // every read's rows sorted where they lie, its chains counted and the counts scanned
    a.hits = m->hits.p, a.chain_off = m->chain_off.p;
    r = launch_seedmap_chains(a, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_map_sort launch", static_cast<hipError_t>(r));
    if ((rc = fetch_total(ctx, m->chain_off.p + n_reads, m->chains)) != NPR_OK) return rc;
    fwd.release(), rev.release();  // (the reads' codes have served; the kernels that read them have finished)
    // the chain spans, then the chain kernels on the rows where they lie
    DevBuf<SeedChainSpan> d_span;
    DevBuf<int32_t> d_len;
    std::vector<int32_t> len32(ix->ref_len);  // reference lengths, then read lengths
    len32.resize(static_cast<size_t>(ix->n_refs + n_reads));
    for (int64_t i = 0; i < n_reads; ++i) len32[static_cast<size_t>(ix->n_refs + i)] = static_cast<int32_t>(off[i + 1] - off[i]);
    if ((e = d_span.alloc(static_cast<size_t>(m->chains))) != hipSuccess || (e = d_len.alloc(len32.size())) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, what, e);
    HIP_TRY(ctx, hipMemcpyAsync(d_len.p, len32.data(), d_len.bytes(), hipMemcpyHostToDevice, ctx->stream));
    a.span = d_span.p;
    r = launch_seedmap_spans(a, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_map_spans launch", static_cast<hipError_t>(r));
    SeedChainRun run;
    if ((rc = run.count(ctx, what, m->hits.p, m->rows, d_span.p, m->chains, max_gap, d_len.p, d_len.p + ix->n_refs)) != NPR_OK) return rc;
    if ((rc = run.write(ctx, what)) != NPR_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the scratch of the chain kernels and the spans go when this returns)
    m->pairs = run.pairs;
    m->chain_rows.take(run.chains), m->ops_off.take(run.n_ops), m->ops.take(run.ops);
    return NPR_OK;
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
    try {
        std::vector<int64_t> off;
        int32_t rc = seed_check_reads(ctx, "npr_seed_map_create", n_reads, text, begin, end, off);
        if (rc != NPR_OK) return rc;
        std::unique_ptr<npr_seed_map> m(new npr_seed_map);
        m->ctx = ctx, m->n_reads = n_reads;
        if (off[n_reads] != 0) {  // (without a base there is no row: nothing to launch)
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            rc = fill_map(m.get(), ix, min_len, strands, max_gap, text, begin, end, off);
            if (rc != NPR_OK) return rc;
        }
        *out = m.release();
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_seed_map_create: out of host memory");
    }
}

int32_t npr_seed_map_counts(const npr_seed_map *m, int64_t counts[3]) {
    if (!m || !counts) return NPR_ERR_INVALID;
    counts[0] = m->rows, counts[1] = m->chains, counts[2] = m->pairs;
    return NPR_OK;
}

int32_t npr_seed_map_fetch(npr_seed_map *m, int64_t *hit_off, int32_t *hits, int64_t *chain_off, int32_t *chains, int64_t *ops_off, int32_t *ops) {
    if (!m) return NPR_ERR_INVALID;
    npr_ctx *ctx = m->ctx;
    if (m->rows == 0) {  // no buffer on the device: the empty, well-formed result
        if (hit_off) std::fill(hit_off, hit_off + m->n_reads + 1, int64_t(0));
        if (chain_off) std::fill(chain_off, chain_off + m->n_reads + 1, int64_t(0));
        if (ops_off) ops_off[0] = 0;
        return NPR_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto fetch = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; };
    HIP_TRY(ctx, fetch(hit_off, m->hit_off.p, m->hit_off.bytes()));
    HIP_TRY(ctx, fetch(hits, m->hits.p, m->hits.bytes()));
    HIP_TRY(ctx, fetch(chain_off, m->chain_off.p, m->chain_off.bytes()));
    HIP_TRY(ctx, fetch(chains, m->chain_rows.p, m->chain_rows.bytes()));
    HIP_TRY(ctx, fetch(ops_off, m->ops_off.p, m->ops_off.bytes()));
    HIP_TRY(ctx, fetch(ops, m->ops.p, m->ops.bytes()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

void npr_seed_map_destroy(npr_seed_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    delete m;
}

}  // extern "C"
