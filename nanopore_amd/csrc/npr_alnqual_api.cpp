// npr_alnqual_api.cpp -- npr_pileup_coverage, npr_align_quality: the checks, the staging and the launches of the alignment-quality kernels
// (npr_alnqual.hip), and the tables as the header defines them
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

static_assert(AQ_WIN_WORDS == NPR_AQ_WIN_WORDS && AQ_TOTALS == NPR_AQ_TOTALS && AQ_HOMOPOLYMER == NPR_AQ_HOMOPOLYMER && AQ_MAX_WINDOWS == NPR_AQ_MAX_WINDOWS &&
                  AQ_TILE == NPR_AQ_TILE,
              "the kernels' constants are the header's");

extern "C" {

int32_t npr_pileup_coverage(npr_pileup *pl, const uint8_t *ref, const int64_t *ref_off, int32_t n_windows, int64_t *win, int64_t *depth_hist,
                            int64_t *start_hist, int64_t *totals) {
    if (!pl || !win || !depth_hist || !start_hist || !totals) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    const int64_t n_refs = static_cast<int64_t>(pl->len.size()), T = pl->rows;
    if (n_windows < 1 || n_windows > AQ_MAX_WINDOWS) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_coverage: n_windows outside 1 .. NPR_AQ_MAX_WINDOWS");
    if ((n_refs && !ref_off) || (T && !ref)) return NPR_ERR_INVALID;
    for (int64_t k = 0; k < n_refs; ++k)
        if (ref_off[k + 1] - ref_off[k] != pl->len[k]) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_coverage: a reference sequence is not as long as the pileup's");
    const size_t W = static_cast<size_t>(n_windows), words = W * AQ_WIN_WORDS + 2 * RQ_POS_BINS + AQ_TOTALS + 1;
    return guarded(ctx, "npr_pileup_coverage", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> out(words, 0);
        if (T > 0) {
            pileup_scan(dev, pl);
            DevBuf<uint8_t> d_ref;
            DevBuf<unsigned long long> d_out;
            dev.upload(d_ref, ref + ref_off[0], static_cast<size_t>(T));
            dev.alloc(d_out, words);
            dev.zero(d_out);
            CoverageArgs a{};
            a.tab = pl->tab.p, a.ref = d_ref.p, a.rows = T, a.n_windows = n_windows;
            a.win = d_out.p, a.depth_hist = a.win + W * AQ_WIN_WORDS, a.start_hist = a.depth_hist + RQ_POS_BINS, a.totals = a.start_hist + RQ_POS_BINS;
            a.max_depth = a.totals + AQ_TOTALS;
            // the largest depth first: depth^2 summed over the longest window must stay inside int64
            dev.launched(launch_coverage_max(a, ctx->stream), "k_coverage_max");
            int64_t max_depth = 0;
            dev.fetch(&max_depth, a.max_depth, sizeof(int64_t));
            dev.sync();
            const int64_t longest = (T + n_windows - 1) / n_windows;
            if (static_cast<unsigned __int128>(max_depth) * static_cast<unsigned __int128>(max_depth) * static_cast<unsigned __int128>(longest) >>
                63)
                return fail(ctx, NPR_ERR_CAPACITY, "npr_pileup_coverage: the sum of depth^2 over a window could leave int64 (more windows make them shorter)");
            dev.launched(launch_pileup_coverage(a, ctx->stream), "k_pileup_coverage");
            dev.fetch(out.data(), d_out.p, d_out.bytes());
            dev.sync();
            // the totals the windows' sums give; the kernel leaves the largest start count in word 4 and the insertion markers in word 7
            int64_t *t = out.data() + W * AQ_WIN_WORDS + 2 * RQ_POS_BINS;
            t[2] = max_depth;
            for (size_t w = 0; w < W; ++w) {
                const int64_t *v = out.data() + w * AQ_WIN_WORDS;
                t[0] += v[0], t[1] += v[1], t[3] += v[3], t[5] += v[6], t[6] += v[7];
            }
        }
        const int64_t *p = out.data();
        auto take = [&](int64_t *dst, size_t n) { std::copy(p, p + n, dst), p += n; };
        take(win, W * AQ_WIN_WORDS), take(depth_hist, RQ_POS_BINS), take(start_hist, RQ_POS_BINS), take(totals, AQ_TOTALS);
        return NPR_OK;
    });
}

int32_t npr_align_quality(npr_ctx *ctx, int64_t n, const int32_t *ref_index, const uint8_t *read, const int64_t *read_begin, const int64_t *read_end,
                          const int32_t *ops, const int64_t *ops_off, const int64_t *start, const uint8_t *use, const int32_t *mapq, const int64_t *clip,
                          int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, int32_t n_windows, int64_t *mapq_hist, int64_t *win_mapq,
                          int64_t *pos_base, int64_t *clip_hist, int64_t *gc_hist, int64_t *indel, int64_t *indel_len, int64_t *totals) {
    if (!ctx || n < 0 || n_refs < 0 || !mapq_hist || !win_mapq || !pos_base || !clip_hist || !gc_hist || !indel || !indel_len || !totals ||
        (n_refs && !ref_off) || (n && (!ref_index || !read_begin || !ops_off || !mapq || !clip)))
        return NPR_ERR_INVALID;
    if (n_windows < 1 || n_windows > AQ_MAX_WINDOWS) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: n_windows outside 1 .. NPR_AQ_MAX_WINDOWS");
    if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: too many records");
    std::vector<int64_t> base(static_cast<size_t>(n_refs) + 1, 0);  // first row of every sequence
    for (int64_t k = 0; k < n_refs; ++k) {
        const int64_t len = ref_off[k + 1] - ref_off[k];
        if (len < 0 || len >= (int64_t(1) << 31) - 1) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: reference offsets decrease, or a sequence of 2^31 bases and more");
        base[k + 1] = base[k] + len;
    }
    const int64_t T = base[n_refs];
    if (T && !ref) return NPR_ERR_INVALID;
    const int64_t o0 = n ? ops_off[0] : 0, n_ops = n ? ops_off[n] - o0 : 0;
    if (n_ops < 0 || (n_ops && !ops)) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: operation offsets decrease");
    for (int64_t i = 0; i < n; ++i) {
        if (ops_off[i + 1] < ops_off[i]) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: operation offsets decrease");
        if (!read_end && read_begin[i + 1] < read_begin[i]) return fail(ctx, NPR_ERR_INVALID, "npr_align_quality: read offsets decrease");
    }
    const size_t W = static_cast<size_t>(n_windows);
    return guarded(ctx, "npr_align_quality", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> out(AQ_TABLE_WORDS + 2 * W, 0);
        int32_t bad = 0;
        if (n > 0) {
            std::vector<AlnQualRec> recs(n, AlnQualRec{0, 0, 0, 0, 0, 0, -1, 0, 0, 0});
            std::vector<int64_t> off(n + 1);
            std::vector<uint8_t> malformed(n, 0);
            std::vector<uint32_t> packed(static_cast<size_t>(n_ops));
            for (int64_t i = 0; i <= n; ++i) off[i] = ops_off[i] - o0;
            parallel_for(n, ctx->host_threads, [&](int64_t i) {
                const bool selected = !use || use[i];
                const int64_t k = ref_index[i], sx = start ? start[2 * i] : 0, sy = start ? start[2 * i + 1] : 0;
                const int64_t len = (read_end ? read_end[i] : read_begin[i + 1]) - read_begin[i];
                bool ok = k >= 0 && k < n_refs && len >= 0 && len < (int64_t(1) << 31) && sx >= 0 && sy >= 0 && sy <= len;
                ok = ok && sx <= base[k + 1] - base[k];
                ok = ok && mapq[i] >= 0 && mapq[i] <= 255 && clip[2 * i] >= 0 && clip[2 * i + 1] >= 0 && clip[2 * i] < (int64_t(1) << 42) &&
                     clip[2 * i + 1] < (int64_t(1) << 42);
                for (int64_t q = off[i]; ok && q < off[i + 1]; ++q) {
                    const int32_t op = ops[2 * (o0 + q)], ln = ops[2 * (o0 + q) + 1];
                    ok = op >= 0 && op <= 2 && ln >= 0 && ln < (1 << 30);
                    packed[q] = static_cast<uint32_t>(ln) << 2 | static_cast<uint32_t>(op);
                }
                if (!ok) std::fill(packed.begin() + off[i], packed.begin() + off[i + 1], 0u);
                if (!selected) return;
                if (!ok) {
                    malformed[i] = 1;
                    return;
                }
                recs[i] = AlnQualRec{base[k] + sx, base[k], base[k + 1], 0, clip[2 * i], clip[2 * i + 1], static_cast<int32_t>(base[k + 1] - base[k] - sx),
                                     static_cast<int32_t>(len), static_cast<int32_t>(sy), mapq[i]};
            });
            // the selected records' whole reads: uploaded as they are when the reads lie back to back, else gathered first
            DevBuf<uint8_t> d_seq, d_ref;
            std::unique_ptr<uint8_t[]> gathered;
            int64_t bytes = 0;
            const uint8_t *src = nullptr;
            if (!read_end) {
                bytes = read_begin[n] - read_begin[0];
                if (bytes && !read) return NPR_ERR_INVALID;
                src = bytes ? read + read_begin[0] : nullptr;
                for (int64_t i = 0; i < n; ++i)
                    if (recs[i].xlen >= 0) recs[i].y_off = read_begin[i] - read_begin[0];
            } else {
                for (int64_t i = 0; i < n; ++i)
                    if (recs[i].xlen >= 0) recs[i].y_off = bytes, bytes += recs[i].span;
                if (bytes && !read) return NPR_ERR_INVALID;
                gathered.reset(new uint8_t[bytes + 1]);
                parallel_for(n, ctx->host_threads, [&](int64_t i) {
                    if (recs[i].xlen >= 0 && recs[i].span) std::memcpy(gathered.get() + recs[i].y_off, read + read_begin[i], static_cast<size_t>(recs[i].span));
                });
                src = gathered.get();
            }
            dev.alloc(d_seq, static_cast<size_t>(bytes) + 1);
            dev.copy_up(d_seq.p, src, static_cast<size_t>(bytes));
            dev.alloc(d_ref, static_cast<size_t>(T) + 1);
            dev.copy_up(d_ref.p, T ? ref + ref_off[0] : nullptr, static_cast<size_t>(T));
            DeviceCigars c;
            cigars_from_host(dev, packed.data(), off, c);
            DevBuf<AlnQualRec> d_recs;
            DevBuf<unsigned long long> d_out;
            DevBuf<int32_t> d_bad;
            dev.upload(d_recs, recs);
            dev.alloc(d_out, out.size());
            dev.zero(d_out);
            dev.alloc(d_bad, 1);
            dev.zero(d_bad);
            const AlnQualArgs a{n, c.off, c.ops, d_recs.p, d_seq.p, d_ref.p, T, n_windows, d_out.p, d_out.p + AQ_TABLE_WORDS, d_bad.p};
            dev.launched(launch_align_quality(a, ctx->stream), "k_align_quality");
            dev.fetch(out.data(), d_out.p, d_out.bytes());
            dev.fetch(&bad, d_bad.p, sizeof(int32_t));
            dev.sync();
            for (int64_t i = 0; i < n; ++i) bad |= malformed[i];
        }
        const int64_t *p = out.data();
        auto take = [&](int64_t *dst, size_t words) { std::copy(p, p + words, dst), p += words; };
        take(mapq_hist, AQ_MAPQ_COLS), take(pos_base, static_cast<size_t>(RQ_POS_BINS) * RQ_BASE_COLS), take(clip_hist, RQ_POS_BINS), take(gc_hist, RQ_GC_COLS);
        take(indel, 2 * AQ_CLASSES), take(indel_len, 2 * RQ_POS_BINS), take(totals, AQ_TOTALS), take(win_mapq, 2 * W);
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_align_quality: a record is malformed or its cigar runs past its sequences (the record was left out)") : NPR_OK;
    });
}

}  // extern "C"
