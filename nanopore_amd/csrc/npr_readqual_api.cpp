// npr_readqual_api.cpp -- npr_read_quality: the checks, the staging of the counted reads' bytes, the work list and the launch of the
// read-quality kernels (npr_readqual.hip), and the tables as the header defines them
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

static_assert(RQ_POS_BINS == NPR_RQ_POS_BINS && RQ_QUAL_COLS == NPR_RQ_QUAL_COLS && RQ_GC_COLS == NPR_RQ_GC_COLS && RQ_TOTALS == NPR_RQ_TOTALS &&
                  RQ_MAX_GROUPS == NPR_RQ_MAX_GROUPS && RQ_TILE == NPR_RQ_TILE,
              "the kernels' constants are the header's");

namespace {

// the tables of groups without a read: zeros, and -1 where the header says so
void empty_tables(size_t G, int64_t *pos_qual, int64_t *pos_base, int64_t *len_hist, int64_t *meanq_hist, int64_t *gc_hist, int64_t *totals) {
    std::fill(pos_qual, pos_qual + G * RQ_POS_BINS * RQ_QUAL_COLS, int64_t(0));
    std::fill(pos_base, pos_base + G * RQ_POS_BINS * RQ_BASE_COLS, int64_t(0));
    std::fill(len_hist, len_hist + G * RQ_POS_BINS, int64_t(0));
    std::fill(meanq_hist, meanq_hist + G * RQ_QUAL_COLS, int64_t(0));
    std::fill(gc_hist, gc_hist + G * RQ_GC_COLS, int64_t(0));
    std::fill(totals, totals + G * RQ_TOTALS, int64_t(0));
    for (size_t g = 0; g < G; ++g)
        for (int w = 2; w <= 5; ++w) totals[g * RQ_TOTALS + w] = -1;
}

}  // namespace

extern "C" {

int32_t npr_read_quality(npr_ctx *ctx, int64_t n_reads, const uint8_t *text, const int64_t *seq_begin, const int64_t *seq_end, const int64_t *qual_begin,
                         const int64_t *qual_end, const int32_t *group, int32_t n_groups, int64_t *pos_qual, int64_t *pos_base, int64_t *len_hist,
                         int64_t *meanq_hist, int64_t *gc_hist, int64_t *totals) {
    if (!ctx || n_reads < 0 || n_groups < 1 || n_groups > RQ_MAX_GROUPS || !pos_qual || !pos_base || !len_hist || !meanq_hist || !gc_hist || !totals ||
        (n_reads && (!seq_begin || !seq_end || !qual_begin || !qual_end || !group)))
        return NPR_ERR_INVALID;
    const size_t G = static_cast<size_t>(n_groups);
    return guarded(ctx, "npr_read_quality", [&](const Call &dev) -> int32_t {
        // nothing is counted and no table touched when an argument is wrong
        int64_t n = 0, bytes = 0, n_items = 0;
        for (int64_t i = 0; i < n_reads; ++i) {
            if (group[i] < -1 || group[i] >= n_groups) return fail(ctx, NPR_ERR_INVALID, "npr_read_quality: a group outside -1 .. n_groups - 1");
            if (seq_end[i] < seq_begin[i] || seq_begin[i] < 0 || qual_end[i] < qual_begin[i] || qual_begin[i] < 0)
                return fail(ctx, NPR_ERR_INVALID, "npr_read_quality: a span that ends before it begins");
            if (group[i] < 0) continue;
            const int64_t len = seq_end[i] - seq_begin[i];
            if (qual_end[i] - qual_begin[i] != len) return fail(ctx, NPR_ERR_INVALID, "npr_read_quality: a quality line that is not as long as its sequence");
            if (len >= (int64_t(1) << 42)) return fail(ctx, NPR_ERR_INVALID, "npr_read_quality: a read of 2^42 bases or more");
            ++n, bytes += (len + RQ_ALIGN - 1) / RQ_ALIGN * RQ_ALIGN, n_items += (len + RQ_TILE - 1) / RQ_TILE;
        }
        if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_read_quality: 2^31 reads and more in one call (give the reads in several)");
        empty_tables(G, pos_qual, pos_base, len_hist, meanq_hist, gc_hist, totals);
        if (n == 0) return NPR_OK;
        if (bytes && !text) return NPR_ERR_INVALID;
        bytes += RQ_ALIGN;

        // the counted reads in the order given: where their bytes go in the staging, and the work list ordered by (group, tile class) --
        // a histogram over the keys, one prefix sum, one scatter
        std::vector<int64_t> meta(2 * static_cast<size_t>(n)), src(2 * static_cast<size_t>(n));
        std::vector<int32_t> grp(static_cast<size_t>(n));
        int64_t *const start = meta.data(), *const len = meta.data() + n;
        std::vector<int64_t> first(G * RQ_TILE_CLASSES + 1, 0);
        {
            int64_t r = 0, at = 0;
            for (int64_t i = 0; i < n_reads; ++i) {
                if (group[i] < 0) continue;
                start[r] = at, len[r] = seq_end[i] - seq_begin[i], grp[r] = group[i];
                src[2 * r] = seq_begin[i], src[2 * r + 1] = qual_begin[i];
                at += (len[r] + RQ_ALIGN - 1) / RQ_ALIGN * RQ_ALIGN;
                const int64_t tiles = (len[r] + RQ_TILE - 1) / RQ_TILE;
                int64_t *const f = first.data() + static_cast<size_t>(group[i]) * RQ_TILE_CLASSES + 1;
                for (int64_t t = 0; t < std::min<int64_t>(tiles, RQ_TILE_CLASSES - 1); ++t) ++f[t];
                if (tiles >= RQ_TILE_CLASSES) f[RQ_TILE_CLASSES - 1] += tiles - (RQ_TILE_CLASSES - 1);
                ++r;
            }
        }
        for (size_t k = 1; k < first.size(); ++k) first[k] += first[k - 1];
        std::vector<unsigned long long> items(static_cast<size_t>(n_items));
        for (int64_t r = 0; r < n; ++r) {
            const int64_t tiles = (len[r] + RQ_TILE - 1) / RQ_TILE;
            int64_t *const f = first.data() + static_cast<size_t>(grp[r]) * RQ_TILE_CLASSES;
            for (int64_t t = 0; t < tiles; ++t)
                items[f[std::min<int64_t>(t, RQ_TILE_CLASSES - 1)]++] = (static_cast<unsigned long long>(r) << 32) | static_cast<unsigned long long>(t);
        }

        dev.passed(grow_pin_stage(ctx, 2 * static_cast<size_t>(bytes), "npr_read_quality: hipHostMalloc"));
        uint8_t *const h_seq = static_cast<uint8_t *>(ctx->pin_stage), *const h_qual = h_seq + bytes;
        parallel_for((n + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t r = c * 256, hi = std::min(n, (c + 1) * 256); r < hi; ++r) {
                if (len[r] == 0) continue;
                std::memcpy(h_seq + start[r], text + src[2 * r], static_cast<size_t>(len[r]));
                std::memcpy(h_qual + start[r], text + src[2 * r + 1], static_cast<size_t>(len[r]));
            }
        });
        DevBuf<uint8_t> d_bytes;
        DevBuf<int64_t> d_meta;
        DevBuf<int32_t> d_grp;
        DevBuf<unsigned long long> d_items, d_rows, d_tab;
        const size_t tab_words = G * RQ_GROUP_WORDS;
        dev.upload(d_bytes, h_seq, 2 * static_cast<size_t>(bytes));
        dev.upload(d_meta, meta);
        dev.upload(d_grp, grp);
        dev.upload(d_items, items);
        dev.alloc(d_rows, static_cast<size_t>(n) * RQ_ROW);
        dev.alloc(d_tab, tab_words);
        dev.zero(d_rows);
        dev.zero(d_tab);
        ReadQualArgs a{};
        a.seq = d_bytes.p, a.qual = d_bytes.p + bytes, a.start = d_meta.p, a.len = d_meta.p + n, a.group = d_grp.p, a.items = d_items.p;
        a.n = n, a.n_items = n_items, a.n_groups = n_groups, a.rows = d_rows.p;
        a.pos_qual = d_tab.p;
        a.pos_base = a.pos_qual + G * RQ_POS_BINS * RQ_QUAL_COLS;
        a.len_hist = a.pos_base + G * RQ_POS_BINS * RQ_BASE_COLS;
        a.meanq_hist = a.len_hist + G * RQ_POS_BINS;
        a.gc_hist = a.meanq_hist + G * RQ_QUAL_COLS;
        a.totals = a.gc_hist + G * RQ_GC_COLS;
        dev.launched(launch_read_quality(a, ctx->stream), "k_read_quality");
        std::vector<int64_t> tab(tab_words);
        dev.fetch(tab.data(), d_tab.p, d_tab.bytes());
        dev.sync();
        const int64_t *p = tab.data();
        auto take = [&](int64_t *dst, size_t words) { std::copy(p, p + words, dst), p += words; };
        take(pos_qual, G * RQ_POS_BINS * RQ_QUAL_COLS), take(pos_base, G * RQ_POS_BINS * RQ_BASE_COLS), take(len_hist, G * RQ_POS_BINS);
        take(meanq_hist, G * RQ_QUAL_COLS), take(gc_hist, G * RQ_GC_COLS);
        for (size_t g = 0; g < G; ++g) {  // the extremes back from the form the device keeps them in; a group without a read (a base) keeps its -1
            const int64_t *t = p + g * RQ_TOTALS;
            int64_t *o = totals + g * RQ_TOTALS;
            o[0] = t[0], o[1] = t[1], o[6] = t[6], o[7] = t[7];
            if (t[0]) o[2] = static_cast<int64_t>(RQ_LEN_TOP) - t[2], o[3] = t[3];
            if (t[1]) o[4] = 255 - t[4], o[5] = t[5];
        }
        return NPR_OK;
    });
}

}  // extern "C"
