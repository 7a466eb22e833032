// npr_pileup_api.cpp -- the device pileup (npr_pileup.hip): per-position base counts and depth of the alignments added to it, from finished
// batches where their cigars lie or from records given on the host
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace {

// k_pileup_add over n records; returns whether some record's cigar ran past what it has
int32_t run_pileup_add(const Call &dev, npr_pileup *pl, int64_t n, const DeviceCigars &c, const std::vector<PileupRec> &recs, const uint8_t *d_seq, bool ascii) {
    DevBuf<PileupRec> rc;
    dev.upload(rc, recs);
    dev.zero(pl->bad);
    const PileupArgs a{n, c.off, c.ops, rc.p, d_seq, ascii ? 1 : 0, pl->tab.p, pl->diff.p, pl->bad.p};
    dev.launched(launch_pileup_add(a, dev.ctx->stream), "k_pileup_add");
    int32_t bad = 0;
    dev.fetch(&bad, pl->bad.p, sizeof(int32_t));
    dev.sync();  // (the cigars may lie in the arena, whose lock the caller holds until here)
    return bad;
}

}  // namespace

void npr_impl::pileup_scan(const Call &dev, npr_pileup *pl) {
    const int64_t n_refs = static_cast<int64_t>(pl->len.size()), n_slots = pl->rows + n_refs;
    const PileupScanArgs a{n_slots, n_refs, pl->dbase.p, pl->diff.p, pl->tile.p, pl->tab.p};
    dev.launched(launch_pileup_scan(a, dev.ctx->stream), "k_pileup_scan");
}

extern "C" {

int32_t npr_pileup_create(npr_ctx *ctx, int64_t n_refs, const int64_t *ref_len, npr_pileup **out) {
    if (!ctx || !out || n_refs < 0 || (n_refs && !ref_len)) return NPR_ERR_INVALID;
    *out = nullptr;
    return guarded(ctx, "npr_pileup_create", [&](const Call &dev) -> int32_t {
        std::unique_ptr<npr_pileup> pl(new npr_pileup);
        pl->ctx = ctx;
        pl->len.assign(ref_len, ref_len + n_refs);
        pl->base.assign(n_refs + 1, 0);
        std::vector<int64_t> dbase(n_refs + 1, 0);
        for (int64_t k = 0; k < n_refs; ++k) {
            if (ref_len[k] < 0 || ref_len[k] >= (int64_t(1) << 31) - 1) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_create: a reference length is negative or 2^31 and more");
            pl->base[k + 1] = pl->base[k] + ref_len[k];
            dbase[k + 1] = pl->base[k + 1] + k + 1;
        }
        pl->rows = pl->base[n_refs];
        const int64_t n_slots = pl->rows + n_refs;
        dev.alloc(pl->tab, static_cast<size_t>(pl->rows) * NPR_PILEUP_WORDS);
        dev.alloc(pl->diff, static_cast<size_t>(n_slots));
        dev.alloc(pl->tile, static_cast<size_t>(scan_tiles(n_slots)));
        dev.alloc(pl->bad, 1);
        dev.zero(pl->tab);
        dev.zero(pl->diff);
        dev.upload(pl->dbase, dbase);
        dev.sync();
        *out = pl.release();
        return NPR_OK;
    });
}

void npr_pileup_destroy(npr_pileup *pl) {
    if (!pl) return;
    (void)hipSetDevice(pl->ctx->device);
    delete pl;
}

int32_t npr_pileup_add_batch(npr_pileup *pl, npr_batch *b, const uint8_t *use) {
    if (!pl || !b || b->ctx != pl->ctx) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = pl->ctx;
    return guarded(ctx, "npr_pileup_add_batch", [&](const Call &dev) -> int32_t {
        const int64_t n = b->n_reads, n_refs = static_cast<int64_t>(pl->len.size());
        if (n == 0) return NPR_OK;
        // a read's window: the batch holds its base codes whole (reference part, then read part, from the first base of the read's first
        // task back to position 0, as npr_batch_indel_kmers uses them); its first reference position is the window start it was staged with
        std::vector<PileupRec> recs(n, PileupRec{0, 0, 0, -1, 0});
        int32_t unfit = 0, bad = 0;
        for (int64_t i = 0; i < n; ++i) {
            if ((use && !use[i]) || b->results[i].status != NPR_OK || b->read_ntasks[i] <= 0) continue;
            const int64_t k = b->ref_id[i], gx = b->gstart[2 * i];
            if (k < 0 || k >= n_refs || gx < 0 || gx + b->ref_len[i] > pl->len[k]) {
                unfit = 1;
                continue;
            }
            const Task &t = b->tasks[b->task_of[b->read_first_task[i]]];
            recs[i] = PileupRec{pl->base[k] + gx, pl->base[k] + k + gx, t.y_off - t.ys, static_cast<int32_t>(b->ref_len[i]), static_cast<int32_t>(b->read_len[i])};
        }
        with_batch_cigars(dev, b, [&](const DeviceCigars &c) { bad = run_pileup_add(dev, pl, n, c, recs, b->d_seq.p, false); });
        if (unfit) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_batch: a read's window does not fit its reference in the pileup (the read was left out)");
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_batch: a cigar runs past its window (the read was left out)") : NPR_OK;
    });
}

int32_t npr_pileup_add(npr_pileup *pl, int64_t n, const int32_t *ref_index, const uint8_t *read, const int64_t *read_begin, const int64_t *read_end,
                       const int32_t *ops, const int64_t *ops_off, const int64_t *start, const uint8_t *use) {
    if (!pl || n < 0 || (n && (!ref_index || !read_begin || !ops_off))) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (n == 0) return NPR_OK;
    if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: too many records");
    return guarded(ctx, "npr_pileup_add", [&](const Call &dev) -> int32_t {
        const int64_t n_refs = static_cast<int64_t>(pl->len.size()), o0 = ops_off[0], n_ops = ops_off[n] - o0;
        if (n_ops < 0 || (n_ops && !ops)) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: operation offsets decrease");
        std::vector<PileupRec> recs(n, PileupRec{0, 0, 0, -1, 0});
        std::vector<int64_t> off(n + 1), ylen(n, 0);
        std::vector<uint8_t> malformed(n, 0);
        std::vector<uint32_t> packed(static_cast<size_t>(n_ops));
        for (int64_t i = 0; i <= n; ++i) {
            off[i] = ops_off[i] - o0;
            if (i && off[i] < off[i - 1]) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: operation offsets decrease");
        }
        parallel_for(n, ctx->host_threads, [&](int64_t i) {
            const bool selected = !use || use[i];
            const int64_t k = ref_index[i], sx = start ? start[2 * i] : 0, sy = start ? start[2 * i + 1] : 0;
            const int64_t len = (read_end ? read_end[i] : read_begin[i + 1]) - read_begin[i];
            bool ok = k >= 0 && k < n_refs && len >= 0 && len < (int64_t(1) << 31) && sx >= 0 && sy >= 0 && sy <= len;
            ok = ok && sx <= pl->len[k];
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
            ylen[i] = len - sy;
            recs[i] = PileupRec{pl->base[k] + sx, pl->base[k] + k + sx, 0, static_cast<int32_t>(pl->len[k] - sx), static_cast<int32_t>(len - sy)};
        });
        // the read bases the selected records' cigars start at: uploaded as they are when the reads lie back to back, else gathered first
        DevBuf<uint8_t> d_seq;
        std::unique_ptr<uint8_t[]> gathered;
        int64_t bytes = 0;
        const uint8_t *src = nullptr;
        if (!read_end) {
            bytes = read_begin[n] - read_begin[0];
            if (bytes < 0 || (bytes && !read)) return NPR_ERR_INVALID;
            src = bytes ? read + read_begin[0] : nullptr;
            for (int64_t i = 0; i < n; ++i)
                if (recs[i].xlen >= 0) recs[i].y_off = read_begin[i] - read_begin[0] + (start ? start[2 * i + 1] : 0);
        } else {
            for (int64_t i = 0; i < n; ++i)
                if (recs[i].xlen >= 0) recs[i].y_off = bytes, bytes += ylen[i];
            if (bytes && !read) return NPR_ERR_INVALID;
            gathered.reset(new uint8_t[bytes + 1]);
            parallel_for(n, ctx->host_threads, [&](int64_t i) {
                if (recs[i].xlen >= 0 && ylen[i]) std::memcpy(gathered.get() + recs[i].y_off, read + read_begin[i] + (start ? start[2 * i + 1] : 0), static_cast<size_t>(ylen[i]));
            });
            src = gathered.get();
        }
        dev.alloc(d_seq, static_cast<size_t>(bytes) + 1);
        dev.copy_up(d_seq.p, src, static_cast<size_t>(bytes));
        DeviceCigars c;
        cigars_from_host(dev, packed.data(), off, c);
        int32_t bad = run_pileup_add(dev, pl, n, c, recs, d_seq.p, true);
        for (int64_t i = 0; i < n; ++i) bad |= malformed[i];
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: a record is malformed or its cigar runs past its sequences (the record was left out)") : NPR_OK;
    });
}

int32_t npr_pileup_counts(npr_pileup *pl, int32_t *counts) {
    if (!pl || (pl->rows && !counts)) return NPR_ERR_INVALID;
    if (pl->rows == 0) return NPR_OK;
    return guarded(pl->ctx, "npr_pileup_counts", [&](const Call &dev) -> int32_t {
        pileup_scan(dev, pl);
        dev.fetch(counts, pl->tab.p, pl->tab.bytes());
        dev.sync();
        return NPR_OK;
    });
}

int32_t npr_pileup_depth(npr_pileup *pl, int32_t *depth, uint8_t *covered) {
    if (!pl || (pl->rows && (!depth || !covered))) return NPR_ERR_INVALID;
    if (pl->rows == 0) return NPR_OK;
    return guarded(pl->ctx, "npr_pileup_depth", [&](const Call &dev) -> int32_t {
        pileup_scan(dev, pl);
        DevBuf<int32_t> d_depth;
        DevBuf<uint8_t> d_cov;
        dev.alloc(d_depth, static_cast<size_t>(pl->rows));
        dev.alloc(d_cov, static_cast<size_t>(pl->rows));
        dev.launched(launch_pileup_depth(pl->tab.p, pl->rows, d_depth.p, d_cov.p, dev.ctx->stream), "k_pileup_depth");
        dev.fetch(depth, d_depth.p, d_depth.bytes());
        dev.fetch(covered, d_cov.p, d_cov.bytes());
        dev.sync();
        return NPR_OK;
    });
}

}  // extern "C"
