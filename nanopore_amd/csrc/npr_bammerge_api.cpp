// npr_bammerge_api.cpp -- npr_bam_streams_bam, npr_bam_merge_last, npr_bam_index: the checks, the launches of npr_bammerge.hip between the sort, the
// frames and the index kernels of npr_bam.hip / npr_deflate.hip, and the tables as the header defines them ("BAM streams to BAM files")
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h; the writer from SAM text: npr_bam_api.cpp)
#include "npr_api_internal.h"
#include "npr_bamrec.h"

namespace {

// the header of a BAM stream on the host: its n_ref l_ref values; false when it is not exactly a header (magic, l_text, n_ref, the names with their NULs)
bool header_refs(const uint8_t *h, int64_t len, std::vector<int64_t> &ref_len) {
    auto i32 = [&](int64_t at) {
        int32_t v;
        std::memcpy(&v, h + at, 4);
        return static_cast<int64_t>(v);
    };
    if (len < 12 || std::memcmp(h, "BAM\1", 4) != 0) return false;
    const int64_t l_text = i32(4);
    if (l_text < 0 || 12 + l_text > len) return false;
    int64_t at = 8 + l_text;
    const int64_t n_ref = i32(at);
    at += 4;
    if (n_ref < 0 || n_ref > (len - at) / 9) return false;
    ref_len.assign(static_cast<size_t>(n_ref), 0);
    for (int64_t k = 0; k < n_ref; ++k) {
        if (at + 4 > len) return false;
        const int64_t l_name = i32(at);
        if (l_name < 1 || at + 8 + l_name > len || h[at + 4 + l_name - 1] != 0) return false;
        ref_len[k] = i32(at + 4 + l_name);
        at += 8 + l_name;
    }
    return at == len;
}

std::vector<int64_t> linear_windows(const Call &dev, const std::vector<int64_t> &ref_len) {
    std::vector<int64_t> lin_off(ref_len.size() + 1, 0);
    for (size_t k = 0; k < ref_len.size(); ++k) {
        if (ref_len[k] < 1) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": a reference length below 1").c_str());
        lin_off[k + 1] = lin_off[k] + ((ref_len[k] - 1) >> 14) + 1;
    }
    return lin_off;
}

// The records of a list on the device measured (k_merge_measure) and, with `order`, placed (k_merge_place, the scan): the buffers of both.
struct MergeRun {
    DevBuf<const uint8_t *> src, place_src;
    DevBuf<BamRec> recs;
    DevBuf<BamMeasure> meas;
    DevBuf<int32_t> tid, flag, bad;
    DevBuf<int64_t> pos, size, tile;
    DevBuf<uint32_t> place_bin;
    MergeArgs a{};
    void alloc(const Call &dev, int64_t n) {
        const size_t room = static_cast<size_t>(std::max<int64_t>(n, 1));
        dev.alloc(src, room), dev.alloc(place_src, room), dev.alloc(recs, room), dev.alloc(meas, room), dev.alloc(tid, room), dev.alloc(flag, room), dev.alloc(pos, room);
        dev.alloc(size, room + 1), dev.alloc(tile, static_cast<size_t>(scan_tiles(n))), dev.alloc(place_bin, room);
        dev.alloc(bad, 1), dev.zero(bad);
        a.n = n, a.src = src.p, a.recs = recs.p, a.meas = meas.p, a.tid = tid.p, a.flag = flag.p, a.pos = pos.p, a.bad = bad.p;
        a.size_sorted = size.p, a.place_src = place_src.p, a.place_bin = place_bin.p;
    }
    void add(const Call &dev, const npr_bam_stream *bs, int64_t at) {
        dev.launched(launch_merge_sources(bs->stream.p, bs->rec_off.p, bs->n, src.p + at, dev.ctx->stream), "k_merge_sources");
    }
    // the records' bytes behind the header; refuses what k_merge_measure (and k_merge_ordered, when asked) refused
    int64_t place(const Call &dev, const uint32_t *order) {
        a.order = order;
        int64_t bytes = 0;
        int32_t why = 0;
        if (a.n) {
            dev.launched(launch_merge_place(a, dev.ctx->stream), "k_merge_place");
            dev.launched(launch_scan_tiled<int64_t, int64_t>(size.p, size.p, a.n, tile.p, dev.ctx->stream), "scan");
            dev.fetch(&bytes, size.p + a.n, sizeof(bytes));
        }
        dev.fetch(&why, bad.p, sizeof(why));
        dev.sync();
        const std::string entry(dev.entry);
        if (why == -1) dev.refuse(NPR_ERR_INVALID, (entry + ": the records are not in coordinate order").c_str());
        if (why == BR_WHY_OP) dev.refuse(NPR_ERR_INVALID, (entry + ": a cigar operation above 8").c_str());
        if (why != 0) dev.refuse(NPR_ERR_INVALID, (entry + ": malformed auxiliary fields under a placeholder cigar").c_str());
        return bytes;
    }
};

}  // namespace

extern "C" {

int64_t npr_bam_streams_bam(npr_ctx *ctx, npr_bam_stream *const *streams, int64_t n_streams, const uint8_t *header, int64_t header_len, int32_t sorted,
                            int32_t compress, uint8_t *bam_out, int64_t cap, int64_t *n_records, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin,
                            uint64_t *run_beg, uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor) {
    if (!ctx || !streams || n_streams < 1 || !header || header_len < 0 || cap < 0) return NPR_ERR_INVALID;
    int64_t n = 0;
    for (int64_t k = 0; k < n_streams; ++k) {
        if (!streams[k]) return NPR_ERR_INVALID;
        if (streams[k]->ctx != ctx) return fail(ctx, NPR_ERR_INVALID, "npr_bam_streams_bam: a stream of another context");
        if (streams[k]->ref_len != streams[0]->ref_len || streams[k]->name_off != streams[0]->name_off || streams[k]->names != streams[0]->names)
            return fail(ctx, NPR_ERR_INVALID, "npr_bam_streams_bam: the streams' reference sequences differ (their number, a length or a name)");
        n += streams[k]->n;
    }
    if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_bam_streams_bam: 2^31 records and more");
    const std::vector<int64_t> &ref_len = streams[0]->ref_len;
    const int64_t n_refs = static_cast<int64_t>(ref_len.size());
    std::vector<int64_t> header_ref_len;
    if (!header_refs(header, header_len, header_ref_len) || header_ref_len != ref_len)
        return fail(ctx, NPR_ERR_INVALID, "npr_bam_streams_bam: `header` is not a BAM header with the streams' n_ref and l_ref values");
    const bool index = sorted && bam_out;
    if (index && (!n_runs || !n_no_coor || (n && (!run_tid || !run_bin || !run_beg || !run_end)) || (n_refs && (!linear || !meta)))) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bam_streams_bam", [&](const Call &dev) -> int64_t {
        std::vector<int64_t> lin_off;
        if (index) lin_off = linear_windows(dev, ref_len);
        MergeRun run;
        run.alloc(dev, n);
        for (int64_t k = 0, at = 0; k < n_streams; at += streams[k]->n, ++k) run.add(dev, streams[k], at);
        dev.launched(launch_merge_measure(run.a, ctx->stream), "k_merge_measure");
        DevBuf<unsigned long long> d_keys;
        DevBuf<uint32_t> d_order;
        if (sorted && n) {
            dev.alloc(d_keys, n);
            dev.launched(launch_bam_sort_keys(n, run.tid.p, run.pos.p, run.flag.p, static_cast<int32_t>(n_refs), d_keys.p, ctx->stream), "k_sort_keys");
            sort_order(dev, d_keys, n, 33 + bits_of(static_cast<unsigned long long>(n_refs)), d_order);
        }
        const int64_t stream_len = header_len + run.place(dev, d_order.p), total = bgzf_length(stream_len);
        if (n_records) *n_records = n;
        if (!bam_out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        if (total / BGZF_PAYLOAD + 2 >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_bam_streams_bam: 2^31 BGZF blocks and more");

        DevBuf<uint8_t> d_raw, d_out;
        dev.alloc(d_raw, static_cast<size_t>(stream_len));
        dev.copy_up(d_raw.p, header, static_cast<size_t>(header_len));
        run.a.header_len = header_len, run.a.stream_len = stream_len, run.a.raw = d_raw.p;
        dev.check(hipEventRecord(ctx->ev0, ctx->stream), "hipEventRecord");
        dev.launched(launch_merge_gather(run.a, ctx->stream), "k_merge_gather");
        dev.check(hipEventRecord(ctx->ev1, ctx->stream), "hipEventRecord");
        BamArgs a{};
        a.n = n, a.header_len = header_len, a.n_refs = n_refs;
        a.recs = run.recs.p, a.meas = run.meas.p, a.order = d_order.p, a.size_sorted = run.size.p;
        DeflateRun deflate;
        int64_t written = total;
        if (compress) {
            deflate.launch(dev, d_raw.p, stream_len);
            written = deflate.finish(dev);
            dev.fetch(bam_out, deflate.packed.p, static_cast<size_t>(written));
            a.block_off = deflate.block_len.p;
        } else {
            dev.alloc(d_out, static_cast<size_t>(total));
            BgzfArgs z{};
            z.data = d_raw.p, z.len = stream_len, z.out = d_out.p;
            bgzf_constants(z);
            dev.launched(launch_bgzf_frame(z, ctx->stream), "k_bgzf_frame");
            dev.fetch(bam_out, d_out.p, static_cast<size_t>(total));
        }
        if (index) bam_index_tables(dev, a, lin_off, n_runs, run_tid, run_bin, run_beg, run_end, linear, meta, n_no_coor);
        else dev.sync();
        float ms = 0.f;
        dev.check(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1), "hipEventElapsedTime");
        ctx->merge_last[0] = n, ctx->merge_last[1] = stream_len, ctx->merge_last[2] = stream_len - header_len;
        ctx->merge_last[3] = static_cast<int64_t>(static_cast<double>(ms) * 1e6);
        return written;
    });
}

int32_t npr_bam_merge_last(npr_ctx *ctx, int64_t *out) {
    if (!ctx || !out) return NPR_ERR_INVALID;
    std::copy(ctx->merge_last, ctx->merge_last + 4, out);
    return NPR_OK;
}

int64_t npr_bam_index(npr_ctx *ctx, const uint8_t *file, int64_t len, int64_t *n_refs, int64_t *ref_len, int64_t cap_refs, int64_t *n_runs, int32_t *run_tid,
                      uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end, int64_t cap_runs, uint64_t *linear, int64_t cap_linear, uint64_t *meta,
                      int64_t *n_no_coor) {
    if (!ctx || !file || len < 0 || !n_refs || !n_runs || !n_no_coor || cap_refs < 0 || cap_runs < 0 || cap_linear < 0 || (cap_refs && (!ref_len || !meta)) ||
        (cap_runs && (!run_tid || !run_bin || !run_beg || !run_end)) || (cap_linear && !linear))
        return NPR_ERR_INVALID;
    npr_bam_stream *opened = nullptr;
    const int32_t rc = npr_bam_open(ctx, file, len, &opened);
    if (rc != NPR_OK) return rc;
    const std::unique_ptr<npr_bam_stream, void (*)(npr_bam_stream *)> bs(opened, npr_bam_close);
    return guarded(ctx, "npr_bam_index", [&](const Call &dev) -> int64_t {
        // the blocks, as npr_bam_open scanned them
        const std::vector<int64_t> &block_off = bs->block_off, &stream_off = bs->stream_off;
        const int64_t blocks = static_cast<int64_t>(block_off.size()) - 1;
        const int64_t n = bs->n, refs = static_cast<int64_t>(bs->ref_len.size());
        const std::vector<int64_t> lin_off = linear_windows(dev, bs->ref_len);

        MergeRun run;
        run.alloc(dev, n);
        run.add(dev, bs.get(), 0);
        dev.launched(launch_merge_measure(run.a, ctx->stream), "k_merge_measure");
        dev.launched(launch_merge_ordered(run.a, ctx->stream), "k_merge_ordered");
        const int64_t records_bytes = run.place(dev, nullptr);

        DevBuf<int64_t> d_block_off, d_stream_off;
        dev.upload(d_block_off, block_off), dev.upload(d_stream_off, stream_off);
        BamArgs a{};
        a.n = n, a.header_len = bs->stream_len - records_bytes, a.n_refs = refs;  // (the records of a file opened whole lie back to back behind its header)
        a.recs = run.recs.p, a.meas = run.meas.p, a.size_sorted = run.size.p;
        a.block_off = d_block_off.p, a.stream_off = d_stream_off.p, a.n_blocks = blocks;
        std::vector<int32_t> tid(static_cast<size_t>(n) + 1);
        std::vector<uint32_t> bin(static_cast<size_t>(n) + 1);
        std::vector<uint64_t> beg(static_cast<size_t>(n) + 1), end(static_cast<size_t>(n) + 1), lin(static_cast<size_t>(lin_off[refs]) + 1), mt(4 * static_cast<size_t>(refs) + 1);
        int64_t runs = 0, no_coor = 0;
        bam_index_tables(dev, a, lin_off, &runs, tid.data(), bin.data(), beg.data(), end.data(), lin.data(), mt.data(), &no_coor);
        *n_refs = refs, *n_runs = runs;  // (both needed counts are set on NPR_ERR_CAPACITY, and the runs are known only now: the caps are looked at here)
        if (refs > cap_refs || runs > cap_runs || lin_off[refs] > cap_linear) return NPR_ERR_CAPACITY;
        std::copy(bs->ref_len.begin(), bs->ref_len.end(), ref_len);
        std::copy(tid.begin(), tid.begin() + runs, run_tid), std::copy(bin.begin(), bin.begin() + runs, run_bin);
        std::copy(beg.begin(), beg.begin() + runs, run_beg), std::copy(end.begin(), end.begin() + runs, run_end);
        std::copy(lin.begin(), lin.begin() + lin_off[refs], linear), std::copy(mt.begin(), mt.begin() + 4 * refs, meta);
        *n_no_coor = no_coor;
        return n;
    });
}

}  // extern "C"
