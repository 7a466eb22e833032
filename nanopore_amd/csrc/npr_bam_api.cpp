// npr_bam_api.cpp -- npr_bam_sort_order, npr_bgzf_frame, npr_bgzf_deflate, npr_deflate_last, npr_bgzf_inflate, npr_inflate_last, npr_sam_bam, npr_sam_bam_deflate,
// npr_bam_sam, npr_bam_open / _close / _stream_info / _stream_refs, npr_pileup_add_bam, npr_bam_open_region, npr_bam_stream_restrict, npr_bam_stream_sam: the checks, the records as the
// kernels take them, the launches of npr_bam.hip, npr_deflate.hip, npr_inflate.hip, npr_bamread.hip, npr_bampile.hip and npr_bamregion.hip, and the tables as the header defines them ("coordinate-sorted BAM")
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

static_assert(BGZF_PAYLOAD == NPR_BGZF_PAYLOAD && BAM_TILE == NPR_BAM_TILE, "the kernels' constants are the header's");

// ---- what npr_bammerge_api.cpp shares with the writer here (declared in npr_api_internal.h, with DeflateRun) ----
namespace npr_impl {

constexpr uint32_t kCrcPoly = 0xEDB88320u;

static uint32_t gf_mul(uint32_t a, uint32_t b) {  // a * b modulo the CRC polynomial, reflected (bit 31 is x^0)
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

void bgzf_constants(BgzfArgs &a) {
    a.x2n[0] = 0x40000000u;  // x^1
    for (int k = 1; k < 32; ++k) a.x2n[k] = gf_mul(a.x2n[k - 1], a.x2n[k - 1]);
    for (int lv = 0; lv < 8; ++lv) {  // x^(8 * BGZF_SLICE * 2^lv)
        uint32_t p = 0x80000000u;
        uint32_t bytes = static_cast<uint32_t>(BGZF_SLICE) << lv;
        for (int k = 3; bytes; bytes >>= 1, ++k)
            if (bytes & 1) p = gf_mul(a.x2n[k & 31], p);
        a.level[lv] = p;
    }
}

int64_t bgzf_length(int64_t len) { return len + BGZF_OVERHEAD * ((len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD) + BGZF_EOF; }

int bits_of(unsigned long long v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// The stable order of n keys of at most `bits` bits that lie on the device: d_order[j] = index of the key at place j (the identity without a pass).
// The keys are overwritten.
void sort_order(const Call &dev, DevBuf<unsigned long long> &keys, int64_t n, int bits, DevBuf<uint32_t> &d_order) {
    const int64_t blocks = bam_sort_blocks(n);
    DevBuf<unsigned long long> keys2;
    DevBuf<uint32_t> vals2, hist;
    DevBuf<int32_t> tile;
    dev.alloc(d_order, n), dev.alloc(vals2, n), dev.alloc(keys2, n);
    dev.alloc(hist, BAM_SORT_DIGITS * blocks + 1);
    dev.alloc(tile, scan_tiles(BAM_SORT_DIGITS * blocks));
    const int passes = std::max(1, (bits + BAM_SORT_BITS - 1) / BAM_SORT_BITS);
    // the last pass writes into d_order: with an odd number of passes the first one does too
    unsigned long long *kin = keys.p, *kout = keys2.p;
    uint32_t *vin = nullptr, *vout = (passes & 1) ? d_order.p : vals2.p;
    for (int p = 0; p < passes; ++p) {
        BamSortArgs a{n, p * BAM_SORT_BITS, kin, vin, kout, vout, hist.p, tile.p};
        dev.launched(launch_bam_sort_pass(a, dev.ctx->stream), "k_sort_hist / scan / k_sort_scatter");
        std::swap(kin, kout);
        vin = vout, vout = vout == d_order.p ? vals2.p : d_order.p;
    }
    dev.sync();  // (the scratch of the passes goes out of scope)
}

}  // namespace npr_impl

namespace {

int64_t sam_bam(const char *entry, bool compress, npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields, const int64_t *tail,
                int64_t n, const int64_t *tag_off, const uint8_t *tags, const uint8_t *header, int64_t header_len, int64_t n_refs, const int64_t *ref_len,
                int32_t sorted, uint8_t *bam_out, int64_t cap, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end,
                uint64_t *linear, uint64_t *meta, int64_t *n_no_coor);

// npr_bgzf_scan into vectors of blocks + 1 entries: one pass over the file as a rule (room for a block per 16 KiB of file: a block of 64 KiB
// of payload seldom compresses below a quarter), a second one when there are more.  Returns what the scan returns.
int64_t scan_table(const uint8_t *file, int64_t len, std::vector<int64_t> &block_off, std::vector<int64_t> &stream_off) {
    int64_t blocks = 0, cap = len / 16384 + 64;
    for (int pass = 0;; ++pass) {
        block_off.resize(static_cast<size_t>(cap)), stream_off.resize(static_cast<size_t>(cap));
        const int64_t total = npr_bgzf_scan(file, len, block_off.data(), stream_off.data(), cap, &blocks);
        if (total == NPR_ERR_CAPACITY && pass == 0) {
            cap = blocks + 1;
            continue;
        }
        if (total >= 0) block_off.resize(static_cast<size_t>(blocks) + 1), stream_off.resize(static_cast<size_t>(blocks) + 1);
        return total;
    }
}

int dec_digits(uint32_t v) {
    int k = 1;
    while (v >= 10u) v /= 10u, ++k;
    return k;
}

// A BGZF file image inflated on the device: the buffers of one npr_inflate.hip run.  launch() takes the block table npr_bgzf_scan made and
// queues the kernel; finish() fetches the blocks' statuses, waits, fills the context's inflate_last and refuses the file when a block was
// refused; the payloads then lie in stream.
struct InflateRun {
    DevBuf<uint8_t> file, stream;
    DevBuf<int64_t> block_off, stream_off;
    DevBuf<int32_t> status;
    int64_t blocks = 0, stream_len = 0;
    std::vector<int64_t> b_sub;
    void launch(const Call &dev, const uint8_t *image, int64_t len, const std::vector<int64_t> &b_off, const std::vector<int64_t> &s_off) {
        dev.upload(file, image, static_cast<size_t>(len));
        queue(dev, b_off, s_off);
    }
    // The blocks pick[0 ..] of the scan's table alone (ascending indices): only their bytes cross, back to back, a run of neighbours in one copy,
    // and their payloads make a COMPACT stream; s_sub[j] = where the payload of block pick[j] begins in it, last its length.  (k_bgzf_inflate
    // takes a block's size from the next entry of the table: the picked blocks get a table of their own, re-based on the bytes that crossed.)
    void launch_picked(const Call &dev, const uint8_t *image, const std::vector<int64_t> &b_off, const std::vector<int64_t> &s_off, const std::vector<int64_t> &pick,
                       std::vector<int64_t> &s_sub) {
        b_sub.assign(pick.size() + 1, 0);  // (a member: the upload is queued, and waited for in finish())
        s_sub.assign(pick.size() + 1, 0);
        for (size_t j = 0; j < pick.size(); ++j) {
            b_sub[j + 1] = b_sub[j] + (b_off[pick[j] + 1] - b_off[pick[j]]);
            s_sub[j + 1] = s_sub[j] + (s_off[pick[j] + 1] - s_off[pick[j]]);
        }
        dev.alloc(file, static_cast<size_t>(std::max<int64_t>(b_sub.back(), 1)));
        for (size_t j = 0; j < pick.size();) {
            size_t k = j + 1;
            while (k < pick.size() && pick[k] == pick[k - 1] + 1) ++k;
            dev.copy_up(file.p + b_sub[j], image + b_off[pick[j]], static_cast<size_t>(b_sub[k] - b_sub[j]));
            j = k;
        }
        queue(dev, b_sub, s_sub);
    }
    void queue(const Call &dev, const std::vector<int64_t> &b_off, const std::vector<int64_t> &s_off) {
        blocks = static_cast<int64_t>(b_off.size()) - 1, stream_len = s_off.back();
        dev.upload(block_off, b_off), dev.upload(stream_off, s_off);
        dev.alloc(stream, static_cast<size_t>(std::max<int64_t>(stream_len, 1)));
        dev.alloc(status, static_cast<size_t>(std::max<int64_t>(blocks, 1)));
        InflateArgs a{};
        bgzf_constants(a.z);
        a.file = file.p, a.block_off = block_off.p, a.stream_off = stream_off.p, a.blocks = blocks, a.stream = stream.p, a.status = status.p;
        dev.launched(launch_bgzf_inflate(a, dev.ctx->stream), "k_bgzf_inflate");
    }
    void finish(const Call &dev) {
        std::vector<int32_t> st(static_cast<size_t>(blocks), 0);
        dev.fetch(st.data(), status.p, st.size() * sizeof(int32_t));
        dev.sync();
        int64_t *last = dev.ctx->inflate_last;
        last[0] = blocks, last[1] = -1, last[2] = 0, last[3] = stream_len;
        for (int64_t b = 0; b < blocks; ++b)
            if (st[b] != 0) {
                last[1] = b, last[2] = st[b];
                char text[160];
                std::snprintf(text, sizeof(text), "%s: BGZF block %lld is refused (inflate status %d)", dev.entry, static_cast<long long>(b), st[b]);
                dev.refuse(NPR_ERR_INVALID, text);
            }
    }
};

// The header of a BAM stream on the device (npr_bam_sam, npr_bam_open): k_bam_head checks it and gives its end, its bytes cross once for the names
// (back to back, without NULs) and, when asked for, every l_ref.  Refuses a stream without the magic or with a header that runs past it.
struct BamHeader {
    int64_t end, l_text, n_ref;
};
BamHeader bam_header(const Call &dev, const uint8_t *d_stream, int64_t stream_len, std::vector<uint8_t> &names, std::vector<int64_t> &name_off, std::vector<int64_t> *ref_len) {
    DevBuf<int64_t> d_head;
    int64_t head[4] = {0, 0, 0, 0};
    dev.alloc(d_head, 4);
    dev.launched(launch_bam_head(d_stream, stream_len, d_head.p, dev.ctx->stream), "k_bam_head");
    dev.fetch(head, d_head.p, sizeof(head));
    dev.sync();
    if (head[0] != 0) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": no BAM magic, or a header that runs past the stream").c_str());
    const BamHeader h{head[1], head[2], head[3]};
    std::vector<uint8_t> header(static_cast<size_t>(h.end));
    dev.fetch(header.data(), d_stream, header.size());
    dev.sync();
    names.clear(), name_off.assign(static_cast<size_t>(h.n_ref) + 1, 0);
    if (ref_len) ref_len->assign(static_cast<size_t>(h.n_ref), 0);
    for (int64_t k = 0, at = 8 + h.l_text + 4; k < h.n_ref; ++k) {  // (k_bam_head checked every l_name against the header's end)
        int32_t l_name, l_ref;
        std::memcpy(&l_name, header.data() + at, 4);
        std::memcpy(&l_ref, header.data() + at + 4 + l_name, 4);
        names.insert(names.end(), header.begin() + at + 4, header.begin() + at + 4 + l_name - 1);
        name_off[k + 1] = static_cast<int64_t>(names.size());
        if (ref_len) (*ref_len)[k] = l_ref;
        at += 8 + l_name;
    }
    return h;
}

// The records rec_off[0, n) (on the device) of a BAM stream there as SAM text: the header text and a line per record -- what npr_bam_sam and
// npr_bam_stream_sam do once they know where the records lie.  Returns the text's length; sam_out == NULL: only that.
int64_t sam_lines(const Call &dev, const uint8_t *d_stream, int64_t stream_len, int64_t l_text, int64_t n_ref, const std::vector<uint8_t> &names,
                  const std::vector<int64_t> &name_off, const int64_t *d_rec_off, int64_t n, uint8_t *sam_out, int64_t cap, int64_t *n_records) {
    const std::string entry(dev.entry);
    DevBuf<uint8_t> d_names, d_aux, d_text, d_out;
    DevBuf<int64_t> d_name_off, d_aux_off, d_cg, d_text_off, d_line_off, d_tile;
    DevBuf<BamReadRec> d_meas;
    DevBuf<int32_t> d_bad;
    DevBuf<unsigned long long> d_items;
    BamReadArgs a{};
    a.stream = d_stream, a.len = stream_len, a.n_ref = static_cast<int32_t>(n_ref), a.n = n;
    dev.upload(d_names, names), dev.upload(d_name_off, name_off);
    dev.alloc(d_meas, n), dev.alloc(d_bad, 1), dev.zero(d_bad);
    a.names = d_names.p, a.name_off = d_name_off.p, a.rec_off = d_rec_off, a.meas = d_meas.p, a.bad = d_bad.p;
    dev.launched(launch_bam_read_measure(a, dev.ctx->stream), "k_bam_measure");
    std::vector<BamReadRec> meas(static_cast<size_t>(n));
    int32_t bad = 0;
    dev.fetch(meas.data(), d_meas.p, d_meas.bytes());
    dev.fetch(&bad, d_bad.p, sizeof(bad));
    dev.sync();
    if (bad) dev.refuse(NPR_ERR_INVALID, (entry + ": a cigar operation above 8").c_str());

    // the auxiliary bytes: packed, down once, to text on the host, up again
    std::vector<int64_t> aux_off(static_cast<size_t>(n) + 1, 0), text_off(static_cast<size_t>(n) + 1, 0), cg(2 * static_cast<size_t>(n) + 2, -1);
    std::vector<uint8_t> placeholder(static_cast<size_t>(n) + 1, 0);
    for (int64_t i = 0; i < n; ++i) aux_off[i + 1] = aux_off[i] + meas[i].aux_len, placeholder[i] = meas[i].placeholder != 0;
    std::vector<uint8_t> aux(static_cast<size_t>(aux_off[n]) + 1);
    dev.upload(d_aux_off, aux_off), dev.alloc(d_aux, aux.size());
    a.aux_pack_off = d_aux_off.p, a.aux_pack = d_aux.p;
    dev.launched(launch_bam_gather_aux(a, dev.ctx->stream), "k_bam_gather_aux");
    dev.fetch(aux.data(), d_aux.p, static_cast<size_t>(aux_off[n]));
    dev.sync();
    const int64_t text_len = npr_bam_aux_text(aux.data(), aux_off.data(), n, placeholder.data(), text_off.data(), cg.data(), nullptr, 0);
    if (text_len < 0) dev.refuse(static_cast<int32_t>(text_len), (entry + ": a malformed auxiliary field").c_str());
    std::vector<uint8_t> text(static_cast<size_t>(text_len) + 1);
    if (npr_bam_aux_text(aux.data(), aux_off.data(), n, placeholder.data(), text_off.data(), cg.data(), text.data(), text_len) != text_len)
        dev.refuse(NPR_ERR_STATE, (entry + ": the auxiliary text changed its length").c_str());

    // the lines' lengths, their offsets by the device's scan, the (record, tile) items
    std::vector<int64_t> line_len(static_cast<size_t>(n) + 1, 0);
    std::vector<unsigned long long> items;
    int64_t lines = 0;
    for (int64_t i = 0; i < n; ++i) {
        int64_t cig = meas[i].cig_len;
        if (cg[2 * i] >= 0) {
            cig = cg[2 * i + 1] ? 0 : 1;
            const uint8_t *ops = aux.data() + aux_off[i] + cg[2 * i];
            for (int64_t q = 0; q < cg[2 * i + 1]; ++q) {
                uint32_t v;
                std::memcpy(&v, ops + 4 * q, 4);
                cig += dec_digits(v >> 4) + 1;
            }
        }
        const int64_t tl = text_off[i + 1] - text_off[i];
        line_len[i] = meas[i].fixed_len - meas[i].cig_len + cig + (tl ? 1 + tl : 0) + 1;
        lines += line_len[i];
        const int64_t tiles = std::max<int64_t>(1, (static_cast<int64_t>(meas[i].l_seq) + BAM_TILE - 1) / BAM_TILE);
        for (int64_t k = 0; k < tiles; ++k) items.push_back(static_cast<unsigned long long>(i) << 32 | static_cast<unsigned long long>(k));
    }
    if (items.size() >= (size_t(1) << 31)) dev.refuse(NPR_ERR_INVALID, (entry + ": 2^31 tiles and more in one call").c_str());
    const int64_t total = l_text + lines;
    if (!sam_out) {
        if (n_records) *n_records = n;
        return total;
    }
    if (cap < total) return NPR_ERR_CAPACITY;
    dev.upload(d_line_off, line_len), dev.alloc(d_tile, scan_tiles(n));
    dev.launched(launch_scan_tiled<int64_t, int64_t>(d_line_off.p, d_line_off.p, n, d_tile.p, dev.ctx->stream), "scan");
    dev.upload(d_cg, cg), dev.upload(d_text, text), dev.upload(d_text_off, text_off), dev.upload(d_items, items);
    dev.alloc(d_out, static_cast<size_t>(std::max<int64_t>(total, 1)));
    if (l_text) dev.check(hipMemcpyAsync(d_out.p, d_stream + 8, static_cast<size_t>(l_text), hipMemcpyDeviceToDevice, dev.ctx->stream), "D2D");
    a.cg = d_cg.p, a.aux_text = d_text.p, a.aux_text_off = d_text_off.p, a.line_off = d_line_off.p, a.items = d_items.p;
    a.n_items = static_cast<int64_t>(items.size()), a.out = d_out.p + l_text;
    dev.launched(launch_bam_emit(a, dev.ctx->stream), "k_bam_emit");
    dev.fetch(&bad, d_bad.p, sizeof(bad));
    dev.sync();
    if (bad) dev.failed(NPR_ERR_STATE, "k_bam_emit: a line's columns do not add up to its measured length", hipSuccess);
    dev.fetch(sam_out, d_out.p, static_cast<size_t>(total));
    dev.sync();
    if (n_records) *n_records = n;
    return total;
}

// The records d_rec[0, n) of a stream that overlap [beg, end) of reference tid, order preserved, into `kept` (k_bam_overlap, the scan,
// k_bam_gather of npr_bamregion.hip): how many.  Refuses malformed auxiliary fields under a placeholder cigar; `kept` is then not made.
int64_t overlap_filter(const Call &dev, const uint8_t *d_stream, const int64_t *d_rec, int64_t n, int32_t tid, int64_t beg, int64_t end, DevBuf<int64_t> &kept) {
    DevBuf<int64_t> d_keep, d_tile;
    DevBuf<int32_t> d_bad;
    dev.alloc(d_keep, static_cast<size_t>(n) + 1), dev.alloc(d_tile, static_cast<size_t>(scan_tiles(n)));
    dev.alloc(d_bad, 1), dev.zero(d_bad);
    BamOverlapArgs a{d_stream, n, d_rec, tid, beg, end, d_keep.p, d_bad.p, nullptr};
    dev.launched(launch_bam_overlap_flags(a, dev.ctx->stream), "k_bam_overlap");
    dev.launched(launch_scan_tiled<int64_t, int64_t>(d_keep.p, d_keep.p, n, d_tile.p, dev.ctx->stream), "scan");
    int64_t total = 0;
    int32_t bad = 0;
    dev.fetch(&total, d_keep.p + n, sizeof(total));
    dev.fetch(&bad, d_bad.p, sizeof(bad));
    dev.sync();
    if (bad) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": malformed auxiliary fields under a placeholder cigar").c_str());
    DevBuf<int64_t> out;
    dev.alloc(out, static_cast<size_t>(std::max<int64_t>(total, 1)));
    a.kept = out.p;
    dev.launched(launch_bam_overlap_gather(a, dev.ctx->stream), "k_bam_gather");
    dev.sync();  // (the flags go out of scope)
    kept.take(out);
    return total;
}

}  // namespace

extern "C" {

int32_t npr_bam_sort_order(npr_ctx *ctx, int64_t n, const int32_t *tid, const int64_t *pos, const int32_t *flag, int32_t *order) {
    if (!ctx || n < 0 || n >= (int64_t(1) << 31) || (n && (!tid || !pos || !flag || !order))) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bam_sort_order", [&](const Call &dev) -> int32_t {
        int64_t max_pos = 0;
        int32_t max_tid = -1;
        for (int64_t i = 0; i < n; ++i) {
            if (tid[i] < -1 || tid[i] >= (1 << 30) || pos[i] < -1 || pos[i] > (int64_t(1) << 31) - 2) return fail(ctx, NPR_ERR_INVALID, "npr_bam_sort_order: a tid or pos out of range");
            max_pos = std::max(max_pos, pos[i] + 1), max_tid = std::max(max_tid, tid[i]);
        }
        if (n == 0) return NPR_OK;
        const int32_t no_tid = max_tid + 1;
        const int bits = no_tid ? 33 + bits_of(static_cast<unsigned long long>(no_tid)) : bits_of(static_cast<unsigned long long>(max_pos) << 1 | 1);
        DevBuf<int32_t> d_tid, d_flag;
        DevBuf<int64_t> d_pos;
        DevBuf<unsigned long long> keys;
        DevBuf<uint32_t> d_order;
        dev.upload(d_tid, tid, n), dev.upload(d_pos, pos, n), dev.upload(d_flag, flag, n);
        dev.alloc(keys, n);
        dev.launched(launch_bam_sort_keys(n, d_tid.p, d_pos.p, d_flag.p, no_tid, keys.p, ctx->stream), "k_sort_keys");
        sort_order(dev, keys, n, bits, d_order);
        dev.fetch(order, d_order.p, d_order.bytes());
        dev.sync();
        return NPR_OK;
    });
}

int64_t npr_bgzf_frame(npr_ctx *ctx, const uint8_t *data, int64_t len, uint8_t *out, int64_t cap) {
    if (!ctx || len < 0 || (len && !data) || cap < 0) return NPR_ERR_INVALID;
    const int64_t total = bgzf_length(len);
    if (!out) return total;
    if (cap < total) return NPR_ERR_CAPACITY;
    if ((len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD + 1 >= (int64_t(1) << 31)) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bgzf_frame", [&](const Call &dev) -> int64_t {
        DevBuf<uint8_t> d_in, d_out;
        dev.upload(d_in, data, static_cast<size_t>(len));
        dev.alloc(d_out, static_cast<size_t>(total));
        BgzfArgs a{};
        a.data = d_in.p, a.len = len, a.out = d_out.p;
        bgzf_constants(a);
        dev.launched(launch_bgzf_frame(a, ctx->stream), "k_bgzf_frame");
        dev.fetch(out, d_out.p, static_cast<size_t>(total));
        dev.sync();
        return total;
    });
}

int64_t npr_bgzf_deflate(npr_ctx *ctx, const uint8_t *data, int64_t len, uint8_t *out, int64_t cap, int64_t *block_off) {
    if (!ctx || len < 0 || (len && !data) || cap < 0) return NPR_ERR_INVALID;
    const int64_t bound = bgzf_length(len);
    if (!out) return bound;
    if (cap < bound) return NPR_ERR_CAPACITY;
    if ((len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD + 1 >= (int64_t(1) << 31)) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bgzf_deflate", [&](const Call &dev) -> int64_t {
        DevBuf<uint8_t> d_in;
        DeflateRun run;
        dev.upload(d_in, data, static_cast<size_t>(len));
        run.launch(dev, d_in.p, len);
        const int64_t total = run.finish(dev);
        dev.fetch(out, run.packed.p, static_cast<size_t>(total));
        dev.sync();
        if (block_off) std::copy(run.block_off.begin(), run.block_off.end(), block_off);
        return total;
    });
}

int32_t npr_deflate_last(npr_ctx *ctx, int64_t *out) {
    if (!ctx || !out) return NPR_ERR_INVALID;
    std::copy(ctx->deflate_last, ctx->deflate_last + 4, out);
    return NPR_OK;
}

int64_t npr_bgzf_inflate(npr_ctx *ctx, const uint8_t *file, int64_t len, uint8_t *out, int64_t cap) {
    if (!ctx || !file || len < 0 || cap < 0) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bgzf_inflate", [&](const Call &dev) -> int64_t {
        std::vector<int64_t> block_off, stream_off;
        const int64_t total = scan_table(file, len, block_off, stream_off);
        if (total < 0) dev.refuse(NPR_ERR_INVALID, "npr_bgzf_inflate: not a BGZF file that ends with the end-of-file block");
        if (!out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        if (block_off.size() >= (size_t(1) << 31)) return NPR_ERR_INVALID;
        InflateRun run;
        run.launch(dev, file, len, block_off, stream_off);
        run.finish(dev);
        dev.fetch(out, run.stream.p, static_cast<size_t>(total));
        dev.sync();
        return total;
    });
}

int64_t npr_bam_sam(npr_ctx *ctx, const uint8_t *file, int64_t len, uint8_t *sam_out, int64_t cap, int64_t *n_records) {
    if (!ctx || !file || len < 0 || cap < 0) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_bam_sam", [&](const Call &dev) -> int64_t {
        std::vector<int64_t> block_off, stream_off;
        if (scan_table(file, len, block_off, stream_off) < 0) dev.refuse(NPR_ERR_INVALID, "npr_bam_sam: not a BGZF file that ends with the end-of-file block");
        if (block_off.size() >= (size_t(1) << 31)) return NPR_ERR_INVALID;
        InflateRun run;
        run.launch(dev, file, len, block_off, stream_off);
        run.finish(dev);
        const int64_t stream_len = run.stream_len;
        const uint8_t *const d_stream = run.stream.p;

        std::vector<uint8_t> names;
        std::vector<int64_t> name_off;
        const BamHeader h = bam_header(dev, d_stream, stream_len, names, name_off, nullptr);
        const int64_t header_end = h.end, l_text = h.l_text, n_ref = h.n_ref;

        // the records: the block_size chain in rounds into a table of fixed size
        constexpr int64_t kWalk = int64_t(1) << 18;
        DevBuf<int64_t> d_table, d_walk;
        dev.alloc(d_table, kWalk), dev.alloc(d_walk, 3);
        std::vector<int64_t> rec_off;
        for (int64_t at = header_end; at < stream_len;) {
            int64_t w[3] = {0, 0, 0};
            dev.launched(launch_bam_walk(d_stream, stream_len, at, static_cast<int32_t>(n_ref), d_table.p, kWalk, d_walk.p, ctx->stream), "k_bam_walk");
            dev.fetch(w, d_walk.p, sizeof(w));
            dev.sync();
            if (w[2] != 0 || w[0] <= 0) {
                char text[160];
                std::snprintf(text, sizeof(text), "npr_bam_sam: record %lld at stream byte %lld is refused (walk status %lld)", static_cast<long long>(rec_off.size() + w[0]),
                              static_cast<long long>(w[1]), static_cast<long long>(w[2]));
                dev.refuse(NPR_ERR_INVALID, text);
            }
            const size_t had = rec_off.size();
            rec_off.resize(had + static_cast<size_t>(w[0]));
            dev.fetch(rec_off.data() + had, d_table.p, static_cast<size_t>(w[0]) * sizeof(int64_t));
            dev.sync();
            at = w[1];
        }
        const int64_t n = static_cast<int64_t>(rec_off.size());
        if (n >= (int64_t(1) << 31)) dev.refuse(NPR_ERR_INVALID, "npr_bam_sam: 2^31 records and more");

        DevBuf<int64_t> d_rec_off;
        dev.upload(d_rec_off, rec_off);
        return sam_lines(dev, d_stream, stream_len, l_text, n_ref, names, name_off, d_rec_off.p, n, sam_out, cap, n_records);
    });
}

int32_t npr_inflate_last(npr_ctx *ctx, int64_t *out) {
    if (!ctx || !out) return NPR_ERR_INVALID;
    std::copy(ctx->inflate_last, ctx->inflate_last + 4, out);
    return NPR_OK;
}

int32_t npr_bam_open(npr_ctx *ctx, const uint8_t *file, int64_t len, npr_bam_stream **out) {
    if (!ctx || !file || len < 0 || !out) return NPR_ERR_INVALID;
    *out = nullptr;
    return guarded(ctx, "npr_bam_open", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> block_off, stream_off;
        if (scan_table(file, len, block_off, stream_off) < 0) dev.refuse(NPR_ERR_INVALID, "npr_bam_open: not a BGZF file that ends with the end-of-file block");
        if (block_off.size() >= (size_t(1) << 31)) return NPR_ERR_INVALID;
        std::unique_ptr<npr_bam_stream> bs(new npr_bam_stream);
        bs->ctx = ctx;
        {
            InflateRun run;  // (the file image and the block tables go when the stream is made)
            run.launch(dev, file, len, block_off, stream_off);
            run.finish(dev);
            bs->stream_len = run.stream_len;
            bs->stream.take(run.stream);
        }
        const uint8_t *const d_stream = bs->stream.p;
        const BamHeader h = bam_header(dev, d_stream, bs->stream_len, bs->names, bs->name_off, &bs->ref_len);
        bs->l_text = h.l_text;

        // the records: the block_size chain in rounds of fixed size into a table that stays on the device and doubles when it is full
        constexpr int64_t kWalk = int64_t(1) << 18;
        DevBuf<int64_t> d_walk;
        int64_t cap = kWalk, n = 0;
        dev.alloc(bs->rec_off, cap), dev.alloc(d_walk, 3);
        for (int64_t at = h.end; at < bs->stream_len;) {
            if (n + kWalk > cap) {
                DevBuf<int64_t> wider;
                dev.alloc(wider, 2 * cap);
                dev.check(hipMemcpyAsync(wider.p, bs->rec_off.p, static_cast<size_t>(n) * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream), "D2D");
                dev.sync();
                bs->rec_off.take(wider);
                cap *= 2;
            }
            int64_t w[3] = {0, 0, 0};
            dev.launched(launch_bam_walk(d_stream, bs->stream_len, at, static_cast<int32_t>(h.n_ref), bs->rec_off.p + n, kWalk, d_walk.p, ctx->stream), "k_bam_walk");
            dev.fetch(w, d_walk.p, sizeof(w));
            dev.sync();
            if (w[2] != 0 || w[0] <= 0) {
                char text[160];
                std::snprintf(text, sizeof(text), "npr_bam_open: record %lld at stream byte %lld is refused (walk status %lld)", static_cast<long long>(n + w[0]),
                              static_cast<long long>(w[1]), static_cast<long long>(w[2]));
                dev.refuse(NPR_ERR_INVALID, text);
            }
            n += w[0], at = w[1];
        }
        if (n >= (int64_t(1) << 31)) dev.refuse(NPR_ERR_INVALID, "npr_bam_open: 2^31 records and more");
        bs->n = n;
        bs->block_off.swap(block_off), bs->stream_off.swap(stream_off);
        *out = bs.release();
        return NPR_OK;
    });
}

void npr_bam_close(npr_bam_stream *bs) {
    if (!bs) return;
    (void)hipSetDevice(bs->ctx->device);
    delete bs;
}

int64_t npr_bam_stream_info(npr_bam_stream *bs, int64_t *out) {
    if (!bs || !out) return NPR_ERR_INVALID;
    out[0] = bs->n, out[1] = static_cast<int64_t>(bs->ref_len.size()), out[2] = bs->l_text, out[3] = bs->stream_len;
    return bs->n;
}

int64_t npr_bam_stream_refs(npr_bam_stream *bs, int64_t *ref_len, int64_t *name_off, uint8_t *names, int64_t cap) {
    if (!bs || cap < 0) return NPR_ERR_INVALID;
    const int64_t total = static_cast<int64_t>(bs->names.size());
    if (!names) return total;
    if (cap < total) return NPR_ERR_CAPACITY;
    if (ref_len) std::copy(bs->ref_len.begin(), bs->ref_len.end(), ref_len);
    if (name_off) std::copy(bs->name_off.begin(), bs->name_off.end(), name_off);
    std::copy(bs->names.begin(), bs->names.end(), names);
    return total;
}

int32_t npr_pileup_add_bam(npr_pileup *pl, npr_bam_stream *bs, int32_t flag_mask, int64_t *counts) {
    if (!pl || !bs || !counts) return NPR_ERR_INVALID;
    std::fill(counts, counts + 4, int64_t(0));
    npr_ctx *ctx = pl->ctx;
    if (bs->ctx != ctx) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_bam: the stream and the pileup are of two contexts");
    if (bs->ref_len != pl->len) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_bam: the file's reference sequences are not the pileup's (their number or a length)");
    if (bs->n == 0) return NPR_OK;
    return guarded(ctx, "npr_pileup_add_bam", [&](const Call &dev) -> int32_t {
        DevBuf<BamPileRec> d_recs;
        DevBuf<int64_t> d_len;
        DevBuf<unsigned long long> d_counts;
        dev.alloc(d_recs, static_cast<size_t>(bs->n)), dev.upload(d_len, bs->ref_len);
        dev.alloc(d_counts, 4), dev.zero(d_counts);
        const BamPileArgs a{bs->stream.p, bs->stream_len, bs->n, bs->rec_off.p, static_cast<int64_t>(bs->ref_len.size()), d_len.p, pl->dbase.p, flag_mask,
                            d_recs.p, d_counts.p, pl->tab.p, pl->diff.p};
        dev.launched(launch_bampile_check(a, ctx->stream), "k_bampile_check");
        dev.launched(launch_bampile_add(a, ctx->stream), "k_bampile_add");
        unsigned long long got[4] = {0, 0, 0, 0};
        dev.fetch(got, d_counts.p, sizeof(got));
        dev.sync();
        counts[0] = bs->n;
        for (int k = 1; k < 4; ++k) counts[k] = static_cast<int64_t>(got[k]);
        return counts[3] ? fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_bam: a record's cigar does not fit its reference sequence or its read, or its auxiliary fields are malformed (the record was left out)")
                         : NPR_OK;
    });
}

int32_t npr_bam_open_region(npr_ctx *ctx, const uint8_t *file, int64_t len, const uint8_t *bai, int64_t bai_len, int32_t tid, int64_t beg, int64_t end,
                            npr_bam_stream **out) {
    if (!ctx || !file || len < 0 || !bai || bai_len < 0 || !out) return NPR_ERR_INVALID;
    *out = nullptr;
    return guarded(ctx, "npr_bam_open_region", [&](const Call &dev) -> int32_t {
        // the chunks of the query (host)
        int64_t index_refs = -1;
        const int64_t n_chunks = npr_bai_chunks(bai, bai_len, tid, beg, end, nullptr, nullptr, 0, &index_refs);
        if (n_chunks < 0)
            dev.refuse(static_cast<int32_t>(n_chunks), "npr_bam_open_region: a malformed index, a reference sequence it does not have, or a region that is not 0 <= beg < end <= 2^29");
        std::vector<uint64_t> vbeg(static_cast<size_t>(n_chunks) + 1), vend(static_cast<size_t>(n_chunks) + 1);
        if (npr_bai_chunks(bai, bai_len, tid, beg, end, vbeg.data(), vend.data(), n_chunks, &index_refs) != n_chunks)
            dev.refuse(NPR_ERR_STATE, "npr_bam_open_region: the index changed its chunks");
        std::vector<int64_t> block_off, stream_off;
        if (scan_table(file, len, block_off, stream_off) < 0) dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: not a BGZF file that ends with the end-of-file block");
        if (block_off.size() >= (size_t(1) << 31)) return NPR_ERR_INVALID;
        const int64_t blocks = static_cast<int64_t>(block_off.size()) - 1;

        // the header's blocks: block 0, and twice as many while the header runs on
        int64_t head[4] = {1, 0, 0, 0};
        std::vector<int64_t> pick, s_sub;
        {
            DevBuf<int64_t> d_head;
            dev.alloc(d_head, 4);
            for (int64_t hb = std::min<int64_t>(blocks, 1);; hb = std::min(blocks, 2 * hb)) {
                InflateRun run;
                pick.resize(static_cast<size_t>(hb));
                for (int64_t b = 0; b < hb; ++b) pick[b] = b;
                run.launch_picked(dev, file, block_off, stream_off, pick, s_sub);
                run.finish(dev);
                dev.launched(launch_bam_head(run.stream.p, run.stream_len, d_head.p, ctx->stream), "k_bam_head");
                dev.fetch(head, d_head.p, sizeof(head));
                dev.sync();
                if (head[0] == 0) break;
                if (head[0] == 1 || hb == blocks) dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: no BAM magic, or a header that runs past the stream");  // (1: k_bam_head saw no magic)
            }
        }
        if (head[3] != index_refs) dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: the index is of a file with another number of reference sequences");
        const int64_t head_blocks = std::lower_bound(stream_off.begin(), stream_off.begin() + blocks, head[1]) - stream_off.begin();  // those that begin before the header's end

        // the chunks' blocks, and the chunks as spans [u0, u1) of the whole stream
        std::vector<uint8_t> need(static_cast<size_t>(blocks) + 1, 0);
        std::fill(need.begin(), need.begin() + head_blocks, uint8_t(1));
        std::vector<int64_t> u0, u1, first;
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t fb = static_cast<int64_t>(vbeg[c] >> 16), fe = static_cast<int64_t>(vend[c] >> 16), lb = static_cast<int64_t>(vbeg[c] & 0xffffu), le = static_cast<int64_t>(vend[c] & 0xffffu);
            const int64_t ib = std::lower_bound(block_off.begin(), block_off.begin() + blocks, fb) - block_off.begin();
            const int64_t ie = std::lower_bound(block_off.begin(), block_off.end(), fe) - block_off.begin();
            if (ib >= blocks || block_off[ib] != fb || ie > blocks || block_off[ie] != fe)
                dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: a chunk of the index does not begin or end in a block of the file");
            if (lb > stream_off[ib + 1] - stream_off[ib] || le > (ie < blocks ? stream_off[ie + 1] - stream_off[ie] : 0))
                dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: a chunk of the index begins or ends past its block's ISIZE");
            for (int64_t b = ib; b < ie; ++b) need[b] = 1;
            if (le > 0) need[ie] = 1;
            if (stream_off[ie] + le > stream_off[ib] + lb) u0.push_back(stream_off[ib] + lb), u1.push_back(stream_off[ie] + le), first.push_back(ib);
        }
        pick.clear();
        std::vector<int64_t> where(static_cast<size_t>(blocks) + 1, -1);
        for (int64_t b = 0; b < blocks; ++b)
            if (need[b]) where[b] = static_cast<int64_t>(pick.size()), pick.push_back(b);

        std::unique_ptr<npr_bam_stream> bs(new npr_bam_stream);
        bs->ctx = ctx;
        {
            InflateRun run;  // (the blocks' bytes and tables go when the stream is made)
            run.launch_picked(dev, file, block_off, stream_off, pick, s_sub);
            run.finish(dev);
            bs->stream_len = run.stream_len;
            bs->stream.take(run.stream);
        }
        const uint8_t *const d_stream = bs->stream.p;
        const BamHeader h = bam_header(dev, d_stream, bs->stream_len, bs->names, bs->name_off, &bs->ref_len);
        bs->l_text = h.l_text;

        // the chunks in the compact stream: a chunk's blocks are neighbours in the file, so they are neighbours there and one shift serves it
        const int64_t walks = static_cast<int64_t>(u0.size());
        DevBuf<int64_t> d_table;
        int64_t n = 0;
        if (walks) {
            for (int64_t c = 0; c < walks; ++c) {
                const int64_t shift = s_sub[where[first[c]]] - stream_off[first[c]];
                u0[c] += shift, u1[c] += shift;
            }
            DevBuf<int64_t> d_beg, d_end, d_count, d_stop, d_tile;
            DevBuf<int32_t> d_status;
            dev.upload(d_beg, u0), dev.upload(d_end, u1);
            dev.alloc(d_count, static_cast<size_t>(walks) + 1), dev.alloc(d_stop, static_cast<size_t>(walks)), dev.alloc(d_status, static_cast<size_t>(walks));
            dev.alloc(d_tile, static_cast<size_t>(scan_tiles(walks)));
            BamChunkArgs a{d_stream, bs->stream_len, static_cast<int32_t>(h.n_ref), walks, d_beg.p, d_end.p, d_count.p, d_stop.p, d_status.p, nullptr};
            dev.launched(launch_bam_chunk_count(a, ctx->stream), "k_bam_chunk_walk");
            dev.launched(launch_scan_tiled<int64_t, int64_t>(d_count.p, d_count.p, walks, d_tile.p, ctx->stream), "scan");
            std::vector<int64_t> stop(static_cast<size_t>(walks));
            std::vector<int32_t> status(static_cast<size_t>(walks));
            dev.fetch(stop.data(), d_stop.p, d_stop.bytes()), dev.fetch(status.data(), d_status.p, d_status.bytes());
            dev.fetch(&n, d_count.p + walks, sizeof(n));
            dev.sync();
            for (int64_t c = 0; c < walks; ++c)
                if (status[c] != 0) {
                    char text[200];
                    std::snprintf(text, sizeof(text), "npr_bam_open_region: chunk %lld of the index: the record at byte %lld of the inflated blocks is refused (walk status %d)",
                                  static_cast<long long>(c), static_cast<long long>(stop[c]), status[c]);
                    dev.refuse(NPR_ERR_INVALID, text);
                }
            if (n >= (int64_t(1) << 31)) dev.refuse(NPR_ERR_INVALID, "npr_bam_open_region: 2^31 records and more");
            dev.alloc(d_table, static_cast<size_t>(std::max<int64_t>(n, 1)));
            a.table = d_table.p;
            dev.launched(launch_bam_chunk_write(a, ctx->stream), "k_bam_chunk_walk");
            dev.sync();  // (the chunks' tables go out of scope)
        }
        bs->n = overlap_filter(dev, d_stream, d_table.p, n, tid, beg, end, bs->rec_off);
        *out = bs.release();
        return NPR_OK;
    });
}

int64_t npr_bam_stream_restrict(npr_bam_stream *bs, int32_t tid, int64_t beg, int64_t end) {
    if (!bs) return NPR_ERR_INVALID;
    npr_ctx *ctx = bs->ctx;
    if (tid < 0 || tid >= static_cast<int64_t>(bs->ref_len.size()) || beg < 0 || beg >= end)
        return fail(ctx, NPR_ERR_INVALID, "npr_bam_stream_restrict: a reference sequence the file does not have, or a region that is not 0 <= beg < end");
    return guarded(ctx, "npr_bam_stream_restrict", [&](const Call &dev) -> int64_t {
        bs->n = overlap_filter(dev, bs->stream.p, bs->rec_off.p, bs->n, tid, beg, end, bs->rec_off);
        return bs->n;
    });
}

int64_t npr_bam_stream_sam(npr_bam_stream *bs, uint8_t *sam_out, int64_t cap, int64_t *n_records) {
    if (!bs || cap < 0) return NPR_ERR_INVALID;
    return guarded(bs->ctx, "npr_bam_stream_sam", [&](const Call &dev) -> int64_t {
        return sam_lines(dev, bs->stream.p, bs->stream_len, bs->l_text, static_cast<int64_t>(bs->ref_len.size()), bs->names, bs->name_off, bs->rec_off.p, bs->n, sam_out, cap,
                         n_records);
    });
}

int64_t npr_sam_bam(npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields, const int64_t *tail, int64_t n,
                    const int64_t *tag_off, const uint8_t *tags, const uint8_t *header, int64_t header_len, int64_t n_refs, const int64_t *ref_len,
                    int32_t sorted, uint8_t *bam_out, int64_t cap, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg,
                    uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor) {
    return sam_bam("npr_sam_bam", false, ctx, text, text_len, span, fields, tail, n, tag_off, tags, header, header_len, n_refs, ref_len, sorted, bam_out, cap, n_runs,
                   run_tid, run_bin, run_beg, run_end, linear, meta, n_no_coor);
}

int64_t npr_sam_bam_deflate(npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields, const int64_t *tail, int64_t n,
                            const int64_t *tag_off, const uint8_t *tags, const uint8_t *header, int64_t header_len, int64_t n_refs, const int64_t *ref_len,
                            int32_t sorted, uint8_t *bam_out, int64_t cap, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg,
                            uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor) {
    return sam_bam("npr_sam_bam_deflate", true, ctx, text, text_len, span, fields, tail, n, tag_off, tags, header, header_len, n_refs, ref_len, sorted, bam_out, cap,
                   n_runs, run_tid, run_bin, run_beg, run_end, linear, meta, n_no_coor);
}

}  // extern "C"

namespace {

// the body of npr_sam_bam and npr_sam_bam_deflate: they differ in how the stream is framed and where the virtual offsets come from
int64_t sam_bam(const char *entry, bool compress, npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields, const int64_t *tail,
                int64_t n, const int64_t *tag_off, const uint8_t *tags, const uint8_t *header, int64_t header_len, int64_t n_refs, const int64_t *ref_len,
                int32_t sorted, uint8_t *bam_out, int64_t cap, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end,
                uint64_t *linear, uint64_t *meta, int64_t *n_no_coor) {
    const bool index = sorted && bam_out;
    if (!ctx || n < 0 || n >= (int64_t(1) << 31) || text_len < 0 || header_len < 0 || n_refs < 0 || n_refs >= (1 << 30) || cap < 0 || (header_len && !header) ||
        (n && (!text || !span || !fields || !tail || !tag_off)) || (n_refs && !ref_len) ||
        (index && (!n_runs || !n_no_coor || (n && (!run_tid || !run_bin || !run_beg || !run_end)) || (n_refs && (!linear || !meta)))))
        return NPR_ERR_INVALID;
    return guarded(ctx, entry, [&](const Call &dev) -> int64_t {
        // the lines as records, every one checked before anything is launched
        std::vector<BamRec> recs(static_cast<size_t>(n));
        std::vector<int64_t> lin_off(static_cast<size_t>(n_refs) + 1, 0);
        for (int64_t k = 0; k < n_refs; ++k) {
            if (ref_len[k] < 1) return fail(ctx, NPR_ERR_INVALID, (std::string(entry) + ": a reference length below 1").c_str());
            lin_off[k + 1] = lin_off[k] + ((ref_len[k] - 1) >> 14) + 1;
        }
        std::atomic<int> bad{0};
        std::vector<int64_t> tiles(static_cast<size_t>(n) + 1, 0);
        parallel_for((n + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t i = c * 256, hi = std::min(n, (c + 1) * 256); i < hi; ++i) {
                const int64_t *f = fields + i * NPR_SAM_COLS, *t = tail + i * NPR_SAM_TAIL_COLS;
                if (t[7] != NPR_OK || f[15] == NPR_SAM_UNKNOWN_REFERENCE) {
                    bad = 1;
                    continue;
                }
                BamRec &r = recs[i];
                const bool no_seq = f[6] - f[5] == 1 && text[f[5]] == '*', no_qual = t[4] - t[3] == 1 && text[t[3]] == '*';
                r.name = span[2 * i], r.l_name = static_cast<int32_t>(f[0] - span[2 * i]);
                r.cigar_lo = f[3], r.cigar_hi = f[4];
                r.seq = f[5], r.l_seq = no_seq ? 0 : static_cast<int32_t>(f[6] - f[5]);
                r.qual = no_qual ? -1 : t[3];
                r.tag_off = tag_off[i], r.tag_len = static_cast<int32_t>(tag_off[i + 1] - tag_off[i]);
                r.tid = static_cast<int32_t>(f[10]), r.pos = static_cast<int32_t>(f[8]), r.flag = static_cast<int32_t>(f[7]), r.mapq = static_cast<int32_t>(f[9]);
                r.next_tid = static_cast<int32_t>(t[0]), r.next_pos = static_cast<int32_t>(t[1]), r.tlen = static_cast<int32_t>(t[2]);
                const bool inside = span[2 * i] >= 0 && span[2 * i] <= f[0] && f[0] <= f[3] && f[3] <= f[4] && f[4] <= f[5] && f[5] <= f[6] && f[6] <= t[3] && t[3] <= t[4] &&
                                    t[4] <= span[2 * i + 1] && span[2 * i + 1] <= text_len;
                if (!inside || f[6] - f[5] >= (int64_t(1) << 30) || r.tag_len < 0 || r.tid < -1 || r.tid >= n_refs || r.next_tid < -1 || r.next_tid >= n_refs ||
                    r.l_name < 1 || r.l_name > 254 || r.pos < -1 || r.flag < 0 || r.flag > 65535 || r.mapq < 0 || r.mapq > 255 ||
                    (!no_qual && t[4] - t[3] != r.l_seq))
                    bad = 1;
                tiles[i + 1] = std::max<int64_t>(1, (r.l_seq + BAM_TILE - 1) / BAM_TILE);
            }
        });
        if (n && tag_off[n] > tag_off[0] && !tags) return NPR_ERR_INVALID;
        if (bad) return fail(ctx, NPR_ERR_INVALID, (std::string(entry) + ": a line that did not parse, names an unknown reference or lies outside the text").c_str());
        for (int64_t i = 0; i < n; ++i) tiles[i + 1] += tiles[i];
        const int64_t n_items = tiles[n];
        if (n_items >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, (std::string(entry) + ": 2^31 tiles and more in one call").c_str());
        std::vector<unsigned long long> items(static_cast<size_t>(n_items));
        parallel_for((n + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t i = c * 256, hi = std::min(n, (c + 1) * 256); i < hi; ++i)
                for (int64_t k = tiles[i]; k < tiles[i + 1]; ++k) items[k] = static_cast<unsigned long long>(i) << 32 | static_cast<unsigned long long>(k - tiles[i]);
        });

        DevBuf<uint8_t> d_text, d_tags, d_raw, d_out;
        DevBuf<BamRec> d_recs;
        DevBuf<BamMeasure> d_meas;
        DevBuf<int32_t> d_bad, d_tid, d_flag;
        DevBuf<int64_t> d_pos, d_size, d_tile, d_rec_off;
        DevBuf<uint32_t> d_order;
        DevBuf<unsigned long long> d_items, d_keys;
        BamArgs a{};
        a.n = n, a.n_items = n_items, a.header_len = header_len, a.n_refs = n_refs;
        if (n) {
            dev.upload(d_text, text, static_cast<size_t>(text_len));
            dev.upload(d_recs, recs);
            dev.upload(d_tags, tags, static_cast<size_t>(tag_off[n]));
            dev.alloc(d_meas, n);
        }
        dev.alloc(d_bad, 1), dev.zero(d_bad);
        a.text = d_text.p, a.recs = d_recs.p, a.tags = d_tags.p, a.meas = d_meas.p, a.bad = d_bad.p;
        dev.launched(launch_bam_measure(a, ctx->stream), "k_bam_measure");
        if (sorted && n) {
            std::vector<int32_t> tid(static_cast<size_t>(n)), flag(static_cast<size_t>(n));
            std::vector<int64_t> pos(static_cast<size_t>(n));
            int64_t max_pos = 0, max_tid = 0;  // the largest key's bits: from the largest tid' (n_refs for tid -1) and, when that is 0, the largest pos
            for (int64_t i = 0; i < n; ++i) {
                tid[i] = recs[i].tid, pos[i] = recs[i].pos, flag[i] = recs[i].flag;
                max_pos = std::max<int64_t>(max_pos, pos[i] + 1), max_tid = std::max<int64_t>(max_tid, tid[i] < 0 ? n_refs : tid[i]);
            }
            dev.upload(d_tid, tid), dev.upload(d_pos, pos), dev.upload(d_flag, flag);
            dev.alloc(d_keys, n);
            dev.launched(launch_bam_sort_keys(n, d_tid.p, d_pos.p, d_flag.p, static_cast<int32_t>(n_refs), d_keys.p, ctx->stream), "k_sort_keys");
            sort_order(dev, d_keys, n, max_tid ? 33 + bits_of(static_cast<unsigned long long>(max_tid)) : bits_of(static_cast<unsigned long long>(max_pos) << 1 | 1), d_order);
            a.order = d_order.p;
        }
        dev.alloc(d_size, n + 1), dev.alloc(d_tile, scan_tiles(n)), dev.alloc(d_rec_off, std::max<int64_t>(n, 1));
        a.size_sorted = d_size.p, a.tile = d_tile.p, a.rec_off = d_rec_off.p;
        dev.launched(launch_bam_offsets(a, ctx->stream), "k_bam_gather_sizes / scan / k_bam_place");
        int64_t records_bytes = 0;
        int32_t bad_cigar = 0;
        dev.fetch(&records_bytes, d_size.p + n, sizeof(int64_t));
        dev.fetch(&bad_cigar, d_bad.p, sizeof(int32_t));
        dev.sync();
        if (bad_cigar) return fail(ctx, NPR_ERR_INVALID, (std::string(entry) + ": a malformed CIGAR").c_str());
        const int64_t stream_len = header_len + records_bytes, total = bgzf_length(stream_len);
        if (!bam_out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        if (total / BGZF_PAYLOAD + 2 >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, (std::string(entry) + ": 2^31 BGZF blocks and more").c_str());

        dev.alloc(d_raw, static_cast<size_t>(std::max<int64_t>(stream_len, 1)));
        dev.copy_up(d_raw.p, header, static_cast<size_t>(header_len));
        dev.upload(d_items, items);
        a.items = d_items.p, a.raw = d_raw.p;
        dev.launched(launch_bam_encode(a, ctx->stream), "k_bam_cigar / k_bam_encode");
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
        if (!index) {
            dev.sync();
            return written;
        }

        // the index
        bam_index_tables(dev, a, lin_off, n_runs, run_tid, run_bin, run_beg, run_end, linear, meta, n_no_coor);
        return written;
    });
}

}  // namespace

namespace npr_impl {

void bam_index_tables(const Call &dev, BamArgs &a, const std::vector<int64_t> &lin_off, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg,
                      uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor) {
    npr_ctx *const ctx = dev.ctx;
    const int64_t n = a.n, n_refs = a.n_refs;
    *n_runs = 0, *n_no_coor = 0;
    const int64_t windows = lin_off[n_refs];
    DevBuf<unsigned long long> d_linear, d_meta, d_no_coor, d_run_key, d_run_beg, d_run_end, d_out_beg, d_out_end;
    DevBuf<int32_t> d_run_tid, d_head_tile;
    DevBuf<uint32_t> d_run_bin, d_perm, d_head;
    DevBuf<int64_t> d_lin_off;
    std::vector<unsigned long long> meta0(4 * static_cast<size_t>(n_refs), 0);
    for (int64_t k = 0; k < n_refs; ++k) meta0[4 * k] = ~0ull;
    dev.upload(d_meta, meta0);
    dev.alloc(d_linear, windows);
    if (windows) dev.check(hipMemsetAsync(d_linear.p, 0xff, d_linear.bytes(), ctx->stream), "memset");
    dev.alloc(d_no_coor, 1), dev.zero(d_no_coor);
    if (n) {
        dev.upload(d_lin_off, lin_off);
        dev.alloc(d_head, n + 1), dev.alloc(d_head_tile, scan_tiles(n));
        dev.alloc(d_run_key, n), dev.alloc(d_run_beg, n), dev.alloc(d_run_end, n);
        a.lin_off = d_lin_off.p, a.head = d_head.p, a.head_tile = d_head_tile.p;
        a.run_key = d_run_key.p, a.run_beg = d_run_beg.p, a.run_end = d_run_end.p;
        a.linear = d_linear.p, a.meta = d_meta.p, a.no_coor = d_no_coor.p;
        dev.launched(launch_bam_index_heads(a, ctx->stream), "k_bam_index_heads / scan");
        dev.launched(launch_bam_index_runs(a, ctx->stream), "k_bam_index_runs");
        int32_t runs = 0;
        dev.fetch(&runs, d_head.p + n, sizeof(int32_t));
        dev.sync();
        sort_order(dev, d_run_key, runs, 16 + bits_of(static_cast<unsigned long long>(n_refs)), d_perm);
        // (sort_order overwrote the keys' buffer or its twin: the keys are made again for the gather)
        dev.launched(launch_bam_index_runs(a, ctx->stream), "k_bam_index_runs");
        dev.alloc(d_run_tid, runs), dev.alloc(d_run_bin, runs), dev.alloc(d_out_beg, runs), dev.alloc(d_out_end, runs);
        BamGatherArgs g{runs, d_perm.p, d_run_key.p, d_run_beg.p, d_run_end.p, static_cast<int32_t>(n_refs), d_run_tid.p, d_run_bin.p, d_out_beg.p, d_out_end.p};
        dev.launched(launch_bam_gather_runs(g, ctx->stream), "k_bam_gather_runs");
        dev.fetch(run_tid, d_run_tid.p, d_run_tid.bytes()), dev.fetch(run_bin, d_run_bin.p, d_run_bin.bytes());
        dev.fetch(run_beg, d_out_beg.p, d_out_beg.bytes()), dev.fetch(run_end, d_out_end.p, d_out_end.bytes());
        *n_runs = runs;
    }
    unsigned long long no_coor = 0;
    dev.fetch(linear, d_linear.p, d_linear.bytes());
    dev.fetch(meta, d_meta.p, d_meta.bytes());
    dev.fetch(&no_coor, d_no_coor.p, sizeof(no_coor));
    dev.sync();
    *n_no_coor = static_cast<int64_t>(no_coor);
}

}  // namespace npr_impl
