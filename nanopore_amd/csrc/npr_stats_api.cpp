// npr_stats_api.cpp -- post-alignment statistics and the k-mer and indel-k-mer tables on the device (npr_stats.hip, npr_kmer.hip; coverage.py /
// substitutions.py / indels.py; kmerAnalysis.py / indelKmerAnalysis.py), and the cigars of a finished batch as the device consumers take them
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace npr_impl {

void cigars_from_host(const Call &dev, const uint32_t *ops, const std::vector<int64_t> &off, DeviceCigars &c) {
    dev.upload(c.own_ops, ops, static_cast<size_t>(off.back()));
    dev.upload(c.own_off, off);
    c.ops = c.own_ops.p, c.off = c.own_off.p;
}

void with_batch_cigars(const Call &dev, npr_batch *b, const std::function<void(const DeviceCigars &)> &run) {
    npr_ctx *ctx = b->ctx;
    DeviceCigars c;
    std::unique_lock<std::mutex> arena_lock(ctx->arena->mu);  // the resident cigars lie in the arena
    if (b->dev_ops && b->dev_ops_epoch == ctx->arena->epoch) {
        c.ops = b->dev_ops, c.off = b->dev_od;
        return run(c);
    }
    arena_lock.unlock();
    if (b->words_on_device && !b->have_packed_form) dev.passed(fetch_device_words(b));  // (finished with NPR_OPT_FINISH_TEXT: the words were on the device only)
    ensure_packed_form(b);
    cigars_from_host(dev, b->packed.get(), b->ops_off, c);
    run(c);
}

}  // namespace npr_impl

namespace {

// what StatsArgs points to besides the base codes and the cigars, uploaded
struct StatsUpload {
    DevBuf<int32_t> so;
    DevBuf<StatsSeg> sg;
};
StatsArgs stage_stats_args(const Call &dev, int64_t n, const DeviceCigars &c, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs,
                           const uint8_t *d_seq, StatsUpload &up) {
    if (n >= (int64_t(1) << 31)) dev.refuse(NPR_ERR_INVALID, "npr_align_stats: too many reads");
    dev.upload(up.so, seg_off);
    dev.upload(up.sg, segs);
    return StatsArgs{static_cast<int32_t>(n), c.off, c.ops, up.so.p, up.sg.p, d_seq, nullptr};
}

// k_align_stats over n reads
void run_align_stats(const Call &dev, int64_t n, const DeviceCigars &c, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs, const uint8_t *d_seq,
                     int32_t *stats) {
    StatsUpload up;
    StatsArgs a = stage_stats_args(dev, n, c, seg_off, segs, d_seq, up);
    DevBuf<int32_t> out;
    dev.alloc(out, static_cast<size_t>(n) * NPR_STATS_WORDS);
    a.out = out.p;
    dev.launched(launch_align_stats(a, dev.ctx->stream), "k_align_stats");
    dev.fetch(stats, out.p, out.bytes());
    dev.sync();
}

// k_indel_kmers over them (every read with one piece, its whole window, or none); returns whether some cigar ran past its piece
int32_t run_indel_kmers(const Call &dev, int32_t k, int64_t n, const DeviceCigars &c, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs,
                        const uint8_t *d_seq, int64_t *read_counts, int64_t *ref_counts) {
    StatsUpload up;
    IndelKmerArgs a{};
    a.s = stage_stats_args(dev, n, c, seg_off, segs, d_seq, up);
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    DevBuf<unsigned long long> tab;  // read-side table, reference-side table, the flag
    dev.alloc(tab, 2 * nb + 1);
    dev.zero(tab);
    a.k = k, a.read_counts = tab.p, a.ref_counts = tab.p + nb, a.bad = reinterpret_cast<int32_t *>(tab.p + 2 * nb);
    dev.launched(launch_indel_kmers(a, dev.ctx->stream), "k_indel_kmers");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the tables leave the device as int64");
    int32_t bad = 0;
    dev.fetch(read_counts, a.read_counts, nb * sizeof(int64_t));
    dev.fetch(ref_counts, a.ref_counts, nb * sizeof(int64_t));
    dev.fetch(&bad, a.bad, sizeof(int32_t));
    dev.sync();
    return bad;
}

// alignments given on the host (npr_align_stats, npr_align_indel_kmers): every read's window -- the reference / read bases its cigar consumes --
// encoded into one code buffer, one piece per read, the cigars packed; bad[i]: the cigar is malformed or runs past its sequences (it is emptied)
struct Windows {
    std::vector<int64_t> off;
    std::vector<int32_t> seg_off, bad;
    std::vector<StatsSeg> segs;
    std::unique_ptr<uint8_t[]> codes;
    int64_t code_bytes = 0;
    std::vector<uint32_t> packed;
    // ... and on the device
    DevBuf<uint8_t> d_codes;
    DeviceCigars cigars;
};
void encode_windows(const Call &dev, int64_t n, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index, const uint8_t *read,
                    const int64_t *read_off, const int32_t *ops, const int64_t *ops_off, const int64_t *start, Windows &w) {
    const int threads = dev.ctx->host_threads;
    std::vector<int64_t> woff(n + 1, 0);
    w.off.assign(ops_off, ops_off + n + 1);
    w.seg_off.resize(n + 1), w.bad.assign(n, 0), w.segs.resize(n);
    std::vector<int32_t> &bad = w.bad;
    std::vector<int64_t> cx(n), cy(n);
    parallel_for(n, threads, [&](int64_t i) {
        int64_t x = 0, y = 0;
        for (int64_t q = ops_off[i]; q < ops_off[i + 1]; ++q) {
            const int32_t op = ops[2 * q], len = ops[2 * q + 1];
            if (op < 0 || op > 2 || len < 0) bad[i] = 1;
            if (op != NPR_OP_I) x += len;
            if (op != NPR_OP_D) y += len;
        }
        const int64_t k = ref_index ? ref_index[i] : i;
        const int64_t sx = start ? start[2 * i] : 0, sy = start ? start[2 * i + 1] : 0;
        if (k < 0 || k >= n_refs || sx < 0 || sy < 0 || sx + x > ref_off[k + 1] - ref_off[k] || sy + y > read_off[i + 1] - read_off[i] ||
            x >= (int64_t(1) << 30) || y >= (int64_t(1) << 30))
            bad[i] = 1;
        cx[i] = bad[i] ? 0 : x, cy[i] = bad[i] ? 0 : y;
    });
    for (int64_t i = 0; i < n; ++i) woff[i + 1] = woff[i] + cx[i] + cy[i], w.seg_off[i] = static_cast<int32_t>(i);
    w.seg_off[n] = static_cast<int32_t>(n);
    w.code_bytes = woff[n] + 1;
    w.codes.reset(new uint8_t[w.code_bytes]);
    w.packed.resize(ops_off[n]);
    parallel_for(n, threads, [&](int64_t i) {
        const int64_t k = ref_index ? ref_index[i] : i;
        const int64_t sx = start ? start[2 * i] : 0, sy = start ? start[2 * i + 1] : 0;
        uint8_t *c = w.codes.get() + woff[i];
        if (!bad[i]) {
            const uint8_t *xs = ref + ref_off[k] + sx, *ys = read + read_off[i] + sy;
            for (int64_t q = 0; q < cx[i]; ++q) c[q] = encode_base(xs[q]);
            for (int64_t q = 0; q < cy[i]; ++q) c[cx[i] + q] = encode_base(ys[q]);
        }
        w.segs[i] = StatsSeg{0, static_cast<int32_t>(cx[i]), 0, static_cast<int32_t>(cy[i]), woff[i], woff[i] + cx[i]};
        for (int64_t q = ops_off[i]; q < ops_off[i + 1]; ++q)
            w.packed[q] = bad[i] ? 0u : (static_cast<uint32_t>(ops[2 * q + 1]) << 2 | static_cast<uint32_t>(ops[2 * q]));
    });
    dev.upload(w.d_codes, w.codes.get(), static_cast<size_t>(w.code_bytes));
    cigars_from_host(dev, w.packed.data(), w.off, w.cigars);
}

}  // namespace

extern "C" {

int32_t npr_batch_align_stats(npr_batch *b, int32_t *stats) {
    if (!b || (!stats && b->n_reads)) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return guarded(b->ctx, "npr_batch_align_stats", [&](const Call &dev) -> int32_t {
        const int64_t n = b->n_reads;
        if (n == 0) return NPR_OK;
        // the pieces of every read's window whose base codes the batch holds: its tasks' segments
        std::vector<int32_t> seg_off(n + 1, 0);
        for (int64_t i = 0; i < n; ++i) seg_off[i + 1] = seg_off[i] + b->read_ntasks[i];
        std::vector<StatsSeg> segs(seg_off[n]);
        for (int64_t i = 0; i < n; ++i)
            for (int32_t s = 0; s < b->read_ntasks[i]; ++s) {
                const Task &t = b->tasks[b->task_of[b->read_first_task[i] + s]];
                segs[seg_off[i] + s] = StatsSeg{t.xs, t.xs + t.lX, t.ys, t.ys + t.lY, t.x_off, t.y_off};
            }
        with_batch_cigars(dev, b, [&](const DeviceCigars &c) { run_align_stats(dev, n, c, seg_off, segs, b->d_seq.p, stats); });
        for (int64_t i = 0; i < n; ++i)
            if (b->results[i].status != NPR_OK) std::fill(stats + i * NPR_STATS_WORDS, stats + (i + 1) * NPR_STATS_WORDS, 0), stats[i * NPR_STATS_WORDS + 14] = b->results[i].status;
        return NPR_OK;
    });
}

int32_t npr_align_stats(npr_ctx *ctx, int64_t n, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                        const uint8_t *read, const int64_t *read_off, const int32_t *ops, const int64_t *ops_off, const int64_t *start,
                        int32_t *stats) {
    if (!ctx || n < 0 || n_refs < 0 || (n && (!ref_off || !read_off || !ops_off || !stats))) return NPR_ERR_INVALID;
    if (!ref_index && n_refs != n) return fail(ctx, NPR_ERR_INVALID, "npr_align_stats: without ref_index, n_refs must equal n_reads");
    if (n == 0) return NPR_OK;
    return guarded(ctx, "npr_align_stats", [&](const Call &dev) -> int32_t {
        Windows w;
        encode_windows(dev, n, n_refs, ref, ref_off, ref_index, read, read_off, ops, ops_off, start, w);
        run_align_stats(dev, n, w.cigars, w.seg_off, w.segs, w.d_codes.p, stats);
        for (int64_t i = 0; i < n; ++i)
            if (w.bad[i]) std::fill(stats + i * NPR_STATS_WORDS, stats + (i + 1) * NPR_STATS_WORDS, 0), stats[i * NPR_STATS_WORDS + 14] = NPR_ERR_INVALID;
        return NPR_OK;
    });
}

int32_t npr_kmer_counts(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off, int64_t *counts) {
    if (!ctx || k < 1 || k > NPR_KMER_MAX_K || n_seqs < 0 || !counts || (n_seqs && !seq_off)) return NPR_ERR_INVALID;
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    std::fill(counts, counts + nb, int64_t(0));
    if (n_seqs == 0) return NPR_OK;
    return guarded(ctx, "npr_kmer_counts", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> off(n_seqs + 1);
        for (int64_t i = 0; i <= n_seqs; ++i) {
            off[i] = seq_off[i] - seq_off[0];
            if (i && off[i] < off[i - 1]) return fail(ctx, NPR_ERR_INVALID, "npr_kmer_counts: sequence offsets decrease");
        }
        const int64_t total = off[n_seqs];
        if (total == 0) return NPR_OK;
        if (!seq) return NPR_ERR_INVALID;
        DevBuf<uint8_t> d_seq;
        DevBuf<int64_t> d_off;
        DevBuf<unsigned long long> d_counts;
        dev.alloc(d_seq, static_cast<size_t>(total) + NPR_KMER_PAD);
        dev.copy_up(d_seq.p, seq + seq_off[0], static_cast<size_t>(total));
        dev.zero(d_seq.p + total, NPR_KMER_PAD);
        dev.upload(d_off, off);
        dev.alloc(d_counts, nb);
        dev.zero(d_counts);
        const KmerArgs a{d_seq.p, total, d_off.p, n_seqs, k, d_counts.p};
        dev.launched(launch_kmer_spectrum(a, ctx->stream), "k_kmer_spectrum");
        dev.fetch(counts, d_counts.p, nb * sizeof(int64_t));
        dev.sync();
        return NPR_OK;
    });
}

int32_t npr_kmer_counts_groups(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *text, const int64_t *seq_begin, const int64_t *seq_end,
                               const int32_t *group, int32_t n_groups, int64_t *counts) {
    if (!ctx || k < 1 || k > NPR_KMER_MAX_K || n_seqs < 0 || n_groups < 1 || n_groups > NPR_KMER_MAX_GROUPS || !counts ||
        (n_seqs && (!seq_begin || !seq_end || !group)))
        return NPR_ERR_INVALID;
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    return guarded(ctx, "npr_kmer_counts_groups", [&](const Call &dev) -> int32_t {
        // sequences and bases of every group; nothing is counted and no table touched when an argument is wrong
        std::vector<int64_t> seqs_of(n_groups, 0), bases_of(n_groups, 0);
        for (int64_t i = 0; i < n_seqs; ++i) {
            if (group[i] < -1 || group[i] >= n_groups) return fail(ctx, NPR_ERR_INVALID, "npr_kmer_counts_groups: a group outside -1 .. n_groups - 1");
            if (seq_end[i] < seq_begin[i] || seq_begin[i] < 0) return fail(ctx, NPR_ERR_INVALID, "npr_kmer_counts_groups: a span that ends before it begins");
            if (group[i] >= 0) ++seqs_of[group[i]], bases_of[group[i]] += seq_end[i] - seq_begin[i];
        }
        std::fill(counts, counts + nb * static_cast<size_t>(n_groups), int64_t(0));
        // the layout KmerGroupArgs describes: one int64 table {tile0 | seq_first | seq_off}, the bases ordered by group in the pinned staging
        const size_t G = static_cast<size_t>(n_groups);
        const int64_t slots = std::accumulate(seqs_of.begin(), seqs_of.end(), int64_t(0)) + n_groups;  // one offset per sequence and every group's end
        std::vector<int64_t> tab(2 * (G + 1) + static_cast<size_t>(slots), 0);
        int64_t *const tile0 = tab.data(), *const seq_first = tab.data() + G + 1, *const seq_off = tab.data() + 2 * (G + 1);
        for (size_t g = 0; g < G; ++g) {
            tile0[g + 1] = tile0[g] + (bases_of[g] + NPR_KMER_TILE - 1) / NPR_KMER_TILE;
            seq_first[g + 1] = seq_first[g] + seqs_of[g] + 1;
        }
        const int64_t tiles = tile0[G];
        if (tiles == 0) return NPR_OK;
        if (!text) return NPR_ERR_INVALID;
        std::vector<int64_t> src(static_cast<size_t>(slots), -1);  // where the sequence behind seq_off[s] begins in text (-1: a group's end)
        {
            std::vector<int64_t> at(G), pos(G);
            for (size_t g = 0; g < G; ++g) at[g] = seq_first[g], pos[g] = tile0[g] * NPR_KMER_TILE;
            for (int64_t i = 0; i < n_seqs; ++i) {
                if (group[i] < 0) continue;
                const size_t g = static_cast<size_t>(group[i]);
                seq_off[at[g]] = pos[g], src[at[g]++] = seq_begin[i];
                pos[g] += seq_end[i] - seq_begin[i];
            }
            for (size_t g = 0; g < G; ++g) seq_off[at[g]] = pos[g];
        }
        const size_t stage_need = static_cast<size_t>(tiles) * NPR_KMER_TILE + NPR_KMER_PAD;
        dev.passed(grow_pin_stage(ctx, stage_need, "npr_kmer_counts_groups: hipHostMalloc"));
        uint8_t *const h_seq = static_cast<uint8_t *>(ctx->pin_stage);
        parallel_for((slots + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t s = c * 256, hi = std::min(slots, (c + 1) * 256); s < hi; ++s)
                if (src[s] >= 0) std::memcpy(h_seq + seq_off[s], text + src[s], static_cast<size_t>(seq_off[s + 1] - seq_off[s]));
        });
        for (size_t g = 0; g < G; ++g) {  // what a group leaves of its last tile (read as a lane's halo, never counted)
            const int64_t end = seq_off[seq_first[g + 1] - 1];
            std::memset(h_seq + end, 0, static_cast<size_t>(tile0[g + 1] * NPR_KMER_TILE - end));
        }
        std::memset(h_seq + stage_need - NPR_KMER_PAD, 0, NPR_KMER_PAD);
        DevBuf<uint8_t> d_seq;
        DevBuf<int64_t> d_tab;
        DevBuf<unsigned long long> d_counts;
        dev.upload(d_seq, h_seq, stage_need);
        dev.upload(d_tab, tab);
        dev.alloc(d_counts, nb * G);
        dev.zero(d_counts);
        const KmerGroupArgs a{d_seq.p, d_tab.p, d_tab.p + G + 1, d_tab.p + 2 * (G + 1), n_groups, k, d_counts.p};
        dev.launched(launch_kmer_spectrum_groups(a, tiles, ctx->stream), "k_kmer_spectrum_groups");
        dev.fetch(counts, d_counts.p, d_counts.bytes());
        dev.sync();
        return NPR_OK;
    });
}

int32_t npr_align_indel_kmers(npr_ctx *ctx, int32_t k, int64_t n, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                              const uint8_t *read, const int64_t *read_off, const int32_t *ops, const int64_t *ops_off, const int64_t *start,
                              int64_t *read_counts, int64_t *ref_counts) {
    if (!ctx || k < 1 || k > NPR_KMER_MAX_K || n < 0 || n_refs < 0 || !read_counts || !ref_counts || (n && (!ref_off || !read_off || !ops_off)))
        return NPR_ERR_INVALID;
    if (!ref_index && n_refs != n) return fail(ctx, NPR_ERR_INVALID, "npr_align_indel_kmers: without ref_index, n_refs must equal n_reads");
    std::fill(read_counts, read_counts + kmer_bins(k), int64_t(0));
    std::fill(ref_counts, ref_counts + kmer_bins(k), int64_t(0));
    if (n == 0) return NPR_OK;
    return guarded(ctx, "npr_align_indel_kmers", [&](const Call &dev) -> int32_t {
        Windows w;
        encode_windows(dev, n, n_refs, ref, ref_off, ref_index, read, read_off, ops, ops_off, start, w);
        int32_t bad = run_indel_kmers(dev, k, n, w.cigars, w.seg_off, w.segs, w.d_codes.p, read_counts, ref_counts);
        for (int64_t i = 0; i < n; ++i) bad |= w.bad[i];
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_align_indel_kmers: a cigar runs past its sequences (the record was left out)") : NPR_OK;
    });
}

int32_t npr_batch_indel_kmers(npr_batch *b, int32_t k, int64_t *read_counts, int64_t *ref_counts) {
    if (!b || k < 1 || k > NPR_KMER_MAX_K || !read_counts || !ref_counts) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return guarded(b->ctx, "npr_batch_indel_kmers", [&](const Call &dev) -> int32_t {
        const int64_t n = b->n_reads;
        std::fill(read_counts, read_counts + kmer_bins(k), int64_t(0));
        std::fill(ref_counts, ref_counts + kmer_bins(k), int64_t(0));
        if (n == 0) return NPR_OK;
        // one piece per read, its whole window (the batch holds every window whole: reference part, then read part, from the first base of
        // the read's first task back to position 0); a read that failed has none and adds nothing
        std::vector<int32_t> seg_off(n + 1, 0);
        std::vector<StatsSeg> segs;
        for (int64_t i = 0; i < n; ++i) {
            if (b->results[i].status == NPR_OK && b->read_ntasks[i] > 0) {
                const Task &t = b->tasks[b->task_of[b->read_first_task[i]]];
                segs.push_back(StatsSeg{0, static_cast<int32_t>(b->ref_len[i]), 0, static_cast<int32_t>(b->read_len[i]), t.x_off - t.xs, t.y_off - t.ys});
            }
            seg_off[i + 1] = static_cast<int32_t>(segs.size());
        }
        int32_t bad = 0;
        with_batch_cigars(dev, b, [&](const DeviceCigars &c) { bad = run_indel_kmers(dev, k, n, c, seg_off, segs, b->d_seq.p, read_counts, ref_counts); });
        return bad ? fail(b->ctx, NPR_ERR_INVALID, "npr_batch_indel_kmers: a cigar runs past its window (the record was left out)") : NPR_OK;
    });
}

}  // extern "C"
