// npr_aux.cpp -- post-alignment statistics and k-mer tables on the device, base expectations and calls of the marginAlign SNP caller, the device pileup, the planner cross-check (coverage.py / substitutions.py / indels.py; kmerAnalysis.py / indelKmerAnalysis.py; marginAlignSnpCaller.py:150-155)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"
#include "npr_snpmodel.h"

#include <functional>

extern "C" {

namespace {

// what StatsArgs points to besides the base codes, uploaded: n reads whose cigars are either packed on the device already (d_ops / d_off) or given on the host
struct StatsUpload {
    DevBuf<uint32_t> ops;
    DevBuf<int64_t> off;
    DevBuf<int32_t> so;
    DevBuf<StatsSeg> sg;
};
int32_t stage_stats_args(npr_ctx *ctx, int64_t n, const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops,
                         const std::vector<int64_t> *h_off, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs,
                         const uint8_t *d_seq, StatsUpload &up, StatsArgs &a) {
    if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_align_stats: too many reads");
    hipError_t e;
    if (!d_ops) {
        if ((e = up.ops.alloc(h_ops->size())) != hipSuccess || (e = up.off.alloc(h_off->size())) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_align_stats: hipMalloc", e);
        if (!h_ops->empty()) HIP_TRY(ctx, hipMemcpyAsync(up.ops.p, h_ops->data(), up.ops.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(up.off.p, h_off->data(), up.off.bytes(), hipMemcpyHostToDevice, ctx->stream));
        d_ops = up.ops.p, d_off = up.off.p;
    }
    if ((e = up.so.alloc(seg_off.size())) != hipSuccess || (e = up.sg.alloc(segs.size())) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_align_stats: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(up.so.p, seg_off.data(), up.so.bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (!segs.empty()) HIP_TRY(ctx, hipMemcpyAsync(up.sg.p, segs.data(), up.sg.bytes(), hipMemcpyHostToDevice, ctx->stream));
    a = StatsArgs{static_cast<int32_t>(n), d_off, d_ops, up.so.p, up.sg.p, d_seq, nullptr};
    return NPR_OK;
}

// k_align_stats over them
int32_t run_align_stats(npr_ctx *ctx, int64_t n, const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops,
                        const std::vector<int64_t> *h_off, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs,
                        const uint8_t *d_seq, int32_t *stats) {
    StatsUpload up;
    StatsArgs a;
    const int32_t rs = stage_stats_args(ctx, n, d_ops, d_off, h_ops, h_off, seg_off, segs, d_seq, up, a);
    if (rs != NPR_OK) return rs;
    DevBuf<int32_t> out;
    hipError_t e;
    if ((e = out.alloc(static_cast<size_t>(n) * NPR_STATS_WORDS)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_align_stats: hipMalloc", e);
    a.out = out.p;
    const int rc = launch_align_stats(a, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_align_stats launch", static_cast<hipError_t>(rc));
    HIP_TRY(ctx, hipMemcpyAsync(stats, out.p, out.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

// k_indel_kmers over them (every read with one piece, its whole window, or none); *bad: some cigar ran past its piece
int32_t run_indel_kmers(npr_ctx *ctx, int32_t k, int64_t n, const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops,
                        const std::vector<int64_t> *h_off, const std::vector<int32_t> &seg_off, const std::vector<StatsSeg> &segs,
                        const uint8_t *d_seq, int64_t *read_counts, int64_t *ref_counts, int32_t *bad) {
    StatsUpload up;
    IndelKmerArgs a{};
    const int32_t rs = stage_stats_args(ctx, n, d_ops, d_off, h_ops, h_off, seg_off, segs, d_seq, up, a.s);
    if (rs != NPR_OK) return rs;
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    DevBuf<unsigned long long> tab;  // read-side table, reference-side table, the flag
    hipError_t e;
    if ((e = tab.alloc(2 * nb + 1)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_align_indel_kmers: hipMalloc", e);
    HIP_TRY(ctx, hipMemsetAsync(tab.p, 0, tab.bytes(), ctx->stream));
    a.k = k, a.read_counts = tab.p, a.ref_counts = tab.p + nb, a.bad = reinterpret_cast<int32_t *>(tab.p + 2 * nb);
    const int rc = launch_indel_kmers(a, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_indel_kmers launch", static_cast<hipError_t>(rc));
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the tables leave the device as int64");
    HIP_TRY(ctx, hipMemcpyAsync(read_counts, a.read_counts, nb * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ref_counts, a.ref_counts, nb * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(bad, a.bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

// the cigars npr_batch_finish produced, where they lie (packed on the device after the device MEA stage) or uploaded: run(d_ops, d_off, h_ops, h_off)
using CigarFn = std::function<int32_t(const uint32_t *, const int64_t *, const std::vector<uint32_t> *, const std::vector<int64_t> *)>;
int32_t with_batch_cigars(npr_batch *b, const CigarFn &run) {
    npr_ctx *ctx = b->ctx;
    const int64_t n = b->n_reads;
    std::unique_lock<std::mutex> arena_lock(ctx->arena->mu);  // the resident cigars lie in the arena
    if (b->dev_ops && b->dev_ops_epoch == ctx->arena->epoch) return run(b->dev_ops, b->dev_od, nullptr, nullptr);
    arena_lock.unlock();
    if (b->words_on_device && !b->have_packed_form) {  // (finished with NPR_OPT_FINISH_TEXT: the words were on the device only)
        const int32_t rc = fetch_device_words(b);
        if (rc != NPR_OK) return rc;
    }
    ensure_packed_form(b);
    std::vector<uint32_t> packed(b->packed.get(), b->packed.get() + b->ops_off[n]);
    return run(nullptr, nullptr, &packed, &b->ops_off);
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
};
void encode_windows(npr_ctx *ctx, int64_t n, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index, const uint8_t *read,
                    const int64_t *read_off, const int32_t *ops, const int64_t *ops_off, const int64_t *start, Windows &w) {
    std::vector<int64_t> woff(n + 1, 0);
    w.off.assign(ops_off, ops_off + n + 1);
    w.seg_off.resize(n + 1), w.bad.assign(n, 0), w.segs.resize(n);
    std::vector<int32_t> &bad = w.bad;
    std::vector<int64_t> cx(n), cy(n);
    parallel_for(n, ctx->host_threads, [&](int64_t i) {
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
    parallel_for(n, ctx->host_threads, [&](int64_t i) {
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
}

}  // namespace

int32_t npr_batch_align_stats(npr_batch *b, int32_t *stats) {
    if (!b || (!stats && b->n_reads)) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = b->ctx;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
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
        const int32_t rc = with_batch_cigars(b, [&](const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops, const std::vector<int64_t> *h_off) {
            return run_align_stats(ctx, n, d_ops, d_off, h_ops, h_off, seg_off, segs, b->d_seq.p, stats);
        });
        if (rc != NPR_OK) return rc;
        for (int64_t i = 0; i < n; ++i)
            if (b->results[i].status != NPR_OK) std::fill(stats + i * NPR_STATS_WORDS, stats + (i + 1) * NPR_STATS_WORDS, 0), stats[i * NPR_STATS_WORDS + 14] = b->results[i].status;
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_align_stats: out of host memory");
    }
}

int32_t npr_align_stats(npr_ctx *ctx, int64_t n, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                        const uint8_t *read, const int64_t *read_off, const int32_t *ops, const int64_t *ops_off, const int64_t *start,
                        int32_t *stats) {
    if (!ctx || n < 0 || n_refs < 0 || (n && (!ref_off || !read_off || !ops_off || !stats))) return NPR_ERR_INVALID;
    if (!ref_index && n_refs != n) return fail(ctx, NPR_ERR_INVALID, "npr_align_stats: without ref_index, n_refs must equal n_reads");
    if (n == 0) return NPR_OK;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        Windows w;
        encode_windows(ctx, n, n_refs, ref, ref_off, ref_index, read, read_off, ops, ops_off, start, w);
        DevBuf<uint8_t> d_codes;
        if (d_codes.alloc(w.code_bytes) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_align_stats: hipMalloc");
        HIP_TRY(ctx, hipMemcpyAsync(d_codes.p, w.codes.get(), w.code_bytes, hipMemcpyHostToDevice, ctx->stream));
        const int32_t rc = run_align_stats(ctx, n, nullptr, nullptr, &w.packed, &w.off, w.seg_off, w.segs, d_codes.p, stats);
        if (rc != NPR_OK) return rc;
        for (int64_t i = 0; i < n; ++i)
            if (w.bad[i]) std::fill(stats + i * NPR_STATS_WORDS, stats + (i + 1) * NPR_STATS_WORDS, 0), stats[i * NPR_STATS_WORDS + 14] = NPR_ERR_INVALID;
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_align_stats: out of host memory");
    }
}

int32_t npr_kmer_counts(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off, int64_t *counts) {
    if (!ctx || k < 1 || k > NPR_KMER_MAX_K || n_seqs < 0 || !counts || (n_seqs && !seq_off)) return NPR_ERR_INVALID;
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    std::fill(counts, counts + nb, int64_t(0));
    if (n_seqs == 0) return NPR_OK;
    try {
        std::vector<int64_t> off(n_seqs + 1);
        for (int64_t i = 0; i <= n_seqs; ++i) {
            off[i] = seq_off[i] - seq_off[0];
            if (i && off[i] < off[i - 1]) return fail(ctx, NPR_ERR_INVALID, "npr_kmer_counts: sequence offsets decrease");
        }
        const int64_t total = off[n_seqs];
        if (total == 0) return NPR_OK;
        if (!seq) return NPR_ERR_INVALID;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        DevBuf<uint8_t> d_seq;
        DevBuf<int64_t> d_off;
        DevBuf<unsigned long long> d_counts;
        hipError_t e;
        if ((e = d_seq.alloc(static_cast<size_t>(total) + NPR_KMER_PAD)) != hipSuccess || (e = d_off.alloc(off.size())) != hipSuccess || (e = d_counts.alloc(nb)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_kmer_counts: hipMalloc", e);
        HIP_TRY(ctx, hipMemcpyAsync(d_seq.p, seq + seq_off[0], static_cast<size_t>(total), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_seq.p + total, 0, NPR_KMER_PAD, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_off.p, off.data(), d_off.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_counts.p, 0, d_counts.bytes(), ctx->stream));
        const KmerArgs a{d_seq.p, total, d_off.p, n_seqs, k, d_counts.p};
        const int rc = launch_kmer_spectrum(a, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_kmer_spectrum launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_kmer_counts: out of host memory");
    }
}

int32_t npr_kmer_counts_groups(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *text, const int64_t *seq_begin, const int64_t *seq_end,
                               const int32_t *group, int32_t n_groups, int64_t *counts) {
    if (!ctx || k < 1 || k > NPR_KMER_MAX_K || n_seqs < 0 || n_groups < 1 || n_groups > NPR_KMER_MAX_GROUPS || !counts ||
        (n_seqs && (!seq_begin || !seq_end || !group)))
        return NPR_ERR_INVALID;
    const size_t nb = static_cast<size_t>(kmer_bins(k));
    try {
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
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t stage_need = static_cast<size_t>(tiles) * NPR_KMER_TILE + NPR_KMER_PAD;
        const int32_t grown = grow_pin_stage(ctx, stage_need, "npr_kmer_counts_groups: hipHostMalloc");
        if (grown != NPR_OK) return grown;
        hipError_t e;
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
        if ((e = d_seq.alloc(stage_need)) != hipSuccess || (e = d_tab.alloc(tab.size())) != hipSuccess || (e = d_counts.alloc(nb * G)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_kmer_counts_groups: hipMalloc", e);
        HIP_TRY(ctx, hipMemcpyAsync(d_seq.p, h_seq, stage_need, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_tab.p, tab.data(), d_tab.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_counts.p, 0, d_counts.bytes(), ctx->stream));
        const KmerGroupArgs a{d_seq.p, d_tab.p, d_tab.p + G + 1, d_tab.p + 2 * (G + 1), n_groups, k, d_counts.p};
        const int rc = launch_kmer_spectrum_groups(a, tiles, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_kmer_spectrum_groups launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts.p, d_counts.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_kmer_counts_groups: out of host memory");
    }
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
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        Windows w;
        encode_windows(ctx, n, n_refs, ref, ref_off, ref_index, read, read_off, ops, ops_off, start, w);
        DevBuf<uint8_t> d_codes;
        if (d_codes.alloc(w.code_bytes) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_align_indel_kmers: hipMalloc");
        HIP_TRY(ctx, hipMemcpyAsync(d_codes.p, w.codes.get(), w.code_bytes, hipMemcpyHostToDevice, ctx->stream));
        int32_t bad = 0;
        const int32_t rc = run_indel_kmers(ctx, k, n, nullptr, nullptr, &w.packed, &w.off, w.seg_off, w.segs, d_codes.p, read_counts, ref_counts, &bad);
        if (rc != NPR_OK) return rc;
        for (int64_t i = 0; i < n; ++i) bad |= w.bad[i];
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_align_indel_kmers: a cigar runs past its sequences (the record was left out)") : NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_align_indel_kmers: out of host memory");
    }
}

int32_t npr_batch_indel_kmers(npr_batch *b, int32_t k, int64_t *read_counts, int64_t *ref_counts) {
    if (!b || k < 1 || k > NPR_KMER_MAX_K || !read_counts || !ref_counts) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = b->ctx;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
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
        const int32_t rc = with_batch_cigars(b, [&](const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops, const std::vector<int64_t> *h_off) {
            return run_indel_kmers(ctx, k, n, d_ops, d_off, h_ops, h_off, seg_off, segs, b->d_seq.p, read_counts, ref_counts, &bad);
        });
        if (rc != NPR_OK) return rc;
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_batch_indel_kmers: a cigar runs past its window (the record was left out)") : NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_indel_kmers: out of host memory");
    }
}

int64_t npr_batch_plan_check(npr_batch *b, const int32_t *guide_ops) {
    if (!b || (b->n_reads && b->guide_off[b->n_reads] && !guide_ops)) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        {
            const int32_t rc = ensure_coff(b);
            if (rc != NPR_OK) return rc;
        }
        const int64_t n = b->n_reads;
        int64_t mismatches = 0;
        std::vector<int32_t> lo, nn;
        std::vector<uint32_t> co, ctl, want_ctl;
        std::vector<Stripe> st, want_st;
        for (int64_t i = 0; i < n; ++i) {
            if (b->read_status[i] != NPR_OK && b->read_ntasks[i] == 0) continue;
            Plan plan;
            const int32_t rc = build_plan(b->params, b->ref_len[i], b->read_len[i], guide_ops + 2 * b->guide_off[i],
                                          b->guide_off[i + 1] - b->guide_off[i], plan);
            if (rc != NPR_OK || static_cast<int32_t>(plan.segs.size()) != b->read_ntasks[i]) {
                ++mismatches;
                continue;
            }
            for (int32_t s = 0; s < b->read_ntasks[i]; ++s) {
                const int32_t k = b->task_of[b->read_first_task[i] + s];
                const Task &t = b->tasks[k];
                const Segment &sg = plan.segs[s];
                bool ok = t.D == sg.D() && t.xs == sg.xs && t.ys == sg.ys && t.lX == sg.xe - sg.xs && t.lY == sg.ye - sg.ys &&
                          t.flags == ((sg.ragged_start ? 1 : 0) | (sg.ragged_end ? 2 : 0)) && b->task_cells[k] == sg.cells;
                if (ok) {
                    const size_t rows = static_cast<size_t>(t.D) + 1;
                    lo.resize(rows), nn.resize(rows), co.resize(rows);
                    HIP_TRY(ctx, hipMemcpy(lo.data(), b->d_lo.p + t.band_off, rows * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(ctx, hipMemcpy(nn.data(), b->d_n.p + t.band_off, rows * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(ctx, hipMemcpy(co.data(), b->d_coff.p + t.band_off, rows * 4, hipMemcpyDeviceToHost));
                    uint64_t off = 0;
                    for (size_t d = 0; d < rows && ok; ++d) {
                        ok = lo[d] == sg.lo[d] && nn[d] == sg.n[d] && co[d] == static_cast<uint32_t>(off);
                        if (!ok && std::getenv("NPR_TIMING"))
                            std::fprintf(stderr, "[npr plan check] row %zu: device lo %d n %d coff %u | host lo %d n %d coff %u\n", d, lo[d], nn[d], co[d], sg.lo[d],
                                         sg.n[d], static_cast<uint32_t>(off));
                        off += (static_cast<uint64_t>(sg.n[d]) + 3) & ~uint64_t(3);
                    }
                    if (ok && t.ctl_off >= 0) {
                        int cls = -1;  // the class the task was sorted into
                        for (const auto &L : b->launches)
                            if (k >= L.first && k < L.first + L.count) cls = L.cls;
                        ctl.resize(2 * rows), want_ctl.assign(2 * rows, 0);
                        HIP_TRY(ctx, hipMemcpy(ctl.data(), b->d_ctl.p + 2 * t.ctl_off, rows * 8, hipMemcpyDeviceToHost));
                        int64_t cells = 0;
                        ok = cls >= 0 && is_register_class(cls) && build_stair_schedule(sg, kClassTab[cls].R, kClassTab[cls].NW, want_ctl.data(), &cells) &&
                             ctl == want_ctl;
                        if (!ok && std::getenv("NPR_TIMING")) {
                            size_t q = 0;
                            while (q < 2 * rows && ctl[q] == want_ctl[q]) ++q;
                            std::fprintf(stderr, "[npr plan check] class %d, control word %zu of %zu: device %08x host %08x\n", cls, q, 2 * rows,
                                         q < 2 * rows ? ctl[q] : 0u, q < 2 * rows ? want_ctl[q] : 0u);
                        }
                    }
                    if (ok && t.tile_off >= 0) {
                        const int R = kClassTab[kTileClass].R;
                        const size_t S = static_cast<size_t>(stripes_of(sg, R)) + 1;
                        st.resize(S), want_st.assign(S, Stripe{});
                        HIP_TRY(ctx, hipMemcpy(st.data(), b->d_stripes.p + t.tile_off, S * sizeof(Stripe), hipMemcpyDeviceToHost));
                        build_stripes(sg, R, want_st.data(), nullptr);
                        ok = std::memcmp(st.data(), want_st.data(), S * sizeof(Stripe)) == 0;
                        if (ok && R == 2) {  // the packed lane masks of every row
                            const size_t nrows = static_cast<size_t>(want_st[0].K);
                            std::vector<uint32_t> rm(nrows), want_rm(nrows, 0);
                            if (nrows) HIP_TRY(ctx, hipMemcpy(rm.data(), b->d_rowmask.p + t.rowmask_off, nrows * sizeof(uint32_t), hipMemcpyDeviceToHost));
                            for (size_t q = 1; q < S; ++q)
                                for (int32_t d = want_st[q].df; d <= want_st[q].dl; ++d)
                                    want_rm[want_st[q].row0 + static_cast<uint32_t>(d - want_st[q].df)] = tile_row_word(d, sg.lo[d], sg.n[d], want_st[q].X);
                            ok = rm == want_rm;
                            if (!ok && std::getenv("NPR_TIMING")) std::fprintf(stderr, "[npr plan check] row masks differ (%zu rows)\n", nrows);
                        }
                        if (!ok && std::getenv("NPR_TIMING"))
                            for (size_t q = 0; q < S; ++q)
                                if (std::memcmp(&st[q], &want_st[q], sizeof(Stripe)) != 0) {
                                    std::fprintf(stderr, "[npr plan check] stripe entry %zu of %zu: device X %d K %d df %d dl %d row0 %u | host X %d K %d df %d dl %d row0 %u\n", q, S,
                                                 st[q].X, st[q].K, st[q].df, st[q].dl, st[q].row0, want_st[q].X, want_st[q].K, want_st[q].df, want_st[q].dl, want_st[q].row0);
                                    break;
                                }
                    }
                }
                if (!ok && mismatches < 4 && std::getenv("NPR_TIMING"))
                    std::fprintf(stderr, "[npr plan check] read %lld segment %d differs (D %d, widest band row n/a, ctl %lld, stripes %lld)\n", (long long)i, s,
                                 t.D, (long long)t.ctl_off, (long long)t.tile_off);
                mismatches += ok ? 0 : 1;
            }
        }
        return mismatches;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_plan_check: out of host memory");
    }
}

namespace {

// The accumulate-on-device half of npr_batch_base_expectations: the fixed-point sums (npr_stats.hip: exact, hence the same from run to run) and
// the seen bytes of the selected reads of a finished batch, queued on the context's stream and left in HBM for whoever reads them next -- the copy
// to the caller's table, or k_snp_calls.  `base`: first row of every reference sequence, base[n_refs] = rows > 0.
struct DeviceExpectations {
    DevBuf<unsigned long long> e;  // [rows][4]
    DevBuf<uint8_t> seen;          // [rows]
};
int32_t accumulate_base_expectations(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const std::vector<int64_t> &base, const char *unfit,
                                     DeviceExpectations &d) {
    npr_ctx *ctx = b->ctx;
    const int64_t rows = base[n_refs], n = b->n_reads, ntasks = static_cast<int64_t>(b->tasks.size());
    std::vector<int64_t> target(n, 0);
    std::vector<uint8_t> mask(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t k = b->ref_id[i];
        const bool ok = b->results[i].status == NPR_OK && (!use || use[i]) && k >= 0 && k < n_refs &&
                        b->gstart[2 * i] + b->ref_len[i] <= ref_len[k];
        if (use && use[i] && !ok && b->results[i].status == NPR_OK) return fail(ctx, NPR_ERR_INVALID, unfit);
        mask[i] = ok ? 1 : 0;
        target[i] = ok ? base[k] + b->gstart[2 * i] : 0;
    }
    DevBuf<uint8_t> d_use;
    DevBuf<int64_t> d_target;
    hipError_t e;
    if ((e = d.e.alloc(4 * rows)) != hipSuccess || (e = d.seen.alloc(rows)) != hipSuccess || (e = d_use.alloc(n)) != hipSuccess ||
        (e = d_target.alloc(n)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "base expectations: hipMalloc", e);
    HIP_TRY(ctx, hipMemsetAsync(d.e.p, 0, d.e.bytes(), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d.seen.p, 0, d.seen.bytes(), ctx->stream));
    if (!ntasks) return NPR_OK;
    HIP_TRY(ctx, hipMemcpyAsync(d_use.p, mask.data(), d_use.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_target.p, target.data(), d_target.bytes(), hipMemcpyHostToDevice, ctx->stream));
    ExpectArgs a{b->d_tasks.p, b->d_outs.p, static_cast<int32_t>(ntasks), b->d_px.p, b->d_py.p, b->d_pp.p, b->d_seq.p, d_use.p, d_target.p, d.e.p, d.seen.p};
    const int rc = launch_base_expectations(a, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_base_expectations launch", static_cast<hipError_t>(rc));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (mask, target, d_use and d_target end with this call)
    return NPR_OK;
}

// first row of every reference sequence; false: a negative length
bool row_bases(int64_t n_refs, const int64_t *ref_len, std::vector<int64_t> &base) {
    base.assign(n_refs + 1, 0);
    for (int64_t k = 0; k < n_refs; ++k) {
        if (ref_len[k] < 0) return false;
        base[k + 1] = base[k] + ref_len[k];
    }
    return true;
}

static_assert(sizeof(npr_snp_calls) == SNP_OUT_WORDS * sizeof(int64_t) && NPR_SNP_BINS == SNP_BINS && NPR_SNP_MAX_MODELS == kSnpMaxModels,
              "k_snp_calls writes an npr_snp_calls per model");

// The device half of the three SNP-call entry points: k_snp_calls over a table that lies on the device in the form `source` says, with the
// matrices' logs taken already; the base codes are uploaded, n_models structures come back.
int32_t run_snp_calls(npr_ctx *ctx, int64_t rows, int32_t source, const void *d_table, const uint8_t *d_seen, const uint8_t *ref_code,
                      const uint8_t *true_code, int32_t n_models, const double *log_evolution, const double *log_error, npr_snp_calls *out) {
    std::vector<npr_snp_calls> result(n_models);  // (out is written only when everything has worked)
    std::memset(static_cast<void *>(result.data()), 0, result.size() * sizeof(npr_snp_calls));
    if (rows > 0) {
        DevBuf<uint8_t> d_ref, d_true;
        DevBuf<unsigned long long> d_out;
        hipError_t e;
        if ((e = d_ref.alloc(rows)) != hipSuccess || (e = d_true.alloc(true_code ? rows : 0)) != hipSuccess ||
            (e = d_out.alloc(static_cast<size_t>(n_models) * SNP_OUT_WORDS)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "SNP calls: hipMalloc", e);
        HIP_TRY(ctx, hipMemcpyAsync(d_ref.p, ref_code, d_ref.bytes(), hipMemcpyHostToDevice, ctx->stream));
        if (true_code) HIP_TRY(ctx, hipMemcpyAsync(d_true.p, true_code, d_true.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_out.p, 0, d_out.bytes(), ctx->stream));
        SnpCallArgs a{};
        a.rows = rows, a.source = source, a.n_models = n_models, a.table = d_table, a.seen = d_seen, a.ref_code = d_ref.p, a.true_code = d_true.p, a.out = d_out.p;
        std::memcpy(a.log_evolution, log_evolution, sizeof(a.log_evolution));
        std::memcpy(a.log_error, log_error, static_cast<size_t>(n_models) * 16 * sizeof(double));
        const int rc = launch_snp_calls(a, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_snp_calls launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipMemcpyAsync(result.data(), d_out.p, d_out.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::memcpy(static_cast<void *>(out), result.data(), result.size() * sizeof(npr_snp_calls));
    return NPR_OK;
}

// The device half of the three SNP-variant entry points, the table as for run_snp_calls: k_snp_variants_count and the scan, the one word
// the capacity decision needs, then k_snp_variants_emit when the calls fit.  Scratch from the context's cache of released buffers.
// *n_calls and best / qual (each when given) are written in both outcomes, the call arrays only when everything has worked.
int64_t run_snp_variants(npr_ctx *ctx, int64_t rows, int32_t source, const void *d_table, const uint8_t *d_seen, const uint8_t *ref_code,
                         const double *log_evolution, const double *log_error, double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row,
                         uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls) {
    if (rows == 0) return *n_calls = 0;
    const int64_t tiles = snp_variant_tiles(rows);
    DevBuf<uint8_t> d_bytes, d_alt;  // ref_code, best, qual, mask: [4][rows]
    DevBuf<uint32_t> d_tile_calls;
    DevBuf<int64_t> d_tile_off, d_row;
    DevBuf<double> d_p;
    hipError_t e;
    if ((e = d_bytes.alloc_from(ctx, 4 * static_cast<size_t>(rows))) != hipSuccess || (e = d_tile_calls.alloc_from(ctx, tiles)) != hipSuccess ||
        (e = d_tile_off.alloc_from(ctx, tiles + 1)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "SNP variants: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_bytes.p, ref_code, rows, hipMemcpyHostToDevice, ctx->stream));
    SnpCallArgs a{};
    a.rows = rows, a.source = source, a.n_models = 1, a.table = d_table, a.seen = d_seen, a.ref_code = d_bytes.p, a.threshold = threshold;
    a.best = d_bytes.p + rows, a.qual = d_bytes.p + 2 * rows, a.mask = d_bytes.p + 3 * rows, a.tile_calls = d_tile_calls.p, a.tile_off = d_tile_off.p;
    std::memcpy(a.log_evolution, log_evolution, sizeof(a.log_evolution));
    std::memcpy(a.log_error, log_error, 16 * sizeof(double));
    int rc = launch_snp_variants_count(a, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_snp_variants_count launch", static_cast<hipError_t>(rc));
    int64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, d_tile_off.p + tiles, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const bool fits = total <= cap && (total == 0 || (call_row && call_alt && call_p));
    if (fits && total) {
        if ((e = d_row.alloc_from(ctx, total)) != hipSuccess || (e = d_alt.alloc_from(ctx, total)) != hipSuccess || (e = d_p.alloc_from(ctx, total)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "SNP variants: hipMalloc", e);
        a.n_calls = total, a.call_row = d_row.p, a.call_alt = d_alt.p, a.call_p = d_p.p;
        rc = launch_snp_variants_emit(a, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_snp_variants_emit launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipMemcpyAsync(call_row, d_row.p, d_row.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(call_alt, d_alt.p, d_alt.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(call_p, d_p.p, d_p.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (best) HIP_TRY(ctx, hipMemcpyAsync(best, a.best, rows, hipMemcpyDeviceToHost, ctx->stream));
    if (qual) HIP_TRY(ctx, hipMemcpyAsync(qual, a.qual, rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_calls = total;
    if (!fits) return fail(ctx, NPR_ERR_CAPACITY, "SNP variants: more calls than the arrays hold (*n_calls says how many)");
    return total;
}

// what the three entry points check of their model and outputs before anything else: the matrices' logs, or false
bool snp_variant_model(const double *evolution16, const double *error16, double threshold, int64_t cap, const int64_t *n_calls, double *log_evolution,
                       double *log_error) {
    return n_calls && cap >= 0 && threshold >= 0.0 && threshold <= 1.0 && snp_log_matrices(1, evolution16, error16, log_evolution, log_error);
}
const char *const kSnpVariantModel =
    ": a threshold outside [0, 1], a negative capacity, no n_calls, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row";

}  // namespace

int32_t npr_batch_base_expectations(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, double *expect, uint8_t *seen) {
    if (!b || n_refs < 0 || (n_refs && !ref_len) || !expect || !seen) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = b->ctx;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<int64_t> base;
        if (!row_bases(n_refs, ref_len, base)) return NPR_ERR_INVALID;
        const int64_t rows = base[n_refs];
        std::fill(expect, expect + 4 * rows, 0.0);
        std::fill(seen, seen + rows, uint8_t(0));
        if (b->tasks.empty() || !rows) return NPR_OK;
        DeviceExpectations d;
        const int32_t rc = accumulate_base_expectations(b, use, n_refs, ref_len, base, "npr_batch_base_expectations: a read's window does not fit its reference", d);
        if (rc != NPR_OK) return rc;
        static_assert(sizeof(unsigned long long) == sizeof(double), "the caller's table doubles as the staging of the fixed-point sums");
        HIP_TRY(ctx, hipMemcpyAsync(expect, d.e.p, d.e.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(seen, d.seen.p, d.seen.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < 4 * rows; ++i) {
            unsigned long long fixed;
            std::memcpy(&fixed, expect + i, sizeof(fixed));
            expect[i] = static_cast<double>(fixed) / static_cast<double>(EXPECT_FIXED_ONE);
        }
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_base_expectations: out of host memory");
    }
}

int32_t npr_snp_calls_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code, const uint8_t *true_code,
                            int32_t n_models, const double *evolution16, const double *error16, npr_snp_calls *out) {
    if (!ctx) return NPR_ERR_INVALID;
    if (rows < 0 || (rows && (!weights || !seen || !ref_code)) || !out) return fail(ctx, NPR_ERR_INVALID, "npr_snp_calls_table: bad argument");
    double log_evolution[16], log_error[kSnpMaxModels * 16];
    if (!snp_log_matrices(n_models, evolution16, error16, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, "npr_snp_calls_table: n_models outside 1..4, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row");
    try {
        for (int64_t i = 0; i < 4 * rows; ++i)
            if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return fail(ctx, NPR_ERR_INVALID, "npr_snp_calls_table: a weight is negative or not finite");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        DevBuf<double> d_w;
        DevBuf<uint8_t> d_seen;
        hipError_t e;
        if ((e = d_w.alloc(4 * rows)) != hipSuccess || (e = d_seen.alloc(rows)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_snp_calls_table: hipMalloc", e);
        if (rows) {
            HIP_TRY(ctx, hipMemcpyAsync(d_w.p, weights, d_w.bytes(), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_seen.p, seen, d_seen.bytes(), hipMemcpyHostToDevice, ctx->stream));
        }
        return run_snp_calls(ctx, rows, SNP_SRC_DOUBLE, d_w.p, d_seen.p, ref_code, true_code, n_models, log_evolution, log_error, out);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_snp_calls_table: out of host memory");
    }
}

int32_t npr_batch_snp_calls(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code, const uint8_t *true_code,
                            int32_t n_models, const double *evolution16, const double *error16, npr_snp_calls *out) {
    if (!b || n_refs < 0 || (n_refs && !ref_len) || !out) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = b->ctx;
    double log_evolution[16], log_error[kSnpMaxModels * 16];
    if (!snp_log_matrices(n_models, evolution16, error16, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, "npr_batch_snp_calls: n_models outside 1..4, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row");
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<int64_t> base;
        if (!row_bases(n_refs, ref_len, base)) return NPR_ERR_INVALID;
        const int64_t rows = base[n_refs];
        if (rows && !ref_code) return fail(ctx, NPR_ERR_INVALID, "npr_batch_snp_calls: no reference base codes");
        DeviceExpectations d;
        if (rows) {
            const int32_t rc = accumulate_base_expectations(b, use, n_refs, ref_len, base, "npr_batch_snp_calls: a read's window does not fit its reference", d);
            if (rc != NPR_OK) return rc;
        }
        return run_snp_calls(ctx, rows, SNP_SRC_FIXED, d.e.p, d.seen.p, ref_code, true_code, n_models, log_evolution, log_error, out);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_snp_calls: out of host memory");
    }
}

int32_t npr_pileup_snp_calls(npr_pileup *pl, const uint8_t *ref_code, const uint8_t *true_code, int32_t n_models, const double *evolution16,
                             const double *error16, npr_snp_calls *out) {
    if (!pl || !out) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (pl->rows && !ref_code) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_snp_calls: no reference base codes");
    double log_evolution[16], log_error[kSnpMaxModels * 16];
    if (!snp_log_matrices(n_models, evolution16, error16, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, "npr_pileup_snp_calls: n_models outside 1..4, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row");
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        // (words 0-4 are what k_pileup_add wrote on this stream: the running sum of word 5 is not needed)
        return run_snp_calls(ctx, pl->rows, SNP_SRC_PILEUP, pl->tab.p, nullptr, ref_code, true_code, n_models, log_evolution, log_error, out);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_snp_calls: out of host memory");
    }
}

int64_t npr_snp_variants_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code, const double *evolution16,
                               const double *error16, double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p,
                               int64_t cap, int64_t *n_calls) {
    if (!ctx) return NPR_ERR_INVALID;
    if (rows < 0 || (rows && (!weights || !seen || !ref_code))) return fail(ctx, NPR_ERR_INVALID, "npr_snp_variants_table: bad argument");
    double log_evolution[16], log_error[16];
    if (!snp_variant_model(evolution16, error16, threshold, cap, n_calls, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, (std::string("npr_snp_variants_table") + kSnpVariantModel).c_str());
    try {
        for (int64_t i = 0; i < 4 * rows; ++i)
            if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return fail(ctx, NPR_ERR_INVALID, "npr_snp_variants_table: a weight is negative or not finite");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        DevBuf<double> d_w;
        DevBuf<uint8_t> d_seen;
        hipError_t e;
        if ((e = d_w.alloc_from(ctx, 4 * rows)) != hipSuccess || (e = d_seen.alloc_from(ctx, rows)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_snp_variants_table: hipMalloc", e);
        if (rows) {
            HIP_TRY(ctx, hipMemcpyAsync(d_w.p, weights, d_w.bytes(), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_seen.p, seen, d_seen.bytes(), hipMemcpyHostToDevice, ctx->stream));
        }
        return run_snp_variants(ctx, rows, SNP_SRC_DOUBLE, d_w.p, d_seen.p, ref_code, log_evolution, log_error, threshold, best, qual, call_row, call_alt, call_p,
                                cap, n_calls);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_snp_variants_table: out of host memory");
    }
}

int64_t npr_batch_snp_variants(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code, const double *evolution16,
                               const double *error16, double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p,
                               int64_t cap, int64_t *n_calls) {
    if (!b || n_refs < 0 || (n_refs && !ref_len)) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    npr_ctx *ctx = b->ctx;
    double log_evolution[16], log_error[16];
    if (!snp_variant_model(evolution16, error16, threshold, cap, n_calls, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, (std::string("npr_batch_snp_variants") + kSnpVariantModel).c_str());
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<int64_t> base;
        if (!row_bases(n_refs, ref_len, base)) return NPR_ERR_INVALID;
        const int64_t rows = base[n_refs];
        if (rows && !ref_code) return fail(ctx, NPR_ERR_INVALID, "npr_batch_snp_variants: no reference base codes");
        DeviceExpectations d;
        if (rows) {
            const int32_t rc = accumulate_base_expectations(b, use, n_refs, ref_len, base, "npr_batch_snp_variants: a read's window does not fit its reference", d);
            if (rc != NPR_OK) return rc;
        }
        return run_snp_variants(ctx, rows, SNP_SRC_FIXED, d.e.p, d.seen.p, ref_code, log_evolution, log_error, threshold, best, qual, call_row, call_alt, call_p,
                                cap, n_calls);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_snp_variants: out of host memory");
    }
}

int64_t npr_pileup_snp_variants(npr_pileup *pl, const uint8_t *ref_code, const double *evolution16, const double *error16, double threshold, uint8_t *best,
                                uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls) {
    if (!pl) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (pl->rows && !ref_code) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_snp_variants: no reference base codes");
    double log_evolution[16], log_error[16];
    if (!snp_variant_model(evolution16, error16, threshold, cap, n_calls, log_evolution, log_error))
        return fail(ctx, NPR_ERR_INVALID, (std::string("npr_pileup_snp_variants") + kSnpVariantModel).c_str());
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return run_snp_variants(ctx, pl->rows, SNP_SRC_PILEUP, pl->tab.p, nullptr, ref_code, log_evolution, log_error, threshold, best, qual, call_row, call_alt,
                                call_p, cap, n_calls);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_snp_variants: out of host memory");
    }
}

// ---- the device pileup (npr_pileup.hip) ----
namespace {

// k_pileup_add over n records whose cigars are packed on the device already or given on the host (as for run_align_stats); *bad: some
// record's cigar ran past what it has
int32_t run_pileup_add(npr_pileup *pl, int64_t n, const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops,
                       const std::vector<int64_t> *h_off, const std::vector<PileupRec> &recs, const uint8_t *d_seq, bool ascii, int32_t *bad) {
    npr_ctx *ctx = pl->ctx;
    DevBuf<uint32_t> ops;
    DevBuf<int64_t> off;
    DevBuf<PileupRec> rc;
    hipError_t e;
    if (!d_ops) {
        if ((e = ops.alloc(h_ops->size())) != hipSuccess || (e = off.alloc(h_off->size())) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add: hipMalloc", e);
        if (!h_ops->empty()) HIP_TRY(ctx, hipMemcpyAsync(ops.p, h_ops->data(), ops.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(off.p, h_off->data(), off.bytes(), hipMemcpyHostToDevice, ctx->stream));
        d_ops = ops.p, d_off = off.p;
    }
    if ((e = rc.alloc(recs.size())) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(rc.p, recs.data(), rc.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(pl->bad.p, 0, sizeof(int32_t), ctx->stream));
    const PileupArgs a{n, d_off, d_ops, rc.p, d_seq, ascii ? 1 : 0, pl->tab.p, pl->diff.p, pl->bad.p};
    const int r = launch_pileup_add(a, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_pileup_add launch", static_cast<hipError_t>(r));
    HIP_TRY(ctx, hipMemcpyAsync(bad, pl->bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the cigars may lie in the arena, whose lock the caller holds until here)
    return NPR_OK;
}

// word 5 of the table from the difference array
int32_t pileup_scan(npr_pileup *pl) {
    npr_ctx *ctx = pl->ctx;
    const int64_t n_refs = static_cast<int64_t>(pl->len.size()), n_slots = pl->rows + n_refs;
    const PileupScanArgs a{n_slots, n_refs, pileup_scan_tiles(n_slots), pl->dbase.p, pl->diff.p, pl->tile.p, pl->tab.p};
    const int r = launch_pileup_scan(a, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_pileup_scan launch", static_cast<hipError_t>(r));
    return NPR_OK;
}

}  // namespace

int32_t npr_pileup_create(npr_ctx *ctx, int64_t n_refs, const int64_t *ref_len, npr_pileup **out) {
    if (!ctx || !out || n_refs < 0 || (n_refs && !ref_len)) return NPR_ERR_INVALID;
    *out = nullptr;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
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
        hipError_t e;
        if ((e = pl->tab.alloc(static_cast<size_t>(pl->rows) * NPR_PILEUP_WORDS)) != hipSuccess || (e = pl->diff.alloc(static_cast<size_t>(n_slots))) != hipSuccess ||
            (e = pl->tile.alloc(static_cast<size_t>(pileup_scan_tiles(n_slots)))) != hipSuccess || (e = pl->dbase.alloc(dbase.size())) != hipSuccess ||
            (e = pl->bad.alloc(1)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_create: hipMalloc", e);
        if (pl->rows) HIP_TRY(ctx, hipMemsetAsync(pl->tab.p, 0, pl->tab.bytes(), ctx->stream));
        if (n_slots) HIP_TRY(ctx, hipMemsetAsync(pl->diff.p, 0, pl->diff.bytes(), ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(pl->dbase.p, dbase.data(), pl->dbase.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *out = pl.release();
        return NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_create: out of host memory");
    }
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
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
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
        const int32_t rc = with_batch_cigars(b, [&](const uint32_t *d_ops, const int64_t *d_off, const std::vector<uint32_t> *h_ops, const std::vector<int64_t> *h_off) {
            return run_pileup_add(pl, n, d_ops, d_off, h_ops, h_off, recs, b->d_seq.p, false, &bad);
        });
        if (rc != NPR_OK) return rc;
        if (unfit) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_batch: a read's window does not fit its reference in the pileup (the read was left out)");
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_pileup_add_batch: a cigar runs past its window (the read was left out)") : NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add_batch: out of host memory");
    }
}

int32_t npr_pileup_add(npr_pileup *pl, int64_t n, const int32_t *ref_index, const uint8_t *read, const int64_t *read_begin, const int64_t *read_end,
                       const int32_t *ops, const int64_t *ops_off, const int64_t *start, const uint8_t *use) {
    if (!pl || n < 0 || (n && (!ref_index || !read_begin || !ops_off))) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (n == 0) return NPR_OK;
    if (n >= (int64_t(1) << 31)) return fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: too many records");
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
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
        hipError_t e;
        std::unique_ptr<uint8_t[]> gathered;
        if (!read_end) {
            const int64_t bytes = read_begin[n] - read_begin[0];
            if (bytes < 0 || (bytes && !read)) return NPR_ERR_INVALID;
            if ((e = d_seq.alloc(static_cast<size_t>(bytes) + 1)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add: hipMalloc", e);
            if (bytes) HIP_TRY(ctx, hipMemcpyAsync(d_seq.p, read + read_begin[0], static_cast<size_t>(bytes), hipMemcpyHostToDevice, ctx->stream));
            for (int64_t i = 0; i < n; ++i)
                if (recs[i].xlen >= 0) recs[i].y_off = read_begin[i] - read_begin[0] + (start ? start[2 * i + 1] : 0);
        } else {
            int64_t bytes = 0;
            for (int64_t i = 0; i < n; ++i)
                if (recs[i].xlen >= 0) recs[i].y_off = bytes, bytes += ylen[i];
            if (bytes && !read) return NPR_ERR_INVALID;
            gathered.reset(new uint8_t[bytes + 1]);
            parallel_for(n, ctx->host_threads, [&](int64_t i) {
                if (recs[i].xlen >= 0 && ylen[i]) std::memcpy(gathered.get() + recs[i].y_off, read + read_begin[i] + (start ? start[2 * i + 1] : 0), static_cast<size_t>(ylen[i]));
            });
            if ((e = d_seq.alloc(static_cast<size_t>(bytes) + 1)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add: hipMalloc", e);
            if (bytes) HIP_TRY(ctx, hipMemcpyAsync(d_seq.p, gathered.get(), static_cast<size_t>(bytes), hipMemcpyHostToDevice, ctx->stream));
        }
        int32_t bad = 0;
        const int32_t rc = run_pileup_add(pl, n, nullptr, nullptr, &packed, &off, recs, d_seq.p, true, &bad);
        if (rc != NPR_OK) return rc;
        for (int64_t i = 0; i < n; ++i) bad |= malformed[i];
        return bad ? fail(ctx, NPR_ERR_INVALID, "npr_pileup_add: a record is malformed or its cigar runs past its sequences (the record was left out)") : NPR_OK;
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_add: out of host memory");
    }
}

int32_t npr_pileup_counts(npr_pileup *pl, int32_t *counts) {
    if (!pl || (pl->rows && !counts)) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (pl->rows == 0) return NPR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t rc = pileup_scan(pl);
    if (rc != NPR_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(counts, pl->tab.p, pl->tab.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

int32_t npr_pileup_depth(npr_pileup *pl, int32_t *depth, uint8_t *covered) {
    if (!pl || (pl->rows && (!depth || !covered))) return NPR_ERR_INVALID;
    npr_ctx *ctx = pl->ctx;
    if (pl->rows == 0) return NPR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t rc = pileup_scan(pl);
    if (rc != NPR_OK) return rc;
    DevBuf<int32_t> d_depth;
    DevBuf<uint8_t> d_cov;
    hipError_t e;
    if ((e = d_depth.alloc(static_cast<size_t>(pl->rows))) != hipSuccess || (e = d_cov.alloc(static_cast<size_t>(pl->rows))) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_pileup_depth: hipMalloc", e);
    const int r = launch_pileup_depth(pl->tab.p, pl->rows, d_depth.p, d_cov.p, ctx->stream);
    if (r != 0) return fail(ctx, NPR_ERR_HIP, "k_pileup_depth launch", static_cast<hipError_t>(r));
    HIP_TRY(ctx, hipMemcpyAsync(depth, d_depth.p, d_depth.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(covered, d_cov.p, d_cov.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}


}  // extern "C"