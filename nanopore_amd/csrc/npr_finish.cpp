// npr_finish.cpp -- npr_batch_finish and what reads its results: the device MEA stage, the rescore sums, the host stage, cigars and posterior pairs (utils.py:591-609; alignmentUncertainty.py:41)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace npr_impl {

// one of the context's pinned staging buffers (grow-only) of at least `bytes`
static int32_t grow_pinned(npr_ctx *ctx, void *&p, size_t &have, size_t bytes, const char *what) {
    if (bytes <= have) return NPR_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr, have = 0;
    const hipError_t e = hipHostMalloc(&p, bytes + bytes / 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, what, e);
    have = bytes + bytes / 4;
    return NPR_OK;
}
int32_t grow_pin_pairs(npr_ctx *ctx, size_t bytes, const char *what) { return grow_pinned(ctx, ctx->pin_pairs, ctx->pin_pairs_bytes, bytes, what); }
int32_t grow_pin_stage(npr_ctx *ctx, size_t bytes, const char *what) { return grow_pinned(ctx, ctx->pin_stage, ctx->pin_stage_bytes, bytes, what); }

// From the device to pageable host memory through the pinned staging, in pieces: the host threads move a piece out of the staging
// buffer while the next ones cross.
int32_t fetch_pieced(npr_ctx *ctx, const PiecedFetch &f) {
    if (f.count <= 0) return NPR_OK;
    const int32_t grown = grow_pin_pairs(ctx, f.elem * static_cast<size_t>(f.count), f.what_pin);
    if (grown != NPR_OK) return grown;
    constexpr int64_t kMaxPieces = 48;
    const int64_t pieces = std::min(kMaxPieces, (f.count + f.per_piece - 1) / f.per_piece);
    const int64_t piece = ((f.count + pieces - 1) / pieces + f.round_to - 1) / f.round_to * f.round_to;
    while (static_cast<int64_t>(ctx->ops_events.size()) < pieces) {
        hipEvent_t ev;
        const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return fail(ctx, NPR_ERR_HIP, "hipEventCreate", e);
        ctx->ops_events.push_back(ev);
    }
    const char *dev = static_cast<const char *>(f.dev);
    char *pin = static_cast<char *>(ctx->pin_pairs);
    for (int64_t c = 0; c < pieces; ++c) {
        const int64_t lo = std::min(f.count, c * piece), hi = std::min(f.count, lo + piece);
        if (hi > lo) HIP_TRY(ctx, hipMemcpyAsync(pin + f.elem * lo, dev + f.elem * lo, f.elem * static_cast<size_t>(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ops_events[c], ctx->stream));
    }
    std::atomic<int> failed{0};
    parallel_for(pieces, ctx->host_threads, [&](int64_t c) {  // (the items are handed out in order)
        if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(ctx->ops_events[c]) != hipSuccess) {  // (a worker thread starts on device 0)
            failed = 1;
            return;
        }
        const int64_t lo = std::min(f.count, c * piece), hi = std::min(f.count, lo + piece);
        f.move(f.dst, pin, lo, hi);
    });
    if (failed) return fail(ctx, NPR_ERR_HIP, f.what_d2h, hipGetLastError());
    return NPR_OK;
}

// Posterior pairs of every read to the host: one dense D2H, then per read (host threads) its segments' pairs merged
// and sorted by (x, y).  b->task_dst (prefix of the per-task pair counts) and b->pair_off are already set.
int32_t fetch_pairs(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    if (b->pairs_ready) return NPR_OK;
    StageTimer tm("fetch_pairs");
    const int64_t ntasks = static_cast<int64_t>(b->tasks.size());
    const std::vector<int64_t> &dst = b->task_dst;
    const int32_t *hx = nullptr, *hy = nullptr;
    const float *hp = nullptr;
    const int64_t total = ntasks ? dst[ntasks] : 0;
    if (total) {
        DevBuf<int64_t> d_dst;
        DevBuf<int32_t> d_cx, d_cy;
        DevBuf<float> d_cp;
        hipError_t e;
        if ((e = d_dst.alloc_from(ctx, ntasks + 1)) != hipSuccess || (e = d_cx.alloc_from(ctx, total)) != hipSuccess ||
            (e = d_cy.alloc_from(ctx, total)) != hipSuccess || (e = d_cp.alloc_from(ctx, total)) != hipSuccess)
            return fail(ctx, NPR_ERR_NOMEM, "npr_batch_finish: hipMalloc", e);
        HIP_TRY(ctx, hipMemcpyAsync(d_dst.p, dst.data(), d_dst.bytes(), hipMemcpyHostToDevice, ctx->stream));
        CompactArgs ca{b->d_tasks.p, b->d_outs.p, d_dst.p, static_cast<int32_t>(ntasks), b->d_px.p, b->d_py.p, b->d_pp.p, d_cx.p, d_cy.p, d_cp.p};
        const int rc = launch_compact(ca, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_compact launch", static_cast<hipError_t>(rc));
        const int32_t grown = grow_pin_pairs(ctx, static_cast<size_t>(total) * 12, "npr_batch_finish: hipHostMalloc");
        if (grown != NPR_OK) return grown;
        int32_t *px_h = static_cast<int32_t *>(ctx->pin_pairs), *py_h = px_h + total;
        float *pp_h = reinterpret_cast<float *>(py_h + total);
        HIP_TRY(ctx, hipMemcpyAsync(px_h, d_cx.p, d_cx.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(py_h, d_cy.p, d_cy.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(pp_h, d_cp.p, d_cp.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        hx = px_h, hy = py_h, hp = pp_h;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    tm.lap("compact + D2H");
    const int64_t n = b->n_reads;
    b->pairs.resize(b->pair_off[n]);
    parallel_for(n, ctx->host_threads, [&](int64_t i) {
        if (b->read_status[i] != NPR_OK) return;
        Pair *pp = b->pairs.data() + b->pair_off[i];
        int64_t c = 0;
        for (int32_t s = 0; s < b->read_ntasks[i]; ++s) {
            const int32_t k = b->task_of[b->read_first_task[i] + s];
            for (int64_t q = dst[k]; q < dst[k + 1]; ++q) pp[c++] = Pair{hx[q], hy[q], hp[q]};
        }
        // order by (x, y).  The pairs of a read number about two per reference base, so when the reference span is
        // not much longer than the list a counting sort on x (+ insertion sort of the few pairs sharing an x) beats
        // a comparison sort several times over; chained records that span a whole contig keep std::sort.
        const int64_t span = b->ref_len[i];
        if (c > 64 && span <= 4 * c) {
            thread_local std::vector<int32_t> start;
            thread_local std::vector<Pair> tmp;
            start.assign(span + 2, 0);
            bool ok = true;
            for (int64_t q = 0; q < c; ++q) {
                if (pp[q].x < 0 || pp[q].x >= span) {
                    ok = false;
                    break;
                }
                ++start[pp[q].x + 1];
            }
            if (ok) {
                for (int64_t x = 0; x < span; ++x) start[x + 1] += start[x];
                tmp.resize(c);
                for (int64_t q = 0; q < c; ++q) tmp[start[pp[q].x]++] = pp[q];  // start[x] is now the END of group x
                int64_t g = 0;
                for (int64_t q = 0; q < c; ++q) {  // insertion sort inside each x-group
                    if (q > 0 && tmp[q].x != tmp[q - 1].x) g = q;
                    Pair v = tmp[q];
                    int64_t k = q;
                    while (k > g && tmp[k - 1].y > v.y) tmp[k] = tmp[k - 1], --k;
                    tmp[k] = v;
                }
                std::copy(tmp.begin(), tmp.end(), pp);
            } else {
                std::sort(pp, pp + c, [](const Pair &a, const Pair &d) { return a.x != d.x ? a.x < d.x : a.y < d.y; });
            }
        } else {
            std::sort(pp, pp + c, [](const Pair &a, const Pair &d) { return a.x != d.x ? a.x < d.x : a.y < d.y; });
        }
    });
    tm.lap("merge + sort");
    b->pairs_ready = true;
    return NPR_OK;
}

// NPR_MODE_RESCORE_ORIGINAL on the device (npr_stats.hip k_rescore_table / k_rescore_sum; the reference's call site: alignmentUncertainty.py:41,
// the analysis that runs on every experiment by default, pipeline.py:81).  At staging the guide's M runs go up once (12 bytes per run) and are
// spread into a table over the reference positions of each read's window; every pass then is one sweep over the pairs where the DP kernels
// left them and eight bytes per read coming back -- no pair crosses PCIe, and the guide's operations are not copied until somebody asks for
// the cigars.  rescore_stage leaves b->rs_staged false when the fixed-point sum could not be exact (a threshold below 2^-20, a guide of
// 2^(53 - shift) M columns): the host stage scores then.
int32_t rescore_stage(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    const int64_t n = b->n_reads;
    StageTimer tm("rescore_stage");
    b->rs_staged = false;
    b->rs_columns.assign(n, 0), b->rs_kept.assign(n, 0);
    std::vector<int64_t> run_off(n + 1, 0), gx_off(n + 1, 0);
    parallel_for(n, ctx->host_threads, [&](int64_t i) {
        int64_t runs = 0, cols = 0, kept = 0;
        for (int64_t q = b->guide_off[i]; q < b->guide_off[i + 1]; ++q) {
            const int32_t len = b->guide_ops[2 * q + 1];
            kept += len > 0;
            if (b->guide_ops[2 * q] == NPR_OP_M && len > 0) ++runs, cols += len;
        }
        b->rs_columns[i] = cols, b->rs_kept[i] = kept, run_off[i + 1] = b->read_status[i] == NPR_OK ? runs : 0;
    });
    if (ctx->opt[NPR_OPT_HOST_MEA] != 0 || n == 0) return NPR_OK;
    int e2 = 0;
    (void)std::frexp(b->params.posterior_threshold, &e2);  // threshold = m * 2^e2, m in [0.5, 1): an fp32 p >= threshold is a multiple of 2^(e2 - 1 - 23)
    const int shift = 24 - e2;
    if (!(b->params.posterior_threshold > 0.0) || shift > 44 || shift < 0) return NPR_OK;
    for (int64_t i = 0; i < n; ++i) {
        if (b->rs_columns[i] >= (int64_t(1) << (53 - shift))) return NPR_OK;
        run_off[i + 1] += run_off[i];
        gx_off[i + 1] = gx_off[i] + (b->read_status[i] == NPR_OK ? b->ref_len[i] + 1 : 0);
    }
    // the runs through the context's pinned staging buffer when it is there (157 MB for 8192 reads of 8 kb: pageable memory halves the copy's rate)
    std::vector<int32_t> runs_v;
    int32_t *runs = nullptr;
    const size_t run_bytes = sizeof(int32_t) * 3 * static_cast<size_t>(run_off[n]);
    if (ctx->pin_stage && ctx->pin_stage_bytes >= run_bytes) runs = static_cast<int32_t *>(ctx->pin_stage);
    else runs_v.resize(3 * static_cast<size_t>(run_off[n])), runs = runs_v.data();
    parallel_for(n, ctx->host_threads, [&](int64_t i) {
        if (b->read_status[i] != NPR_OK) return;
        int32_t *out = runs + 3 * run_off[i];
        int64_t x = 0, y = 0;
        for (int64_t q = b->guide_off[i]; q < b->guide_off[i + 1]; ++q) {
            const int32_t op = b->guide_ops[2 * q], len = b->guide_ops[2 * q + 1];
            if (op == NPR_OP_M) {
                if (len > 0) out[0] = static_cast<int32_t>(x), out[1] = static_cast<int32_t>(y), out[2] = len, out += 3;
                x += len, y += len;
            } else if (op == NPR_OP_I) {
                y += len;
            } else {
                x += len;
            }
        }
    });
    tm.lap("runs");
    DevBuf<int64_t> d_run_off;
    DevBuf<int32_t> d_runs;
    hipError_t e;
    if ((e = d_run_off.alloc_from(ctx, n + 1)) != hipSuccess || (e = b->d_rs_gx_off.alloc_from(ctx, n + 1)) != hipSuccess ||
        (e = d_runs.alloc_from(ctx, std::max<size_t>(3 * static_cast<size_t>(run_off[n]), 1))) != hipSuccess ||
        (e = b->d_rs_gy.alloc_from(ctx, std::max<int64_t>(gx_off[n], 1))) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc (rescore tables)", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_run_off.p, run_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(b->d_rs_gx_off.p, gx_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (run_bytes) HIP_TRY(ctx, hipMemcpyAsync(d_runs.p, runs, run_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b->d_rs_gy.p, 0xff, sizeof(int32_t) * std::max<int64_t>(gx_off[n], 1), ctx->stream));
    RescoreArgs ra{static_cast<int32_t>(n), 0, d_run_off.p, d_runs.p, b->d_rs_gx_off.p, b->d_rs_gy.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, shift};
    const int rc = launch_rescore_table(ra, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_rescore_table launch", static_cast<hipError_t>(rc));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging buffer and d_runs go back)
    tm.lap("table");
    b->rs_shift = shift, b->rs_staged = true;
    return NPR_OK;
}

int32_t rescore_sum(npr_batch *b, std::vector<double> &score) {
    npr_ctx *ctx = b->ctx;
    const int64_t n = b->n_reads, ntasks = static_cast<int64_t>(b->tasks.size());
    DevBuf<unsigned long long> d_sum;
    hipError_t e;
    if ((e = d_sum.alloc_from(ctx, n)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_finish: hipMalloc (rescore sums)", e);
    HIP_TRY(ctx, hipMemsetAsync(d_sum.p, 0, sizeof(unsigned long long) * n, ctx->stream));
    RescoreArgs ra{static_cast<int32_t>(n), static_cast<int32_t>(ntasks), nullptr, nullptr, b->d_rs_gx_off.p, b->d_rs_gy.p, b->d_tasks.p, b->d_outs.p,
                   b->d_px.p, b->d_py.p, b->d_pp.p, d_sum.p, b->rs_shift};
    const int rc = launch_rescore_sum(ra, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_rescore_sum launch", static_cast<hipError_t>(rc));
    std::vector<unsigned long long> sum(n);
    HIP_TRY(ctx, hipMemcpyAsync(sum.data(), d_sum.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    score.assign(n, 0.0);
    for (int64_t i = 0; i < n; ++i)
        if (b->rs_columns[i] > 0) score[i] = std::ldexp(static_cast<double>(sum[i]), -b->rs_shift) / static_cast<double>(b->rs_columns[i]);
    return NPR_OK;
}

// ---- the device MEA stage (npr_mea.hip): chain + cigar of every read on the device, only the ops cross PCIe ----

constexpr int32_t kHostStage = 1;  // what the stage's steps answer besides NPR_OK and errors: the host stage takes the batch

// One batch in the stage's numbers: the per-read offsets, which reads sort through global memory, the pieces of every chain, the reads' order.
struct MeaPlan {
    int64_t n = 0, total = 0, n_pieces = 0;  // reads, posterior pairs, chain pieces
    size_t ntask_map = 0, n_cnt = 1;         // entries of task_of; cells of the global-memory sort's tables
    int64_t span = 0;                        // the most table entries among the reads that sort in LDS
    bool sort_in_lds = true;
    // rx | ry | rp | ot | cnt_off as m.off takes them, n + 1 each: reference rows, read columns, pairs, the bound of the ops; first count cell or -1
    std::vector<int64_t> offs;
    int64_t stride() const { return n + 1; }
    int64_t *arr(int k) { return offs.data() + k * stride(); }
    int64_t cols() const { return offs[2 * stride() - 1]; }     // ry[n]
    int64_t ops_bound() const { return offs[4 * stride() - 1]; }  // ot[n]
    std::vector<int32_t> order;        // the reads longest first
    std::vector<int32_t> pieces_head;  // np[n] | poff[n] | pboff[n] | lane_read[P] | lane_piece[P] as m.pieces takes them
};

constexpr int64_t kOffArrays = 5, kSortedArrays = 8, kSmallArrays = 6, kVrecWords = 4;

MeaPlan plan_mea(const npr_batch *b) {
    MeaPlan p;
    const int64_t n = p.n = b->n_reads;
    p.offs.assign(kOffArrays * p.stride(), 0);
    int64_t *const rx = p.arr(0), *const ry = p.arr(1), *const rp = p.arr(2), *const ot = p.arr(3), *const cnt_off = p.arr(4);
    for (int64_t i = 0; i < n; ++i) {  // a read that already failed gets empty tables: its pairs are skipped as out of range
        const bool ok = b->results[i].status == NPR_OK;
        const int64_t lX = ok ? b->ref_len[i] : 0, lY = ok ? b->read_len[i] : 0, np = ok ? b->pair_off[i + 1] - b->pair_off[i] : 0;
        rx[i + 1] = rx[i] + lX + 1;
        ry[i + 1] = ry[i] + lY;
        rp[i + 1] = rp[i] + np;
        ot[i + 1] = ot[i] + 3 * std::min({np, lX, lY}) + 2;  // (D, I, M) per chain pair, one trailing (D, I)
    }
    p.total = rp[n];
    // per-position tables of one read in LDS (count, masses, scan, scatter and weights in one kernel) when the longer span fits: one table
    // over the reference positions and one over the read positions
    // ... read by read (round 4: one read of more than 16 k bases used to send its whole batch through the global-memory kernels)
    const int64_t lds_span = b->ctx->opt[NPR_OPT_MEA_GLOBAL_SORT] != 0 ? 0 : kMeaSortLdsSpan;
    int64_t cnt_total = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t sp = std::max(rx[i + 1] - rx[i], ry[i + 1] - ry[i]);
        cnt_off[i] = -1;
        if (sp <= lds_span) p.span = std::max(p.span, (rx[i + 1] - rx[i]) + (ry[i + 1] - ry[i]));
        else cnt_off[i] = cnt_total, cnt_total += rx[i + 1] - rx[i];
    }
    cnt_off[n] = -1;
    p.sort_in_lds = cnt_total == 0;
    p.n_cnt = p.sort_in_lds ? 1 : static_cast<size_t>(cnt_total);
    p.ntask_map = b->task_of.size();
    p.order.resize(n);  // longest first: the per-read kernels end together instead of waiting for a late long read
    std::iota(p.order.begin(), p.order.end(), 0);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t x, int32_t y) { return rp[x + 1] - rp[x] > rp[y + 1] - rp[y]; });
    // the pieces the chain of every read is cut into (npr_mea.hip k_mea_cuts): about 2000 posterior pairs (1200 kept) each
    // ... fewer in a small batch, so that the pieces (one lane each, a serial walk) still fill the chip: 1000 reads of 1 kb as 1000
    // pieces of 1100 kept pairs took 0.9 ms where 14 000 pieces of 80 take 0.1
    constexpr int64_t kMaxPieces = 64, kLanesWanted = 64 * 5 * 256;
    const int64_t kPiecePairs = std::min<int64_t>(2048, std::max<int64_t>(128, p.total / kLanesWanted));
    std::vector<int32_t> np(n);
    for (int64_t i = 0; i < n; ++i) np[i] = static_cast<int32_t>(std::min(kMaxPieces, std::max<int64_t>(1, (rp[i + 1] - rp[i] + kPiecePairs - 1) / kPiecePairs))), p.n_pieces += np[i];
    p.pieces_head.resize(3 * n + 2 * p.n_pieces);
    int32_t *const t_np = p.pieces_head.data(), *const t_poff = t_np + n, *const t_pboff = t_poff + n, *const t_lr = t_pboff + n, *const t_lp = t_lr + p.n_pieces;
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k) {  // lanes in the reads' order
        const int32_t r = p.order[k];
        t_np[r] = np[r], t_poff[r] = static_cast<int32_t>(at), t_pboff[r] = static_cast<int32_t>(at + k);
        for (int32_t j = 0; j < np[r]; ++j) t_lr[at + j] = r, t_lp[at + j] = j;
        at += np[r];
    }
    return p;
}

// The stage's tables.  Five of the buffers hold several arrays one behind the other; what follows is the only place that says how many and how long:
//   off     rx | ry | rp | ot | cnt_off, n + 1 each
//   sorted  sx | sy | sq | back | kx | ky | kq | kback, total + 1 each, then total + 2 records of 16 bytes (vrec), then sw, total + 1
//   small   best_who | read_flag | n_ops | chain_len | kept | max_run, n each
//   map     read_first[n] | read_ntasks[n] | task_of[ntask_map] | order[n]
//   pieces  np[n] | poff[n] | pboff[n] | lane_read[P] | lane_piece[P] | pbest[P] | pb[P + n], P = n_pieces; lanes in the reads' order
static_assert(kSortedArrays % kVrecWords == 0, "vrec starts on a 16-byte boundary of m.sorted (the arena's tables start 256-byte aligned)");
inline int64_t sorted_stride(const MeaPlan &p) { return p.total + 1; }

// every buffer of MeaScratch with its element count for the batch: f(buffer, count) until one fails
template <typename F>
hipError_t for_each_table(MeaScratch &m, const MeaPlan &p, F &&f) {
    hipError_t e = hipSuccess;
    auto one = [&](auto &buf, int64_t count) {
        if (e == hipSuccess) e = f(buf, static_cast<size_t>(count));
    };
    one(m.off, kOffArrays * p.stride());
    one(m.mass, p.n);
    one(m.od, p.n + 1);
    one(m.cnt, p.n_cnt);
    one(m.start, p.n_cnt);
    one(m.col, p.cols() + 1);
    one(m.sorted, kSortedArrays * sorted_stride(p) + kVrecWords * (p.total + 2) + sorted_stride(p));
    one(m.small, kSmallArrays * p.n);
    one(m.tmp, 2 * p.ops_bound());
    one(m.map, 3 * p.n + p.ntask_map);
    one(m.dense, p.ops_bound());  // (the bound ot[n] >= the ops the reads end up with)
    one(m.pieces, 4 * p.n_pieces + 4 * p.n);
    return e;
}

inline size_t table_align(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// the tables as views of the arena's first `need` bytes, one behind the other
int32_t carve_tables(npr_ctx *ctx, MeaScratch &m, const MeaPlan &p, size_t need) {
    if (poison_byte() >= 0) {  // the DP launches are done (their streams feed this one): the tables start from poison
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        poison(ctx->arena->F, need);
    }
    char *cur = ctx->arena->F;
    (void)for_each_table(m, p, [&](auto &buf, size_t count) {
        using T = std::remove_pointer_t<decltype(buf.p)>;
        buf.borrow(reinterpret_cast<T *>(cur), count);
        cur += table_align(sizeof(T) * count);
        return hipSuccess;
    });
    return NPR_OK;
}

// The forward scratch of the DP launches is idle now and usually far larger than what this stage needs: the tables are carved out of it when
// they fit (a batch that fills the device's memory leaves nothing to hipMalloc) -- unless the context runs next to others (NPR_OPT_OVERLAP):
// then they live in grow-only buffers of its own and the stage need not wait for another batch's DP pass.
int32_t obtain_tables(npr_ctx *ctx, MeaScratch &m, const MeaPlan &p, std::unique_lock<std::mutex> &arena_lock) {
    size_t need = 0;
    (void)for_each_table(m, p, [&](auto &buf, size_t count) { return need += table_align(sizeof(*buf.p) * count), hipSuccess; });
    auto arena_fits = [&] { return ctx->arena->F && need <= static_cast<size_t>(ctx->arena->cells.load()) * 8; };
    const bool fits = arena_fits();
    if (!ctx->overlap && fits) return carve_tables(ctx, m, p, need);
    if (for_each_table(m, p, [](auto &buf, size_t count) { return buf.reserve(count); }) == hipSuccess) return NPR_OK;
    (void)hipGetLastError();
    if (!(ctx->overlap && fits)) return kHostStage;  // no room on the device
    // When the own buffers do not fit beside the batches in flight (long reads: 52 bytes per pair, three chunks of a pipelined job on the
    // device) the context waits for the shared scratch after all, and gives back what it had reserved.
    (void)for_each_table(m, p, [](auto &buf, size_t) { return buf.release(), hipSuccess; });
    ctx->cache_flush();
    arena_lock.lock();
    // (`fits` was read before the lock: another context may have released or regrown the shared scratch since)
    if (!arena_fits()) return kHostStage;
    ++ctx->arena->epoch;
    return carve_tables(ctx, m, p, need);
}

// the maps, the pieces and the offsets to the device; `a`: the kernels' view of the tables
int32_t upload_tables(npr_batch *b, const MeaPlan &p, MeaScratch &m, MeaArgs &a) {
    npr_ctx *ctx = b->ctx;
    const int64_t n = p.n, P = p.n_pieces, so = p.stride(), ss = sorted_stride(p);
    a.tasks = b->d_tasks.p, a.outs = b->d_outs.p, a.ntasks = static_cast<int32_t>(b->tasks.size()), a.n_reads = static_cast<int32_t>(n);
    a.px = b->d_px.p, a.py = b->d_py.p, a.pp = b->d_pp.p;
    a.rx_off = m.off.p, a.ry_off = m.off.p + so, a.rp_off = m.off.p + 2 * so, a.ot_off = m.off.p + 3 * so, a.cnt_off = m.off.p + 4 * so;
    a.cnt = m.cnt.p, a.start = m.start.p, a.colsum = m.col.p;
    a.sx = m.sorted.p, a.sy = m.sorted.p + ss, a.sq = m.sorted.p + 2 * ss, a.back = m.sorted.p + 3 * ss;
    a.kx = m.sorted.p + 4 * ss, a.ky = m.sorted.p + 5 * ss, a.kq = m.sorted.p + 6 * ss, a.kback = m.sorted.p + 7 * ss;
    a.vrec = reinterpret_cast<int4 *>(m.sorted.p + kSortedArrays * ss);
    a.sw = m.sorted.p + kSortedArrays * ss + kVrecWords * (p.total + 2);
    a.best_who = m.small.p, a.read_flag = m.small.p + n, a.n_ops = m.small.p + 2 * n, a.chain_len = m.small.p + 3 * n, a.kept = m.small.p + 4 * n, a.max_run = m.small.p + 5 * n;
    a.chain_mass = m.mass.p;
    int32_t *const read_first = m.map.p, *const read_ntasks = read_first + n, *const task_of = read_ntasks + n, *const order = task_of + p.ntask_map;
    a.read_first = read_first, a.read_ntasks = read_ntasks, a.task_of = task_of, a.order = order;
    int32_t *const lanes = m.pieces.p + 3 * n;
    a.np = m.pieces.p, a.poff = m.pieces.p + n, a.pboff = m.pieces.p + 2 * n, a.lane_read = lanes, a.lane_piece = lanes + P, a.pbest = lanes + 2 * P, a.pb = lanes + 3 * P;
    a.n_pieces = static_cast<int32_t>(P);
    a.ops_tmp = m.tmp.p, a.od_off = m.od.p;
    a.gap_gamma = b->params.gap_gamma, a.match_gamma = b->params.match_gamma;
    // the LDS-ring kernel takes the few reads the register window gives up on: as many read positions as the LDS
    // holds with one workgroup per CU; a read whose pairs reach back further than that is reported and the batch takes
    // the host stage
    a.ring = 8192;
    a.ring_only = ctx->opt[NPR_OPT_MEA_RING_ONLY] != 0 ? 1 : 0;
    a.sort_lds_bytes = static_cast<int32_t>(4 * p.span);
    a.sort_threads = ctx->overlap == 1 ? 512 : 0;  // (beside a DP pass: workgroups that fit the half it leaves -- 1024 threads: the job 388 ms instead of 353, 256: 361)
    a.any_global_sort = p.sort_in_lds ? 0 : 1;
    HIP_TRY(ctx, hipMemcpyAsync(read_first, b->read_first_task.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(read_ntasks, b->read_ntasks.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(task_of, b->task_of.data(), sizeof(int32_t) * p.ntask_map, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(order, p.order.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(m.pieces.p, p.pieces_head.data(), sizeof(int32_t) * p.pieces_head.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(m.off.p, p.offs.data(), m.off.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(m.small.p, 0, m.small.bytes(), ctx->stream));
    return NPR_OK;
}

// sort and chain; then the per-read words (m.small) and chain masses on the host
int32_t run_chain(npr_ctx *ctx, const MeaArgs &a, MeaScratch &m, std::vector<int32_t> &small, std::vector<int64_t> &mass) {
    int rc = launch_mea_sort(a, ctx->stream);
    if (rc == 0) rc = launch_mea_chain(a, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "MEA kernel launch", static_cast<hipError_t>(rc));
    small.resize(m.small.count), mass.resize(m.mass.count);
    HIP_TRY(ctx, hipMemcpyAsync(small.data(), m.small.p, m.small.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(mass.data(), m.mass.p, m.mass.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}

// Per read its status, number of ops and score; b->ops_off.  kHostStage when a read's chain reached back further than the prefix-maximum
// ring (nothing of the batch is touched then).  `longest`: the longest run of the batch's cigars.
int32_t collect_results(npr_batch *b, const std::vector<int32_t> &small, const std::vector<int64_t> &mass, int32_t &longest) {
    const int64_t n = b->n_reads;
    const int32_t *flag = small.data() + n, *nops = small.data() + 2 * n, *clen = small.data() + 3 * n, *max_run = small.data() + 5 * n;
    for (int64_t i = 0; i < n; ++i)
        if (b->results[i].status == NPR_OK && flag[i] == NPR_ERR_CAPACITY) return kHostStage;
    std::vector<int64_t> &od = b->ops_off;
    od.assign(n + 1, 0);
    longest = 0;
    for (int64_t i = 0; i < n; ++i) {
        npr_read_result &r = b->results[i];
        if (r.status == NPR_OK && flag[i] != 0) r.status = flag[i];
        const int64_t k = r.status == NPR_OK ? nops[i] : 0;
        od[i + 1] = od[i] + k;
        if (k) longest = std::max(longest, max_run[i]);
        r.n_ops = k;
        r.score = (r.status == NPR_OK && clen[i] > 0) ? static_cast<double>(mass[i]) / (static_cast<double>(clen[i]) * PROB_ONE) : 0.0;
    }
    b->ops_words = 2 * od[n];
    return NPR_OK;
}

// What the two endings share: the ops' offsets up and the gather of the reads' ops into m.dense, one packed word per op (length << 2 | op)
// -- and as their low halves into `dense16` when that is not null.
int32_t gather_ops(npr_batch *b, MeaScratch &m, MeaArgs &a, uint16_t *dense16) {
    npr_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipMemcpyAsync(m.od.p, b->ops_off.data(), m.od.bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (b->ops_off[b->n_reads] == 0) return NPR_OK;
    a.ops_dense = m.dense.p, a.ops_dense16 = dense16;
    const int rc = launch_mea_gather(a, ctx->stream);
    return rc == 0 ? NPR_OK : fail(ctx, NPR_ERR_HIP, "k_mea_gather launch", static_cast<hipError_t>(rc));
}
// ... and where they lie afterwards, for whoever asks while the stage's tables are not overwritten
void words_stay_on_device(npr_batch *b, const MeaScratch &m) { b->dev_ops = m.dense.p, b->dev_od = m.od.p, b->dev_ops_epoch = b->ctx->arena->epoch; }

// The default ending: the packed words to b->packed, through the pinned staging in pieces.  When no run of the batch is longer than 14 bits
// (a deletion of 16 k bases: the rule) the words cross as their low halves, 147 MB instead of 295 for the bench's 24576 reads, and the move
// widens them.
int32_t hand_over_words(npr_batch *b, MeaScratch &m, MeaArgs &a, int32_t longest) {
    npr_ctx *ctx = b->ctx;
    const int64_t words = b->ops_off[b->n_reads];
    b->have_pairs_form = false, b->have_packed_form = true;
    // kept when the batch is finished again; else one a destroyed batch left behind, if it is large enough
    if (words > b->packed_cap) ctx->take_packed(words, b->packed, b->packed_cap);
    if (words > b->packed_cap) {
        b->packed.reset(new uint32_t[words + words / 8]);  // (some room: the chunks of a job are about the same size, not exactly)
        b->packed_cap = words + words / 8;
    }
    if (words == 0) return NPR_OK;
    const bool narrow = longest < (1 << 14) && ctx->opt[NPR_OPT_MEA_WIDE_OPS] == 0 &&
                        sizeof(uint16_t) * static_cast<size_t>(words) <= m.sorted.bytes();  // (the sorted pairs are done with)
    int32_t rc = gather_ops(b, m, a, narrow ? reinterpret_cast<uint16_t *>(m.sorted.p) : nullptr);
    if (rc != NPR_OK) return rc;
    PiecedFetch f{m.dense.p, b->packed.get(), words, sizeof(uint32_t), int64_t(1) << 20, 64, nullptr, "npr_batch_finish: hipHostMalloc", "npr_batch_finish: D2H of the ops"};
    f.move = [](void *dst, const void *pin, int64_t lo, int64_t hi) {
        std::memcpy(static_cast<uint32_t *>(dst) + lo, static_cast<const uint32_t *>(pin) + lo, sizeof(uint32_t) * static_cast<size_t>(hi - lo));
    };
    if (narrow) {
        f.dev = a.ops_dense16, f.elem = sizeof(uint16_t);
        f.move = [](void *dst, const void *pin, int64_t lo, int64_t hi) {
            uint32_t *out = static_cast<uint32_t *>(dst);
            const uint16_t *src = static_cast<const uint16_t *>(pin);
            for (int64_t i = lo; i < hi; ++i) out[i] = src[i];
        };
    }
    if ((rc = fetch_pieced(ctx, f)) != NPR_OK) return rc;
    words_stay_on_device(b, m);
    return NPR_OK;
}

// NPR_OPT_FINISH_TEXT: the text kernels over the words the gather left in m.dense, and the TEXT and its offsets through the pinned staging
// instead of the words (npr_cigtext_api.cpp).  The words stay on the device for npr_batch_ops / npr_batch_ops_packed (fetch_device_words).
int32_t hand_over_text(npr_batch *b, MeaScratch &m, MeaArgs &a) {
    b->have_pairs_form = false, b->have_packed_form = false, b->words_on_device = true;
    int32_t rc = gather_ops(b, m, a, nullptr);
    // (the sorted pairs are done with: the text goes where the default ending puts the 16-bit words)
    if (rc == NPR_OK) rc = device_words_text(b, m.od.p, m.dense.p, reinterpret_cast<char *>(m.sorted.p), m.sorted.bytes());
    if (rc == NPR_OK) words_stay_on_device(b, m);
    return rc;
}

// MEA chain + cigar of every read on the device: only the ops cross PCIe.  kHostStage when some read needs the host stage instead
// (a chain reaching back further than the prefix-maximum ring) or the tables find no room, NPR_OK or an error.
int32_t device_mea(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    // (a context that runs next to others, NPR_OPT_OVERLAP, takes the arena's lock only when it has to use the arena: obtain_tables)
    std::unique_lock<std::mutex> arena_lock(ctx->arena->mu, std::defer_lock);
    if (!ctx->overlap) arena_lock.lock();
    ++ctx->arena->epoch;
    StageTimer tm("device_mea");
    const MeaPlan p = plan_mea(b);
    if (!ctx->mea) ctx->mea = new MeaScratch;
    MeaScratch &m = *ctx->mea;
    MeaArgs a{};
    std::vector<int32_t> small;
    std::vector<int64_t> mass;
    int32_t longest = 0;
    int32_t rc = obtain_tables(ctx, m, p, arena_lock);
    if (rc == NPR_OK) rc = upload_tables(b, p, m, a);
    if (rc == NPR_OK) rc = run_chain(ctx, a, m, small, mass);
    if (rc != NPR_OK) return rc;
    tm.lap("sort + chain + trace");
    if ((rc = collect_results(b, small, mass, longest)) != NPR_OK) return rc;
    rc = ctx->opt[NPR_OPT_FINISH_TEXT] != 0 ? hand_over_text(b, m, a) : hand_over_words(b, m, a, longest);
    if (rc == NPR_OK) tm.lap("gather + D2H of the ops");
    return rc;
}

// ---- npr_batch_finish ----

// per-read results from the task outputs; b->task_dst, b->pair_off
int32_t task_results(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    const int64_t ntasks = static_cast<int64_t>(b->tasks.size());
    const int64_t n = b->n_reads;
    std::vector<int64_t> &dst = b->task_dst;
    dst.assign(ntasks + 1, 0);
    if (ntasks) HIP_TRY(ctx, hipMemcpy(b->outs.data(), b->d_outs.p, b->d_outs.bytes(), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < ntasks; ++k) dst[k + 1] = dst[k] + std::min(b->outs[k].npairs, b->tasks[k].pair_cap);
    b->results.assign(n, npr_read_result{});
    b->pair_off.assign(n + 1, 0);
    b->pairs_ready = false;
    b->text_ready = false, b->words_on_device = false;
    const double LN2 = 0.69314718055994530942;
    for (int64_t i = 0; i < n; ++i) {
        npr_read_result &r = b->results[i];
        r.status = b->read_status[i];
        r.n_segments = b->read_ntasks[i];
        int64_t c = 0;
        if (r.status == NPR_OK)
            for (int32_t s = 0; s < b->read_ntasks[i]; ++s) {
                const int32_t k = b->task_of[b->read_first_task[i] + s];
                const TaskOut &o = b->outs[k];
                if (o.status != NPR_OK && r.status == NPR_OK) r.status = o.status;
                r.cells += b->task_cells[k];
                if (o.tot_m > 0.f) r.loglik += (std::log2(static_cast<double>(o.tot_m)) + o.tot_e) * LN2;
                if (o.btot_m > 0.f) r.loglik_bwd += (std::log2(static_cast<double>(o.btot_m)) + o.btot_e) * LN2;
                c += dst[k + 1] - dst[k];
            }
        r.n_pairs = c;
        b->pair_off[i + 1] = b->pair_off[i] + c;
    }
    return NPR_OK;
}

// the device MEA stage when an estimate of its tables fits the arena or half of the free device memory; kHostStage otherwise
int32_t gated_device_mea(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    int64_t scratch = 0;
    for (int64_t i = 0; i < b->n_reads; ++i) scratch += 8 * (b->ref_len[i] + 1) + 4 * b->read_len[i] + 36 * std::min(b->ref_len[i], b->read_len[i]) + 128;
    scratch += 48 * b->pair_off[b->n_reads];
    size_t mem_free = 0, mem_total = 0;
    const size_t arena_bytes = ctx->arena->cells.load() * 8;
    if (static_cast<size_t>(scratch) <= arena_bytes ||
        (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && static_cast<size_t>(scratch) < mem_free / 2))
        return device_mea(b);
    return kHostStage;
}

// --rescoreOriginalAlignment on the host: ops verbatim (alignmentUncertainty.py:51-52), new score -- `dev_score` when the device summed it.
// The guide's operations are not copied here (10^7-10^8 per batch): npr_batch_ops / npr_batch_ops_packed make the form they are asked for
// from b->guide_ops
void host_rescore(npr_batch *b, const std::vector<double> *dev_score) {
    const int64_t n = b->n_reads;
    b->ops_off.assign(n + 1, 0);
    parallel_for(n, b->ctx->host_threads, [&](int64_t i) {
        npr_read_result &r = b->results[i];
        if (r.status != NPR_OK) return;
        r.n_ops = b->rs_kept[i], b->ops_off[i + 1] = b->rs_kept[i];
        r.score = dev_score ? (*dev_score)[i]
                            : rescore(b->guide_ops.data() + 2 * b->guide_off[i], b->guide_off[i + 1] - b->guide_off[i], b->pairs.data() + b->pair_off[i], r.n_pairs);
    });
    for (int64_t i = 0; i < n; ++i) b->ops_off[i + 1] += b->ops_off[i];
    b->ops_words = 2 * b->ops_off[n];
    b->ops_from_guide = true, b->have_pairs_form = false, b->have_packed_form = false;
}

// chain + cigar of every read on the host, from the pairs fetch_pairs left in b->pairs
void host_mea(npr_batch *b, StageTimer &tm) {
    const int64_t n = b->n_reads;
    std::vector<std::vector<int32_t>> per_read_ops(n);
    parallel_for(n, b->ctx->host_threads, [&](int64_t i) {
        npr_read_result &r = b->results[i];
        if (r.status != NPR_OK) return;
        const int32_t rc = mea_cigar(b->ref_len[i], b->read_len[i], b->pairs.data() + b->pair_off[i], r.n_pairs, b->params.gap_gamma, b->params.match_gamma, per_read_ops[i], r.score);
        if (rc != NPR_OK) r.status = rc;
        r.n_ops = static_cast<int64_t>(per_read_ops[i].size() / 2);
    });
    tm.lap("MEA + cigar");
    b->ops_off.assign(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) b->ops_off[i + 1] = b->ops_off[i] + static_cast<int64_t>(per_read_ops[i].size() / 2);
    b->ops_words = 2 * b->ops_off[n];
    if (b->ops_words > b->ops_cap) {
        b->ops.reset(new int32_t[b->ops_words]);
        b->ops_cap = b->ops_words;
    }
    for (int64_t i = 0; i < n; ++i) std::copy(per_read_ops[i].begin(), per_read_ops[i].end(), b->ops.get() + 2 * b->ops_off[i]);
    b->have_pairs_form = true, b->have_packed_form = false;
    tm.lap("gather ops");
}

int32_t batch_finish_impl(npr_batch *b) {
    if (!b) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    if (!b->ran) return fail(ctx, NPR_ERR_STATE, "npr_batch_finish before npr_batch_run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    StageTimer tm("batch_finish");
    int32_t rc = task_results(b);
    if (rc != NPR_OK) return rc;
    tm.lap("task results");
    const bool on_device = b->n_reads > 0 && !b->tasks.empty() && ctx->opt[NPR_OPT_HOST_MEA] == 0;
    // --- rescore mode: the guide's M columns looked up where the pairs lie (round 5) ---
    std::vector<double> dev_score;
    bool have_dev_score = false;
    if (b->params.mode == NPR_MODE_RESCORE_ORIGINAL && on_device && b->rs_staged) {
        if ((rc = rescore_sum(b, dev_score)) < 0) return rc;
        have_dev_score = true;
        tm.lap("device rescore");
    }
    // --- realign and all-posteriors modes: chain and cigar on the device, the pairs stay in HBM until npr_batch_pairs asks for them ---
    if ((b->params.mode == NPR_MODE_REALIGN || b->params.mode == NPR_MODE_ALL_POSTERIORS) && on_device) {
        if ((rc = gated_device_mea(b)) < 0) return rc;
        if (rc == NPR_OK) {
            tm.lap("device MEA");
            b->finish_stage = 0;
            b->finished = true;
            return NPR_OK;
        }
    }
    // --- host stage: what the device stages could not take (per-position tables that would not fit: records chained across a whole contig;
    // a fixed-point sum that could not be exact), and NPR_OPT_HOST_MEA ---
    if (!have_dev_score && (rc = fetch_pairs(b)) != NPR_OK) return rc;
    if (b->params.mode == NPR_MODE_RESCORE_ORIGINAL) {
        host_rescore(b, have_dev_score ? &dev_score : nullptr);
        tm.lap("scores");
    } else {
        host_mea(b, tm);
    }
    b->finish_stage = have_dev_score ? 0 : 1;
    b->finished = true;
    return NPR_OK;
}

// ---- the two host forms of the cigars, each made from the other the first time it is asked for ----

void ops_from_guide(npr_batch *b) {  // rescore mode: the guide's operations of non-zero length, in the pairs form
    const int64_t total = b->ops_off[b->n_reads];
    if (2 * total > b->ops_cap) b->ops.reset(new int32_t[2 * total]), b->ops_cap = 2 * total;
    parallel_for(b->n_reads, b->ctx->host_threads, [&](int64_t i) {
        if (b->results[i].status != NPR_OK) return;
        const int32_t *g = b->guide_ops.data() + 2 * b->guide_off[i];
        const int64_t ng = b->guide_off[i + 1] - b->guide_off[i];
        int32_t *out = b->ops.get() + 2 * b->ops_off[i];
        for (int64_t q = 0; q < ng; ++q)
            if (g[2 * q + 1] > 0) *out++ = g[2 * q], *out++ = g[2 * q + 1];
    });
    b->have_pairs_form = true;
}
void ensure_pairs_form(npr_batch *b) {
    if (b->have_pairs_form) return;
    if (b->ops_from_guide) return ops_from_guide(b);
    const int64_t total = b->ops_off[b->n_reads];
    if (2 * total > b->ops_cap) b->ops.reset(new int32_t[2 * total]), b->ops_cap = 2 * total;
    const uint32_t *src = b->packed.get();
    int32_t *out = b->ops.get();
    const int64_t chunk = 1 << 19, nchunks = (total + chunk - 1) / chunk;
    parallel_for(nchunks, b->ctx->host_threads, [&](int64_t c) {
        for (int64_t i = c * chunk, hi = std::min(total, (c + 1) * chunk); i < hi; ++i)
            out[2 * i] = static_cast<int32_t>(src[i] & 3u), out[2 * i + 1] = static_cast<int32_t>(src[i] >> 2);
    });
    b->have_pairs_form = true;
}
void ensure_packed_form(npr_batch *b) {
    if (b->have_packed_form) return;
    if (b->ops_from_guide && !b->have_pairs_form) ops_from_guide(b);
    const int64_t total = b->ops_off[b->n_reads];
    if (total > b->packed_cap) b->packed.reset(new uint32_t[total]), b->packed_cap = total;
    const int32_t *src = b->ops.get();
    uint32_t *out = b->packed.get();
    const int64_t chunk = 1 << 19, nchunks = (total + chunk - 1) / chunk;
    parallel_for(nchunks, b->ctx->host_threads, [&](int64_t c) {
        for (int64_t i = c * chunk, hi = std::min(total, (c + 1) * chunk); i < hi; ++i)
            out[i] = static_cast<uint32_t>(src[2 * i + 1]) << 2 | static_cast<uint32_t>(src[2 * i]);
    });
    b->have_packed_form = true;
}

}  // namespace npr_impl

extern "C" {

int32_t npr_batch_finish(npr_batch *b) {
    try {
        return batch_finish_impl(b);
    } catch (const std::exception &) {
        return fail(b ? b->ctx : nullptr, NPR_ERR_NOMEM, "npr_batch_finish: out of host memory");
    }
}

void npr_batch_destroy(npr_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    b->ctx->give_packed(b->packed, b->packed_cap);
    delete b;
}

int32_t npr_batch_get_stats(const npr_batch *b, npr_batch_stats *st) {
    if (!b || !st) return NPR_ERR_INVALID;
    *st = b->stats;
    return NPR_OK;
}

int32_t npr_batch_results(const npr_batch *b, npr_read_result *out) {
    if (!b || (!out && b->n_reads)) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    std::copy(b->results.begin(), b->results.end(), out);
    return NPR_OK;
}

int32_t npr_batch_ops(const npr_batch *b, int64_t *ops_off, int32_t *ops, int64_t cap_pairs) {
    if (!b || !ops_off) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    std::copy(b->ops_off.begin(), b->ops_off.end(), ops_off);
    if (!ops) return NPR_OK;
    if (cap_pairs < b->ops_off[b->n_reads]) return NPR_ERR_CAPACITY;
    try {
        if (b->words_on_device && !b->have_packed_form && !b->have_pairs_form) {  // (finished with NPR_OPT_FINISH_TEXT)
            const int32_t rc = fetch_device_words(const_cast<npr_batch *>(b));
            if (rc != NPR_OK) return rc;
        }
        ensure_pairs_form(const_cast<npr_batch *>(b));
    } catch (const std::exception &) {
        return fail(b->ctx, NPR_ERR_NOMEM, "npr_batch_ops: out of host memory");
    }
    std::copy(b->ops.get(), b->ops.get() + b->ops_words, ops);
    return NPR_OK;
}

int32_t npr_batch_ops_packed(const npr_batch *b, int64_t *ops_off, uint32_t *words, int64_t cap_words) {
    if (!b || !ops_off) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    std::copy(b->ops_off.begin(), b->ops_off.end(), ops_off);
    if (!words) return NPR_OK;
    const int64_t total = b->ops_off[b->n_reads];
    if (cap_words < total) return NPR_ERR_CAPACITY;
    try {
        if (b->words_on_device && !b->have_packed_form) {  // (finished with NPR_OPT_FINISH_TEXT)
            const int32_t rc = fetch_device_words(const_cast<npr_batch *>(b));
            if (rc != NPR_OK) return rc;
        }
        ensure_packed_form(const_cast<npr_batch *>(b));
    } catch (const std::exception &) {
        return fail(b->ctx, NPR_ERR_NOMEM, "npr_batch_ops_packed: out of host memory");
    }
    // (150 MB for a chunk of 12 500 reads, into pages the caller has not touched yet: one thread took 30 ms of the job's tail)
    const uint32_t *src = b->packed.get();
    const int64_t chunk = 1 << 20, nchunks = (total + chunk - 1) / chunk;
    parallel_for(nchunks, b->ctx->host_threads, [&](int64_t c) {
        std::memcpy(words + c * chunk, src + c * chunk, sizeof(uint32_t) * static_cast<size_t>(std::min(total, (c + 1) * chunk) - c * chunk));
    });
    return NPR_OK;
}

int32_t npr_batch_pairs(const npr_batch *b, int64_t *pair_off, int32_t *x, int32_t *y, float *p, int64_t cap) {
    if (!b || !pair_off) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    std::copy(b->pair_off.begin(), b->pair_off.end(), pair_off);
    if (!x) return NPR_OK;
    if (!b->pairs_ready) {  // realign mode left them on the device
        int32_t rc;
        try {
            rc = fetch_pairs(const_cast<npr_batch *>(b));
        } catch (const std::exception &) {
            rc = fail(b->ctx, NPR_ERR_NOMEM, "npr_batch_pairs: out of host memory");
        }
        if (rc != NPR_OK) return rc;
    }
    const int64_t total = b->pair_off[b->n_reads];
    if (cap < total) return NPR_ERR_CAPACITY;
    for (int64_t r = 0; r < b->n_reads; ++r) {  // internal coordinates are relative to the guide's window
        const int32_t gx = static_cast<int32_t>(b->gstart[2 * r]), gy = static_cast<int32_t>(b->gstart[2 * r + 1]);
        for (int64_t i = b->pair_off[r]; i < b->pair_off[r + 1]; ++i) x[i] = b->pairs[i].x + gx, y[i] = b->pairs[i].y + gy, p[i] = b->pairs[i].p;
    }
    return NPR_OK;
}

int32_t npr_batch_debug_set_pairs(npr_batch *b, int64_t read, const int32_t *x, const int32_t *y, const float *p, int64_t n, int32_t task_status) {
    if (!b || read < 0 || read >= b->n_reads || n < 0 || (n > 0 && (!x || !y || !p))) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    if (!b->ran) return fail(ctx, NPR_ERR_STATE, "npr_batch_debug_set_pairs before npr_batch_run");
    if (b->read_ntasks[read] != 1) return fail(ctx, NPR_ERR_INVALID, "npr_batch_debug_set_pairs: the read has more than one segment");
    const int32_t k = b->task_of[b->read_first_task[read]];
    const Task &tk = b->tasks[k];
    if (n > tk.pair_cap) return NPR_ERR_CAPACITY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n) {
        HIP_TRY(ctx, hipMemcpy(b->d_px.p + tk.pair_off, x, sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(b->d_py.p + tk.pair_off, y, sizeof(int32_t) * n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(b->d_pp.p + tk.pair_off, p, sizeof(float) * n, hipMemcpyHostToDevice));
    }
    TaskOut o;
    HIP_TRY(ctx, hipMemcpy(&o, b->d_outs.p + k, sizeof(TaskOut), hipMemcpyDeviceToHost));
    o.npairs = static_cast<int32_t>(n), o.status = task_status;
    HIP_TRY(ctx, hipMemcpy(b->d_outs.p + k, &o, sizeof(TaskOut), hipMemcpyHostToDevice));
    b->finished = false;
    return NPR_OK;
}

int32_t npr_batch_debug_finish_stage(const npr_batch *b) {
    if (!b) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return b->finish_stage;
}

}  // extern "C"