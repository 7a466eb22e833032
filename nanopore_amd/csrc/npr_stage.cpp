// npr_stage.cpp -- npr_batch_create*: band planning, packing, H2D, the device planner, kernel classes and launch geometry of a batch (replaces the per-read fan-out of nanopore/analyses/utils.py:557-574)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace npr_impl {
// Row offsets of the generic kernel (rows padded to 4 cells), made on the device from the band rows the first time a
// generic launch needs them: batches whose tasks all go to the register kernels never pay for them.
int32_t ensure_coff(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    if (b->d_coff.p || b->d_lo.count == 0) return NPR_OK;
    const hipError_t e = b->d_coff.alloc_from(ctx, b->d_lo.count);
    if (e != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "generic row offsets: hipMalloc", e);
    CoffArgs ca{static_cast<int32_t>(b->d_pseg.count), b->d_pseg.p, b->d_n.p, b->d_coff.p};
    const int rc = launch_plan_coff(ca, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_plan_coff launch", static_cast<hipError_t>(rc));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NPR_OK;
}
}  // namespace npr_impl

// The steps of npr_batch_create*, in the order batch_create_at_impl (below) calls them.  Each takes the Stage, reads what earlier steps
// left there and in the batch, and says in its comment what it adds.  The ones that can fail return the code of their fail().
namespace {

constexpr int64_t kChunk = 32;  // reads per chunk of the host planner's worker threads
// (the first task's words start kCtlFrontPad rows into d_ctl: the backward sweep of k_dp_rs reads its control words up to
// three rows below the one it is on, row 0 included, without a clamp)
constexpr int64_t kCtlFrontPad = 4;

// the caller's arrays (include/nprealign.h: npr_batch_create_spans; read i = read[read_begin[i] : read_end[i]])
struct ReadsIn {
    int64_t n_reads, n_refs;
    const uint8_t *ref;
    const int64_t *ref_off;
    const int32_t *ref_index;
    const uint8_t *read;
    const int64_t *read_begin, *read_end;
    const int32_t *guide_ops;
    const int64_t *guide_off, *guide_start;
    const int32_t *model_slot;
    int64_t ref_of(int64_t i) const { return ref_index ? ref_index[i] : i; }
};

// a task's length: the anti-diagonals of its segment, one band row and one pair of control words each
inline int64_t rows_of(const PlanSeg &ps) { return static_cast<int64_t>(ps.lX) + ps.lY + 1; }

// What the steps hand to each other.  Tables indexed [k] are per task in READ order (k = read_first_task[read] + segment);
// the batch's own tables (b->tasks, b->task_cells) are in device order, rank[] maps one to the other.
struct Stage {
    npr_ctx *ctx = nullptr;
    npr_batch *b = nullptr;
    const ReadsIn *in = nullptr;
    // class_rules: the context's switches as the class rules read them
    bool force_generic = false, no_wide = false, use_tile = false, em = false, em_stripes_cs = false, scaled = false;
    // plan_reads
    std::vector<PointPlan> chunk_plan;  // (emptied by stage_windows)
    // flatten_plans
    std::vector<int64_t> chunk_seg0, chunk_pt0, win_off;
    int64_t ntasks = 0, npoints = 0, seq_bytes = 0, band_entries = 0;
    std::vector<SegPlan> seg;
    std::vector<PlanSeg> pseg;
    // stage_windows: the two parts of the context's pinned staging
    PlanPoint *h_points = nullptr;
    uint8_t *h_seq = nullptr;
    // plan_band_rows (the two device tables live until the batch is staged: the schedule and stripe passes read d_summary)
    DevBuf<PlanPoint> d_points;
    DevBuf<SegSummary> d_summary;
    std::vector<SegSummary> summary;
    // frame_candidates, frame_schedules
    std::vector<uint32_t> cand;
    std::vector<int64_t> sched_off, sched_cells;
    std::vector<int32_t> sched_cls;
    int64_t ctl_entries = kCtlFrontPad;
    // base_classes, promote_scaled, choose_mid
    std::vector<int8_t> cls_of;
    std::vector<int32_t> tile_list;
    std::vector<int64_t> tile_off_of, tile_offs;
    int64_t stripe_entries = 0;
    bool any_generic = false, any_pair = false;
    // stripe_tables
    std::vector<int64_t> tile_need, rowmask_off_of;
    // order_tasks
    std::vector<int64_t> pad_of;
    std::vector<int32_t> rank;
    // fill_tasks: totals of the batch and of each class
    int64_t pair_total = 0, max_pad = 0, max_width = 0, total_cells = 0;
    int64_t cls_count[kClasses] = {}, cls_width[kClasses] = {}, cls_cells[kClasses] = {};
    // scratch_budget
    int64_t fixed = 0, budget = 0;
    // lay_out_uniform, lay_out_own
    npr_batch::Launch *tileL = nullptr;
    int64_t tile_min = 0, uniform_grid = 0, uniform_cells = 0, var_total = 0, ring_floats = 0, slots = 0;
    std::vector<int64_t> region;  // first scratch cell of each workgroup of the launches with their own regions
};

// The batch's copy of the parameters and its per-read tables, sized; the guides where the mode needs them again.
void init_batch(npr_batch *b, const npr_params *params, const ReadsIn &in) {
    const int64_t n_reads = in.n_reads;
    b->params = *params;
    if (b->params.max_pairs_per_base <= 0) b->params.max_pairs_per_base = 6;
    b->n_reads = n_reads;
    b->ref_len.resize(n_reads);
    b->read_len.resize(n_reads);
    b->read_status.assign(n_reads, NPR_OK);
    b->gstart.assign(2 * n_reads, 0);
    b->ref_id.resize(n_reads);
    for (int64_t i = 0; i < n_reads; ++i) b->ref_id[i] = static_cast<int32_t>(in.ref_of(i));
    b->read_first_task.assign(n_reads, 0);
    b->read_ntasks.assign(n_reads, 0);
    b->guide_off.assign(in.guide_off, in.guide_off + (n_reads ? n_reads + 1 : 0));
    // the guides themselves are needed again only where the result IS the guide (--rescoreOriginalAlignment); copying
    // them for every realign batch cost 35 ms of a north-star batch's 80 (240 MB, one thread, first touch)
    if (n_reads && b->params.mode == NPR_MODE_RESCORE_ORIGINAL) b->guide_ops.assign(in.guide_ops, in.guide_ops + 2 * in.guide_off[n_reads]);
}

// 1. Host, O(cigar operations) per read: the guide's window, validation, matrix splits and the plan points of every
// segment (npr_host.cpp plan_points).  Worker threads take chunks of reads and append to their chunk's plan.
// -> chunk_plan; the batch's ref_len / read_len / gstart / read_ntasks / read_status
void plan_reads(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    const ReadsIn &in = *S.in;
    const int64_t n_reads = in.n_reads, nchunks = (n_reads + kChunk - 1) / kChunk;
    S.chunk_plan.resize(nchunks);
    parallel_for(nchunks, ctx->host_threads, [&](int64_t c) {
        PointPlan &pp = S.chunk_plan[c];
        for (int64_t i = c * kChunk, hi = std::min(n_reads, (c + 1) * kChunk); i < hi; ++i) {
            const int64_t k = in.ref_of(i);
            if (k < 0 || k >= in.n_refs) {
                b->ref_len[i] = b->read_len[i] = 0;
                b->read_status[i] = NPR_ERR_INVALID;
                continue;
            }
            int64_t lX = in.ref_off[k + 1] - in.ref_off[k], lY = in.read_end[i] - in.read_begin[i];
            int32_t rc = lY < 0 ? NPR_ERR_INVALID : NPR_OK;
            if (in.guide_start) {  // the window the guide covers
                const int64_t gx = in.guide_start[2 * i], gy = in.guide_start[2 * i + 1];
                int64_t sx = 0, sy = 0;
                for (int64_t q = in.guide_off[i]; q < in.guide_off[i + 1]; ++q) {
                    const int32_t op = in.guide_ops[2 * q], len = in.guide_ops[2 * q + 1];
                    if (len < 0) rc = NPR_ERR_INVALID;
                    if (op == NPR_OP_M || op == NPR_OP_D) sx += len;
                    if (op == NPR_OP_M || op == NPR_OP_I) sy += len;
                }
                if (gx < 0 || gy < 0 || gx + sx > lX || gy + sy > lY) rc = NPR_ERR_INVALID;
                b->gstart[2 * i] = gx, b->gstart[2 * i + 1] = gy;
                lX = sx, lY = sy;
            }
            b->ref_len[i] = lX;
            b->read_len[i] = lY;
            const int32_t slot = in.model_slot ? in.model_slot[i] : 0;
            if (slot < 0 || slot >= NPR_MAX_MODELS || !ctx->model_set[slot]) rc = NPR_ERR_MODEL;
            const size_t seg0 = pp.segs.size(), pt0 = pp.points.size();
            if (rc == NPR_OK) rc = plan_points(b->params, lX, lY, in.guide_ops + 2 * in.guide_off[i], in.guide_off[i + 1] - in.guide_off[i], pp);
            if (rc != NPR_OK) {
                pp.segs.resize(seg0), pp.points.resize(pt0);
                b->ref_len[i] = b->read_len[i] = 0;
            }
            for (size_t q = seg0; q < pp.segs.size(); ++q) pp.segs[q].owner = i;
            b->read_ntasks[i] = static_cast<int32_t>(pp.segs.size() - seg0);
            b->read_status[i] = rc;
        }
    });
}

// 2. flatten: segments in read order, their points and band rows at prefix offsets
// -> ntasks, npoints, seq_bytes, band_entries, chunk_seg0 / chunk_pt0, win_off, seg, pseg; the batch's read_first_task
int32_t flatten_plans(Stage &S) {
    npr_batch *b = S.b;
    const int64_t n_reads = S.in->n_reads, nchunks = static_cast<int64_t>(S.chunk_plan.size());
    S.chunk_seg0.assign(nchunks + 1, 0), S.chunk_pt0.assign(nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        S.chunk_seg0[c + 1] = S.chunk_seg0[c] + static_cast<int64_t>(S.chunk_plan[c].segs.size());
        S.chunk_pt0[c + 1] = S.chunk_pt0[c] + static_cast<int64_t>(S.chunk_plan[c].points.size());
    }
    S.ntasks = S.chunk_seg0[nchunks], S.npoints = S.chunk_pt0[nchunks];
    if (S.ntasks >= (int64_t(1) << 31)) return fail(S.ctx, NPR_ERR_INVALID, "npr_batch_create: too many tasks");
    int64_t first = 0;
    for (int64_t i = 0; i < n_reads; ++i) b->read_first_task[i] = static_cast<int32_t>(first), first += b->read_ntasks[i];
    // the read's windows as they stand in the caller's buffers (ASCII), reference part then read part, encoded on the device
    S.win_off.assign(n_reads + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) S.win_off[i + 1] = S.win_off[i] + (b->read_ntasks[i] ? b->ref_len[i] + b->read_len[i] : 0);
    S.seq_bytes = S.win_off[n_reads];
    S.seg.resize(S.ntasks);  // flat, read order
    S.pseg.resize(S.ntasks);
    for (int64_t c = 0; c < nchunks; ++c)
        for (size_t q = 0; q < S.chunk_plan[c].segs.size(); ++q) {
            const int64_t k = S.chunk_seg0[c] + static_cast<int64_t>(q);
            const SegPlan &s = S.seg[k] = S.chunk_plan[c].segs[q];
            PlanSeg &ps = S.pseg[k];
            ps.point_first = S.chunk_pt0[c] + s.point_first;
            ps.band_off = S.band_entries;
            ps.pieces = s.pieces;
            ps.lX = static_cast<int32_t>(s.xe - s.xs), ps.lY = static_cast<int32_t>(s.ye - s.ys), ps.pad = 0;
            S.band_entries += rows_of(ps);
        }
    return NPR_OK;
}

// ... and into pinned staging (kept by the context): plan points, then the sequence windows
// -> h_points, h_seq; chunk_plan is emptied
int32_t stage_windows(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    const ReadsIn &in = *S.in;
    const size_t stage_pts = (static_cast<size_t>(S.npoints) * sizeof(PlanPoint) + 255) & ~size_t(255);
    const int32_t grown = grow_pin_stage(ctx, stage_pts + static_cast<size_t>(S.seq_bytes) + 256, "npr_batch_create: hipHostMalloc");
    if (grown != NPR_OK) return grown;
    S.h_points = static_cast<PlanPoint *>(ctx->pin_stage);
    S.h_seq = static_cast<uint8_t *>(ctx->pin_stage) + stage_pts;
    parallel_for(static_cast<int64_t>(S.chunk_plan.size()), ctx->host_threads, [&](int64_t c) {
        const std::vector<PlanPoint> &pts = S.chunk_plan[c].points;
        if (!pts.empty()) std::memcpy(S.h_points + S.chunk_pt0[c], pts.data(), pts.size() * sizeof(PlanPoint));
        for (int64_t i = c * kChunk, hi = std::min(in.n_reads, (c + 1) * kChunk); i < hi; ++i) {
            if (!b->read_ntasks[i]) continue;
            std::memcpy(S.h_seq + S.win_off[i], in.ref + in.ref_off[in.ref_of(i)] + b->gstart[2 * i], static_cast<size_t>(b->ref_len[i]));
            std::memcpy(S.h_seq + S.win_off[i] + b->ref_len[i], in.read + in.read_begin[i] + b->gstart[2 * i + 1], static_cast<size_t>(b->read_len[i]));
        }
    });
    S.chunk_plan.clear();
    return NPR_OK;
}

// 3. device: band rows of every anti-diagonal, per-segment summaries; the sequences travel and are encoded on the side stream meanwhile.
// Reads whose band is too wide for any kernel are refused.
// -> the batch's d_pseg / d_lo / d_n / d_seq; d_points, d_summary, summary
int32_t plan_band_rows(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    const int64_t ntasks = S.ntasks;
    hipError_t e;
    if ((e = S.d_points.alloc_from(ctx, S.npoints)) != hipSuccess || (e = b->d_pseg.alloc_from(ctx, ntasks)) != hipSuccess || (e = S.d_summary.alloc_from(ctx, ntasks)) != hipSuccess ||
        (e = b->d_lo.alloc_from(ctx, S.band_entries + 16)) != hipSuccess || (e = b->d_n.alloc_from(ctx, S.band_entries + 16)) != hipSuccess ||  // (+16: the schedule's walkers read rows four at a time, up to eight past a segment's last)
        (e = b->d_seq.alloc_from(ctx, S.seq_bytes + 16)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    S.summary.resize(ntasks);
    if (ntasks) {
        HIP_TRY(ctx, hipMemcpyAsync(S.d_points.p, S.h_points, S.d_points.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(b->d_pseg.p, S.pseg.data(), b->d_pseg.bytes(), hipMemcpyHostToDevice, ctx->stream));
        PlanArgs pa{static_cast<int32_t>(ntasks), b->params.band_mode == NPR_BAND_FIXED ? 1 : 0,
                    b->params.band_mode == NPR_BAND_FIXED ? b->params.fixed_width / 2 : b->params.diagonal_expansion,
                    S.d_points.p, b->d_pseg.p, b->d_lo.p, b->d_n.p, S.d_summary.p};
        int rc = launch_plan_bands(pa, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_plan_bands launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipMemcpyAsync(S.summary.data(), S.d_summary.p, S.d_summary.bytes(), hipMemcpyDeviceToHost, ctx->stream));
        // the sequences travel and are encoded while the host looks at the summaries
        if (S.seq_bytes) {
            HIP_TRY(ctx, hipMemcpyAsync(b->d_seq.p, S.h_seq, static_cast<size_t>(S.seq_bytes), hipMemcpyHostToDevice, ctx->side[0]));
            if ((rc = launch_encode(b->d_seq.p, S.seq_bytes, ctx->side[0])) != 0) return fail(ctx, NPR_ERR_HIP, "k_encode launch", static_cast<hipError_t>(rc));
            HIP_TRY(ctx, hipEventRecord(ctx->side_done[0], ctx->side[0]));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int64_t k = 0; k < ntasks; ++k)
        if (S.summary[k].max_width > (1 << 22) || S.summary[k].cells >= (int64_t(1) << 40)) b->read_status[S.seg[k].owner] = NPR_ERR_BAND_TOO_WIDE;
    // (a read refused here keeps its tasks -- they are cheap to run and its status says the results do not count)
    return NPR_OK;
}

// 4. kernel classes.  The register kernels on a frame that follows the anti-diagonal take bands whose frame schedule
// exists, tried from the smallest frame up (on the device: the schedule is sequential per segment); bands too wide for
// one wavefront's frame go to the stripe kernel (k_dp_tile), whatever their shape.  A batch staged for the E-step
// (NPR_MODE_EXPECTATIONS) keeps the classes that have an E-step kernel.
// The switches the rules below read -> force_generic, no_wide, use_tile, em, em_stripes_cs, scaled
void class_rules(Stage &S) {
    const npr_ctx *ctx = S.ctx;
    S.force_generic = ctx->opt[NPR_OPT_KERNEL] == 1;  // no register kernel (A/B runs, tests)
    S.no_wide = ctx->opt[NPR_OPT_NO_WIDE] != 0;  // no multi-wavefront register kernel (A/B runs, tests)
    S.use_tile = !S.force_generic && ctx->opt[NPR_OPT_NO_TILE] == 0;  // (E-step batches too: k_em_tile)
    S.em = S.b->params.mode == NPR_MODE_EXPECTATIONS;
    // the row- and column-scaled arithmetic (npr_rs.h) needs loaded models that let a row's values be renormalised every NPR_RS_K anti-diagonals
    const bool rs_ok = model_shape(ctx).rs_ok;
    // E-step batches whose stripe tasks run in column-scaled arithmetic (k_dp_tile_cs's E-step instance, below): the four-slot frame class goes there
    // too -- k_em_stair<4> is one long dependent chain per task.  (Not the two-slot class: bands of 150 / 200 cells gain 19 / 9 % on the stripes, but
    // one wavefront walks a task's stripes one after the other, and the long thin tasks of that class -- 24 000 stripe rows where the frame has
    // 16 000 anti-diagonals -- become the launch's critical path: the bench's batch 51 -> 60 ms.)
    S.em_stripes_cs = S.em && S.use_tile && ctx->opt[NPR_OPT_ARITH] != 1 && ctx->opt[NPR_OPT_EM_TILE] != 1 && ctx->opt[NPR_OPT_TILE_RS] != 2 && rs_ok;
    // NPR_OPT_ARITH = 1: the per-cell-exponent kernels throughout (A/B)
    S.scaled = ctx->opt[NPR_OPT_ARITH] != 1 && !S.force_generic && rs_ok;
}

// The frame classes each task may try, by its widest anti-diagonal and its length, and where its control words go.
// -> cand, sched_off, ctl_entries
void frame_candidates(Stage &S) {
    S.cand.assign(S.ntasks, 0);
    S.sched_off.assign(S.ntasks, -1);
    for (int64_t k = 0; k < S.ntasks; ++k) {
        if (S.force_generic) break;
        for (int c = 0; c < kSchedClasses; ++c) {
            if (kClassTab[c].kind == K_WIDE && (S.use_tile || S.no_wide)) continue;
            if (S.em_stripes_cs && kClassTab[c].kind == K_STAIR && kClassTab[c].R == 4) continue;
            if (kClassTab[c].kind == K_STAIR && !stair_fits(rows_of(S.pseg[k]), kClassTab[c].slots())) continue;
            if (S.summary[k].max_width <= stair_max_width(kClassTab[c].R, kClassTab[c].NW)) S.cand[k] |= 1u << c;
        }
        if (S.cand[k]) S.sched_off[k] = S.ctl_entries, S.ctl_entries += rows_of(S.pseg[k]);
    }
}

// The device walks every candidate's frame schedule: the smallest frame that follows the band, its control words and its scratch cells.
// -> the batch's d_ctl; sched_cls (-1: no frame follows the band), sched_cells
int32_t frame_schedules(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    const int64_t ntasks = S.ntasks;
    hipError_t e;
    S.sched_cls.assign(ntasks, -1);
    S.sched_cells.assign(ntasks, 0);
    if ((e = b->d_ctl.alloc_from(ctx, 2 * S.ctl_entries + 16)) != hipSuccess)  // (+16: k_dp_rs reads its control words two rows ahead, k_dp_mid_rs up to six)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    if (S.ctl_entries == kCtlFrontPad) return NPR_OK;
    DevBuf<uint32_t> d_cand;
    DevBuf<int64_t> d_off, d_cells;
    DevBuf<int32_t> d_cls;
    if ((e = d_cand.alloc_from(ctx, ntasks)) != hipSuccess || (e = d_off.alloc_from(ctx, ntasks)) != hipSuccess || (e = d_cells.alloc_from(ctx, ntasks)) != hipSuccess ||
        (e = d_cls.alloc_from(ctx, ntasks)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_cand.p, S.cand.data(), d_cand.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_off.p, S.sched_off.data(), d_off.bytes(), hipMemcpyHostToDevice, ctx->stream));
    SchedArgs sa{static_cast<int32_t>(ntasks), b->d_pseg.p, S.d_summary.p, b->d_lo.p, b->d_n.p, d_off.p, d_cand.p, b->d_ctl.p, d_cls.p, d_cells.p};
    // the walk of a segment in chunks that compose (npr_plan.hip): chunk tables
    std::vector<int64_t> chunk_off(ntasks + 1, 0);
    uint32_t cand_union = 0;
    for (int64_t k = 0; k < ntasks; ++k) {
        chunk_off[k + 1] = chunk_off[k] + (S.cand[k] ? plan_sched_chunks_of(rows_of(S.pseg[k]) - 1) : 0);
        cand_union |= S.cand[k];
    }
    const int64_t n_chunks = chunk_off[ntasks];
    DevBuf<int64_t> d_chunk_off;
    DevBuf<uint8_t> d_chunks;
    DevBuf<int32_t> d_cur;
    if ((e = d_chunk_off.alloc_from(ctx, ntasks + 1)) != hipSuccess || (e = d_chunks.alloc_from(ctx, plan_sched_chunk_bytes(n_chunks))) != hipSuccess ||
        (e = d_cur.alloc_from(ctx, ntasks + kSchedClasses)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_chunk_off.p, chunk_off.data(), d_chunk_off.bytes(), hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_plan_sched(sa, d_chunk_off.p, n_chunks, d_chunks.p, d_cur.p, cand_union, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_plan_sched launch", static_cast<hipError_t>(rc));
    HIP_TRY(ctx, hipMemcpyAsync(S.sched_cls.data(), d_cls.p, d_cls.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(S.sched_cells.data(), d_cells.p, d_cells.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the tables above go out of scope
    return NPR_OK;
}

// Every task's base class: the frame class its schedule found, else the stripes, else (no stripe kernel) a generic class by width.
// -> cls_of, tile_list / tile_offs / tile_off_of / stripe_entries (the stripe tasks and where their tables go), any_generic
void base_classes(Stage &S) {
    const int lds_max_w = generic_max_wcap();
    S.cls_of.resize(S.ntasks);
    S.tile_off_of.assign(S.ntasks, -1);
    for (int64_t k = 0; k < S.ntasks; ++k) {
        int c = S.sched_cls[k];
        if (c < 0) {
            const int64_t w = S.summary[k].max_width;
            c = S.use_tile ? kTileClass : (w <= 512 ? kFirstGeneric : (w <= 1024 ? kFirstGeneric + 1 : (w <= lds_max_w ? kFirstGeneric + 2 : kFirstGeneric + 3)));
        }
        S.cls_of[k] = static_cast<int8_t>(c);
        // the stripe kernels address a stripe's rows (1 KiB each) with a 32-bit byte offset behind one descriptor: a stripe of
        // 2^21 rows or more would wrap.  No stripe has more rows than its task has anti-diagonals.
        if (kClassTab[c].kind == K_TILE && rows_of(S.pseg[k]) >= (int64_t(1) << 21)) S.b->read_status[S.seg[k].owner] = NPR_ERR_BAND_TOO_WIDE;
        if (kClassTab[c].kind == K_TILE) {
            S.tile_list.push_back(static_cast<int32_t>(k));
            S.tile_off_of[k] = S.stripe_entries;
            S.tile_offs.push_back(S.stripe_entries);
            S.stripe_entries += 1 + S.pseg[k].lX / (64 * kClassTab[c].R) + 1;
        }
        S.any_generic |= kClassTab[c].kind == K_GENERIC_LDS || kClassTab[c].kind == K_GENERIC_GLOBAL;
    }
}

// The one-wavefront frame tasks run in row-scaled arithmetic (npr_rs.h) -- every one of them, provided the loaded models let a row's
// values be renormalised every NPR_RS_K anti-diagonals (rs_model_ok); a task for which one exponent per row turns out not to be
// enough says so and npr_batch_run runs it again in class 0-2's kernel.  NPR_OPT_ARITH = 1: none (the per-cell-exponent kernels
// throughout, A/B).
// -> cls_of (classes 0-2 to kFirstRs + c, kTileClass to kTileRsClass); the batch's pair_rs
void promote_scaled(Stage &S) {
    const npr_ctx *ctx = S.ctx;
    // (the E-step has kernels in this arithmetic for the stripe tasks only: k_dp_tile_cs's E-step instance, NPR_OPT_EM_TILE)
    const bool rs = S.scaled && !S.em;
    S.b->pair_rs = rs;
    if (!S.scaled || (S.em && ctx->opt[NPR_OPT_EM_TILE] == 1)) return;
    for (int64_t k = 0; k < S.ntasks; ++k) {
        if (rs && S.cls_of[k] >= 0 && S.cls_of[k] < 3) S.cls_of[k] = static_cast<int8_t>(kFirstRs + S.cls_of[k]);
        // the stripe tasks run in column-scaled arithmetic (k_dp_tile_cs, round 6: one exponent per lane of a stripe; same bits, and a
        // per-lane range certificate that the reference's 3000-cell-wide rectangles pass -- DESIGN.md 5.1f); NPR_OPT_TILE_RS = 2: the
        // per-cell-exponent k_dp_tile throughout (A/B)
        else if (S.cls_of[k] == kTileClass && ctx->opt[NPR_OPT_TILE_RS] != 2) S.cls_of[k] = static_cast<int8_t>(kTileRsClass);
    }
}

// A read on ONE wavefront is a serial chain of 2 * (lX + lY) steps: a launch lasts at least as long as its longest task, and a class
// with fewer tasks than the chip has wavefront slots leaves the rest idle.  k_dp_mid_rs (classes 12-14, round 5) runs a task's two
// sweeps on two wavefronts that meet in the middle: half the chain for the bytes and instructions of k_dp_rs, so EVERY row-scaled
// task of MID_MIN_D anti-diagonals or more goes there (a 1/8 shard of configs[3]: DP launch 41.7 -> 28.5 ms, configs[1] 1.27 -> 0.75 ms,
// the headline batch 138.9 -> 131.6 ms with round 5's other changes); shorter ones stay with k_dp_rs.  (Rounds 3-4 had kernels with both
// sweeps whole and a third pass over the rows of both, k_dp_pair / k_dp_pair_rs, for classes that filled at most half of the chip.)
// NPR_OPT_PAIR 1: never; 2: only the tasks longer than a wavefront's fair share of their class, as far as second wavefronts are free;
// 0 / 3: every task.
// -> cls_of (kFirstRs + c to kFirstPair + c), any_pair
void choose_mid(Stage &S) {
    const npr_ctx *ctx = S.ctx;
    const std::vector<PlanSeg> &pseg = S.pseg;
    const int64_t pe = ctx->opt[NPR_OPT_PAIR];
    const bool pair_off = pe == 1, pair_long = pe == 2;
    if (!S.b->pair_rs || pair_off) return;
    for (int c = 0; c < 3; ++c) {
        std::vector<int32_t> mine;
        int64_t cost = 0;
        for (int64_t k = 0; k < S.ntasks; ++k)
            if (S.cls_of[k] == kFirstRs + c) mine.push_back(static_cast<int32_t>(k)), cost += rows_of(pseg[k]);
        if (mine.empty()) continue;
        const int64_t slots = static_cast<int64_t>(ctx->cu_count) * mid_waves_per_cu(kClassTab[c].R);
        const int64_t n = static_cast<int64_t>(mine.size()), fair = cost / slots;
        int64_t room = !pair_long ? n : (n < slots ? slots - n : n);  // second wavefronts to be had
        std::sort(mine.begin(), mine.end(), [&](int32_t x, int32_t y) { return pseg[x].lX + pseg[x].lY > pseg[y].lX + pseg[y].lY; });
        for (int32_t k : mine) {
            const int64_t len = rows_of(pseg[k]);
            if (room <= 0 || (pair_long && (len <= fair || len < 256))) break;
            if (len - 1 < MID_MIN_D) break;  // (sorted by length: the rest is shorter still; k_dp_mid_rs needs a block on either side of its cut)
            S.cls_of[k] = static_cast<int8_t>(kFirstPair + c), --room, S.any_pair = true;
        }
    }
}

// The stripe tasks' tables and the lane masks of their rows, made on the device.
// k_dp_tile tasks are ordered by the forward scratch they need (one row per anti-diagonal of a stripe: also what a
// task costs): a workgroup's region is sized by its FIRST task, every later one from the queue is smaller
// -> the batch's d_stripes / d_rowmask; tile_need, rowmask_off_of
int32_t stripe_tables(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    hipError_t e;
    S.tile_need.assign(S.ntasks, 0), S.rowmask_off_of.assign(S.ntasks, -1);
    if ((e = b->d_stripes.alloc_from(ctx, S.stripe_entries)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    if (S.tile_list.empty()) return NPR_OK;
    const std::vector<int32_t> &tile_list = S.tile_list;
    DevBuf<int32_t> d_list;
    DevBuf<int64_t> d_toff, d_rows;
    const size_t nt = tile_list.size();
    if ((e = d_list.alloc_from(ctx, nt)) != hipSuccess || (e = d_toff.alloc_from(ctx, nt)) != hipSuccess || (e = d_rows.alloc_from(ctx, nt)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_list.p, tile_list.data(), d_list.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_toff.p, S.tile_offs.data(), d_toff.bytes(), hipMemcpyHostToDevice, ctx->stream));
    StripeArgs ta{static_cast<int32_t>(nt), kClassTab[kTileClass].R, d_list.p, b->d_pseg.p, S.d_summary.p, b->d_lo.p, b->d_n.p, d_toff.p, b->d_stripes.p, d_rows.p};
    const int rc = launch_plan_stripes(ta, ctx->stream);
    if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_plan_stripes launch", static_cast<hipError_t>(rc));
    std::vector<int64_t> rows(nt);
    HIP_TRY(ctx, hipMemcpyAsync(rows.data(), d_rows.p, d_rows.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < nt; ++q) S.tile_need[tile_list[q]] = (tile_scratch_cells(rows[q], kClassTab[kTileClass].R) + 63) & ~int64_t(63);
    // the lane masks of all those rows, one word each
    std::vector<int64_t> moff(nt);
    int64_t mask_rows = 0;
    for (size_t q = 0; q < nt; ++q) moff[q] = mask_rows, S.rowmask_off_of[tile_list[q]] = mask_rows, mask_rows += rows[q];
    DevBuf<int64_t> d_moff;
    if ((e = d_moff.alloc_from(ctx, nt)) != hipSuccess || (e = b->d_rowmask.alloc_from(ctx, mask_rows)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    HIP_TRY(ctx, hipMemcpyAsync(d_moff.p, moff.data(), d_moff.bytes(), hipMemcpyHostToDevice, ctx->stream));
    RowMaskArgs ma{static_cast<int32_t>(nt), d_list.p, b->d_pseg.p, b->d_lo.p, b->d_n.p, d_toff.p, b->d_stripes.p, d_moff.p, b->d_rowmask.p};
    const int rc2 = launch_plan_rowmask(ma, ctx->stream);
    if (rc2 != 0) return fail(ctx, NPR_ERR_HIP, "k_plan_rowmask launch", static_cast<hipError_t>(rc2));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // d_list / d_toff / d_moff go out of scope
    return NPR_OK;
}

// 5. tasks, grouped by class, the costliest first
// (the frame kernels' tasks by the forward scratch they need, which is what they cost too: a workgroup's scratch region
// may then be sized by its FIRST task, as the stripe kernel's are -- everything the queue hands it later is smaller)
// -> pad_of, rank (device order -> read order); the batch's task_of (the other way)
void order_tasks(Stage &S) {
    const int64_t ntasks = S.ntasks;
    S.pad_of.resize(ntasks);
    for (int64_t k = 0; k < ntasks; ++k) S.pad_of[k] = std::max(S.summary[k].generic_cells, is_register_class(S.cls_of[k]) ? S.sched_cells[k] : 0);  // either kernel may run the task
    S.rank.resize(ntasks);
    std::iota(S.rank.begin(), S.rank.end(), 0);
    std::stable_sort(S.rank.begin(), S.rank.end(), [&](int32_t a, int32_t c) {
        if (S.cls_of[a] != S.cls_of[c]) return S.cls_of[a] < S.cls_of[c];
        if (S.tile_need[a] != S.tile_need[c]) return S.tile_need[a] > S.tile_need[c];
        if (is_register_class(S.cls_of[a]) && S.pad_of[a] != S.pad_of[c]) return S.pad_of[a] > S.pad_of[c];
        return S.summary[a].cells > S.summary[c].cells;
    });
    S.b->task_of.assign(ntasks, 0);
    for (int64_t k = 0; k < ntasks; ++k) S.b->task_of[S.rank[k]] = static_cast<int32_t>(k);
}

// The Task records in device order, and what the launches are sized by.
// -> the batch's tasks / task_cells; pair_total, max_pad, max_width, total_cells, cls_count / cls_width / cls_cells
int32_t fill_tasks(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    const int32_t *model_slot = S.in->model_slot;
    b->tasks.resize(S.ntasks);
    b->task_cells.resize(S.ntasks);
    for (int64_t k = 0; k < S.ntasks; ++k) {
        const int32_t g = S.rank[k];
        const SegPlan &s = S.seg[g];
        const int64_t i = s.owner;
        Task &t = b->tasks[k];
        t.x_off = S.win_off[i] + s.xs;
        t.y_off = S.win_off[i] + b->ref_len[i] + s.ys;
        t.band_off = S.pseg[g].band_off;
        t.lX = S.pseg[g].lX;
        t.lY = S.pseg[g].lY;
        t.D = t.lX + t.lY;
        t.flags = (s.ragged_start ? 1 : 0) | (s.ragged_end ? 2 : 0);
        t.model = model_slot ? model_slot[i] : 0;
        t.xs = static_cast<int32_t>(s.xs);
        t.ys = static_cast<int32_t>(s.ys);
        t.read = static_cast<int32_t>(i);
        const int64_t cells = S.summary[g].cells;
        const int64_t cap = std::min<int64_t>(cells, static_cast<int64_t>(b->params.max_pairs_per_base) * std::min(t.lX, t.lY) + 64);
        t.pair_cap = static_cast<int32_t>(std::min<int64_t>(cap, INT32_MAX));
        t.pair_off = S.pair_total;
        S.pair_total += t.pair_cap;
        b->task_cells[k] = cells;
        S.total_cells += cells;
        S.max_width = std::max<int64_t>(S.max_width, S.summary[g].max_width);
        const int c = S.cls_of[g];
        t.ctl_off = is_register_class(c) ? S.sched_off[g] : -1;
        t.tile_off = S.tile_off_of[g];
        t.rowmask_off = S.rowmask_off_of[g];
        const int64_t pad = S.pad_of[g];
        if (pad >= (int64_t(1) << 32)) return fail(ctx, NPR_ERR_INVALID, "npr_batch_create: segment too large");
        t.cells_pad = static_cast<int32_t>(std::min<int64_t>(pad, INT32_MAX));
        S.max_pad = std::max(S.max_pad, pad);
        ++S.cls_count[c];
        S.cls_width[c] = std::max<int64_t>(S.cls_width[c], S.summary[g].max_width);
        S.cls_cells[c] += cells;
    }
    // whatever the main stream does from here on comes after the sequences' copy and encoding on the side stream
    if (S.seq_bytes) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_done[0], 0));
    return NPR_OK;
}

// 6. launch geometry and the remaining device buffers
// What the forward scratch of all launches may take: nine tenths of what is free, cached or in the arena now, less the batch's other tables.
// -> the batch's slot_stride; fixed, budget
int32_t scratch_budget(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    b->slot_stride = (S.max_pad + 63) & ~int64_t(63);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    // (sequences, band rows, control words and stripe tables are allocated already)
    S.fixed = S.pair_total * 12 + S.ntasks * (int64_t)(sizeof(Task) + sizeof(TaskOut)) + (S.any_generic ? 0 : S.band_entries * 4);
    const size_t arena_now = ctx->arena->cells.load();
    S.budget = static_cast<int64_t>((free_b + ctx->cache_bytes + arena_now * 8) * 0.9) - S.fixed;
    if (b->slot_stride > 0 && S.budget / (b->slot_stride * 8) < 1)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: not enough device memory for one forward scratch region");
    return NPR_OK;
}

// One class's launch: workgroup size, LDS, the width its kernel is built for (wcap) and as many workgroups as stay resident, or as it has tasks.
npr_batch::Launch launch_shape(const npr_ctx *ctx, int c, int64_t count, int64_t width) {
    const KClass &kc = kClassTab[c];
    npr_batch::Launch L{};
    L.cls = c;
    L.count = static_cast<int>(count);
    L.width = width;
    int waves_per_cu;
    if (kc.kind == K_MID) {  // workgroups of two wavefronts
        waves_per_cu = mid_waves_per_cu(kc.R) / 2;
        // NPR_OPT_OVERLAP = 1: half of every SIMD's wavefront slots, and 224 of its 512 registers, left to the staging and MEA kernels of
        // the batches this one runs next to.  A persistent DP launch that fills the chip (7 x 72 registers) leaves room for nothing: every
        // other kernel of the job then waits for the launch's last wavefronts (profiles/r05_c3_job_trace.txt).  Measured on the files ->
        // file job of 50 000 reads, wavefronts per SIMD 7 / 6 / 5 / 4 / 3: 372 / 372 / 371 / 352-361 / 388 ms.
        if (ctx->overlap == 1 && kc.R <= 2) waves_per_cu = std::min(waves_per_cu, 8);
        L.wcap = 0;
        L.lds = stair_lds_bytes();
        L.threads = 128;
    } else if (is_one_wave_kind(kc.kind)) {  // VGPR-limited: 71 / 80 (held there by amdgpu_waves_per_eu) / 162 registers: 7 / 6 / 3 waves per SIMD
        waves_per_cu = kc.kind == K_RS ? rs_waves_per_cu(kc.R) : stair_waves_per_cu(kc.R);
        if (ctx->overlap == 1 && kc.R <= 2) waves_per_cu = std::min(waves_per_cu, 16);  // (four per SIMD, as for the two-wavefront classes above)
        L.wcap = 0;
        L.lds = stair_lds_bytes();
        L.threads = 64;
    } else if (kc.kind == K_WIDE) {  // workgroups per CU by VGPRs: 111 (R = 2) -> 4 waves per SIMD, 168-176 (R = 4) -> 2-3
        const int nw = kc.NW;
        // workgroups per CU: 111 VGPRs (R = 2) and 128 (4 x 8, held there by amdgpu_waves_per_eu) -> 4 waves per SIMD;
        // 4 x 12: 168 VGPRs, 3 waves per SIMD
        waves_per_cu = (kc.R == 2 || nw <= 8) ? 16 / nw : 1;
        L.wcap = 0;
        L.lds = wide_lds_bytes(nw);
        L.threads = 64 * nw;
    } else if (is_tile_kind(kc.kind)) {
        // 80 VGPRs: 6 wavefronts per SIMD, 24 per CU, shared by workgroups of NW wavefronts.  A read's band offers a
        // parallelism of about four stripes on average (rectangles of ~1000 columns, each stripe starting 128 + 16..31
        // anti-diagonals after its left neighbour): measured on 8192 x 8 kb reads in the reference's band, 2 / 3 / 4 / 6 / 8
        // wavefronts per task give 1.26 / 1.71 / 2.06 / 1.42 / 1.64e11 cells/s (more tasks in flight need more scratch)
        // (k_dp_tile_cs, round 6, same batch: 2 / 3 / 4 / 6 / 8 wavefronts per task 338 / 281 / 294 / 396 / 365 ms -- its steps are shorter, the
        // hand-overs are not, so a fourth wavefront waits more than it works)
        int nw = kc.kind == K_TILE_RS ? 3 : 4;
        if (ctx->opt[NPR_OPT_TILE_WAVES] > 0) nw = static_cast<int>(std::min<int64_t>(8, ctx->opt[NPR_OPT_TILE_WAVES]));
        waves_per_cu = std::max(1, 24 / nw);
        L.wcap = nw;
        L.lds = kc.kind == K_TILE_RS ? tile_cs_lds_bytes(nw) : tile_lds_bytes(nw);
        L.threads = 64 * nw;
    } else if (kc.kind == K_GENERIC_LDS) {
        // several wavefronts per task: these tasks are big, their forward scratch caps how many can be
        // resident, and one wavefront each would leave the SIMDs idle
        L.wcap = static_cast<int>((std::max<int64_t>(width, 64) + 3) & ~int64_t(3));
        L.lds = generic_lds_bytes(L.wcap);
        const int wg_per_cu = std::max<int>(1, static_cast<int>((160 * 1024) / (L.lds + 256)));
        L.threads = wg_per_cu >= 2 ? 256 : 512;                     // a lone workgroup on a CU gets 8 wavefronts
        waves_per_cu = std::min(wg_per_cu, 2048 / L.threads);        // workgroups per CU
    } else {
        L.wcap = static_cast<int>((width + 3) & ~int64_t(3));
        L.lds = generic_lds_bytes(0);
        L.threads = 512;
        waves_per_cu = 2;  // workgroups per CU
    }
    L.grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(count, static_cast<int64_t>(ctx->cu_count) * waves_per_cu)));
    return L;
}

// One launch per class present, in class order, which is the order of the tasks.  -> the batch's launches
void build_launches(Stage &S) {
    int64_t first = 0;
    for (int c = 0; c < kClasses; ++c) {
        if (!S.cls_count[c]) continue;
        npr_batch::Launch L = launch_shape(S.ctx, c, S.cls_count[c], S.cls_width[c]);
        L.first = static_cast<int>(first);
        L.cells = S.cls_cells[c];
        first += S.cls_count[c];
        if (std::getenv("NPR_TIMING"))
            std::fprintf(stderr, "[npr] class %d (kind %d R %d NW %d): %lld tasks, %lld cells, widest %lld, grid %d x %d threads\n", c,
                         kClassTab[c].kind, kClassTab[c].R, kClassTab[c].NW, (long long)S.cls_count[c], (long long)S.cls_cells[c],
                         (long long)S.cls_width[c], L.grid, L.threads);
        S.b->launches.push_back(L);
    }
}

// whether a launch's workgroups work in uniform regions of slot_stride cells (else: regions of their own, lay_out_own)
bool uniform_regions(const Stage &S, const npr_batch::Launch &L) {
    return &L != S.tileL && kClassTab[L.cls].kind != K_MID && !(S.b->variable_regions && is_one_wave_kind(kClassTab[L.cls].kind));
}

// The launches run concurrently, each on its own scratch regions: the regions of all of them must fit.  Uniform regions
// of slot_stride cells (the largest task of the batch) for the generic / multi-wavefront launches, and for the
// one-wavefront frame launches of a small batch; the stripe launch one region per workgroup, sized by the workgroup's
// first task (its tasks are sorted by need, so everything the queue hands out later is smaller) -- and so the
// one-wavefront frame launches of a big realign batch (round 3): 6144 uniform regions sized for the one 20 kb read of a
// config-3 chunk took 252 GB where the reads that actually start in them need 130, which is what lets a pipelined job keep
// three batches on the device.  (Not for batches staged for the E-step, whose kernels index the planes of a region by
// slot_stride; npr_batch_expectations refuses a batch laid out this way.)
// Which launches are uniform, their grids cut to what the budget holds, and their first regions.
// -> tileL, tile_min, uniform_grid, uniform_cells, ring_floats; the batch's variable_regions; grid and slot_base of the uniform launches
int32_t lay_out_uniform(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    for (auto &L : b->launches)
        if (is_tile_kind(kClassTab[L.cls].kind)) S.tileL = &L;
    S.tile_min = S.tileL ? S.tile_need[S.rank[S.tileL->first]] : 0;
    int64_t stair_grid = 0;
    for (auto &L : b->launches)
        if (is_one_wave_kind(kClassTab[L.cls].kind)) stair_grid += L.grid;
    const int64_t var_min_bytes = int64_t(32) << 30;  // uniform stair scratch above this goes variable
    b->variable_regions = !S.em && stair_grid > 0 && stair_grid * b->slot_stride * 8 >= var_min_bytes && !S.force_generic;
    if (S.any_pair) b->variable_regions = true;  // (their regions hold two sets of rows: not a layout the E-step kernels know)
    int64_t sum_grid = 0, others = 0;
    for (auto &L : b->launches)
        if (uniform_regions(S, L)) sum_grid += L.grid, ++others;
    if (S.tileL && S.tile_min * 8 > S.budget) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: not enough device memory for the forward scratch of the largest task");
    const int64_t fit = b->slot_stride > 0 ? (S.budget - S.tile_min * 8) / (b->slot_stride * 8) : INT32_MAX;
    if (sum_grid > fit) {
        if (fit < others) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: not enough device memory for one forward scratch region per kernel class");
        const double shrink = static_cast<double>(fit) / static_cast<double>(sum_grid);
        for (auto &L : b->launches)
            if (uniform_regions(S, L)) L.grid = std::max(1, static_cast<int>(L.grid * shrink));
    }
    sum_grid = 0;
    for (auto &L : b->launches) {
        if (!uniform_regions(S, L)) continue;
        L.slot_base = static_cast<int>(sum_grid);
        sum_grid += L.grid;
        if (kClassTab[L.cls].kind == K_GENERIC_GLOBAL) S.ring_floats = static_cast<int64_t>(L.grid) * 18 * L.wcap;
    }
    S.uniform_grid = sum_grid;
    // (at least one uniform region: npr_batch_dense runs any task there)
    S.uniform_cells = b->slot_stride * std::max<int64_t>(sum_grid, S.ntasks ? 1 : 0);
    return NPR_OK;
}

// One region per workgroup of L behind the uniform ones, each sized by the task the workgroup starts with (need[] in read order, rounded
// up to 64 cells); the grid is cut where the room ends.  -> region, var_total, the batch's region_end (stripe launch); L
int32_t own_regions(Stage &S, npr_batch::Launch &L, const std::vector<int64_t> &need_of) {
    L.region_first = static_cast<int>(S.region.size());
    const int64_t room = S.budget / 8 - S.uniform_cells - (S.tileL && &L != S.tileL ? S.tile_min : 0);
    int g = 0;
    for (; g < L.grid; ++g) {
        const int64_t need = (need_of[S.rank[L.first + g]] + 63) & ~int64_t(63);
        if (S.var_total + need > room) break;
        S.region.push_back(S.uniform_cells + S.var_total);
        S.var_total += need;
        if (&L == S.tileL) S.b->region_end.push_back(S.uniform_cells + S.var_total);
    }
    if (g == 0) return fail(S.ctx, NPR_ERR_NOMEM, "npr_batch_create: not enough device memory for the forward scratch of the largest task");
    L.grid = g;
    L.slot_base = 0;
    L.own_regions = true;
    return NPR_OK;
}

// The launches with regions of their own: the two-wavefront and (variable_regions) one-wavefront frame launches, then the stripe launch.
// -> region, slots; the batch's scratch_cells
int32_t lay_out_own(Stage &S) {
    npr_batch *b = S.b;
    int32_t rc;
    for (auto &L : b->launches) {
        const int kind = kClassTab[L.cls].kind;
        if (!(is_one_wave_kind(kind) && !uniform_regions(S, L)) && kind != K_MID) continue;
        // (k_dp_mid_rs's two sweeps share one set of rows: the forward one stores up to the cut, the backward one above it)
        if ((rc = own_regions(S, L, S.pad_of)) != NPR_OK) return rc;
    }
    if (S.tileL && (rc = own_regions(S, *S.tileL, S.tile_need)) != NPR_OK) return rc;  // (tile_need is rounded already)
    int64_t own_grid = 0;
    for (auto &L : b->launches) own_grid += L.own_regions ? L.grid : 0;
    S.slots = S.ntasks ? S.uniform_grid + own_grid : 0;
    b->scratch_cells = static_cast<size_t>(S.uniform_cells) + static_cast<size_t>(S.var_total);
    return NPR_OK;
}

// the batch's remaining device tables: tasks and their results, the queue, the generic ring, the regions, the posterior triples
int32_t allocate_batch(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    hipError_t e;
    if ((e = b->d_tasks.alloc_from(ctx, S.ntasks)) != hipSuccess || (e = b->d_outs.alloc_from(ctx, S.ntasks)) != hipSuccess ||
        (e = b->d_queue.alloc_from(ctx, kQueueSlots)) != hipSuccess || (e = b->d_ring.alloc_from(ctx, S.ring_floats)) != hipSuccess ||
        (e = b->d_region.alloc_from(ctx, S.region.size())) != hipSuccess ||
        (e = b->d_px.alloc_from(ctx, S.pair_total)) != hipSuccess ||
        (e = b->d_py.alloc_from(ctx, S.pair_total)) != hipSuccess || (e = b->d_pp.alloc_from(ctx, S.pair_total)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc", e);
    return NPR_OK;
}

// The arena only grows, so a batch that fits what is there now goes on without the mutex -- staging the next batch must
// not wait for the DP pass of the current one, which holds it.  Growing it (or poisoning it) waits for whatever another
// context's batch is running there.
int32_t grow_arena(npr_ctx *ctx, size_t cells) {
    if (cells <= ctx->arena->cells.load() && poison_byte() < 0) return NPR_OK;
    DeviceArena &ar = *ctx->arena;
    std::lock_guard<std::mutex> lock(ar.mu);
    if (cells > ar.cells) {
        if (ar.F) (void)hipFree(ar.F - DeviceArena::kPad);
        ar.F = nullptr, ar.cells = 0, ++ar.epoch;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&ar.F), cells * 8 + 2 * DeviceArena::kPad);
        if (e != hipSuccess && !ctx->cache.empty()) {  // the buffers kept from earlier batches are in the way
            (void)hipGetLastError();
            ctx->cache_flush();
            e = hipMalloc(reinterpret_cast<void **>(&ar.F), cells * 8 + 2 * DeviceArena::kPad);
        }
        if (e != hipSuccess) {
            ar.F = nullptr;
            return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: hipMalloc of the forward scratch", e);
        }
        ar.F += DeviceArena::kPad;
        ar.cells = cells;
    }
    if (poison_byte() >= 0) poison(ar.F, ar.cells * 8), ++ar.epoch;
    return NPR_OK;
}

// the tasks and the regions to the device
int32_t upload_batch(Stage &S) {
    npr_ctx *ctx = S.ctx;
    npr_batch *b = S.b;
    if (!S.ntasks) return NPR_OK;
    HIP_TRY(ctx, hipMemcpyAsync(b->d_tasks.p, b->tasks.data(), b->d_tasks.bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (!S.region.empty()) HIP_TRY(ctx, hipMemcpyAsync(b->d_region.p, S.region.data(), b->d_region.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the sequences are in place too: the stream waited for their copy)
    return NPR_OK;
}

void fill_stats(const Stage &S) {
    npr_batch *b = S.b;
    b->outs.resize(S.ntasks);
    b->stats.n_reads = b->n_reads;
    b->stats.n_tasks = S.ntasks;
    b->stats.cells = S.total_cells;
    b->stats.diagonals = S.band_entries;
    b->stats.max_width = S.max_width;
    b->stats.slots = S.slots;
    int64_t best = -1;  // report the class that carries most cells
    for (const auto &L : b->launches)
        if (L.cells > best) best = L.cells, b->stats.kernel_variant = is_tile_kind(kClassTab[L.cls].kind) ? 2 : (is_register_class(L.cls) ? 1 : 0);
    b->stats.device_bytes = S.fixed + static_cast<int64_t>(b->scratch_cells) * 8 + S.ring_floats * 4;
}

int32_t batch_create_at_impl(npr_ctx *ctx, const npr_params *params, const ReadsIn &in, npr_batch **out) {
    const int64_t n_reads = in.n_reads;
    if (!ctx || !params || !out || n_reads < 0 || in.n_refs < 0) return NPR_ERR_INVALID;
    if (!in.ref_index && in.n_refs != n_reads) return fail(ctx, NPR_ERR_INVALID, "npr_batch_create: without ref_index, n_refs must equal n_reads");
    if (n_reads > 0 && (!in.ref_off || !in.read_begin || !in.read_end || !in.guide_off)) return fail(ctx, NPR_ERR_INVALID, "npr_batch_create: null offsets");
    // the MEA stage's weights are 32-bit on the device (posterior quantum - gapGamma * gap mass, npr_mea.hip k_mea_weigh): gammas are weights between 0 and 1
    // (matchGamma down to -1: "keep every pair"); gapGamma = 250 would wrap them.  !(..): NaN is refused as well
    if (!(params->gap_gamma >= 0.0 && params->gap_gamma <= 1.0) || !(params->match_gamma >= -1.0 && params->match_gamma <= 1.0))
        return fail(ctx, NPR_ERR_INVALID, "npr_batch_create: gap_gamma must lie in [0, 1] and match_gamma in [-1, 1]");
    *out = nullptr;
    std::unique_ptr<npr_batch> b(new (std::nothrow) npr_batch);
    if (!b) return NPR_ERR_NOMEM;
    b->ctx = ctx;
    // Every error return below may leave copies and planner kernels queued on the context's streams that read or write
    // buffers of this batch (and the context's pinned staging): released buffers go to the context's cache, not to hipFree
    // (which would synchronise), so nothing may still be in flight when they do.  Declared after `b`: runs before its
    // destructor.
    struct DrainOnError {
        npr_ctx *c;
        bool armed = true;
        ~DrainOnError() {
            if (!armed) return;
            (void)hipStreamSynchronize(c->side[0]);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain{ctx};
    init_batch(b.get(), params, in);
    Stage S;
    S.ctx = ctx, S.b = b.get(), S.in = &in;

    StageTimer tm("batch_create");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    plan_reads(S);
    tm.lap("plan points");
    int32_t rc = flatten_plans(S);
    if (rc == NPR_OK) rc = stage_windows(S);
    if (rc != NPR_OK) return rc;
    tm.lap("flatten + stage");
    if ((rc = plan_band_rows(S)) != NPR_OK) return rc;
    tm.lap("device band rows");
    class_rules(S);
    frame_candidates(S);
    if ((rc = frame_schedules(S)) != NPR_OK) return rc;
    tm.lap("device frame schedules");
    base_classes(S);
    promote_scaled(S);
    choose_mid(S);
    rc = stripe_tables(S);
    if (rc == NPR_OK && S.any_generic) rc = ensure_coff(b.get());
    if (rc != NPR_OK) return rc;
    tm.lap("device stripe tables");
    order_tasks(S);
    if ((rc = fill_tasks(S)) != NPR_OK) return rc;
    tm.lap("tasks");
    if ((rc = scratch_budget(S)) != NPR_OK) return rc;
    build_launches(S);
    rc = lay_out_uniform(S);
    if (rc == NPR_OK) rc = lay_out_own(S);
    if (rc == NPR_OK) rc = allocate_batch(S);
    if (rc == NPR_OK) rc = grow_arena(ctx, b->scratch_cells);
    if (rc != NPR_OK) return rc;
    tm.lap("hipMalloc");
    if ((rc = upload_batch(S)) != NPR_OK) return rc;
    tm.lap("H2D");
    fill_stats(S);
    if (b->params.mode == NPR_MODE_RESCORE_ORIGINAL && (rc = rescore_stage(b.get())) != NPR_OK) return rc;
    drain.armed = false;
    *out = b.release();
    return NPR_OK;
}

// no exception crosses the C ABI: allocation failures of the host stages come back as NPR_ERR_NOMEM
int32_t batch_create_guarded(npr_ctx *ctx, const npr_params *params, const ReadsIn &in, npr_batch **out) {
    try {
        return batch_create_at_impl(ctx, params, in, out);
    } catch (const std::exception &) {
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_create: out of host memory");
    }
}

}  // namespace

extern "C" {

int32_t npr_batch_create_spans(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                               const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                               const uint8_t *read, const int64_t *read_begin, const int64_t *read_end,
                               const int32_t *guide_ops, const int64_t *guide_off, const int64_t *guide_start,
                               const int32_t *model_slot, npr_batch **out) {
    return batch_create_guarded(ctx, params, ReadsIn{n_reads, n_refs, ref, ref_off, ref_index, read, read_begin, read_end, guide_ops, guide_off, guide_start, model_slot}, out);
}

int32_t npr_batch_create_at(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                            const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                            const uint8_t *read, const int64_t *read_off, const int32_t *guide_ops,
                            const int64_t *guide_off, const int64_t *guide_start, const int32_t *model_slot,
                            npr_batch **out) {
    return npr_batch_create_spans(ctx, params, n_reads, n_refs, ref, ref_off, ref_index, read, read_off, read_off ? read_off + 1 : nullptr, guide_ops,
                                  guide_off, guide_start, model_slot, out);
}

int32_t npr_batch_create(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                         const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                         const uint8_t *read, const int64_t *read_off, const int32_t *guide_ops,
                         const int64_t *guide_off, const int32_t *model_slot, npr_batch **out) {
    return npr_batch_create_at(ctx, params, n_reads, n_refs, ref, ref_off, ref_index, read, read_off, guide_ops, guide_off,
                               nullptr, model_slot, out);
}


// the planner cross-check: what the device planner staged for every task against the host planner's plan of the same guide; the number of tasks that differ
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

}  // extern "C"
