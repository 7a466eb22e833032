// npr_run.cpp -- npr_batch_run: the DP launches of a staged batch and the second pass of the tasks without a range certificate; the Baum-Welch E-step; the dense dumps the tests read (cactus_realign's forward / backward pass, utils.py:587)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace npr_impl {
KernelArgs make_args(npr_batch *b) {
    KernelArgs a{};
    a.tasks = b->d_tasks.p;
    a.outs = b->d_outs.p;
    a.queue = b->d_queue.p;
    a.ntasks = static_cast<int32_t>(b->tasks.size());
    a.models = b->ctx->d_models;
    a.seq = b->d_seq.p;
    a.lo = b->d_lo.p;
    a.n = b->d_n.p;
    a.coff = b->d_coff.p;
    a.ctl = b->d_ctl.p;
    a.stripes = b->d_stripes.p;
    a.rowmask = b->d_rowmask.p;
    a.region = nullptr;  // set per launch (own_regions)
    a.F = b->ctx->arena->F;  // (the caller holds the arena's mutex)
    a.slot_stride = b->slot_stride;
    a.px = b->d_px.p;
    a.py = b->d_py.p;
    a.pp = b->d_pp.p;
    a.threshold = static_cast<float>(b->params.posterior_threshold);
    a.ring = b->d_ring.p;
    return a;
}
}  // namespace npr_impl

namespace {
// The arguments of one launch over the tasks [first, first + count) of the batch: its counter of the work queue, its ring capacity, its first
// uniform scratch region and (a class laid out in regions of its own, own_regions) its entries of the region table.
KernelArgs launch_args(npr_batch *b, int first, int count, int queue_slot, int wcap, int slot_base, const int64_t *region) {
    KernelArgs a = make_args(b);
    a.tasks += first, a.outs += first, a.ntasks = count;
    a.queue += queue_slot, a.wcap = wcap, a.slot_base = slot_base, a.region = region;
    return a;
}

// Streams and events of a pass of n launches that run side by side: all but the last on the context's side streams, each behind ev0; the last (every
// one of a serial pass) on the main stream, which then waits for the others, so that ev0 -> ev1 brackets the whole pass.  The caller records ev0.
struct FanOut {
    npr_ctx *ctx;
    size_t n;  // launches of the pass
    bool serial;
    bool on_main(size_t i) const { return serial || i + 1 == n; }
    hipStream_t stream(size_t i) const { return on_main(i) ? ctx->stream : ctx->side[i % npr_ctx::kSideStreams]; }
    int32_t before(size_t i) const {
        if (!on_main(i)) HIP_TRY(ctx, hipStreamWaitEvent(stream(i), ctx->ev0, 0));
        return NPR_OK;
    }
    int32_t after(size_t i) const {
        if (!on_main(i)) HIP_TRY(ctx, hipEventRecord(ctx->side_done[i % npr_ctx::kSideStreams], stream(i)));
        return NPR_OK;
    }
    int32_t join(float *kernel_ms) const {
        for (size_t i = 0; !serial && i + 1 < n; ++i) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_done[i % npr_ctx::kSideStreams], 0));
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
        return NPR_OK;
    }
};

// The second pass of a launch: the tasks its row- / column-scaled kernel reported as TASK_RERUN (npr_device.h), gathered for the per-cell-exponent kernel
// of their class, which runs them on the scratch regions (task j of `again` is no larger than the j-th task of the class) and queue counter of the first.
struct Rerun {
    std::vector<int32_t> again;  // their indices in b->tasks
    DevBuf<Task> d_tasks;        // ... the tasks themselves
    DevBuf<TaskOut> d_outs;      // ... and where their results go
    int32_t ntasks() const { return static_cast<int32_t>(again.size()); }
};

// collects them among [first, first + count) of b->outs; if there are any, uploads them (buffers from the context's cache if `cached`) and resets the launch's queue counter
int32_t stage_rerun(npr_batch *b, int first, int count, int queue_slot, bool cached, const char *nomem, Rerun *r) {
    npr_ctx *ctx = b->ctx;
    for (int k = first; k < first + count; ++k)
        if (b->outs[k].status == TASK_RERUN) r->again.push_back(k);
    if (r->again.empty()) return NPR_OK;
    const size_t n = r->again.size();
    std::vector<Task> sub(n);
    for (size_t j = 0; j < n; ++j) sub[j] = b->tasks[r->again[j]];
    const bool ok = cached ? r->d_tasks.alloc_from(ctx, n) == hipSuccess && r->d_outs.alloc_from(ctx, n) == hipSuccess
                           : r->d_tasks.alloc(n) == hipSuccess && r->d_outs.alloc(n) == hipSuccess;
    if (!ok) return fail(ctx, NPR_ERR_NOMEM, nomem);
    HIP_TRY(ctx, hipMemcpy(r->d_tasks.p, sub.data(), sizeof(Task) * n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemsetAsync(b->d_queue.p + queue_slot, 0, sizeof(int32_t), ctx->stream));
    return NPR_OK;
}

// ... and once the kernel has finished: their results take the place of the first pass's in b->outs
int32_t merge_rerun(npr_batch *b, const Rerun &r) {
    std::vector<TaskOut> subout(r.again.size());
    HIP_TRY(b->ctx, hipMemcpy(subout.data(), r.d_outs.p, sizeof(TaskOut) * subout.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < r.again.size(); ++j) b->outs[r.again[j]] = subout[j];
    return NPR_OK;
}
const int64_t *own_region(const npr_batch *b, const npr_batch::Launch &L) { return L.own_regions ? b->d_region.p + L.region_first : nullptr; }

// One E-step launch per kernel class of the batch (tasks are grouped by class): which kernel counts the class, and where.
enum class EmKind {
    generic,  // k_dp_generic<.., EM> (LDS ring while the band fits, global ring beyond): what has no E-step kernel of its own, and everything under NPR_OPT_EM_GENERIC
    stair,    // k_em_stair<R>: the one-wavefront frame classes
    wide,     // k_dp_wide<R, NW, EM>: R slots per lane on NW wavefronts per task
    tile,     // k_em_tile<R>: the stripe class, scratch regions per workgroup as in the DP launch
    tile_cs   // k_dp_tile_cs<.., EM>: ... in column-scaled arithmetic first; what its certificate refuses goes to k_em_tile
};
struct EmLaunch {
    const npr_batch::Launch *dp;  // the DP launch of the class: its tasks, its cells and (stripe class) its scratch regions in the batch's table
    EmKind kind;
    int R, NW;  // stair / wide / tile / tile_cs: slots per lane; wide: wavefronts per task
    int grid, wcap;  // wcap: ring capacity of the generic kernel
    size_t lds;      // ... and its LDS
    bool global_ring;
    bool uses_others_regions;  // a generic launch over a class without uniform regions: not beside the others
    int slot_base;    // first uniform forward-scratch region: the one its class had in the DP launch (the classes run concurrently)
    int dp_grid;      // ... and how many of them that launch owned
    size_t fx_off, ring_off;  // where its planes of the other four states / its HBM ring start (floats)
    bool stripes() const { return kind == EmKind::tile || kind == EmKind::tile_cs; }
};

// The kernel and launch geometry that count the class of one DP launch.  The launches run concurrently, like the DP launches of
// npr_batch_run (serialised, a batch in the trainer's band spent 63 ms where its longest class takes 38: profiles/r03_em_*): each
// class keeps the forward-scratch regions its DP launch owned (so at most that many workgroups) and gets its own planes and ring.
EmLaunch plan_em_launch(const npr_batch *b, const npr_batch::Launch &dl, const ModelShape &shape) {
    const npr_ctx *ctx = b->ctx;
    const KClass &kc = kClassTab[dl.cls];
    const bool own_kernels = ctx->opt[NPR_OPT_EM_GENERIC] == 0;
    int64_t per_cu;  // workgroups
    EmLaunch l{};
    l.dp = &dl, l.slot_base = dl.slot_base, l.dp_grid = dl.grid;
    if (is_one_wave_kind(kc.kind) && own_kernels) {
        // 127 / 161 / 223 VGPRs and 9 KiB of LDS bins per wavefront: 16 / 12 / 8 wavefronts per CU
        l.kind = EmKind::stair, l.R = kc.R;
        per_cu = l.R == 4 ? 8 : (l.R == 2 ? 12 : 16);
    } else if (is_tile_kind(kc.kind) && kc.R == 2 && own_kernels) {
        // 164 VGPRs: 3 wavefronts per SIMD, 12 per CU -> 3 workgroups of 4; the workgroups keep the scratch regions the DP
        // launch gave them (region i is sized for task i, and everything the queue hands out later is smaller)
        const bool cs = kc.kind == K_TILE_RS && ctx->opt[NPR_OPT_TILE_RS] != 2 && ctx->opt[NPR_OPT_EM_TILE] != 1;
        // (a model that is not rs_model_ok takes k_em_tile on the workgroups the column-scaled kernel would have had)
        l.kind = cs && shape.rs_ok ? EmKind::tile_cs : EmKind::tile, l.R = 2;
        per_cu = cs ? em_tile_cs_waves_per_cu() / em_tile_cs_waves() : em_tile_waves_per_cu() / em_tile_waves();
    } else if (kc.kind == K_WIDE && kc.R == 2 && own_kernels) {
        // 157 VGPRs: 3 wavefronts per SIMD, 12 per CU -> 3 / 1 tasks per CU on 4 / 8 wavefronts each
        l.kind = EmKind::wide, l.R = 2, l.NW = kc.NW;
        per_cu = 12 / l.NW;
    } else {
        l.kind = EmKind::generic;
        l.wcap = static_cast<int>((std::max<int64_t>(dl.width, 64) + 3) & ~int64_t(3));
        l.lds = generic_lds_bytes(l.wcap) + em_extra_lds_bytes();
        l.global_ring = l.lds > 160 * 1024;  // the bins take 12 KiB of the LDS the ring would otherwise have
        if (l.global_ring) l.lds = generic_lds_bytes(0) + em_extra_lds_bytes();
        per_cu = l.global_ring ? 8 : std::min<int>(12, static_cast<int>(std::max<size_t>(1, (160 * 1024) / (l.lds + 256))));
    }
    l.grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(dl.count, static_cast<int64_t>(ctx->cu_count) * per_cu)));
    if (l.kind == EmKind::generic && dl.own_regions) {
        // A class laid out in scratch regions of its own (the stripe class under NPR_OPT_EM_GENERIC) has no uniform regions: the generic kernel
        // counts it in regions 0, 1, .. of the arena, which belong to the other classes' launches -- so one launch after the other then, and no
        // more workgroups than the arena has room for.  (Until round 6 the launches ran side by side there: NaN counts on a batch of four classes.)
        l.uses_others_regions = true, l.slot_base = 0;
        const int64_t arena_cells = b->region_end.empty() ? b->slot_stride : b->region_end.back();
        l.grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(l.grid, arena_cells / std::max<int64_t>(b->slot_stride, 1))));
        l.dp_grid = l.grid;
    }
    l.grid = std::max(1, std::min(l.grid, l.dp_grid));  // (uniform regions or the stripe class's own: those of the DP launch's workgroups)
    return l;
}

// The planes of the other four states: 16 bytes per cell of forward scratch in use.  The stripe kernel's mirror its regions
// of the forward scratch, but only those of the workgroups the E-step launches (far fewer than the DP launch had): when
// the device has no room for them, fewer workgroups yet.  Sets fx_off / ring_off (and may halve grid) of every launch and grows ctx->arena_Fx.
int32_t lay_out_planes(npr_batch *b, std::vector<EmLaunch> &launches, size_t *ring_floats) {
    npr_ctx *ctx = b->ctx;
    for (;;) {
        // uniform classes: planes packed one class after the other; the stripe class: a mirror of its scratch regions, which
        // lie behind all uniform regions of the arena (so behind the packed planes too)
        size_t fx_cells = 0;
        *ring_floats = 0;
        for (auto &l : launches) {
            if (l.stripes()) continue;
            l.fx_off = fx_cells;
            fx_cells += static_cast<size_t>(l.grid) * 4 * static_cast<size_t>(b->slot_stride);
            l.ring_off = *ring_floats;
            if (l.global_ring) *ring_floats += static_cast<size_t>(l.grid) * 18 * l.wcap;
        }
        for (auto &l : launches)
            if (l.stripes() && !b->region_end.empty()) {
                l.fx_off = 0;
                fx_cells = std::max(fx_cells, 4 * static_cast<size_t>(b->region_end[std::min<size_t>(static_cast<size_t>(l.grid), b->region_end.size()) - 1]));
            }
        if (fx_cells <= ctx->arena_fx_cells) return NPR_OK;
        if (ctx->arena_Fx) (void)hipFree(reinterpret_cast<char *>(ctx->arena_Fx) - npr_ctx::kArenaPad);
        ctx->arena_Fx = nullptr, ctx->arena_fx_cells = 0;
        char *raw = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&raw), fx_cells * sizeof(float) + 2 * npr_ctx::kArenaPad);
        if (e != hipSuccess && !ctx->cache.empty()) {  // the buffers kept from closed batches are in the way
            (void)hipGetLastError();
            ctx->cache_flush();
            e = hipMalloc(reinterpret_cast<void **>(&raw), fx_cells * sizeof(float) + 2 * npr_ctx::kArenaPad);
        }
        if (e == hipSuccess) {
            ctx->arena_Fx = reinterpret_cast<float *>(raw + npr_ctx::kArenaPad), ctx->arena_fx_cells = fx_cells;
            return NPR_OK;
        }
        (void)hipGetLastError();
        bool shrunk = false;
        for (auto &l : launches)
            if (l.grid > 1) l.grid = (l.grid + 1) / 2, shrunk = true;
        if (!shrunk) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_expectations: hipMalloc of the forward planes", e);
    }
}

// the arguments of an E-step launch (either pass): its tasks, its planes (indexed from a.Fx by workgroup; by scratch region in the stripe kernel), the sums it adds to
KernelArgs em_args(npr_batch *b, const EmLaunch &l, int queue_slot, double *em_T, double *em_E) {
    KernelArgs a = launch_args(b, l.dp->first, l.dp->count, queue_slot, l.wcap, l.slot_base, own_region(b, *l.dp));
    a.Fx = b->ctx->arena_Fx + l.fx_off;
    a.em_T = em_T, a.em_E = em_E;
    return a;
}

// the kernels' compact emission bins (EM_BINS per model, npr_device.h) as the 80-entry table of a model: a gap state's count per base goes evenly to its 4 entries
void unpack_bins(const double *bins, double *E_exp) {
    for (int m = 0; m < NPR_MAX_MODELS; ++m) {
        const double *s = bins + m * EM_BINS;
        double *d = E_exp + m * 80;
        for (int i = 0; i < 16; ++i) d[i] = s[i];
        for (int x = 0; x < 4; ++x)
            for (int y = 0; y < 4; ++y) {
                d[16 + x * 4 + y] = 0.25 * s[16 + x];  // shortGapX: count of reference base x
                d[48 + x * 4 + y] = 0.25 * s[20 + x];  // longGapX
                d[32 + x * 4 + y] = 0.25 * s[24 + y];  // shortGapY: count of read base y
                d[64 + x * 4 + y] = 0.25 * s[28 + y];  // longGapY
            }
    }
}
}  // namespace

extern "C" {

int32_t npr_batch_run(npr_batch *b, float *kernel_ms) {
    if (!b) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (kernel_ms) *kernel_ms = 0.f;
    std::vector<uint8_t> refuse;  // (npr_batch_debug_refuse: this run's, and gone after it however it ends)
    refuse.swap(b->debug_refuse);
    if (b->tasks.empty()) {
        b->ran = true;
        return NPR_OK;
    }
    std::lock_guard<std::mutex> arena_lock(ctx->arena->mu);  // until the DP pass has finished
    ++ctx->arena->epoch;
    HIP_TRY(ctx, hipMemsetAsync(b->d_queue.p, 0, sizeof(int32_t) * kQueueSlots, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    // all classes at once, the smallest first, each on its own stream (FanOut)
    std::vector<const npr_batch::Launch *> order;
    for (const auto &L : b->launches) order.push_back(&L);
    std::sort(order.begin(), order.end(), [](const npr_batch::Launch *x, const npr_batch::Launch *y) { return x->cells < y->cells; });
    bool scaled = b->pair_rs;  // (staged for the row- / column-scaled kernels under the models of that moment)
    for (const auto &L : b->launches) scaled |= kClassTab[L.cls].kind == K_TILE_RS;
    const ModelShape shape = model_shape(ctx);
    if (scaled && !shape.rs_ok)
        return fail(ctx, NPR_ERR_MODEL, "npr_batch_run: a model loaded after the batch was staged grows faster than the row-scaled kernels allow: stage the batch again");
    const FanOut fan{ctx, order.size(), false};
    int32_t rc;
    for (size_t i = 0; i < order.size(); ++i) {
        const npr_batch::Launch &L = *order[i];
        hipStream_t s = fan.stream(i);
        if ((rc = fan.before(i)) != NPR_OK) return rc;
        const KernelArgs a = launch_args(b, L.first, L.count, L.cls, L.wcap, L.slot_base, own_region(b, L));
        const KClass &kc = kClassTab[L.cls];
        const int lrc = kc.kind == K_MID   ? launch_mid_rs(a, kc.R, L.grid, s, shape.sw, shape.flat)
                        : kc.kind == K_RS    ? launch_rs(a, kc.R, L.grid, s, shape.sw, shape.flat)
                        : kc.kind == K_STAIR ? launch_stair(a, kc.R, L.grid, s)
                        : kc.kind == K_TILE ? launch_tile(a, kc.R, L.wcap, L.grid, s, shape.flat_gaps)
                        : kc.kind == K_TILE_RS ? launch_tile_cs(a, L.wcap, L.grid, s, shape.sw, shape.flat)
                        : kc.kind == K_WIDE ? launch_wide(a, kc.R, kc.NW, L.grid, s)
                                            : launch_generic(a, L.grid, L.threads, L.lds, false, kc.kind == K_GENERIC_GLOBAL, s);
        if (lrc != 0) return fail(ctx, NPR_ERR_HIP, "DP kernel launch", static_cast<hipError_t>(lrc));
        if ((rc = fan.after(i)) != NPR_OK) return rc;
    }
    if ((rc = fan.join(kernel_ms)) != NPR_OK) return rc;
    // The row-scaled kernels report the tasks for which one exponent per row may not have been enough (TASK_RERUN,
    // npr_device.h): those run again here, with the per-cell-exponent kernel of their frame class, on the scratch regions the
    // first launch had.  Rare -- a row of the alignment ~110 binary orders below the product of the row's largest forward and
    // backward values: an indel of 70+ bases --, so one more small launch per class at most.
    b->outs.resize(b->tasks.size());
    b->task_rerun.assign(b->tasks.size(), 0);
    for (const auto &L : b->launches) {
        const KClass &kc = kClassTab[L.cls];
        if (kc.kind != K_RS && kc.kind != K_TILE_RS && kc.kind != K_MID) continue;
        HIP_TRY(ctx, hipMemcpy(b->outs.data() + L.first, b->d_outs.p + L.first, sizeof(TaskOut) * L.count, hipMemcpyDeviceToHost));
        for (int k = L.first; !refuse.empty() && k < L.first + L.count; ++k)  // (test hook: as if the kernel had refused them, on both sides)
            if (refuse[k] && b->outs[k].status != TASK_RERUN) {
                b->outs[k].status = TASK_RERUN;
                HIP_TRY(ctx, hipMemcpy(b->d_outs.p + k, &b->outs[k], sizeof(TaskOut), hipMemcpyHostToDevice));
            }
        Rerun r;
        if ((rc = stage_rerun(b, L.first, L.count, L.cls, false, "npr_batch_run: hipMalloc", &r)) != NPR_OK) return rc;
        if (r.again.empty()) continue;
        // (what the second launch's addressing rests on, checked where a test chose the tasks: workgroup j starts in the region of the class's j-th task)
        for (size_t j = 0; !refuse.empty() && j < r.again.size(); ++j)
            if (r.again[j] < L.first + static_cast<int32_t>(j)) return fail(ctx, NPR_ERR_STATE, "npr_batch_run: a task of the second pass is larger than the task its scratch region was sized for");
        if (std::getenv("NPR_TIMING"))
            for (const int32_t k : r.again)
                std::fprintf(stderr, "[npr] task %d (D %d) runs again; the first pass left in its result: npairs (k_dp_mid_rs: why, 1 nothing at the cut / 2 no total / 3 exponents apart / 4 totals apart / 5 range certificate; k_dp_tile_cs: its certificate value) %d, btot_m (k_dp_mid_rs: total' / total) %.9g, btot_e (k_dp_mid_rs: exponent difference) %d, total %g x 2^%d\n", k, b->tasks[k].D, b->outs[k].npairs, b->outs[k].btot_m, b->outs[k].btot_e, b->outs[k].tot_m, b->outs[k].tot_e);
        KernelArgs a = launch_args(b, L.first, L.count, L.cls, L.wcap, L.slot_base, own_region(b, L));
        a.tasks = r.d_tasks.p, a.outs = r.d_outs.p, a.ntasks = r.ntasks();
        const int grid = std::min(r.ntasks(), L.grid);
        const int lrc = kc.kind == K_TILE_RS ? launch_tile(a, 2, L.wcap, grid, ctx->stream) : launch_stair(a, kc.R, grid, ctx->stream);
        if (lrc != 0) return fail(ctx, NPR_ERR_HIP, "DP kernel launch (second pass)", static_cast<hipError_t>(lrc));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = merge_rerun(b, r)) != NPR_OK) return rc;
        for (const int32_t k : r.again) {  // (the finish reads the results on the device)
            b->task_rerun[k] = 1;
            HIP_TRY(ctx, hipMemcpy(b->d_outs.p + k, &b->outs[k], sizeof(TaskOut), hipMemcpyHostToDevice));
        }
        if (std::getenv("NPR_TIMING")) std::fprintf(stderr, "[npr] class %d: %zu of %d tasks run again with a per-cell exponent\n", L.cls, r.again.size(), L.count);
    }
    b->ran = true;
    b->finished = false;
    return NPR_OK;
}

int32_t npr_batch_debug_refuse(npr_batch *b, const uint8_t *mark, int64_t n_segments) {
    if (!b || !mark) return NPR_ERR_INVALID;
    int64_t n = 0;
    for (int64_t r = 0; r < b->n_reads; ++r) n += b->read_ntasks[r];
    if (n_segments != n) return fail(b->ctx, NPR_ERR_INVALID, "npr_batch_debug_refuse: one mark per segment, in npr_batch_segment_arith's order");
    b->debug_refuse.assign(b->tasks.size(), 0);
    n = 0;
    for (int64_t r = 0; r < b->n_reads; ++r)
        for (int32_t s = 0; s < b->read_ntasks[r]; ++s, ++n) b->debug_refuse[b->task_of[b->read_first_task[r] + s]] = mark[n] != 0;
    return NPR_OK;
}

int32_t npr_batch_class_stats(const npr_batch *b, int64_t *tasks, int64_t *cells, int32_t cap) {
    if (!b) return NPR_ERR_INVALID;
    for (int c = 0; c < kClasses && c < cap; ++c) {
        if (tasks) tasks[c] = 0;
        if (cells) cells[c] = 0;
    }
    for (const auto &L : b->launches)
        if (L.cls < cap) {
            if (tasks) tasks[L.cls] = L.count;
            if (cells) cells[L.cls] = L.cells;
        }
    return kClasses;
}

int32_t npr_batch_segment_arith(const npr_batch *b, int64_t *seg_off, int32_t *arith, int64_t cap) {
    if (!b || !seg_off) return NPR_ERR_INVALID;
    std::vector<int8_t> of_task(b->tasks.size(), 0);
    for (const auto &L : b->launches)
        if (kClassTab[L.cls].kind == K_RS || kClassTab[L.cls].kind == K_MID)
            for (int k = L.first; k < L.first + L.count; ++k) of_task[k] = (static_cast<size_t>(k) < b->task_rerun.size() && b->task_rerun[k]) ? 0 : 1;
    int64_t n = 0;
    for (int64_t r = 0; r < b->n_reads; ++r) {
        seg_off[r] = n;
        for (int32_t s2 = 0; s2 < b->read_ntasks[r]; ++s2, ++n)
            if (arith && n < cap) arith[n] = of_task[b->task_of[b->read_first_task[r] + s2]];
    }
    seg_off[b->n_reads] = n;
    return NPR_OK;
}

int32_t npr_batch_expectations(npr_batch *b, double *T_exp, double *E_exp, double *loglik, float *kernel_ms) {
    if (!b || !T_exp || !E_exp || !loglik) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> arena_lock(ctx->arena->mu);  // the E-step keeps its forward rows in the arena
    ++ctx->arena->epoch;
    std::fill(T_exp, T_exp + NPR_MAX_MODELS * 25, 0.0);
    std::fill(E_exp, E_exp + NPR_MAX_MODELS * 80, 0.0);
    std::fill(loglik, loglik + NPR_MAX_MODELS, 0.0);
    if (kernel_ms) *kernel_ms = 0.f;
    const int64_t ntasks = static_cast<int64_t>(b->tasks.size());
    if (!ntasks) return NPR_OK;
    if (b->variable_regions)
        return fail(ctx, NPR_ERR_STATE, "npr_batch_expectations: this batch was laid out for realignment only (scratch regions of their own size); "
                                        "stage it with NPR_MODE_EXPECTATIONS");
    int32_t rc = ensure_coff(b);  // classes without a register E-step take the generic kernel
    if (rc != NPR_OK) return rc;
    const ModelShape shape = model_shape(ctx);
    std::vector<EmLaunch> launches;
    for (const auto &dl : b->launches) launches.push_back(plan_em_launch(b, dl, shape));
    size_t ring_floats = 0;
    if ((rc = lay_out_planes(b, launches, &ring_floats)) != NPR_OK) return rc;
    DevBuf<float> ring;
    DevBuf<double> d_T, d_E;
    hipError_t e;
    // (from the context's cache of released buffers: the trainer calls this hundreds of times on one staged batch -- no hipMalloc / hipFree per call)
    if ((e = ring.alloc_from(ctx, ring_floats)) != hipSuccess || (e = d_T.alloc_from(ctx, NPR_MAX_MODELS * 25)) != hipSuccess ||
        (e = d_E.alloc_from(ctx, NPR_MAX_MODELS * EM_BINS)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_expectations: hipMalloc", e);
    HIP_TRY(ctx, hipMemsetAsync(d_T.p, 0, d_T.bytes(), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_E.p, 0, d_E.bytes(), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b->d_queue.p, 0, sizeof(int32_t) * kQueueSlots, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    // all classes at once, the smallest first, each on its own stream (FanOut); launch i has counter i of the work queue (at most
    // kClasses launches, kQueueSlots counters)
    std::stable_sort(launches.begin(), launches.end(), [](const EmLaunch &x, const EmLaunch &y) { return x.dp->cells < y.dp->cells; });
    bool serial = false;
    for (const auto &l : launches) serial |= l.uses_others_regions;
    const FanOut fan{ctx, launches.size(), serial};
    for (size_t i = 0; i < launches.size(); ++i) {
        const EmLaunch &l = launches[i];
        hipStream_t st = fan.stream(i);
        if ((rc = fan.before(i)) != NPR_OK) return rc;
        KernelArgs a = em_args(b, l, static_cast<int>(i), d_T.p, d_E.p);
        a.ring = ring.p ? ring.p + l.ring_off : nullptr;
        if (l.kind == EmKind::tile_cs) a.wcap = ctx->opt[NPR_OPT_EM_TILE] == 2 ? 1 : 0;  // (the column-scaled kernel has no ring: the field carries the test switch)
        const int lrc = l.kind == EmKind::tile_cs ? launch_em_tile_cs(a, em_tile_cs_waves(), l.grid, st, shape.sw, shape.flat)
                        : l.kind == EmKind::tile  ? launch_em_tile(a, l.R, l.grid, st)
                        : l.kind == EmKind::wide  ? launch_em_wide(a, l.R, l.NW, l.grid, st)
                        : l.kind == EmKind::stair ? launch_em_stair(a, l.R, l.grid, st)
                                                  : launch_em(a, l.grid, l.lds, l.global_ring, st);
        if (lrc != 0) return fail(ctx, NPR_ERR_HIP, "E-step kernel launch", static_cast<hipError_t>(lrc));
        if ((rc = fan.after(i)) != NPR_OK) return rc;
    }
    if ((rc = fan.join(kernel_ms)) != NPR_OK) return rc;
    b->outs.resize(b->tasks.size());
    HIP_TRY(ctx, hipMemcpy(b->outs.data(), b->d_outs.p, b->d_outs.bytes(), hipMemcpyDeviceToHost));
    // The tasks the column-scaled kernel did not count (TASK_RERUN: its range certificate, or backward values far above a lane's scale) are counted
    // here by k_em_tile, on the scratch regions and planes the first launch had, into the same sums.
    for (size_t i = 0; i < launches.size(); ++i) {
        const EmLaunch &l = launches[i];
        if (l.kind != EmKind::tile_cs) continue;
        Rerun r;
        if ((rc = stage_rerun(b, l.dp->first, l.dp->count, static_cast<int>(i), true, "npr_batch_expectations: hipMalloc", &r)) != NPR_OK) return rc;
        if (std::getenv("NPR_TIMING")) std::fprintf(stderr, "[npr] E-step: %zu of %d stripe tasks counted again with a per-cell exponent\n", r.again.size(), l.dp->count);
        if (r.again.empty()) continue;
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        KernelArgs a = em_args(b, l, static_cast<int>(i), d_T.p, d_E.p);
        a.tasks = r.d_tasks.p, a.outs = r.d_outs.p, a.ntasks = r.ntasks();
        const int lrc = launch_em_tile(a, l.R, std::min(r.ntasks(), l.grid), ctx->stream);
        if (lrc != 0) return fail(ctx, NPR_ERR_HIP, "E-step kernel launch (second pass)", static_cast<hipError_t>(lrc));
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (kernel_ms) {
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            *kernel_ms += ms;
        }
        if ((rc = merge_rerun(b, r)) != NPR_OK) return rc;
    }
    std::vector<double> bins(NPR_MAX_MODELS * EM_BINS);
    HIP_TRY(ctx, hipMemcpy(T_exp, d_T.p, d_T.bytes(), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bins.data(), d_E.p, d_E.bytes(), hipMemcpyDeviceToHost));
    unpack_bins(bins.data(), E_exp);
    const double LN2 = 0.69314718055994530942;
    for (int64_t k = 0; k < ntasks; ++k) {
        const TaskOut &o = b->outs[k];
        if (o.status != NPR_OK) return fail(ctx, o.status, "npr_batch_expectations: a segment has zero probability under the model");
        loglik[b->tasks[k].model] += (std::log2(static_cast<double>(o.tot_m)) + o.tot_e) * LN2;
    }
    b->ran = false;  // the task outputs now belong to the E-step
    return NPR_OK;
}

int32_t npr_batch_dense(npr_batch *b, int64_t read_index, float *Fm_v, int32_t *Fm_e, float *Bm_v, int32_t *Bm_e, int64_t cap) {
    if (!b || read_index < 0 || read_index >= b->n_reads || !Fm_v || !Fm_e || !Bm_v || !Bm_e) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    if (b->read_status[read_index] != NPR_OK) return b->read_status[read_index];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        const int32_t rc = ensure_coff(b);  // the dense dump runs the generic kernel
        if (rc != NPR_OK) return rc;
    }
    std::lock_guard<std::mutex> arena_lock(ctx->arena->mu);  // the dump runs the read in region 0 of the arena
    ++ctx->arena->epoch;
    int64_t written = 0;
    DevBuf<float> d_Bv;
    DevBuf<int32_t> d_Be;
    DevBuf<TaskOut> d_out1;
    hipError_t e;
    if ((e = d_Bv.alloc(b->slot_stride)) != hipSuccess || (e = d_Be.alloc(b->slot_stride)) != hipSuccess || (e = d_out1.alloc(1)) != hipSuccess)
        return fail(ctx, NPR_ERR_NOMEM, "npr_batch_dense: hipMalloc", e);
    // band rows are needed to strip the row padding
    for (int32_t s = 0; s < b->read_ntasks[read_index]; ++s) {
        const int32_t k = b->task_of[b->read_first_task[read_index] + s];
        const Task &t = b->tasks[k];
        // width of this task decides LDS vs global ring
        std::vector<int32_t> wn(t.D + 1);
        HIP_TRY(ctx, hipMemcpy(wn.data(), b->d_n.p + t.band_off, sizeof(int32_t) * (t.D + 1), hipMemcpyDeviceToHost));
        const int w = (*std::max_element(wn.begin(), wn.end()) + 3) & ~3;
        const bool global_ring = w > generic_max_wcap();
        KernelArgs a = launch_args(b, k, 1, 0, std::max(w, 64), 0, nullptr);
        a.outs = d_out1.p;
        a.Bv = d_Bv.p;
        a.Be = d_Be.p;
        DevBuf<float> ring1;
        if (global_ring) {
            if ((e = ring1.alloc(static_cast<size_t>(18) * w)) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_dense: hipMalloc", e);
            a.ring = ring1.p;
        }
        HIP_TRY(ctx, hipMemsetAsync(b->d_queue.p, 0, sizeof(int32_t) * kQueueSlots, ctx->stream));
        const int rc = launch_generic(a, 1, 256, generic_lds_bytes(global_ring ? 0 : a.wcap), true, global_ring, ctx->stream);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_dp_generic<dense> launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<int32_t> n(t.D + 1);
        std::vector<uint32_t> co(t.D + 1);
        HIP_TRY(ctx, hipMemcpy(n.data(), b->d_n.p + t.band_off, sizeof(int32_t) * (t.D + 1), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(co.data(), b->d_coff.p + t.band_off, sizeof(uint32_t) * (t.D + 1), hipMemcpyDeviceToHost));
        std::vector<float> fv(t.cells_pad), bv(t.cells_pad);
        std::vector<int32_t> fe(t.cells_pad), be(t.cells_pad);
        // slot 0 of the generic layout: mantissa plane, then exponent plane
        HIP_TRY(ctx, hipMemcpy(fv.data(), ctx->arena->F, sizeof(float) * t.cells_pad, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(fe.data(), ctx->arena->F + sizeof(float) * b->slot_stride, sizeof(int32_t) * t.cells_pad, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(bv.data(), d_Bv.p, sizeof(float) * t.cells_pad, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(be.data(), d_Be.p, sizeof(int32_t) * t.cells_pad, hipMemcpyDeviceToHost));
        for (int32_t d = 0; d <= t.D; ++d)
            for (int32_t j = 0; j < n[d]; ++j) {
                if (written >= cap) return NPR_ERR_CAPACITY;
                Fm_v[written] = fv[co[d] + j], Fm_e[written] = fe[co[d] + j];
                Bm_v[written] = bv[co[d] + j], Bm_e[written] = be[co[d] + j];
                ++written;
            }
    }
    b->ran = false;  // the pair buffers of this read were overwritten by the debug launch
    return NPR_OK;
}

int32_t npr_batch_rs_forward(npr_batch *b, int64_t read_index, float *Fm_v, int32_t *Fm_e, int64_t cap) {
    if (!b || read_index < 0 || read_index >= b->n_reads || !Fm_v || !Fm_e) return NPR_ERR_INVALID;
    npr_ctx *ctx = b->ctx;
    if (b->read_status[read_index] != NPR_OK) return b->read_status[read_index];
    if (!b->ran) return fail(ctx, NPR_ERR_STATE, "npr_batch_rs_forward before npr_batch_run (which sizes the forward scratch)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> arena_lock(ctx->arena->mu);  // the task runs in region 0 of the arena
    ++ctx->arena->epoch;
    DevBuf<TaskOut> d_out1;
    if (d_out1.alloc(1) != hipSuccess) return fail(ctx, NPR_ERR_NOMEM, "npr_batch_rs_forward: hipMalloc");
    const ModelShape shape = model_shape(ctx);
    int64_t written = 0;
    for (int32_t s = 0; s < b->read_ntasks[read_index]; ++s) {
        const int32_t k = b->task_of[b->read_first_task[read_index] + s];
        const Task &t = b->tasks[k];
        int R = 0;
        for (const auto &L : b->launches)
            if (k >= L.first && k < L.first + L.count && (kClassTab[L.cls].kind == K_RS || kClassTab[L.cls].kind == K_MID)) R = kClassTab[L.cls].R;
        if (R == 0 || t.ctl_off < 0) return fail(ctx, NPR_ERR_STATE, "npr_batch_rs_forward: the read has a segment that k_dp_rs does not run");
        KernelArgs a = launch_args(b, k, 1, 0, 0, 0, nullptr);
        a.outs = d_out1.p;
        HIP_TRY(ctx, hipMemsetAsync(b->d_queue.p, 0, sizeof(int32_t) * kQueueSlots, ctx->stream));
        const int rc = launch_rs(a, R, 1, ctx->stream, shape.sw, shape.flat);
        if (rc != 0) return fail(ctx, NPR_ERR_HIP, "k_dp_rs launch", static_cast<hipError_t>(rc));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int64_t half = rs_half_cells(static_cast<int64_t>(static_cast<uint32_t>(t.cells_pad)));
        std::vector<float> fv(static_cast<size_t>(t.cells_pad));
        std::vector<int32_t> fe(static_cast<size_t>(t.D / NPR_RS_K + 1));
        std::vector<uint32_t> ctl(2 * (static_cast<size_t>(t.D) + 1));
        HIP_TRY(ctx, hipMemcpy(fv.data(), ctx->arena->F, sizeof(float) * fv.size(), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(fe.data(), ctx->arena->F + 4 * half, sizeof(int32_t) * fe.size(), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(ctl.data(), b->d_ctl.p + 2 * t.ctl_off, sizeof(uint32_t) * ctl.size(), hipMemcpyDeviceToHost));
        const int rshift = stair_rshift(R);
        for (int32_t d = 0; d <= t.D; ++d) {
            const uint32_t w0 = ctl[2 * d], w1 = ctl[2 * d + 1];
            int64_t first;  // scratch cell of the row's first band cell
            int32_t n;
            if (stair_packed(R, 1)) {
                const uint32_t lo0 = w1 & 127u, lo1 = (w1 >> 7) & 127u;
                n = static_cast<int32_t>(((w1 >> 14) & 127u) + ((w1 >> 21) & 127u));
                // (word 0 is where lane 0 WOULD land: below the region's start for a row whose first lanes are outside the band)
                first = static_cast<int64_t>(static_cast<int32_t>(w0 - row_bias<2>()) >> 3) + 2 * lo1 + ((lo0 + lo1) - 2 * lo1);
            } else {
                const int32_t jlo = static_cast<int32_t>(w1 & 8191u);
                n = static_cast<int32_t>((w1 >> 13) & 8191u);
                first = static_cast<int64_t>(w0) + (jlo - ((jlo >> rshift) << rshift));
            }
            for (int32_t j = 0; j < n; ++j) {
                if (written >= cap) return NPR_ERR_CAPACITY;
                if (first + j < 0 || first + j >= static_cast<int64_t>(fv.size())) return fail(ctx, NPR_ERR_STATE, "npr_batch_rs_forward: a control word points outside the task's scratch");
                Fm_v[written] = fv[static_cast<size_t>(first + j)], Fm_e[written] = fe[static_cast<size_t>(d / NPR_RS_K)];
                ++written;
            }
        }
    }
    b->ran = false;  // the pair buffers of this read were overwritten by the debug launch
    return NPR_OK;
}

}  // extern "C"
