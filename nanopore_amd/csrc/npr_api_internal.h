// npr_api_internal.h -- what the translation units of the C ABI share (round 6: npr_api.cpp was one file of 3 000 lines):
// the context and batch structures, device buffers, the kernel class table, error plumbing.  Internal to libnprealign; not installed.
//   npr_api.cpp     context, options, models, the plan-inspection entry points, the small public helpers
//   npr_stage.cpp   npr_batch_create*: plan points, packing, H2D, the device planner and its cross-check, kernel classes and launch geometry
//   npr_run.cpp     npr_batch_run (launch policy, second pass of tasks without a range certificate), the E-step, the dense dumps
//   npr_finish.cpp  npr_batch_finish and what reads its results: the device MEA stage and its pieced D2H, the rescore sums, the host stage, ops / pairs
//   npr_stats_api.cpp  post-alignment statistics, k-mer and indel-k-mer tables (npr_stats.hip, npr_kmer.hip)
//   npr_snp_api.cpp  base expectations, SNP calls and variants (npr_stats.hip, npr_snpcall.hip)
//   npr_pileup_api.cpp  the device pileup (npr_pileup.hip)
//   npr_text.cpp    cigar and SAM record text (the transport forms a job ships)
//   npr_seed_api.cpp  exact-match seeding (npr_seed.hip): the index, the matches, their SAM records
//   npr_seedchain_api.cpp  the chains of seed rows given on the host as guides (npr_seedchain.hip), their SAM records
//   npr_seedmap_api.cpp  reads -> rows, chains and guides in one device-resident object (npr_seedmap.hip between the two above)
//   npr_bam_api.cpp  SAM text to sorted BAM and BAI, BGZF both ways, BAM to SAM text, BAM streams into a pileup, region queries (npr_bam.hip, npr_deflate.hip, npr_inflate.hip, npr_bamread.hip, npr_bampile.hip, npr_bamregion.hip)
//   npr_bammerge_api.cpp  BAM streams to sorted, merged BAM files, the index of a file as it stands (npr_bammerge.hip)
//   npr_cigtext_api.cpp  cigar text made on the device (npr_cigtext.hip): npr_cigar_text_packed, npr_batch_cigar_text, NPR_OPT_FINISH_TEXT
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "npr_device.h"
#include "npr_internal.h"
#include "npr_sched.h"
#include "npr_threads.h"

using namespace npr;

struct npr_plan {
    Plan plan;
};

namespace npr_impl {
struct MeaScratch;

// Forward-value scratch of ONE device (one region per resident wavefront), shared by every context on that device and only
// growing: a hipMalloc of ~100 GB costs seconds, far more than the DP pass it serves, and a pipelined job keeps two
// batches in flight on two contexts of the same GPU (nanopore_amd/job.py) -- their DP launches each fill the chip and so
// run one after the other anyway, and one arena instead of two is the difference between fitting the device and not
// (config 3: ~130-250 GB).  `mu` is held by whatever launches kernels that read or write the arena (the DP pass, the device
// MEA stage whose tables are carved out of it, the E-step, the dense dump) until they have finished, and while it is
// regrown.  `epoch` is bumped whenever its contents may have been overwritten: a finished batch may use the packed cigars
// the MEA stage left there only while its stamp is current.
// The arena points kArenaPad bytes into its allocation and is followed by as much: the register E-step loads forward rows
// with a slot shift of up to two and may touch a few cells before / after a region.
struct DeviceArena {
    static constexpr size_t kPad = 1024;
    std::mutex mu;
    char *F = nullptr;  // 8 bytes per cell
    std::atomic<size_t> cells{0};  // (read without the mutex where only its size matters: staging must not wait for a DP pass)
    std::atomic<uint64_t> epoch{1};
    int users = 0;
};
constexpr int kMaxDevices = 64;
extern DeviceArena g_arena[kMaxDevices];  // (npr_api.cpp)
}  // namespace npr_impl
using namespace npr_impl;

struct npr_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // one side stream per kernel class so that the classes of a mixed batch run concurrently instead of each
    // leaving the chip idle during its tail
    static constexpr int kSideStreams = 6;
    hipStream_t side[kSideStreams] = {};
    hipEvent_t side_done[kSideStreams] = {};
    int cu_count = 0;
    size_t total_mem = 0;
    bool model_set[NPR_MAX_MODELS] = {};
    DevModel models[NPR_MAX_MODELS];
    DevModel *d_models = nullptr;
    std::string last_error;
    int host_threads = 1;
    DeviceArena *arena = nullptr;  // the device's forward scratch (shared with the other contexts on this device)
    int overlap = 0;               // NPR_OPT_OVERLAP: see include/nprealign.h (1: own MEA tables + half of every SIMD left free by the DP launches; 2: own MEA tables only)
    int64_t deflate_last[4] = {};  // npr_deflate_last: blocks emitted as (a), (b), (c) and the stream's length, of the last compressed stream
    int64_t inflate_last[4] = {0, -1, 0, 0};  // npr_inflate_last: blocks, the first refused one (-1: none), its status and the stream's length, of the last file inflated
    int64_t merge_last[4] = {};    // npr_bam_merge_last: records, stream bytes, bytes k_merge_gather moved and its nanoseconds, of the last BAM image written from streams
    int64_t opt[NPR_OPT_COUNT] = {};  // npr_ctx_option: the test / bring-up switches (all 0 by default)
    static constexpr size_t kArenaPad = DeviceArena::kPad;
    float *arena_Fx = nullptr;  // E-step only: four more forward planes (per context)
    size_t arena_fx_cells = 0;
    // pinned host staging for the posterior triples of npr_batch_finish (grow-only): a pageable destination halves
    // the D2H rate and the copy is a GB per batch
    void *pin_pairs = nullptr;
    size_t pin_pairs_bytes = 0;
    std::vector<hipEvent_t> ops_events;  // one per piece of a D2H through pin_pairs (fetch_pieced)
    // the packed cigars of the last batch or two that were destroyed: a batch's 75-150 MB, whose pages cost 3 ms to touch when the
    // next batch is finished and 6 ms to give back when it is destroyed (with a caller waiting for the context)
    struct HostWords {
        std::unique_ptr<uint32_t[]> p;
        int64_t cap = 0;
    };
    std::vector<HostWords> packed_pool;
    // a buffer of at least `words` out of the pool into (p, cap), when it has one
    void take_packed(int64_t words, std::unique_ptr<uint32_t[]> &p, int64_t &cap) {
        for (size_t i = 0; i < packed_pool.size(); ++i)
            if (packed_pool[i].cap >= words) {
                p = std::move(packed_pool[i].p), cap = packed_pool[i].cap;
                packed_pool.erase(packed_pool.begin() + static_cast<std::ptrdiff_t>(i));
                return;
            }
    }
    // ... and a destroyed batch's buffer into it: the pool keeps the two largest
    void give_packed(std::unique_ptr<uint32_t[]> &p, int64_t cap) {
        if (!p) return;
        if (packed_pool.size() < 2) {
            packed_pool.push_back(HostWords{std::move(p), cap});
            return;
        }
        auto &smallest = *std::min_element(packed_pool.begin(), packed_pool.end(), [](const HostWords &x, const HostWords &y) { return x.cap < y.cap; });
        if (smallest.cap < cap) smallest.p = std::move(p), smallest.cap = cap;
    }
    // pinned host staging of npr_batch_create (plan points + sequence windows), grow-only
    void *pin_stage = nullptr;
    size_t pin_stage_bytes = 0;
    MeaScratch *mea = nullptr;
    // Device buffers of destroyed batches, kept for the next batch (DevBuf::alloc_from): hipMalloc / hipFree of the
    // gigabyte-sized band, control-word and pair arrays cost more than the kernels that fill them (0.1 s per batch of
    // 50 k reads), and a pipeline stages batch after batch of the same shape.
    struct Cached {
        void *p;
        size_t bytes;
    };
    std::vector<Cached> cache;
    size_t cache_bytes = 0;
    void cache_flush() {
        for (const Cached &c : cache) (void)hipFree(c.p);
        cache.clear();
        cache_bytes = 0;
    }
};

namespace npr_impl {

// NPR_POISON=<byte>: every device buffer is filled with that byte when it is handed out (and the forward scratch before
// every batch), so that a kernel reading memory nobody wrote gives the same wrong answer on every box instead of
// depending on what the previous owner of the memory left there.  Test / bring-up switch.
inline int poison_byte() {
    const char *e = std::getenv("NPR_POISON");
    return e && e[0] ? static_cast<int>(std::strtol(e, nullptr, 0)) & 0xff : -1;
}
inline void poison(void *p, size_t bytes) {
    if (poison_byte() >= 0 && p && bytes) {
        (void)hipMemset(p, poison_byte(), bytes);
        (void)hipDeviceSynchronize();
    }
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t count = 0, cap = 0;
    hipError_t alloc(size_t n) {
        release();
        count = n;
        if (n == 0) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (e == hipSuccess) poison(p, n * sizeof(T));
        return e;
    }
    void release() {
        if (p && !borrowed) {
            if (owner && owner->cache.size() < 160) {
                owner->cache.push_back(npr_ctx::Cached{p, held});
                owner->cache_bytes += held;
            } else {
                (void)hipFree(p);
            }
        }
        p = nullptr;
        count = 0, cap = 0, borrowed = false, owner = nullptr, held = 0;
    }
    // a view of memory owned elsewhere (the forward scratch arena, idle between the DP launch and the next one)
    bool borrowed = false;
    void borrow(T *ptr, size_t n) {
        release();
        p = ptr, count = n, borrowed = true;
    }
    size_t bytes() const { return count * sizeof(T); }
    // what `o` holds becomes this buffer's, and `o` is left empty (an object that keeps a result its maker allocated)
    void take(DevBuf &o) {
        release();
        p = o.p, count = o.count, cap = o.cap, borrowed = o.borrowed, owner = o.owner, held = o.held;
        o.p = nullptr;
        o.release();
    }
    // a buffer from the context's cache of released ones (the smallest that fits without wasting more than half), else a
    // fresh one; it goes back to the cache when released
    npr_ctx *owner = nullptr;
    size_t held = 0;
    hipError_t alloc_from(npr_ctx *ctx, size_t n) {
        release();
        count = n;
        if (n == 0) return hipSuccess;
        const size_t need = n * sizeof(T);
        // small ones come in 256 KiB pieces and any cached piece up to 1 MiB serves them: a batch makes a dozen tables of a few
        // words per task, and hipFree of each (synchronous) cost 2-3 ms when the batch was staged
        constexpr size_t kSmall = size_t(1) << 20, kPiece = size_t(256) << 10;
        int best = -1;
        for (size_t i = 0; i < ctx->cache.size(); ++i)
            if (ctx->cache[i].bytes >= need && (ctx->cache[i].bytes <= 2 * need || ctx->cache[i].bytes <= kSmall) &&
                (best < 0 || ctx->cache[i].bytes < ctx->cache[best].bytes))
                best = static_cast<int>(i);
        if (best >= 0) {
            p = static_cast<T *>(ctx->cache[best].p), held = ctx->cache[best].bytes, owner = ctx;
            ctx->cache_bytes -= held;
            ctx->cache.erase(ctx->cache.begin() + best);
            poison(p, held);
            return hipSuccess;
        }
        const size_t take = need < kSmall ? (need + kPiece - 1) / kPiece * kPiece : need + need / 8;  // a little headroom: the next batch of the same shape differs by a few percent
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), take);
        if (e != hipSuccess && !ctx->cache.empty()) {
            (void)hipGetLastError();
            ctx->cache_flush();
            e = hipMalloc(reinterpret_cast<void **>(&p), take);
        }
        if (e == hipSuccess) held = take, owner = ctx, poison(p, take);
        return e;
    }
    // grow-only use (scratch kept from batch to batch): count is the size asked for, cap what is allocated
    hipError_t reserve(size_t n) {
        if (n <= cap && p) {
            count = n;
            return hipSuccess;
        }
        const hipError_t e = alloc(n + n / 4 + 1);
        cap = e == hipSuccess ? count : 0;
        count = e == hipSuccess ? n : 0;
        return e;
    }
    ~DevBuf() { release(); }
};

// scratch of the device MEA stage (npr_mea.hip), kept by the context: hipMalloc / hipFree of gigabytes per batch
// cost more than the kernels
struct MeaScratch {
    DevBuf<int64_t> off, mass, od;
    DevBuf<int32_t> cnt, start, col, sorted, small, tmp, map, pieces;
    DevBuf<uint32_t> dense;
};

inline int32_t fail(npr_ctx *ctx, int32_t code, const char *what, hipError_t e = hipSuccess) {
    // a launch or copy that finds the device full (a kernel's private segment is allocated at launch) is the same condition as
    // a failed hipMalloc: callers halve the batch and try again on NPR_ERR_NOMEM
    if (code == NPR_ERR_HIP && e == hipErrorOutOfMemory) code = NPR_ERR_NOMEM, (void)hipGetLastError();
    if (ctx) {
        ctx->last_error = what;
        if (e != hipSuccess) {
            ctx->last_error += ": ";
            ctx->last_error += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                  \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) return fail((ctx), NPR_ERR_HIP, #expr, _e);   \
    } while (0)

// ---- the analysis entry points (everything but the hot path, which keeps HIP_TRY): one guard at the ABI boundary, one vocabulary for device steps ----
// what a failed step or a refused argument throws once ctx->last_error says why; guarded() turns it into the entry point's return value
struct EntryFailure {
    int32_t code;
};

// The device steps of one entry point, all on the context's stream.  A step that fails records "<entry>: <step>: <hip error>" through fail(), waits
// for the stream -- a copy or kernel queued earlier may still use a DevBuf or host vector of the frames about to unwind -- and throws.
struct Call {
    npr_ctx *ctx;
    const char *entry;
    [[noreturn]] void failed(int32_t code, const char *step, hipError_t e) const {
        char text[160];
        std::snprintf(text, sizeof(text), "%s: %s", entry, step);
        code = fail(ctx, code, text, e);
        (void)hipStreamSynchronize(ctx->stream);
        throw EntryFailure{code};
    }
    void check(hipError_t e, const char *step) const {
        if (e != hipSuccess) failed(NPR_ERR_HIP, step, e);
    }
    // a refused argument: `text` as it is (none: last_error stays)
    [[noreturn]] void refuse(int32_t code, const char *text = nullptr) const { throw EntryFailure{text ? fail(ctx, code, text) : code}; }
    // a step of the hot-path units, which report through fail() themselves
    void passed(int32_t rc) const {
        if (rc == NPR_OK) return;
        (void)hipStreamSynchronize(ctx->stream);
        throw EntryFailure{rc};
    }
    template <typename T>
    void alloc(DevBuf<T> &b, size_t n) const {
        const hipError_t e = b.alloc(n);
        if (e != hipSuccess) failed(NPR_ERR_NOMEM, "hipMalloc", e);
    }
    template <typename T>
    void alloc_cached(DevBuf<T> &b, size_t n) const {  // from the context's cache of released buffers
        const hipError_t e = b.alloc_from(ctx, n);
        if (e != hipSuccess) failed(NPR_ERR_NOMEM, "hipMalloc", e);
    }
    void copy_up(void *dst, const void *src, size_t bytes) const {
        if (bytes) check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "H2D");
    }
    template <typename T>
    void upload(DevBuf<T> &b, const T *src, size_t n) const {
        alloc(b, n);
        copy_up(b.p, src, b.bytes());
    }
    template <typename T>
    void upload(DevBuf<T> &b, const std::vector<T> &v) const { upload(b, v.data(), v.size()); }
    void zero(void *p, size_t bytes) const {
        if (bytes) check(hipMemsetAsync(p, 0, bytes, ctx->stream), "memset");
    }
    template <typename T>
    void zero(DevBuf<T> &b) const { zero(b.p, b.bytes()); }
    void fetch(void *dst, const void *src, size_t bytes) const {
        if (bytes) check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), "D2H");
    }
    void launched(int rc, const char *kernel) const {
        if (rc != 0) failed(NPR_ERR_HIP, kernel, static_cast<hipError_t>(rc));
    }
    void sync() const { check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"); }
};

// An entry point's body behind the C ABI: guarded(ctx, "npr_entry", [&](const Call &dev) -> T { ... }), T the int32_t or int64_t it returns.  Sets the
// device, runs the body; an EntryFailure becomes its code, any other exception NPR_ERR_NOMEM.  ctx may be null for host code (no device, no text).
template <typename F>
auto guarded(npr_ctx *ctx, const char *entry, F &&body) -> decltype(body(std::declval<const Call &>())) {
    using T = decltype(body(std::declval<const Call &>()));
    static_assert(std::is_same<T, int32_t>::value || std::is_same<T, int64_t>::value, "an entry point returns a status or a count");
    const Call dev{ctx, entry};
    try {
        if (ctx) dev.check(hipSetDevice(ctx->device), "hipSetDevice");
        return body(dev);
    } catch (const EntryFailure &f) {
        return f.code;
    } catch (const std::exception &) {
        char text[160];
        std::snprintf(text, sizeof(text), "%s: out of host memory", entry);
        return fail(ctx, NPR_ERR_NOMEM, text);
    }
}

// NPR_TIMING=1 prints host-stage wall times to stderr (bring-up / DESIGN.md host-inclusive numbers)
struct StageTimer {
    bool on;
    std::chrono::steady_clock::time_point t0;
    const char *what;
    explicit StageTimer(const char *w) : on(std::getenv("NPR_TIMING") != nullptr), t0(std::chrono::steady_clock::now()), what(w) {}
    void lap(const char *label) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[npr timing] %s / %s: %.1f ms\n", what, label, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

}  // namespace npr_impl
using namespace npr_impl;

struct npr_batch {
    npr_ctx *ctx = nullptr;
    npr_params params{};
    int64_t n_reads = 0;
    // host copies needed by finish()
    std::vector<int64_t> ref_len, read_len;  // spans of the guide's window
    std::vector<int64_t> gstart;             // per read: first reference / read position of the window
    std::vector<int32_t> ref_id;             // per read: its reference sequence
    std::vector<int32_t> guide_ops;
    std::vector<int64_t> guide_off;
    std::vector<int32_t> read_status;    // planning status per read
    std::vector<int32_t> read_first_task, read_ntasks;
    std::vector<Task> tasks;             // device order (sorted longest first)
    std::vector<int32_t> task_of;        // [read_first_task[r] + s] -> index into tasks
    std::vector<int64_t> task_cells;     // in-band lattice cells per task (device order)
    std::vector<TaskOut> outs;
    std::vector<uint8_t> task_rerun;     // row-scaled tasks npr_batch_run ran again with a per-cell exponent
    std::vector<uint8_t> debug_refuse;   // per task (empty: none): the next npr_batch_run takes it as refused by its range certificate (npr_batch_debug_refuse)
    npr_batch_stats stats{};
    // device
    DevBuf<Task> d_tasks;
    DevBuf<TaskOut> d_outs;
    DevBuf<int32_t> d_queue;
    DevBuf<uint8_t> d_seq;
    DevBuf<int32_t> d_lo, d_n;
    DevBuf<uint32_t> d_coff;
    DevBuf<uint32_t> d_ctl;  // register-kernel tasks: frame schedule, two words per anti-diagonal
    DevBuf<Stripe> d_stripes;  // k_dp_tile tasks: stripe tables
    DevBuf<uint32_t> d_rowmask;  // ... and the packed lane masks of every row of every stripe (tile_row_word)
    DevBuf<PlanSeg> d_pseg;    // the segments as the device planner sees them (read order)
    DevBuf<int64_t> d_region;  // k_dp_tile: first scratch cell of each resident workgroup
    std::vector<int64_t> region_end;  // ... and one past its last (host copy: the E-step sizes its planes for the regions it uses)
    size_t scratch_cells = 0;  // forward scratch this batch needs from the context arena
    bool variable_regions = false;  // the one-wavefront frame launches have regions of their own size (not E-step capable)
    bool pair_rs = false;  // the batch was staged for the row-scaled kernels (classes 12-17: k_dp_mid_rs, k_dp_rs)
    DevBuf<int32_t> d_px, d_py;
    DevBuf<float> d_pp;
    int64_t slot_stride = 0;
    // One DP launch per kernel class present in the batch (tasks are grouped by class, longest first).
    struct Launch {
        int cls;      // index into kClassTab; (historical note) 0..2 register staircase kernel with 1/2/4 cells per lane; 3..5 generic kernel with an LDS ring for
                      // bands of at most 512 / 1024 / 2270 cells; 6 generic kernel with the ring in HBM/L2
        int first, count, grid, wcap;
        int threads;  // generic kernel: workgroup size (wavefronts per task x 64)
        size_t lds;
        int64_t cells;
        int64_t width;  // widest anti-diagonal of the class
        int slot_base;  // first forward-scratch region of this launch
        int region_first;  // own_regions: index of its first entry in d_region
        bool own_regions;  // one region per workgroup sized by its first task (d_region) instead of uniform ones
    };
    std::vector<Launch> launches;
    DevBuf<float> d_ring;
    bool ran = false, finished = false;
    int32_t finish_stage = 0;  // which stage the last npr_batch_finish took: 0 the device stage, 1 the host stage (npr_batch_debug_finish_stage)
    // results
    std::vector<npr_read_result> results;
    std::vector<int64_t> ops_off;
    std::unique_ptr<int32_t[]> ops;      // (op, length) pairs of all reads; not a vector: no zero-fill of 100s of MB
    int64_t ops_words = 0, ops_cap = 0;
    // the same cigars as one 32-bit word per op (length << 2 | op): how the device MEA stage hands them over.  Either
    // form is made from the other the first time it is asked for.
    std::unique_ptr<uint32_t[]> packed;
    int64_t packed_cap = 0;
    bool have_pairs_form = false, have_packed_form = false;
    // NPR_MODE_RESCORE_ORIGINAL: the cigars are the guide's (operations of length 0 left out), made from b->guide_ops the first time somebody asks
    bool ops_from_guide = false;
    // ... and what npr_batch_create leaves for npr_batch_finish: the guide's M columns as a table on the device (rescore_stage), per read the
    // number of M columns and of operations kept; rs_staged = false: the host stage scores (NPR_OPT_HOST_MEA, or a sum that could not be exact)
    bool rs_staged = false;
    int rs_shift = 0;
    std::vector<int64_t> rs_columns, rs_kept;
    DevBuf<int32_t> d_rs_gy;
    DevBuf<int64_t> d_rs_gx_off;
    std::vector<int64_t> pair_off;
    std::vector<Pair> pairs;             // filled by fetch_pairs(): at finish in the host modes, on demand after the device MEA
    bool pairs_ready = false;
    std::vector<int64_t> task_dst;       // prefix of the per-task pair counts
    // packed cigars left on the device by the device MEA stage (valid while dev_ops_epoch == the arena's epoch)
    const uint32_t *dev_ops = nullptr;
    const int64_t *dev_od = nullptr;
    uint64_t dev_ops_epoch = 0;
    // the cigars as SAM text on the host (npr_cigtext_api.cpp): made by npr_batch_finish under NPR_OPT_FINISH_TEXT, else the first time
    // npr_batch_cigar_text asks.  words_on_device: such a finish left the packed words on the device only (fetch_device_words)
    std::unique_ptr<char[]> text;
    int64_t text_cap = 0;
    std::vector<int64_t> text_off;
    bool text_ready = false, words_on_device = false;
};

// the device pileup (npr_pileup_api.cpp, npr_pileup.hip): the table and the difference array of its deletion columns live on the device from
// npr_pileup_create to npr_pileup_destroy and are added to by every npr_pileup_add / npr_pileup_add_batch
struct npr_pileup {
    npr_ctx *ctx = nullptr;
    std::vector<int64_t> len;    // positions of every reference sequence
    std::vector<int64_t> base;   // [n_refs + 1] first row of every sequence
    int64_t rows = 0;
    DevBuf<int32_t> tab;         // [rows][NPR_PILEUP_WORDS]; word 5 is written by the scan
    DevBuf<int32_t> diff;        // [rows + n_refs]: sequence k's slots start at base[k] + k, the last one is spare
    DevBuf<int32_t> tile;        // the scan's tile sums
    DevBuf<int64_t> dbase;       // [n_refs + 1] first slot of every sequence
    DevBuf<int32_t> bad;         // one word: a record of the current call ran past what it has
};

// an inflated BAM stream and the offsets of its records (npr_bam_api.cpp, npr_bam_open): on the device from npr_bam_open to npr_bam_close; the
// header's fields on the host
struct npr_bam_stream {
    npr_ctx *ctx = nullptr;
    int64_t stream_len = 0, l_text = 0, n = 0;  // n: records
    DevBuf<uint8_t> stream;
    DevBuf<int64_t> rec_off;        // [n] stream offset of every record's block_size
    std::vector<int64_t> ref_len;   // [n_ref] l_ref
    std::vector<int64_t> name_off;  // [n_ref + 1]
    std::vector<uint8_t> names;     // back to back, without NULs
    std::vector<int64_t> block_off, stream_off;  // npr_bam_open only: the file's block tables (npr_bgzf_scan), [blocks + 1] each, what npr_bam_index searches
};

// the index of one reference set (npr_seed_api.cpp): lives on the device from npr_seed_index_create to npr_seed_index_destroy
struct npr_seed_index {
    npr_ctx *ctx = nullptr;
    int32_t k = 0, kb = 0;
    int64_t n_refs = 0, bytes = 0;  // bytes of the code buffer
    std::vector<int32_t> ref_len;   // [n_refs] bases of every sequence (what the chain kernels take as ref_len)
    DevBuf<uint8_t> codes;
    DevBuf<int64_t> off;            // [n_refs + 1] ASCII offsets of the sequences
    DevBuf<int32_t> table, pos;
};

// the rows, chains and guides of one call's reads (npr_seedmap_api.cpp): on the device from npr_seed_map_create to npr_seed_map_destroy.
// Without a row there is no buffer at all (rows > 0 means chains > 0 and op pairs > 0: every row lies in a chain, every chain has an M)
struct npr_seed_map {
    npr_ctx *ctx = nullptr;
    int64_t n_reads = 0, rows = 0, chains = 0, pairs = 0;
    DevBuf<int64_t> hit_off, chain_off, ops_off;  // [n_reads + 1], [n_reads + 1], [chains + 1]
    DevBuf<int32_t> hits, chain_rows, ops;        // [rows][4], [chains][4], [pairs][2]
};

// --------------------------------------------------------------------------------------------------
// Frame schedule of the register kernel (npr_kernel_stair.hip).  The wavefront holds a frame of C = 64*R slots of the
// current anti-diagonal (times NW wavefronts for k_dp_wide), slot j = lattice point (x0 + j, y0 - j); the frame takes an X-step (x0 += 1) into every odd
// anti-diagonal and a Y-step (y0 += 1) into every even one, so its first x-y, flo, just alternates.  The band (first
// x-y `lo`, n cells) must stay inside the frame; when it drifts to an edge the frame is REBASED by one slot
// (flo +- 2) between two anti-diagonals.  A rebase towards higher x-y may only precede an X-step and one towards
// lower x-y a Y-step (the kernel re-injects the base that left the wavefront at the step before), so the decision
// looks one anti-diagonal ahead.  Control words per anti-diagonal: row offset in the forward scratch (cells), and
// jlo | n << 13 | (rebase + 1) << 26.  Returns false when the band cannot be followed; `ctl` and `cells` may be null.
// --------------------------------------------------------------------------------------------------
namespace npr_impl {

inline bool build_stair_schedule(const Segment &s, int R, int NW, uint32_t *ctl, int64_t *cells) {
    if (s.n.empty()) return false;
    return stair_schedule(s.lo.data(), s.n.data(), s.D(), s.max_width, R, NW, ctl, cells);
}

}  // namespace npr_impl
using namespace npr_impl;

// Kernel classes of a batch, each launched on its own.  On the frame schedule, R slots per lane: k_dp_stair (K_STAIR,
// one wavefront per task, one exponent per cell), k_dp_wide (K_WIDE, NW wavefronts per task), k_dp_rs (K_RS, K_STAIR's
// classes in row-scaled arithmetic), k_dp_mid_rs (K_MID, the same with the two sweeps on two wavefronts).  On column
// stripes: k_dp_tile (K_TILE, one exponent per cell), k_dp_tile_cs (K_TILE_RS, one per lane).  Everything else:
// k_dp_generic with its ring in LDS (K_GENERIC_LDS, three width classes) or in HBM (K_GENERIC_GLOBAL).
namespace npr_impl {
enum { K_STAIR = 0, K_WIDE = 1, K_GENERIC_LDS = 2, K_GENERIC_GLOBAL = 3, K_TILE = 4, K_MID = 5, K_RS = 6, K_TILE_RS = 7 };
struct KClass {
    int kind, R, NW;
    int slots() const { return 64 * R * NW; }
};
constexpr int kClasses = 19;
constexpr KClass kClassTab[kClasses] = {{K_STAIR, 1, 1}, {K_STAIR, 2, 1}, {K_STAIR, 4, 1}, {K_WIDE, 2, 4}, {K_WIDE, 2, 8},
                                        {K_WIDE, 4, 8}, {K_WIDE, 4, 12}, {K_GENERIC_LDS, 0, 0}, {K_GENERIC_LDS, 0, 0},
                                        {K_GENERIC_LDS, 0, 0}, {K_GENERIC_GLOBAL, 0, 0}, {K_TILE, 2, 0},
                                        // k_dp_mid_rs<R>: the one-wavefront frame classes in row-scaled arithmetic with the two sweeps on two wavefronts that meet in the middle
                                        {K_MID, 1, 1}, {K_MID, 2, 1}, {K_MID, 4, 1},
                                        // k_dp_rs<R>: the one-wavefront frame classes 0-2 in row-scaled arithmetic (npr_rs.h)
                                        {K_RS, 1, 1}, {K_RS, 2, 1}, {K_RS, 4, 1},
                                        // k_dp_tile_cs: class 11's column stripes in column-scaled arithmetic (one exponent per lane of a stripe)
                                        {K_TILE_RS, 2, 0}};
constexpr int kFirstGeneric = 7, kTileClass = 11, kFirstPair = 12, kFirstRs = 15, kTileRsClass = 18, kQueueSlots = 24;
inline bool is_register_class(int c) { return kClassTab[c].kind <= K_WIDE || kClassTab[c].kind == K_MID || kClassTab[c].kind == K_RS; }
inline bool is_one_wave_kind(int kind) { return kind == K_STAIR || kind == K_RS; }  // one wavefront per task on the frame schedule
inline bool is_tile_kind(int kind) { return kind == K_TILE || kind == K_TILE_RS; }  // column stripes, NW wavefronts per task
// resident wavefronts per CU of the one-wavefront frame kernels (VGPR-limited: 71 / 80 / 162 registers: 7 / 6 / 3 per SIMD)
inline int stair_waves_per_cu(int R) { return R == 1 ? 28 : (R == 2 ? 24 : 12); }
// ... and of k_dp_rs<R> (72 / 72 / 105 registers: 7 / 7 / 4 per SIMD; R = 2 measured at 6 / 7 / 8 per SIMD in round 4: 7 is best)
inline int rs_waves_per_cu(int R) { return R == 1 ? 28 : (R == 2 ? 28 : 16); }

// Whether the row-scaled arithmetic (npr_rs.h) may be used with a model: its rows are renormalised to 2^NPR_RS_TOP every
// NPR_RS_K anti-diagonals with 2^6 of headroom, so nothing may grow by more than 2^(6 / NPR_RS_K) per anti-diagonal -- the sum of
// the transitions into a state times that state's largest emission (0.57 for the shipped models: values only shrink).
inline bool rs_model_ok(const DevModel &m) {
    double grow = 0.0, em_max = 0.0;
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) em_max = std::max(em_max, static_cast<double>(m.em[x * 5 + y]));
    for (int to = 0; to < 5; ++to) {
        double col = 0.0, e = em_max;
        for (int from = 0; from < 5; ++from) col += static_cast<double>(m.T[from * 5 + to]);
        if (to > 0) {
            e = 0.0;
            for (int b2 = 0; b2 < 5; ++b2) e = std::max(e, static_cast<double>((to == 1 || to == 3) ? m.ex[to * 5 + b2] : m.ey[to * 5 + b2]));
        }
        grow = std::max(grow, col * e);
    }
    // ... and the backward sweep grows by the ROW sums: a state's value is the sum over its successors of transition times the
    // successor's emission (a stochastic model's rows sum to 1; a user's model need not be stochastic)
    auto emax = [&](int st) {
        if (st == 0) return em_max;
        double e = 0.0;
        for (int b2 = 0; b2 < 5; ++b2) e = std::max(e, static_cast<double>((st == 1 || st == 3) ? m.ex[st * 5 + b2] : m.ey[st * 5 + b2]));
        return e;
    };
    for (int from = 0; from < 5; ++from) {
        double row = 0.0;
        for (int to = 0; to < 5; ++to) row += static_cast<double>(m.T[from * 5 + to]) * emax(to);
        grow = std::max(grow, row);
    }
    return grow <= std::exp2(6.0 / NPR_RS_K);
}

// What the launches ask of the loaded models.  flat_gaps: every one emits every base from every gap state with probability exactly 2^-2 (N included:
// make_dev_model gives it 1/4): the row-scaled kernels then take the gap emissions from a select instead of their LDS tables (npr_rs.h rs_cell_emissions;
// same bits).  sw: one has a short-gap switch (shortGapX <-> shortGapY); the row- / column-scaled kernels leave out the two switch terms of a cell when
// none has (the shipped ones have none): exact zeros either way (npr_rs.h).  flat: no switch, and flat_gaps.  rs_ok: rs_model_ok for every one.
struct ModelShape { bool sw, flat_gaps, flat, rs_ok; };
inline ModelShape model_shape(const npr_ctx *ctx) {
    ModelShape s{false, true, false, true};
    for (int sl = 0; sl < NPR_MAX_MODELS; ++sl) {
        if (!ctx->model_set[sl]) continue;
        const DevModel &m = ctx->models[sl];
        if (m.T[1 * 5 + 2] != 0.f || m.T[2 * 5 + 1] != 0.f) s.sw = true;
        if (!rs_model_ok(m)) s.rs_ok = false;
        for (int b2 = 0; b2 < 5; ++b2)
            if (m.ex[5 + b2] != 0.25f || m.ex[15 + b2] != 0.25f || m.ey[10 + b2] != 0.25f || m.ey[20 + b2] != 0.25f) s.flat_gaps = false;
    }
    s.flat = !s.sw && s.flat_gaps;
    return s;
}

// Stripe table of k_dp_tile for one segment (npr_kernel_tile.hip): the lattice columns 0..lX cut into stripes of 64*R
// columns; per stripe the first / last anti-diagonal on which the band has cells in it and the index of its first row in
// the task's scratch (one row per anti-diagonal of a stripe).  out[0] is the header {stripes, rows}.
inline void build_stripes(const Segment &s, int R, Stripe *out, int64_t *rows_out) {
    const int64_t S = (s.xe - s.xs) / (64 * R) + 1;
    int64_t rows;
    if (out) {
        rows = stripe_ranges(s.lo.data(), s.n.data(), s.D(), s.xe - s.xs, R, &out[1].df, &out[1].dl, static_cast<int>(sizeof(Stripe) / sizeof(int32_t)));
        stripe_fill(out, s.xe - s.xs, R);
    } else {
        thread_local std::vector<int32_t> df, dl;
        df.resize(S), dl.resize(S);
        rows = stripe_ranges(s.lo.data(), s.n.data(), s.D(), s.xe - s.xs, R, df.data(), dl.data(), 1);
    }
    if (rows_out) *rows_out = rows;
}
inline int64_t stripes_of(const Segment &s, int R) { return (s.xe - s.xs) / (64 * R) + 1; }
}  // namespace npr_impl
using namespace npr_impl;

// ---- functions one translation unit defines and another calls ----
namespace npr_impl {
int32_t rescore_stage(npr_batch *b);                       // npr_finish.cpp: NPR_MODE_RESCORE_ORIGINAL, the guide's M columns as a device table (called when a batch is staged)
KernelArgs make_args(npr_batch *b);                        // npr_run.cpp: the kernel arguments of a staged batch
int32_t ensure_coff(npr_batch *b);                         // npr_stage.cpp: the generic kernel's row offsets, made on demand
int32_t release_scratch(npr_ctx *ctx, bool caches_only);   // npr_api.cpp
void ensure_packed_form(npr_batch *b);                     // npr_finish.cpp: the batch's cigars as one word per operation
int32_t grow_pin_stage(npr_ctx *ctx, size_t bytes, const char *what);  // npr_finish.cpp: the context's pinned staging (pin_stage, grow-only) of at least `bytes`
int32_t device_words_text(npr_batch *b, const int64_t *d_off, const uint32_t *d_words, char *lend, size_t lend_bytes);  // npr_cigtext_api.cpp: the batch's text from words on the device
// `count` elements of `elem` bytes from the device to `dst` through the context's pinned staging, in pieces (npr_finish.cpp)
using PieceMove = void (*)(void *dst, const void *pin, int64_t lo, int64_t hi);  // elements [lo, hi) of the staging buffer to their place in dst
struct PiecedFetch {
    const void *dev;
    void *dst;
    int64_t count;
    size_t elem;
    int64_t per_piece, round_to;  // elements: one piece per `per_piece` of them (48 pieces at most), each rounded up to a multiple of `round_to`
    PieceMove move;               // what a host thread does with a piece that has crossed
    const char *what_pin, *what_d2h;  // the caller's error texts
};
int32_t fetch_pieced(npr_ctx *ctx, const PiecedFetch &f);
int32_t fetch_device_words(npr_batch *b);                  // npr_cigtext_api.cpp: the packed words such a finish left on the device, while they are there
// npr_seedchain_api.cpp: the chain kernels on rows and chain spans that lie on the device, wherever they came from (npr_seed_chains uploads
// them, npr_seed_map_create made them there).  count: k_chain_dp, k_chain_trace<false>, the scan; `chains` and `n_ops` (the guides'
// offsets) are final and `pairs` is on the host.  write: k_chain_trace<true> into `ops`; queued on the context's stream, not waited for.
struct SeedChainRun {
    DevBuf<int32_t> node, back, run_end, chains, ops;
    DevBuf<int64_t> n_ops;
    SeedChainArgs a{};
    int64_t pairs = 0;
    void count(const Call &dev, const int32_t *d_hits, int64_t rows, const SeedChainSpan *d_span, int64_t n_chains, int64_t max_gap, const int32_t *d_ref_len,
               const int32_t *d_read_len);
    void write(const Call &dev);
};
// npr_seed_api.cpp: the steps npr_seed_matches and npr_seed_map_create share
void seed_check_reads(const Call &dev, int64_t n_reads, const uint8_t *text, const int64_t *begin, const int64_t *end, std::vector<int64_t> &off);
void seed_stage_reads(const Call &dev, int32_t strands, int64_t n_reads, const uint8_t *text, const int64_t *begin, const int64_t *end, const std::vector<int64_t> &off,
                      DevBuf<uint8_t> &fwd, DevBuf<uint8_t> &rev, DevBuf<int64_t> &d_off);
SeedMatchArgs seed_match_args(const npr_seed_index *ix, int64_t min_len, const std::vector<int64_t> &off, const int64_t *d_off, uint32_t *d_count, const int64_t *d_hit_off);
void seed_match_pass(const Call &dev, SeedMatchArgs &a, int32_t strands, const uint8_t *fwd, const uint8_t *rev, bool emit);
void pileup_scan(const Call &dev, npr_pileup *pl);         // npr_pileup_api.cpp: word 5 of the pileup's table from its difference array
// npr_stats_api.cpp: a set of reads' cigars packed on the device (one word per operation, off[n + 1]), with the upload it may own ...
struct DeviceCigars {
    const uint32_t *ops = nullptr;
    const int64_t *off = nullptr;
    DevBuf<uint32_t> own_ops;
    DevBuf<int64_t> own_off;
};
// ... made from the host form (off.back() words at `ops`), queued on the context's stream ...
void cigars_from_host(const Call &dev, const uint32_t *ops, const std::vector<int64_t> &off, DeviceCigars &c);
// ... and the ones npr_batch_finish produced handed to `run`: where the device MEA stage left them (in the arena, whose lock is held until `run`
// returns: it waits for its kernels), else uploaded from the batch's packed host form
void with_batch_cigars(const Call &dev, npr_batch *b, const std::function<void(const DeviceCigars &)> &run);
// npr_bam_api.cpp: what the SAM -> BAM writer there and the BAM -> BAM writer of npr_bammerge_api.cpp share
void bgzf_constants(BgzfArgs &a);   // the CRC constants of the BGZF kernels
int64_t bgzf_length(int64_t len);   // a stream's length as stored blocks with the end-of-file block
int bits_of(unsigned long long v);
// The stable order of n keys of at most `bits` bits that lie on the device: d_order[j] = index of the key at place j (the identity without a pass).
// The keys are overwritten.
void sort_order(const Call &dev, DevBuf<unsigned long long> &keys, int64_t n, int bits, DevBuf<uint32_t> &d_order);
// The stream d_data[0, len) as compressed BGZF blocks: the buffers of one npr_deflate.hip run.  launch() queues the kernels; finish() fetches
// the block table (block_off[0 .. blocks], host), waits, and returns the file's length; the image then lies in packed.
struct DeflateRun {
    DevBuf<uint8_t> slots, packed;
    DevBuf<uint16_t> dist;
    DevBuf<int64_t> block_len, tile;
    DevBuf<uint32_t> chosen;
    std::vector<int64_t> block_off;
    int64_t blocks = 0, stream_len = 0;
    void launch(const Call &dev, const uint8_t *d_data, int64_t len) {
        blocks = (len + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD, stream_len = len;
        dev.alloc(slots, static_cast<size_t>(blocks * DEFLATE_SLOT + 8)), dev.alloc(packed, static_cast<size_t>(bgzf_length(len)));
        dev.alloc(dist, static_cast<size_t>(std::max<int64_t>(deflate_groups(blocks), 1) * BGZF_PAYLOAD));
        dev.alloc(block_len, blocks + 1), dev.alloc(tile, scan_tiles(blocks));
        dev.alloc(chosen, 4), dev.zero(chosen);
        DeflateArgs d{};
        d.z.data = d_data, d.z.len = len, d.z.out = slots.p;
        bgzf_constants(d.z);
        d.dist = dist.p, d.block_len = block_len.p, d.tile = tile.p, d.chosen = chosen.p, d.packed = packed.p;
        dev.launched(launch_bgzf_deflate(d, dev.ctx->stream), "k_bgzf_deflate / scan / k_bgzf_pack");
    }
    int64_t finish(const Call &dev) {
        uint32_t how[4] = {0, 0, 0, 0};
        block_off.assign(static_cast<size_t>(blocks) + 1, 0);
        dev.fetch(block_off.data(), block_len.p, block_len.bytes());
        dev.fetch(how, chosen.p, sizeof(how));
        dev.sync();
        if (how[3]) dev.failed(NPR_ERR_STATE, "k_bgzf_deflate: the emitted bits of a block are not the measured ones", hipSuccess);
        for (int k = 0; k < 3; ++k) dev.ctx->deflate_last[k] = how[k];
        dev.ctx->deflate_last[3] = stream_len;
        return block_off[blocks] + BGZF_EOF;
    }
};
// The index tables of n records in sorted order from what a measure pass left in `a` (recs, meas, order, size_sorted scanned, header_len, n_refs and
// the blocks' tables), by the INDEX paragraph of npr_sam_bam: k_bam_index_heads, the scan, k_bam_index_runs, the sort over (tid, bin),
// k_bam_gather_runs.  lin_off: [n_refs + 1] first window of every reference.  The outputs are host arrays; waits for the stream.
void bam_index_tables(const Call &dev, BamArgs &a, const std::vector<int64_t> &lin_off, int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg,
                      uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor);
}  // namespace npr_impl
