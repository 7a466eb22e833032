// npr_snp_api.cpp -- the marginAlign SNP caller on the device (npr_stats.hip, npr_snpcall.hip; marginAlignSnpCaller.py:150-155): per-position base
// expectations of a finished batch, and the calls, variants and consensus from such a table wherever it comes from
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"
#include "npr_snpmodel.h"

namespace {

// first row of every reference sequence; false: a negative length
bool row_bases(int64_t n_refs, const int64_t *ref_len, std::vector<int64_t> &base) {
    base.assign(n_refs + 1, 0);
    for (int64_t k = 0; k < n_refs; ++k) {
        if (ref_len[k] < 0) return false;
        base[k + 1] = base[k] + ref_len[k];
    }
    return true;
}

// The accumulate-on-device half of npr_batch_base_expectations: the fixed-point sums (npr_stats.hip: exact, hence the same from run to run) and
// the seen bytes of the selected reads of a finished batch, left in HBM for whoever reads them next -- the copy to the caller's table, or the
// SNP kernels.  `base`: first row of every reference sequence, base[n_refs] = rows > 0.
struct DeviceExpectations {
    DevBuf<unsigned long long> e;  // [rows][4]
    DevBuf<uint8_t> seen;          // [rows]
};
void accumulate_base_expectations(const Call &dev, npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const std::vector<int64_t> &base,
                                  DeviceExpectations &d) {
    const int64_t rows = base[n_refs], n = b->n_reads, ntasks = static_cast<int64_t>(b->tasks.size());
    std::vector<int64_t> target(n, 0);
    std::vector<uint8_t> mask(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t k = b->ref_id[i];
        const bool ok = b->results[i].status == NPR_OK && (!use || use[i]) && k >= 0 && k < n_refs &&
                        b->gstart[2 * i] + b->ref_len[i] <= ref_len[k];
        if (use && use[i] && !ok && b->results[i].status == NPR_OK)
            dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": a read's window does not fit its reference").c_str());
        mask[i] = ok ? 1 : 0;
        target[i] = ok ? base[k] + b->gstart[2 * i] : 0;
    }
    DevBuf<uint8_t> d_use;
    DevBuf<int64_t> d_target;
    dev.alloc(d.e, 4 * rows);
    dev.alloc(d.seen, rows);
    dev.zero(d.e);
    dev.zero(d.seen);
    if (!ntasks) return;
    dev.upload(d_use, mask);
    dev.upload(d_target, target);
    ExpectArgs a{b->d_tasks.p, b->d_outs.p, static_cast<int32_t>(ntasks), b->d_px.p, b->d_py.p, b->d_pp.p, b->d_seq.p, d_use.p, d_target.p, d.e.p, d.seen.p};
    dev.launched(launch_base_expectations(a, dev.ctx->stream), "k_base_expectations");
    dev.sync();  // (mask, target, d_use and d_target end with this call)
}

// A table of per-position base weights on the device in the form `kind` says (SNP_SRC_*), with the buffers it owns: what the SNP kernels read.
struct SnpSource {
    int64_t rows = 0;
    int32_t kind = 0;
    const void *table = nullptr;
    const uint8_t *seen = nullptr;
    DevBuf<double> w;
    DevBuf<uint8_t> w_seen;
    DeviceExpectations d;
};

// ... the caller's table of doubles, looked at and uploaded
void snp_source_table(const Call &dev, int64_t rows, const double *weights, const uint8_t *seen, SnpSource &s) {
    for (int64_t i = 0; i < 4 * rows; ++i)
        if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": a weight is negative or not finite").c_str());
    dev.alloc_cached(s.w, 4 * rows);
    dev.alloc_cached(s.w_seen, rows);
    dev.copy_up(s.w.p, weights, s.w.bytes());
    dev.copy_up(s.w_seen.p, seen, s.w_seen.bytes());
    s.rows = rows, s.kind = SNP_SRC_DOUBLE, s.table = s.w.p, s.seen = s.w_seen.p;
}

// ... the fixed-point expectations of the selected reads of a finished batch
void snp_source_batch(const Call &dev, npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code, SnpSource &s) {
    std::vector<int64_t> base;
    if (!row_bases(n_refs, ref_len, base)) dev.refuse(NPR_ERR_INVALID);
    s.rows = base[n_refs], s.kind = SNP_SRC_FIXED;
    if (s.rows && !ref_code) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": no reference base codes").c_str());
    if (s.rows) accumulate_base_expectations(dev, b, use, n_refs, ref_len, base, s.d);
    s.table = s.d.e.p, s.seen = s.d.seen.p;
}

// ... the counts of a pileup (words 0-4 are what k_pileup_add wrote on this stream: the running sum of word 5 is not needed)
void snp_source_pileup(const Call &dev, npr_pileup *pl, const uint8_t *ref_code, SnpSource &s) {
    if (pl->rows && !ref_code) dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": no reference base codes").c_str());
    s.rows = pl->rows, s.kind = SNP_SRC_PILEUP, s.table = pl->tab.p;
}

// the matrices' logs, as the kernels take them
struct SnpModel {
    double log_evolution[16], log_error[kSnpMaxModels * 16];
};
// what the call entry points check of their model ...
void snp_calls_model(const Call &dev, int32_t n_models, const double *evolution16, const double *error16, SnpModel &m) {
    if (!snp_log_matrices(n_models, evolution16, error16, m.log_evolution, m.log_error))
        dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": n_models outside 1..4, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row").c_str());
}
// ... and the variant entry points of their model and outputs
void snp_variants_model(const Call &dev, const double *evolution16, const double *error16, double threshold, int64_t cap, const int64_t *n_calls, SnpModel &m) {
    if (!(n_calls && cap >= 0 && threshold >= 0.0 && threshold <= 1.0 && snp_log_matrices(1, evolution16, error16, m.log_evolution, m.log_error)))
        dev.refuse(NPR_ERR_INVALID, (std::string(dev.entry) + ": a threshold outside [0, 1], a negative capacity, no n_calls, an error probability that is not a finite number above zero, or an evolution matrix with a negative entry or an all-zero row").c_str());
}

static_assert(sizeof(npr_snp_calls) == SNP_OUT_WORDS * sizeof(int64_t) && NPR_SNP_BINS == SNP_BINS && NPR_SNP_MAX_MODELS == kSnpMaxModels,
              "k_snp_calls writes an npr_snp_calls per model");

// The device half of the SNP-call entry points: k_snp_calls over a source; the base codes are uploaded, n_models structures come back.
int32_t run_snp_calls(const Call &dev, const SnpSource &s, const uint8_t *ref_code, const uint8_t *true_code, int32_t n_models, const SnpModel &m, npr_snp_calls *out) {
    std::vector<npr_snp_calls> result(n_models);  // (out is written only when everything has worked)
    std::memset(static_cast<void *>(result.data()), 0, result.size() * sizeof(npr_snp_calls));
    if (s.rows > 0) {
        DevBuf<uint8_t> d_ref, d_true;
        DevBuf<unsigned long long> d_out;
        dev.upload(d_ref, ref_code, static_cast<size_t>(s.rows));
        dev.upload(d_true, true_code, true_code ? static_cast<size_t>(s.rows) : 0);
        dev.alloc(d_out, static_cast<size_t>(n_models) * SNP_OUT_WORDS);
        dev.zero(d_out);
        SnpCallArgs a{};
        a.rows = s.rows, a.source = s.kind, a.n_models = n_models, a.table = s.table, a.seen = s.seen, a.ref_code = d_ref.p, a.true_code = d_true.p, a.out = d_out.p;
        std::memcpy(a.log_evolution, m.log_evolution, sizeof(a.log_evolution));
        std::memcpy(a.log_error, m.log_error, static_cast<size_t>(n_models) * 16 * sizeof(double));
        dev.launched(launch_snp_calls(a, dev.ctx->stream), "k_snp_calls");
        dev.fetch(result.data(), d_out.p, d_out.bytes());
        dev.sync();
    }
    std::memcpy(static_cast<void *>(out), result.data(), result.size() * sizeof(npr_snp_calls));
    return NPR_OK;
}

// The device half of the SNP-variant entry points: k_snp_variants_count and the scan, the one word the capacity decision needs, then
// k_snp_variants_emit when the calls fit.  Scratch from the context's cache of released buffers.  *n_calls and best / qual (each when given)
// are written in both outcomes, the call arrays only when everything has worked.
int64_t run_snp_variants(const Call &dev, const SnpSource &s, const uint8_t *ref_code, const SnpModel &m, double threshold, uint8_t *best, uint8_t *qual,
                         int64_t *call_row, uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls) {
    const int64_t rows = s.rows;
    if (rows == 0) return *n_calls = 0;
    const int64_t tiles = snp_variant_tiles(rows);
    DevBuf<uint8_t> d_bytes, d_alt;  // ref_code, best, qual, mask: [4][rows]
    DevBuf<uint32_t> d_tile_calls;
    DevBuf<int64_t> d_tile_off, d_row;
    DevBuf<double> d_p;
    dev.alloc_cached(d_bytes, 4 * static_cast<size_t>(rows));
    dev.alloc_cached(d_tile_calls, tiles);
    dev.alloc_cached(d_tile_off, tiles + 1);
    dev.copy_up(d_bytes.p, ref_code, rows);
    SnpCallArgs a{};
    a.rows = rows, a.source = s.kind, a.n_models = 1, a.table = s.table, a.seen = s.seen, a.ref_code = d_bytes.p, a.threshold = threshold;
    a.best = d_bytes.p + rows, a.qual = d_bytes.p + 2 * rows, a.mask = d_bytes.p + 3 * rows, a.tile_calls = d_tile_calls.p, a.tile_off = d_tile_off.p;
    std::memcpy(a.log_evolution, m.log_evolution, sizeof(a.log_evolution));
    std::memcpy(a.log_error, m.log_error, 16 * sizeof(double));
    dev.launched(launch_snp_variants_count(a, dev.ctx->stream), "k_snp_variants_count");
    int64_t total = 0;
    dev.fetch(&total, d_tile_off.p + tiles, sizeof(total));
    dev.sync();
    const bool fits = total <= cap && (total == 0 || (call_row && call_alt && call_p));
    if (fits && total) {
        dev.alloc_cached(d_row, total);
        dev.alloc_cached(d_alt, total);
        dev.alloc_cached(d_p, total);
        a.n_calls = total, a.call_row = d_row.p, a.call_alt = d_alt.p, a.call_p = d_p.p;
        dev.launched(launch_snp_variants_emit(a, dev.ctx->stream), "k_snp_variants_emit");
        dev.fetch(call_row, d_row.p, d_row.bytes());
        dev.fetch(call_alt, d_alt.p, d_alt.bytes());
        dev.fetch(call_p, d_p.p, d_p.bytes());
    }
    if (best) dev.fetch(best, a.best, rows);
    if (qual) dev.fetch(qual, a.qual, rows);
    dev.sync();
    *n_calls = total;
    if (!fits) return fail(dev.ctx, NPR_ERR_CAPACITY, "SNP variants: more calls than the arrays hold (*n_calls says how many)");
    return total;
}

}  // namespace

extern "C" {

int32_t npr_batch_base_expectations(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, double *expect, uint8_t *seen) {
    if (!b || n_refs < 0 || (n_refs && !ref_len) || !expect || !seen) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return guarded(b->ctx, "npr_batch_base_expectations", [&](const Call &dev) -> int32_t {
        std::vector<int64_t> base;
        if (!row_bases(n_refs, ref_len, base)) return NPR_ERR_INVALID;
        const int64_t rows = base[n_refs];
        std::fill(expect, expect + 4 * rows, 0.0);
        std::fill(seen, seen + rows, uint8_t(0));
        if (b->tasks.empty() || !rows) return NPR_OK;
        DeviceExpectations d;
        accumulate_base_expectations(dev, b, use, n_refs, ref_len, base, d);
        static_assert(sizeof(unsigned long long) == sizeof(double), "the caller's table doubles as the staging of the fixed-point sums");
        dev.fetch(expect, d.e.p, d.e.bytes());
        dev.fetch(seen, d.seen.p, d.seen.bytes());
        dev.sync();
        for (int64_t i = 0; i < 4 * rows; ++i) {
            unsigned long long fixed;
            std::memcpy(&fixed, expect + i, sizeof(fixed));
            expect[i] = static_cast<double>(fixed) / static_cast<double>(EXPECT_FIXED_ONE);
        }
        return NPR_OK;
    });
}

int32_t npr_snp_calls_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code, const uint8_t *true_code,
                            int32_t n_models, const double *evolution16, const double *error16, npr_snp_calls *out) {
    if (!ctx) return NPR_ERR_INVALID;
    if (rows < 0 || (rows && (!weights || !seen || !ref_code)) || !out) return fail(ctx, NPR_ERR_INVALID, "npr_snp_calls_table: bad argument");
    return guarded(ctx, "npr_snp_calls_table", [&](const Call &dev) -> int32_t {
        SnpModel m;
        SnpSource s;
        snp_calls_model(dev, n_models, evolution16, error16, m);
        snp_source_table(dev, rows, weights, seen, s);
        return run_snp_calls(dev, s, ref_code, true_code, n_models, m, out);
    });
}

int32_t npr_batch_snp_calls(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code, const uint8_t *true_code,
                            int32_t n_models, const double *evolution16, const double *error16, npr_snp_calls *out) {
    if (!b || n_refs < 0 || (n_refs && !ref_len) || !out) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return guarded(b->ctx, "npr_batch_snp_calls", [&](const Call &dev) -> int32_t {
        SnpModel m;
        SnpSource s;
        snp_calls_model(dev, n_models, evolution16, error16, m);
        snp_source_batch(dev, b, use, n_refs, ref_len, ref_code, s);
        return run_snp_calls(dev, s, ref_code, true_code, n_models, m, out);
    });
}

int32_t npr_pileup_snp_calls(npr_pileup *pl, const uint8_t *ref_code, const uint8_t *true_code, int32_t n_models, const double *evolution16,
                             const double *error16, npr_snp_calls *out) {
    if (!pl || !out) return NPR_ERR_INVALID;
    return guarded(pl->ctx, "npr_pileup_snp_calls", [&](const Call &dev) -> int32_t {
        SnpModel m;
        SnpSource s;
        snp_source_pileup(dev, pl, ref_code, s);
        snp_calls_model(dev, n_models, evolution16, error16, m);
        return run_snp_calls(dev, s, ref_code, true_code, n_models, m, out);
    });
}

int64_t npr_snp_variants_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code, const double *evolution16,
                               const double *error16, double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p,
                               int64_t cap, int64_t *n_calls) {
    if (!ctx) return NPR_ERR_INVALID;
    if (rows < 0 || (rows && (!weights || !seen || !ref_code))) return fail(ctx, NPR_ERR_INVALID, "npr_snp_variants_table: bad argument");
    return guarded(ctx, "npr_snp_variants_table", [&](const Call &dev) -> int64_t {
        SnpModel m;
        SnpSource s;
        snp_variants_model(dev, evolution16, error16, threshold, cap, n_calls, m);
        snp_source_table(dev, rows, weights, seen, s);
        return run_snp_variants(dev, s, ref_code, m, threshold, best, qual, call_row, call_alt, call_p, cap, n_calls);
    });
}

int64_t npr_batch_snp_variants(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code, const double *evolution16,
                               const double *error16, double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p,
                               int64_t cap, int64_t *n_calls) {
    if (!b || n_refs < 0 || (n_refs && !ref_len)) return NPR_ERR_INVALID;
    if (!b->finished) return NPR_ERR_STATE;
    return guarded(b->ctx, "npr_batch_snp_variants", [&](const Call &dev) -> int64_t {
        SnpModel m;
        SnpSource s;
        snp_variants_model(dev, evolution16, error16, threshold, cap, n_calls, m);
        snp_source_batch(dev, b, use, n_refs, ref_len, ref_code, s);
        return run_snp_variants(dev, s, ref_code, m, threshold, best, qual, call_row, call_alt, call_p, cap, n_calls);
    });
}

int64_t npr_pileup_snp_variants(npr_pileup *pl, const uint8_t *ref_code, const double *evolution16, const double *error16, double threshold, uint8_t *best,
                                uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls) {
    if (!pl) return NPR_ERR_INVALID;
    return guarded(pl->ctx, "npr_pileup_snp_variants", [&](const Call &dev) -> int64_t {
        SnpModel m;
        SnpSource s;
        snp_source_pileup(dev, pl, ref_code, s);
        snp_variants_model(dev, evolution16, error16, threshold, cap, n_calls, m);
        return run_snp_variants(dev, s, ref_code, m, threshold, best, qual, call_row, call_alt, call_p, cap, n_calls);
    });
}

}  // extern "C"
