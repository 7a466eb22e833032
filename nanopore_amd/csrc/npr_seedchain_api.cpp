// npr_seedchain_api.cpp -- the co-linear chains of seed rows as guide alignments on the device (npr_seedchain.hip), and the chains as the records
// chainSamFile writes (host code)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"
#include "npr_textout.h"

namespace npr_impl {

void SeedChainRun::count(const Call &dev, const int32_t *d_hits, int64_t rows, const SeedChainSpan *d_span, int64_t n_chains, int64_t max_gap, const int32_t *d_ref_len,
                         const int32_t *d_read_len) {
    dev.alloc(node, static_cast<size_t>(rows) * 4);
    dev.alloc(back, static_cast<size_t>(rows));
    dev.alloc(run_end, static_cast<size_t>(n_chains) * 4);
    dev.alloc(chains, static_cast<size_t>(n_chains) * 4);
    dev.alloc(n_ops, static_cast<size_t>(n_chains) + 1);
    a = SeedChainArgs{d_hits, d_span, n_chains, static_cast<uint32_t>(std::min<int64_t>(max_gap, UINT32_MAX)), d_ref_len, d_read_len, node.p, back.p,
                      run_end.p, chains.p, n_ops.p, nullptr};
    dev.launched(launch_seed_chain_dp(a, dev.ctx->stream), "k_chain_dp");
    dev.fetch(&pairs, n_ops.p + n_chains, sizeof(pairs));
    dev.sync();
}

void SeedChainRun::write(const Call &dev) {
    dev.alloc(ops, static_cast<size_t>(pairs) * 2);
    a.ops = ops.p;
    dev.launched(launch_seed_chain_write(a, dev.ctx->stream), "k_chain_trace");
}

}  // namespace npr_impl

namespace {

inline uint32_t strand_of(const int32_t *h) { return static_cast<uint32_t>(h[2]) >> 31; }
inline int64_t read_pos_of(const int32_t *h) { return static_cast<uint32_t>(h[2]) & 0x7fffffffu; }

// the (read, reference) pairs of one read's rows lo .. hi, which are sorted by (strand, reference, a, b): f(reference, first row and one past
// the last of the forward run, the same of the reverse run), in ascending reference index
template <typename F>
void for_each_span(const int32_t *hits, int64_t lo, int64_t hi, F f) {
    int64_t mid = lo;
    while (mid < hi && strand_of(hits + 4 * mid) == 0) ++mid;
    int64_t p = lo, q = mid;
    while (p < mid || q < hi) {
        const int32_t rp = p < mid ? hits[4 * p] : INT32_MAX, rq = q < hi ? hits[4 * q] : INT32_MAX, r = std::min(rp, rq);
        const int64_t p0 = p, q0 = q;
        while (p < mid && hits[4 * p] == r) ++p;
        while (q < hi && hits[4 * q] == r) ++q;
        f(r, p0, p, q0, q);
    }
}

// whether the rows of read i are what npr_seed_chains accepts
bool rows_valid(const int32_t *hits, int64_t lo, int64_t hi, int64_t read_len, int64_t n_refs, const int64_t *ref_len) {
    for (int64_t q = lo; q < hi; ++q) {
        const int32_t *h = hits + 4 * q;
        const int64_t r = h[0], a = h[1], b = read_pos_of(h), L = h[3];
        if (r < 0 || r >= n_refs || a < 0 || L < 1 || a + L > ref_len[r] || b + L > read_len) return false;
        if (q > lo) {
            const int32_t *g = h - 4;
            const int64_t kg[4] = {strand_of(g), g[0], g[1], read_pos_of(g)}, kh[4] = {strand_of(h), r, a, b};
            if (std::lexicographical_compare(kh, kh + 4, kg, kg + 4)) return false;
        }
    }
    return true;
}

}  // namespace

extern "C" {

int64_t npr_seed_chains(npr_ctx *ctx, int64_t max_gap, int64_t n_reads, const int64_t *read_len, int64_t n_refs, const int64_t *ref_len, const int64_t *hit_off,
                        const int32_t *hits, int64_t *chain_off, int32_t *chains, int64_t cap_chains, int64_t *ops_off, int32_t *ops, int64_t cap_ops) {
    if (!ctx) return NPR_ERR_INVALID;
    if (max_gap < 0) return fail(ctx, NPR_ERR_INVALID, "npr_seed_chains: a negative max_gap");
    if (n_reads < 0 || n_refs < 0 || cap_chains < 0 || cap_ops < 0 || !hit_off || !chain_off || (n_reads && !read_len) || (n_refs && !ref_len)) return NPR_ERR_INVALID;
    return guarded(ctx, "npr_seed_chains", [&](const Call &dev) -> int64_t {
        // everything is checked before anything is written or indexed with: the offsets, the lengths, then the rows read by read
        if (hit_off[0] != 0) return fail(ctx, NPR_ERR_INVALID, "npr_seed_chains: hit_off does not start at 0");
        for (int64_t i = 0; i < n_reads; ++i)
            if (hit_off[i + 1] < hit_off[i] || read_len[i] < 0 || read_len[i] > INT32_MAX) return fail(ctx, NPR_ERR_INVALID, "npr_seed_chains: row offsets decrease, or a read length outside 0 .. 2^31 - 1");
        for (int64_t r = 0; r < n_refs; ++r)
            if (ref_len[r] < 0 || ref_len[r] > INT32_MAX) return fail(ctx, NPR_ERR_INVALID, "npr_seed_chains: a reference length outside 0 .. 2^31 - 1");
        const int64_t total = hit_off[n_reads];
        if (total && !hits) return NPR_ERR_INVALID;
        std::vector<int64_t> first_chain(n_reads + 1, 0);  // (chain_off itself stays as it is until the rows have passed)
        std::atomic<int> bad{0};
        parallel_for((n_reads + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t i = c * 256, hi = std::min(n_reads, (c + 1) * 256); i < hi; ++i) {
                if (!rows_valid(hits, hit_off[i], hit_off[i + 1], read_len[i], n_refs, ref_len)) {
                    bad = 1;
                    return;
                }
                int64_t k = 0;
                for_each_span(hits, hit_off[i], hit_off[i + 1], [&](int32_t, int64_t, int64_t, int64_t, int64_t) { ++k; });
                first_chain[i + 1] = k;
            }
        });
        if (bad) return fail(ctx, NPR_ERR_INVALID, "npr_seed_chains: a row outside its read or its reference, of length 0, or out of (strand, reference, a, b) order");
        for (int64_t i = 0; i < n_reads; ++i) first_chain[i + 1] += first_chain[i];
        std::copy(first_chain.begin(), first_chain.end(), chain_off);
        const int64_t n_chains = first_chain[n_reads];
        if (n_chains == 0) {
            if (ops_off) ops_off[0] = 0;
            return 0;
        }
        if (!chains || !ops_off || n_chains > cap_chains) return fail(ctx, NPR_ERR_CAPACITY, "npr_seed_chains: more chains than the buffer holds (chain_off says how many)");

        std::vector<SeedChainSpan> span(static_cast<size_t>(n_chains));
        parallel_for((n_reads + 255) / 256, ctx->host_threads, [&](int64_t c) {
            for (int64_t i = c * 256, hi = std::min(n_reads, (c + 1) * 256); i < hi; ++i) {
                SeedChainSpan *s = span.data() + first_chain[i];
                for_each_span(hits, hit_off[i], hit_off[i + 1], [&](int32_t r, int64_t p0, int64_t p1, int64_t q0, int64_t q1) {
                    *s++ = SeedChainSpan{{p0, q0}, {static_cast<int32_t>(p1 - p0), static_cast<int32_t>(q1 - q0)}, static_cast<int32_t>(i), r};
                });
            }
        });
        std::vector<int32_t> len32(static_cast<size_t>(n_refs + n_reads));  // reference lengths, then read lengths
        std::copy(ref_len, ref_len + n_refs, len32.begin());
        std::copy(read_len, read_len + n_reads, len32.begin() + n_refs);

        // the upload, then the chain kernels on rows that lie on the device
        DevBuf<int32_t> d_hits, d_len;
        DevBuf<SeedChainSpan> d_span;
        dev.upload(d_hits, hits, static_cast<size_t>(total) * 4);
        dev.upload(d_len, len32);
        dev.upload(d_span, span);
        SeedChainRun run;
        run.count(dev, d_hits.p, total, d_span.p, n_chains, max_gap, d_len.p, d_len.p + n_refs);
        if (run.pairs > cap_ops || (run.pairs && !ops)) {
            ops_off[0] = run.pairs;
            return fail(ctx, NPR_ERR_CAPACITY, "npr_seed_chains: more op pairs than the buffer holds (ops_off[0] says how many)");
        }
        run.write(dev);
        dev.fetch(chains, run.chains.p, run.chains.bytes());
        dev.fetch(ops, run.ops.p, run.ops.bytes());
        dev.fetch(ops_off, run.n_ops.p, run.n_ops.bytes());
        dev.sync();
        return n_chains;
    });
}

int64_t npr_seed_chain_sam_text(int64_t n_reads, const uint8_t *text, const int64_t *name_span, const int64_t *begin, const int64_t *end, const char *rnames,
                                const int64_t *rname_off, int64_t n_refs, const int64_t *chain_off, const int32_t *chains, const int64_t *ops_off, const int32_t *ops,
                                int64_t *rec_off, char *out, int64_t cap) {
    if (n_reads < 0 || n_refs < 0 || !chain_off || !rec_off || (n_reads && (!text || !name_span || !begin || !end))) return NPR_ERR_INVALID;
    const int64_t total = chain_off[n_reads];
    if (chain_off[0] != 0 || total < 0 || (total && (!chains || !ops_off || !rnames || !rname_off))) return NPR_ERR_INVALID;
    if (total && (ops_off[0] != 0 || (ops_off[total] && !ops))) return NPR_ERR_INVALID;
    return guarded(nullptr, "npr_seed_chain_sam_text", [&](const Call &) -> int64_t {  // (host code)
        const int threads = usable_cpus();
        for (int64_t i = 0; i < n_reads; ++i)
            if (chain_off[i + 1] < chain_off[i] || end[i] < begin[i] || name_span[2 * i + 1] < name_span[2 * i]) return NPR_ERR_INVALID;
        // the reads by name (bytes; a shorter name before its extensions): their rank orders the records of one reference
        auto name_less = [&](int64_t x, int64_t y) {
            const int64_t nx = name_span[2 * x + 1] - name_span[2 * x], ny = name_span[2 * y + 1] - name_span[2 * y];
            const int c = std::memcmp(text + name_span[2 * x], text + name_span[2 * y], static_cast<size_t>(std::min(nx, ny)));
            return c != 0 ? c < 0 : nx < ny;
        };
        std::vector<int64_t> by_name(static_cast<size_t>(n_reads)), rank(static_cast<size_t>(n_reads));
        std::iota(by_name.begin(), by_name.end(), int64_t(0));
        std::sort(by_name.begin(), by_name.end(), name_less);
        for (int64_t k = 0; k < n_reads; ++k) {
            if (k && !name_less(by_name[k - 1], by_name[k])) return NPR_ERR_INVALID;  // two reads of one name
            rank[by_name[k]] = k;
        }
        // record k of the output is chain order[k]: sorted by (reference index, name)
        struct Key {
            int64_t ref, rank, chain, read;
        };
        std::vector<Key> order(static_cast<size_t>(total));
        std::atomic<int> bad{0};
        parallel_for((n_reads + 255) / 256, threads, [&](int64_t c) {
            for (int64_t i = c * 256, hi = std::min(n_reads, (c + 1) * 256); i < hi; ++i)
                for (int64_t q = chain_off[i]; q < chain_off[i + 1]; ++q) {
                    const int32_t *ch = chains + 4 * q;
                    if (ch[0] < 0 || ch[0] >= n_refs || (ch[1] != 0 && ch[1] != 1) || ops_off[q + 1] < ops_off[q]) bad = 1;
                    for (int64_t u = ops_off[q]; !bad && u < ops_off[q + 1]; ++u)
                        if (ops[2 * u] < 0 || ops[2 * u] > 8 || ops[2 * u + 1] < 0) bad = 1;
                    order[q] = Key{ch[0], rank[i], q, i};
                }
        });
        if (bad) return NPR_ERR_INVALID;
        std::sort(order.begin(), order.end(), [](const Key &x, const Key &y) { return x.ref != y.ref ? x.ref < y.ref : x.rank < y.rank; });
        // qname, flag, rname, "1", "255", cigar, "*", "0", "0", seq, "*"
        return format_records(total, threads, rec_off, out, cap, [&](int64_t k, auto &s) {
            const Key &o = order[k];
            const int64_t len = end[o.read] - begin[o.read];
            const bool reverse = chains[4 * o.chain + 1] != 0;
            s.bytes(text + name_span[2 * o.read], name_span[2 * o.read + 1] - name_span[2 * o.read]);
            s.ch('\t');
            s.num(reverse ? 16 : 0);
            s.ch('\t');
            s.bytes(rnames + rname_off[o.ref], rname_off[o.ref + 1] - rname_off[o.ref]);
            s.lit("\t1\t255\t");
            s.cigar_pairs(ops + 2 * ops_off[o.chain], ops_off[o.chain + 1] - ops_off[o.chain], kOpsSam);  // (looked at above, before the sort)
            s.lit("\t*\t0\t0\t");
            if (!reverse) {
                s.bytes(text + begin[o.read], len);
            } else {
                s.revcomp(text + begin[o.read], len);
            }
            s.lit("\t*\n");
            return true;
        });
    });
}

}  // extern "C"
