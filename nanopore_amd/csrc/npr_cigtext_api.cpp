// npr_cigtext_api.cpp -- cigar text made on the device (npr_cigtext.hip): npr_cigar_text_packed, npr_batch_cigar_text, and the text the
// device MEA stage hands over under NPR_OPT_FINISH_TEXT (utils.py:597-605: the writer loop's `aR.cigar = ...`)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"

namespace npr_impl {
namespace {

// what the text kernels need besides the words: offsets, the scan's scratch, the flag; and the text when nobody lends a buffer
struct TextBufs {
    DevBuf<int64_t> off, tile;
    DevBuf<int32_t> bad;
    DevBuf<char> text;
    char *text_p = nullptr;
};

// Lengths, offsets and (want_text) the text of n lists whose words are on the device.  str_off[n + 1] is on the host when the call returns;
// the text stays on the device at bufs.text_p -- in `lend` (lend_bytes) when it fits there.  An op outside M I D is refused (NPR_ERR_INVALID);
// false: want_text and the total is above cap (the offsets are valid then).  Nothing is written in either case.
bool run_cigtext(const Call &dev, int64_t n, const int64_t *d_word_off, const int64_t *d_n_ops, const uint32_t *d_words, bool want_text, int64_t cap, char *lend,
                 size_t lend_bytes, TextBufs &bufs, int64_t *str_off) {
    dev.alloc_cached(bufs.off, n + 1);
    dev.alloc_cached(bufs.tile, scan_tiles(n));
    dev.alloc_cached(bufs.bad, 1);
    dev.zero(bufs.bad.p, sizeof(int32_t));
    CigTextArgs a{n, d_word_off, d_n_ops, d_words, bufs.off.p, bufs.tile.p, bufs.bad.p, nullptr};
    dev.launched(launch_cigtext_offsets(a, dev.ctx->stream), "k_cigtext_len / scan");
    int32_t bad = 0;
    dev.fetch(str_off, bufs.off.p, sizeof(int64_t) * (n + 1));
    dev.fetch(&bad, bufs.bad.p, sizeof(int32_t));
    dev.sync();
    if (bad) dev.refuse(NPR_ERR_INVALID, "cigar text: an operation outside M / I / D");
    if (!want_text) return true;
    const int64_t total = str_off[n];
    if (cap < total) return false;
    if (static_cast<size_t>(total) <= lend_bytes) {
        bufs.text_p = lend;
    } else {
        dev.alloc_cached(bufs.text, total);
        bufs.text_p = bufs.text.p;
    }
    a.out = bufs.text_p;
    dev.launched(launch_cigtext_write(a, dev.ctx->stream), "k_cigtext_write");
    return true;
}

void keep_text(const Call &dev, npr_batch *b, const TextBufs &bufs, std::vector<int64_t> &off) {
    const int64_t total = off[b->n_reads];
    if (total > b->text_cap) b->text.reset(new char[total + total / 8]), b->text_cap = total + total / 8;
    // through the context's pinned staging in pieces of 4 MiB
    const PiecedFetch fetch{bufs.text_p, b->text.get(), total, 1, 4 << 20, 256,
                            [](void *dst, const void *pin, int64_t lo, int64_t hi) {
                                std::memcpy(static_cast<char *>(dst) + lo, static_cast<const char *>(pin) + lo, static_cast<size_t>(hi - lo));
                            },
                            "cigar text: hipHostMalloc", "cigar text: D2H"};
    dev.passed(fetch_pieced(b->ctx, fetch));
    b->text_off.swap(off);
    b->text_ready = true;
}

// The text of a batch whose packed words (offsets d_off[n + 1]) are on the device, to b->text and b->text_off.  `lend`: device memory the text
// may use (lend_bytes).  The stream is drained when it returns.
void words_text(const Call &dev, npr_batch *b, const int64_t *d_off, const uint32_t *d_words, char *lend, size_t lend_bytes) {
    std::vector<int64_t> off(b->n_reads + 1, 0);
    TextBufs bufs;
    run_cigtext(dev, b->n_reads, d_off, nullptr, d_words, true, INT64_MAX, lend, lend_bytes, bufs, off.data());
    keep_text(dev, b, bufs, off);
}

// the text of a finished batch on the host (b->text, b->text_off), made once: from the packed words where the device MEA stage left them
// while they are still there, else from the batch's host form, uploaded
void ensure_text(const Call &dev, npr_batch *b) {
    if (b->text_ready) return;
    npr_ctx *ctx = b->ctx;
    const int64_t n = b->n_reads;
    if (n == 0) {
        std::vector<int64_t> off(1, 0);
        return keep_text(dev, b, TextBufs{}, off);
    }
    {
        std::unique_lock<std::mutex> arena_lock(ctx->arena->mu);  // the resident cigars lie in the arena
        if (b->dev_ops && b->dev_ops_epoch == ctx->arena->epoch) return words_text(dev, b, b->dev_od, b->dev_ops, nullptr, 0);  // (the lock goes after it)
    }
    if (b->words_on_device && !b->have_packed_form) dev.passed(fetch_device_words(b));  // (fails: the words are gone)
    ensure_packed_form(b);
    const int64_t words = b->ops_off[n];
    DevBuf<uint32_t> d_words;
    DevBuf<int64_t> d_off;
    dev.alloc_cached(d_words, std::max<int64_t>(words, 1));
    dev.alloc_cached(d_off, n + 1);
    dev.copy_up(d_words.p, b->packed.get(), sizeof(uint32_t) * static_cast<size_t>(words));
    dev.copy_up(d_off.p, b->ops_off.data(), sizeof(int64_t) * (n + 1));
    words_text(dev, b, d_off.p, d_words.p, nullptr, 0);
}

}  // namespace

// what npr_finish.cpp calls under NPR_OPT_FINISH_TEXT
int32_t device_words_text(npr_batch *b, const int64_t *d_off, const uint32_t *d_words, char *lend, size_t lend_bytes) {
    return guarded(b->ctx, "cigar text", [&](const Call &dev) -> int32_t {
        words_text(dev, b, d_off, d_words, lend, lend_bytes);
        return NPR_OK;
    });
}

// a batch finished with NPR_OPT_FINISH_TEXT has its packed words on the device only: to the host while they are still there
int32_t fetch_device_words(npr_batch *b) {
    npr_ctx *ctx = b->ctx;
    return guarded(ctx, "packed cigars", [&](const Call &dev) -> int32_t {
        const int64_t total = b->ops_off[b->n_reads];
        std::unique_lock<std::mutex> arena_lock(ctx->arena->mu);
        if (!(b->dev_ops && b->dev_ops_epoch == ctx->arena->epoch))
            return fail(ctx, NPR_ERR_STATE, "the batch was finished with NPR_OPT_FINISH_TEXT and its packed cigars have since been overwritten on the device: "
                                            "fetch them before the next batch is finished, or use npr_batch_cigar_text");
        if (total > b->packed_cap) b->packed.reset(new uint32_t[total]), b->packed_cap = total;
        dev.fetch(b->packed.get(), b->dev_ops, sizeof(uint32_t) * static_cast<size_t>(total));
        dev.sync();
        b->have_packed_form = true;
        return NPR_OK;
    });
}

}  // namespace npr_impl

extern "C" {

int64_t npr_cigar_text_packed(npr_ctx *ctx, int64_t n, const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, int64_t *str_off,
                              char *out, int64_t cap) {
    if (!ctx) return NPR_ERR_INVALID;
    if (n < 0 || (n && (!word_off || !n_ops || !str_off || !words))) return fail(ctx, NPR_ERR_INVALID, "npr_cigar_text_packed: bad argument");
    return guarded(ctx, "npr_cigar_text_packed", [&](const Call &dev) -> int64_t {
        if (n == 0) {
            if (str_off) str_off[0] = 0;
            return 0;
        }
        // the part of `words` the lists cover goes up, the offsets relative to it
        int64_t lo = INT64_MAX, hi = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (n_ops[i] < 0 || (n_ops[i] && word_off[i] < 0)) return fail(ctx, NPR_ERR_INVALID, "npr_cigar_text_packed: a negative count or offset");
            if (n_ops[i]) lo = std::min(lo, word_off[i]), hi = std::max(hi, word_off[i] + n_ops[i]);
        }
        if (hi == 0) lo = 0;
        std::vector<int64_t> rel(n);
        for (int64_t i = 0; i < n; ++i) rel[i] = n_ops[i] ? word_off[i] - lo : 0;
        DevBuf<uint32_t> d_words;
        DevBuf<int64_t> d_off, d_nops;
        dev.alloc_cached(d_words, std::max<int64_t>(hi - lo, 1));
        dev.alloc_cached(d_off, n);
        dev.alloc_cached(d_nops, n);
        dev.copy_up(d_words.p, words + lo, sizeof(uint32_t) * static_cast<size_t>(hi - lo));
        dev.copy_up(d_off.p, rel.data(), sizeof(int64_t) * n);
        dev.copy_up(d_nops.p, n_ops, sizeof(int64_t) * n);
        std::vector<int64_t> off(n + 1, 0);
        TextBufs bufs;
        const bool fits = run_cigtext(dev, n, d_off.p, d_nops.p, d_words.p, out != nullptr, cap, nullptr, 0, bufs, off.data());  // (an op outside M I D: str_off is not written either)
        std::copy(off.begin(), off.end(), str_off);
        if (!fits) return NPR_ERR_CAPACITY;
        if (out) {
            dev.fetch(out, bufs.text_p, static_cast<size_t>(off[n]));
            dev.sync();
        }
        return off[n];
    });
}

int64_t npr_batch_cigar_text(npr_batch *b, int64_t *str_off, char *out, int64_t cap) {
    if (!b || !str_off) return NPR_ERR_INVALID;
    if (!b->finished) return fail(b->ctx, NPR_ERR_STATE, "npr_batch_cigar_text before npr_batch_finish");
    return guarded(b->ctx, "npr_batch_cigar_text", [&](const Call &dev) -> int64_t {
        ensure_text(dev, b);
        std::copy(b->text_off.begin(), b->text_off.end(), str_off);
        const int64_t total = b->text_off[b->n_reads];
        if (!out) return total;
        if (cap < total) return NPR_ERR_CAPACITY;
        const char *src = b->text.get();
        const int64_t chunk = 4 << 20, nchunks = (total + chunk - 1) / chunk;
        parallel_for(nchunks, b->ctx->host_threads, [&](int64_t c) {
            std::memcpy(out + c * chunk, src + c * chunk, static_cast<size_t>(std::min(total, (c + 1) * chunk) - c * chunk));
        });
        return total;
    });
}

}  // extern "C"
