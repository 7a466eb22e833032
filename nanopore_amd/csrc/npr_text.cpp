// npr_text.cpp -- cigar and SAM record text: the forms a job formats its output in (utils.py:597-605)
// (one of the translation units of the C ABI, include/nprealign.h; what they share: npr_api_internal.h)
#include "npr_api_internal.h"
#include "npr_textout.h"

static_assert(kTextErrInvalid == NPR_ERR_INVALID && kTextErrCapacity == NPR_ERR_CAPACITY, "npr_textout.h restates the codes of nprealign.h");

extern "C" {

int64_t npr_format_cigars(int64_t n, const int64_t *ops_off, const int32_t *ops, int64_t *str_off, char *out, int64_t cap) {
    if (n < 0 || (n && (!ops_off || !str_off)) || (n && ops_off[n] > 0 && !ops)) return NPR_ERR_INVALID;
    try {
        return format_records(n, usable_cpus(), str_off, out, cap,
                              [&](int64_t i, auto &s) { return s.cigar_pairs(ops + 2 * ops_off[i], ops_off[i + 1] - ops_off[i], kOpsMID); });
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_format_sam_records(int64_t n, const char *qnames, const int64_t *qname_off, const int32_t *flag, const char *rnames,
                               const int64_t *rname_off, const int32_t *ref_index, const int64_t *pos, const int32_t *mapq,
                               const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, const char *seq, const int64_t *seq_off,
                               int64_t *rec_off, char *out, int64_t cap) {
    if (n < 0 || (n && (!qnames || !qname_off || !rnames || !rname_off || !ref_index || !pos || !word_off || !n_ops || !seq || !seq_off || !rec_off)))
        return NPR_ERR_INVALID;
    try {
        return format_records(n, usable_cpus(), rec_off, out, cap, [&](int64_t i, auto &s) {
            const int64_t r = ref_index[i], sl = seq_off[i + 1] - seq_off[i];
            if (n_ops[i] < 0 || pos[i] < 0 || (flag && flag[i] < 0) || (mapq && mapq[i] < 0) || r < 0) return false;
            s.bytes(qnames + qname_off[i], qname_off[i + 1] - qname_off[i]);
            s.ch('\t');
            s.num(flag ? flag[i] : 0);
            s.ch('\t');
            s.bytes(rnames + rname_off[r], rname_off[r + 1] - rname_off[r]);
            s.ch('\t');
            s.num(pos[i]);
            s.ch('\t');
            s.num(mapq ? mapq[i] : 255);
            s.ch('\t');
            const bool ok = s.cigar_words(words + word_off[i], n_ops[i]);
            s.lit("\t*\t0\t0\t");
            if (sl == 0) s.ch('*');  // an empty SEQ is "*" in SAM
            s.bytes(seq + seq_off[i], sl);
            s.lit("\t*\n");
            return ok;
        });
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

int64_t npr_format_cigars_packed(int64_t n, const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, int64_t *str_off, char *out,
                                 int64_t cap) {
    if (n < 0 || (n && (!word_off || !n_ops || !str_off || !words))) return NPR_ERR_INVALID;
    try {
        return format_records(n, usable_cpus(), str_off, out, cap, [&](int64_t i, auto &s) { return s.cigar_words(words + word_off[i], n_ops[i]); });
    } catch (const std::exception &) {
        return NPR_ERR_NOMEM;
    }
}

void npr_encode_bases(const uint8_t *ascii, int64_t n, uint8_t *codes) {
    for (int64_t i = 0; i < n; ++i) codes[i] = encode_base(ascii[i]);
}

}  // extern "C"
