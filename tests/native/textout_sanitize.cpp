// textout_sanitize.cpp -- the record writer (csrc/npr_textout.h) and the formatters that compile without HIP under AddressSanitizer and
// UBSan: every output buffer is a heap block of exactly the computed size, so a record that is longer than the counting sink said is a
// heap-buffer-overflow report, and one that is shorter fails the comparison.  A host program, built and run on the CPU by
// `make -C nanopore_amd/csrc check-textout` (g++, with npr_io.cpp: the two splices).  With -DNPR_WITH_TEXT_CPP and npr_text.cpp on the line
// (hipcc -x hip -Xarch_host -fsanitize=address,undefined), its three formatters run too.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nprealign.h"
#include "npr_textout.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

// run lengths across every digit boundary of the packed form: 0, 9, 10, 99, 100, ... 10^9, 2^30 - 1
std::vector<int64_t> boundary_lengths() {
    std::vector<int64_t> v{0};
    for (int64_t p = 10; p <= INT64_C(1000000000); p *= 10) v.push_back(p - 1), v.push_back(p);
    v.push_back((INT64_C(1) << 30) - 1);
    return v;
}

std::string cigar_of(const std::vector<int32_t> &pairs, const char *letters) {
    std::string s;
    for (size_t q = 0; q < pairs.size(); q += 2) s += std::to_string(pairs[q + 1]) + letters[pairs[q]];
    return s.empty() ? "*" : s;
}

std::string revcomp_of(const std::string &seq) {
    std::string r(seq.rbegin(), seq.rend());
    for (char &c : r) {
        const char *from = "ACGTacgt", *to = "TGCAtgca";
        for (int k = 0; k < 8; ++k)
            if (c == from[k]) {
                c = to[k];
                break;
            }
    }
    return r;
}

// format_records into a block of exactly the size the sizing call returned, then one byte short
template <typename Call>
void exact_fill(int64_t n, const std::vector<std::string> &want, Call call) {
    std::string all;
    for (const std::string &r : want) all += r;
    std::vector<int64_t> off(static_cast<size_t>(n) + 1, -7);
    const int64_t total = call(off.data(), nullptr, 0);
    EXPECT(total == static_cast<int64_t>(all.size()));
    if (total < 0) return;
    EXPECT(off[n] == total);
    char *out = static_cast<char *>(std::malloc(static_cast<size_t>(total) + (total == 0)));
    EXPECT(call(off.data(), out, total) == total);
    EXPECT(std::string(out, static_cast<size_t>(total)) == all);
    for (int64_t i = 0; i < n; ++i) EXPECT(off[i + 1] - off[i] == static_cast<int64_t>(want[i].size()));
    std::free(out);
    if (total > 0) {
        char *small = static_cast<char *>(std::malloc(static_cast<size_t>(total) - 1 + (total == 1)));
        EXPECT(call(off.data(), small, total - 1) == NPR_ERR_CAPACITY);  // (and not a byte written: the block is one short)
        std::free(small);
    }
}

// every member of the sinks in one record shape, over the driver: numbers of every width, both cigar forms and tables, literals, bytes,
// reverse complements
void sinks() {
    const std::vector<int64_t> lens = boundary_lengths();
    std::vector<int64_t> numbers = lens;
    for (int64_t v : {INT64_C(2147483647), INT64_C(9999999999), INT64_C(10000000000), INT64_C(999999999999999999), INT64_C(1000000000000000000), INT64_MAX}) numbers.push_back(v);
    std::vector<uint32_t> words;
    std::vector<int32_t> mid, sam;
    for (size_t k = 0; k < lens.size(); ++k) {
        words.push_back(static_cast<uint32_t>(lens[k]) << 2 | static_cast<uint32_t>(k % 3));
        mid.push_back(static_cast<int32_t>(k % 3)), mid.push_back(static_cast<int32_t>(lens[k]));
        sam.push_back(static_cast<int32_t>(k % 9)), sam.push_back(static_cast<int32_t>(lens[k]));
    }
    sam.push_back(8), sam.push_back(INT32_MAX);
    const std::string seq = "ACGTNacgtnRYKM-*";
    const int64_t n = static_cast<int64_t>(numbers.size());
    std::vector<std::string> want;
    for (int64_t i = 0; i < n; ++i) {
        // record i takes the first i operations of each list (record 0: none, "*") and the first i % 17 bases
        const size_t m = std::min<size_t>(static_cast<size_t>(i), lens.size()), b = static_cast<size_t>(i % 17);
        want.push_back(std::to_string(numbers[i]) + "\t" + cigar_of(std::vector<int32_t>(mid.begin(), mid.begin() + 2 * m), "MID") + "\t*\t0\t0\t" +
                       cigar_of(std::vector<int32_t>(mid.begin(), mid.begin() + 2 * m), "MID") + ";" +
                       cigar_of(std::vector<int32_t>(sam.begin(), sam.begin() + 2 * std::min<size_t>(static_cast<size_t>(i), sam.size() / 2)), "MIDNSHP=X") + seq.substr(0, b) +
                       revcomp_of(seq.substr(0, b)) + "\n");
    }
    for (int threads : {1, 3})
        exact_fill(n, want, [&](int64_t *off, char *out, int64_t cap) {
            return npr::format_records(n, threads, off, out, cap, [&](int64_t i, auto &s) {
                const int64_t m = std::min<int64_t>(i, static_cast<int64_t>(lens.size())), b = i % 17;
                s.num(numbers[i]);
                s.ch('\t');
                bool ok = s.cigar_words(words.data(), m);
                s.lit("\t*\t0\t0\t");
                ok = s.cigar_pairs(mid.data(), m, npr::kOpsMID) && ok;
                s.ch(';');
                ok = s.cigar_pairs(sam.data(), std::min<int64_t>(i, static_cast<int64_t>(sam.size() / 2)), npr::kOpsSam) && ok;
                s.bytes(seq.data(), b);
                s.revcomp(reinterpret_cast<const uint8_t *>(seq.data()), b);
                s.ch('\n');
                return ok;
            });
        });
    // an invalid record: nothing is written, not even the offsets
    std::vector<int64_t> off(3, -7);
    char *one = static_cast<char *>(std::malloc(1));
    *one = 'x';
    const uint32_t bad_word = 5u << 2 | 3u;
    const int32_t bad_pairs[3][2] = {{9, 5}, {-1, 5}, {0, -1}};
    EXPECT(npr::format_records(2, 2, off.data(), one, 1, [&](int64_t i, auto &s) { return s.cigar_words(&bad_word, i); }) == NPR_ERR_INVALID);
    for (const auto &p : bad_pairs) EXPECT(npr::format_records(2, 2, off.data(), one, 1, [&](int64_t i, auto &s) { return s.cigar_pairs(p, i, npr::kOpsSam); }) == NPR_ERR_INVALID);
    EXPECT(npr::format_records(2, 2, off.data(), one, 1, [&](int64_t, auto &s) { return s.cigar_pairs(bad_pairs[0], 1, npr::kOpsSam); }) == NPR_ERR_INVALID);
    EXPECT(*one == 'x' && off[0] == -7 && off[1] == -7 && off[2] == -7);
    EXPECT(npr::format_records(0, 2, off.data(), one, 0, [&](int64_t, auto &) { return false; }) == 0 && off[0] == 0);
    std::free(one);
}

// the two splices of npr_io.cpp: lines with their CIGAR column replaced
void splices() {
    const std::vector<int64_t> lens = boundary_lengths();
    const std::vector<std::string> head{"r0\t0\tchr1\t1\t60\t", "\t4\t*\t0\t0\t", "r2\t16\tchr2\t2147483647\t255\t", "last\t0\tchr1\t9\t9\t"},
        old_cigar{"5M", "*", "3M1I2D7M", "1M"}, tail{"\t*\t0\t0\tACGTA\tIIIII\tNM:i:0", "\t*\t0\t0\t*\t*", "\t=\t7\t-9\tacgtn\t*", "\t*\t0\t0\tA\t*\tXX:Z:a tag\twith\ttabs"};
    const int64_t n = static_cast<int64_t>(head.size());
    std::string text = "@HD\tVN:1.0\n";
    std::vector<int64_t> span, fields(static_cast<size_t>(n) * NPR_SAM_COLS, 0);
    for (int64_t i = 0; i < n; ++i) {
        span.push_back(static_cast<int64_t>(text.size()));
        fields[i * NPR_SAM_COLS + 3] = static_cast<int64_t>(text.size() + head[i].size());
        fields[i * NPR_SAM_COLS + 4] = fields[i * NPR_SAM_COLS + 3] + static_cast<int64_t>(old_cigar[i].size());
        text += head[i] + old_cigar[i] + tail[i];
        span.push_back(static_cast<int64_t>(text.size()));
        text += i == 1 ? "\r\n" : "\n";
    }
    // packed lists: every length, none, the largest alone, three short ones -- laid out in reverse order
    std::vector<std::vector<int32_t>> lists(4);
    for (size_t k = 0; k < lens.size(); ++k) lists[0].push_back(static_cast<int32_t>(k % 3)), lists[0].push_back(static_cast<int32_t>(lens[k]));
    lists[2] = {0, (1 << 30) - 1};
    lists[3] = {1, 9, 2, 10, 0, 0};
    std::vector<uint32_t> words;
    std::vector<int64_t> word_off(4), n_ops(4);
    for (int i = 3; i >= 0; --i) {
        word_off[i] = static_cast<int64_t>(words.size()), n_ops[i] = static_cast<int64_t>(lists[i].size() / 2);
        for (size_t q = 0; q < lists[i].size(); q += 2) words.push_back(static_cast<uint32_t>(lists[i][q + 1]) << 2 | static_cast<uint32_t>(lists[i][q]));
    }
    std::vector<std::string> want, cigars;
    for (int64_t i = 0; i < n; ++i) cigars.push_back(cigar_of(lists[i], "MID")), want.push_back(head[i] + cigars.back() + tail[i] + "\n");
    exact_fill(n, want, [&](int64_t *off, char *out, int64_t cap) {
        return npr_sam_splice(text.data(), span.data(), fields.data(), n, word_off.data(), n_ops.data(), words.data(), off, out, cap);
    });
    exact_fill(0, {}, [&](int64_t *off, char *out, int64_t cap) {
        return npr_sam_splice(text.data(), span.data(), fields.data(), 0, word_off.data(), n_ops.data(), words.data(), off, out, cap);
    });
    // no operation anywhere and no words
    std::vector<std::string> starred;
    const std::vector<int64_t> none(4, 0);
    for (int64_t i = 0; i < n; ++i) starred.push_back(head[i] + "*" + tail[i] + "\n");
    exact_fill(n, starred, [&](int64_t *off, char *out, int64_t cap) {
        return npr_sam_splice(text.data(), span.data(), fields.data(), n, word_off.data(), none.data(), nullptr, off, out, cap);
    });
    // the same cigars as text; then no text at all
    std::string ctext;
    std::vector<int64_t> str_off{0};
    for (const std::string &c : cigars) ctext += c, str_off.push_back(static_cast<int64_t>(ctext.size()));
    exact_fill(n, want, [&](int64_t *off, char *out, int64_t cap) {
        return npr_sam_splice_text(text.data(), span.data(), fields.data(), n, str_off.data(), ctext.data(), off, out, cap);
    });
    std::vector<std::string> bare;
    const std::vector<int64_t> flat(static_cast<size_t>(n) + 1, 5);
    for (int64_t i = 0; i < n; ++i) bare.push_back(head[i] + tail[i] + "\n");
    exact_fill(n, bare, [&](int64_t *off, char *out, int64_t cap) {
        return npr_sam_splice_text(text.data(), span.data(), fields.data(), n, flat.data(), nullptr, off, out, cap);
    });
    std::vector<int64_t> off(static_cast<size_t>(n) + 1);
    words[static_cast<size_t>(word_off[3]) + 1] |= 3u;
    EXPECT(npr_sam_splice(text.data(), span.data(), fields.data(), n, word_off.data(), n_ops.data(), words.data(), off.data(), nullptr, 0) == NPR_ERR_INVALID);
    EXPECT(npr_sam_splice(text.data(), span.data(), fields.data(), n, word_off.data(), n_ops.data(), nullptr, off.data(), nullptr, 0) == NPR_ERR_INVALID);
    str_off[2] = str_off[1] - 1;
    EXPECT(npr_sam_splice_text(text.data(), span.data(), fields.data(), n, str_off.data(), ctext.data(), off.data(), nullptr, 0) == NPR_ERR_INVALID);
}

#ifdef NPR_WITH_TEXT_CPP
// the three formatters of npr_text.cpp
void cigars_and_records() {
    const std::vector<int64_t> lens = boundary_lengths();
    std::vector<std::vector<int32_t>> lists(5);
    for (size_t k = 0; k < lens.size(); ++k) lists[1].push_back(static_cast<int32_t>(k % 3)), lists[1].push_back(static_cast<int32_t>(lens[k]));
    lists[3] = {2, (1 << 30) - 1};
    lists[4] = {1, 9, 0, 10};
    const int64_t n = static_cast<int64_t>(lists.size());
    std::vector<int32_t> ops;
    std::vector<uint32_t> words;
    std::vector<int64_t> ops_off{0}, word_off, n_ops;
    std::vector<std::string> want;
    for (const auto &l : lists) {
        word_off.push_back(static_cast<int64_t>(words.size())), n_ops.push_back(static_cast<int64_t>(l.size() / 2));
        for (size_t q = 0; q < l.size(); q += 2) words.push_back(static_cast<uint32_t>(l[q + 1]) << 2 | static_cast<uint32_t>(l[q]));
        ops.insert(ops.end(), l.begin(), l.end());
        ops_off.push_back(static_cast<int64_t>(ops.size() / 2));
        want.push_back(cigar_of(l, "MID"));
    }
    exact_fill(n, want, [&](int64_t *off, char *out, int64_t cap) { return npr_format_cigars(n, ops_off.data(), ops.data(), off, out, cap); });
    exact_fill(n, want, [&](int64_t *off, char *out, int64_t cap) { return npr_format_cigars_packed(n, word_off.data(), n_ops.data(), words.data(), off, out, cap); });
    // records: numbers at 0 and at their largest values, an empty name, an empty SEQ
    const std::vector<std::string> qname{"read/0", "", "r", "another read", std::string(300, 'x')}, seq{"ACGTNacgtn", "", "A", "", std::string(400, 'c')}, ref{"chr1", "", "a reference with words"};
    const std::vector<int32_t> flag{0, INT32_MAX, 16, 99, 100}, mapq{0, INT32_MAX, 9, 10, 255}, ref_index{0, 2, 1, 0, 2};
    const std::vector<int64_t> pos{0, INT64_MAX, 9, 10, INT64_C(1000000000000000000)};
    std::string qn, sq, rn;
    std::vector<int64_t> qoff{0}, soff{0}, roff{0};
    for (int64_t i = 0; i < n; ++i) qn += qname[i], qoff.push_back(static_cast<int64_t>(qn.size())), sq += seq[i], soff.push_back(static_cast<int64_t>(sq.size()));
    for (const std::string &r : ref) rn += r, roff.push_back(static_cast<int64_t>(rn.size()));
    for (int with = 0; with < 2; ++with) {
        std::vector<std::string> rec;
        for (int64_t i = 0; i < n; ++i)
            rec.push_back(qname[i] + "\t" + std::to_string(with ? flag[i] : 0) + "\t" + ref[ref_index[i]] + "\t" + std::to_string(pos[i]) + "\t" + std::to_string(with ? mapq[i] : 255) + "\t" + want[i] +
                          "\t*\t0\t0\t" + (seq[i].empty() ? "*" : seq[i]) + "\t*\n");
        exact_fill(n, rec, [&](int64_t *off, char *out, int64_t cap) {
            return npr_format_sam_records(n, qn.data(), qoff.data(), with ? flag.data() : nullptr, rn.data(), roff.data(), ref_index.data(), pos.data(), with ? mapq.data() : nullptr,
                                          word_off.data(), n_ops.data(), words.data(), sq.data(), soff.data(), off, out, cap);
        });
    }
}
#endif

}  // namespace

int main() {
    sinks();
    splices();
#ifdef NPR_WITH_TEXT_CPP
    cigars_and_records();
#endif
    std::printf(failures ? "%d checks failed\n" : "textout: clean\n", failures);
    return failures ? 1 : 0;
}
