// The host side of the SAM -> BAM conversion (csrc/npr_bam_host.cpp: npr_sam_parse_tail, npr_bam_tags, npr_bam_header, npr_bai_write)
// under AddressSanitizer and UBSan: a host program (make -C nanopore_amd/csrc check-bam).  Every text is copied into a heap block of
// exactly its length and every output is a heap block of exactly the size the sizing call returned, so a parser that reads past a line
// or a writer that is longer than it said is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nprealign.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

namespace {

struct Heap {  // exactly n bytes
    char *p;
    int64_t n;
    explicit Heap(const std::string &s) : p(static_cast<char *>(std::malloc(s.size() ? s.size() : 1))), n(static_cast<int64_t>(s.size())) { std::memcpy(p, s.data(), s.size()); }
    ~Heap() { std::free(p); }
};

// the tags of one line: the bytes, or the error code as a one-byte string "!"
std::string tags_of(const std::string &tags, int32_t *status = nullptr) {
    const std::string body = std::string("r\t0\tchr1\t1\t9\t4M\t=\t5\t-3\tACGT\tIIII") + (tags.empty() ? "" : "\t" + tags);
    const Heap text(body);
    const char names[] = "chr1chr2";
    const int64_t name_off[3] = {0, 4, 8};
    int64_t span[2] = {0, text.n}, fields[NPR_SAM_COLS], tail[NPR_SAM_TAIL_COLS], off[2];
    CHECK(npr_sam_parse(text.p, span, 1, names, name_off, 2, fields) == NPR_OK);
    CHECK(npr_sam_parse_tail(text.p, span, fields, 1, names, name_off, 2, tail) == NPR_OK);
    CHECK(tail[7] == NPR_OK && tail[0] == 0 && tail[1] == 4 && tail[2] == -3 && tail[4] - tail[3] == 4 && tail[6] == text.n);
    const int64_t total = npr_bam_tags(text.p, tail, 1, off, nullptr, 0);
    if (status) *status = total < 0 ? static_cast<int32_t>(total) : NPR_OK;
    if (total < 0) return "!";
    std::vector<uint8_t> out(static_cast<size_t>(total));  // exactly
    if (total) CHECK(npr_bam_tags(text.p, tail, 1, off, out.data(), total - 1) == NPR_ERR_CAPACITY);
    CHECK(npr_bam_tags(text.p, tail, 1, off, out.data(), total) == total && off[0] == 0 && off[1] == total);
    return std::string(out.begin(), out.end());
}

std::string le(uint64_t v, int w) {
    std::string s;
    for (int k = 0; k < w; ++k) s += static_cast<char>(v >> (8 * k));
    return s;
}

}  // namespace

int main() {
    // tags: every type, the integer widths at their edges, malformed fields
    CHECK(tags_of("").empty());
    CHECK(tags_of("XA:A:q") == "XAAq");
    CHECK(tags_of("XZ:Z:a b") == std::string("XZZa b\0", 7) && tags_of("XH:H:0aF1") == std::string("XHH0aF1\0", 8));
    const struct { long long v; char t; int w; } ints[] = {{-129, 's', 2}, {-128, 'c', 1}, {127, 'C', 1}, {128, 'C', 1}, {255, 'C', 1}, {256, 'S', 2}, {65535, 'S', 2},
                                                           {65536, 'I', 4}, {2147483647LL, 'I', 4}, {2147483648LL, 'I', 4}, {-2147483648LL, 'i', 4}, {4294967295LL, 'I', 4}};
    for (const auto &c : ints) CHECK(tags_of("XI:i:" + std::to_string(c.v)) == std::string("XI") + c.t + le(static_cast<uint64_t>(c.v), c.w));
    CHECK(tags_of("XF:f:1.5") == std::string("XFf") + le(0x3fc00000u, 4));
    CHECK(tags_of("XB:B:s,-2,3") == std::string("XBBs") + le(2, 4) + le(0xfffe, 2) + le(3, 2));
    CHECK(tags_of("XB:B:f") == std::string("XBBf") + le(0, 4) && tags_of("XB:B:f,0.5") == std::string("XBBf") + le(1, 4) + le(0x3f000000u, 4));
    CHECK(tags_of("NM:i:1\tXZ:Z:") == std::string("NMC\1XZZ\0", 8));
    for (const char *bad : {"X:i:1", "XX:i:", "XX:i:1.5", "XX:i:4294967296", "XX:i:-2147483649", "XX:q:1", "XX:A:ab", "XX:A:", "XX:f:x", "XX:H:ABC", "XX:B:c,128", "XX:B:",
                            "XX:B:c,", "XX:B:c1", "XX:i:1\t", "XX:i:1\t\tYY:i:2", "XX"}) {
        int32_t status = 0;
        (void)tags_of(bad, &status);
        CHECK(status == NPR_ERR_INVALID);
    }

    // the tail parser on lines that end where the heap block ends: 10 columns, a short QUAL, CRLF is the indexer's business (no "\r" in a span)
    {
        const char names[] = "chr1";
        const int64_t name_off[2] = {0, 4};
        for (const char *line : {"r\t0\tchr1\t1\t9\t4M\t*\t0\t0\tACGT", "r\t0\tchr1\t1\t9\t4M\t*\t0\t0\tACGT\tIII", "r\t0\tchr1\t1\t9\t4M\t*\t0\t0\t*\tI", "r", "",
                                 "r\t0\tchr1\t1\t9\t4M\t*\t0\tx\tACGT\tIIII", "r\t70000\tchr1\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "\t0\tchr1\t1\t9\t4M\t*\t0\t0\tACGT\tIIII"}) {
            const Heap text(line);
            int64_t span[2] = {0, text.n}, fields[NPR_SAM_COLS], tail[NPR_SAM_TAIL_COLS], off[2];
            CHECK(npr_sam_parse(text.p, span, 1, names, name_off, 1, fields) == NPR_OK);
            CHECK(npr_sam_parse_tail(text.p, span, fields, 1, names, name_off, 1, tail) == NPR_OK);
            CHECK(tail[7] == NPR_ERR_INVALID);
            CHECK(npr_bam_tags(text.p, tail, 1, off, nullptr, 0) == 0);
        }
        const Heap ok("r\t4\t*\t0\t0\t*\tchr1\t9\t0\t*\t*\tXX:i:-1");
        int64_t span[2] = {0, ok.n}, fields[NPR_SAM_COLS], tail[NPR_SAM_TAIL_COLS];
        CHECK(npr_sam_parse(ok.p, span, 1, names, name_off, 1, fields) == NPR_OK && fields[15] == NPR_SAM_NO_REFERENCE);
        CHECK(npr_sam_parse_tail(ok.p, span, fields, 1, names, name_off, 1, tail) == NPR_OK && tail[7] == NPR_OK && tail[0] == 0 && tail[1] == 8);
    }

    // the header
    {
        const std::string sq = "@SQ\tSN:chr1\tLN:1000\n@SQ\tLN:5\tSN:b\n";
        for (const std::string &head : {std::string(""), std::string("@HD\tVN:1.4\n"), std::string("@HD\tVN:1.4\tSO:queryname\n"), std::string("@HD\tSO:unknown\tVN:1.4\n")}) {
            const Heap text(head + sq);
            int64_t n_refs = 0, len[2] = {0, 0};
            const int64_t total = npr_bam_header(text.p, text.n, 1, nullptr, 0, &n_refs, nullptr, 0);
            CHECK(total > 0 && n_refs == 2);
            std::vector<uint8_t> out(static_cast<size_t>(total));
            CHECK(npr_bam_header(text.p, text.n, 1, out.data(), total - 1, &n_refs, len, 2) == NPR_ERR_CAPACITY);
            CHECK(npr_bam_header(text.p, text.n, 1, out.data(), total, &n_refs, len, 1) == NPR_ERR_CAPACITY);
            CHECK(npr_bam_header(text.p, text.n, 1, out.data(), total, &n_refs, len, 2) == total && len[0] == 1000 && len[1] == 5);
            const std::string got(out.begin(), out.end());
            CHECK(got.compare(0, 4, "BAM\1") == 0 && got.find("SO:coordinate") != std::string::npos && got.find("queryname") == std::string::npos);
            CHECK(got.substr(got.size() - 10) == le(2, 4) + std::string("b\0", 2) + le(5, 4));
        }
        for (const char *bad : {"", "@HD\tVN:1.0\n", "@SQ\tSN:a\n", "@SQ\tLN:5", "@SQ\tSN:a\tLN:0\n", "@SQ\tSN:a\tLN:"}) {
            const Heap text(bad);
            int64_t n_refs = 0;
            CHECK(npr_bam_header(text.p, text.n, 0, nullptr, 0, &n_refs, nullptr, 0) == NPR_ERR_INVALID);
        }
    }

    // the BAI writer: tables of exactly their sizes
    {
        const uint64_t none = ~uint64_t(0);
        const std::vector<int64_t> ref_len = {40000, 10, 100000};
        const std::vector<int32_t> run_tid = {0, 0, 0, 2, -1};
        const std::vector<uint32_t> run_bin = {0, 4681, 4681, 4683, 4680};
        const std::vector<uint64_t> run_beg = {5, 100, 300, 400, 900}, run_end = {100, 200, 400, 900, 950};
        const std::vector<uint64_t> linear = {none, 100, 300, none, none, none, 400, none, none, none, none};
        const std::vector<uint64_t> meta = {5, 400, 3, 1, none, 0, 0, 0, 400, 900, 2, 0};
        const int64_t total = npr_bai_write(3, ref_len.data(), 5, run_tid.data(), run_bin.data(), run_beg.data(), run_end.data(), linear.data(), meta.data(), 4, nullptr, 0);
        // magic + n_ref; ref 0: 3 bins (1 + 2 chunks) + pseudo-bin + 3 windows; ref 1: nothing; ref 2: 1 bin + pseudo-bin + 3 windows; n_no_coor
        CHECK(total == 8 + (4 + 8 + 16 + 8 + 32 + 8 + 32 + 4 + 24) + (4 + 4) + (4 + 8 + 16 + 8 + 32 + 4 + 24) + 8);
        std::vector<uint8_t> out(static_cast<size_t>(total));
        CHECK(npr_bai_write(3, ref_len.data(), 5, run_tid.data(), run_bin.data(), run_beg.data(), run_end.data(), linear.data(), meta.data(), 4, out.data(), total - 1) == NPR_ERR_CAPACITY);
        CHECK(npr_bai_write(3, ref_len.data(), 5, run_tid.data(), run_bin.data(), run_beg.data(), run_end.data(), linear.data(), meta.data(), 4, out.data(), total) == total);
        CHECK(std::memcmp(out.data(), "BAI\1", 4) == 0 && out[total - 8] == 4);
        const std::vector<int32_t> unordered = {2, 0};
        CHECK(npr_bai_write(3, ref_len.data(), 2, unordered.data(), run_bin.data(), run_beg.data(), run_end.data(), linear.data(), meta.data(), 0, nullptr, 0) == NPR_ERR_INVALID);
        CHECK(npr_bai_write(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) == 16);
    }
    std::printf("bam_host_sanitize: ok\n");
    return 0;
}
