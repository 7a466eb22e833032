// The FASTQ scanners of npr_io.cpp (npr_fastq_index, npr_fastq_qual_index) under AddressSanitizer and UBSan: a host program
// (make -C nanopore_amd/csrc check-fastqqual).  Every text is copied into a heap block of exactly its length, so a scanner that
// reads one byte past the end is caught; the spans are compared with the lines of the text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nprealign.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, const std::string &text) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s on text of %zu bytes\n", what, text.size());
        ++failures;
    }
}

// the quality lines the scanner must find (records: how many npr_fastq_index must count)
void check(const std::string &text, const std::vector<std::string> &want) {
    char *heap = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));
    std::memcpy(heap, text.data(), text.size());
    const int64_t len = static_cast<int64_t>(text.size());
    const int64_t n = npr_fastq_index(heap, len, nullptr, 0);
    expect(n == static_cast<int64_t>(want.size()), "record count", text);
    if (n == static_cast<int64_t>(want.size())) {
        std::vector<int64_t> rec(4 * want.size() + 1), qual(2 * want.size() + 1, -7);
        expect(npr_fastq_index(heap, len, rec.data(), n) == n, "index", text);
        expect(npr_fastq_qual_index(heap, len, rec.data(), n, qual.data()) == NPR_OK, "quality index", text);
        for (size_t k = 0; k < want.size(); ++k) {
            const int64_t a = qual[2 * k], b = qual[2 * k + 1];
            expect(a >= 0 && a <= b && b <= len && std::string(heap + a, heap + b) == want[k], "quality line", text);
        }
        expect(qual[2 * want.size()] == -7, "nothing written past the last record", text);
    }
    std::free(heap);
}

}  // namespace

int main() {
    check("@r0 first\nACGT\n+r0 first\nIIII\n@r1\n\n+\n\n@r2\r\nAC\r\n+\r\n#5\r\n@r3\nACGTN\n+\n!~ZZ@", {"IIII", "", "#5", "!~ZZ@"});
    check("@r0\nACGT\n+\nIIII\n", {"IIII"});
    check("@r0\nACGT\n+\n", {""});       // the last record cut off after its '+' line
    check("@r0\nACGT\n+", {""});         // ... inside it
    check("@r0\nACGT\n+\nII", {"II"});   // ... inside its quality line
    check("@r0\nACGT\n+\nIIII\r", {"IIII"});
    check("\n\n@r0\nA\n+\n#\n\n\n@r1\nC\n+x\n$\n", {"#", "$"});
    check("", {});
    {  // spans that npr_fastq_index did not give are refused without a read outside the text
        const std::string text = "@r0\nACGT\n+\nIIII\n";
        char *heap = static_cast<char *>(std::malloc(text.size()));
        std::memcpy(heap, text.data(), text.size());
        const int64_t len = static_cast<int64_t>(text.size());
        int64_t qual[2] = {-7, -7};
        const int64_t past[4] = {1, 3, 4, len + 1}, reversed[4] = {1, 3, 8, 4}, negative[4] = {1, 3, -1, 4}, no_plus[4] = {1, 3, 0, 2}, at_end[4] = {1, 3, len, len};
        for (const int64_t *rec : {past, reversed, negative, no_plus, at_end})
            expect(npr_fastq_qual_index(heap, len, rec, 1, qual) == NPR_ERR_INVALID, "a refused record", text);
        std::free(heap);
    }
    if (failures) return 1;
    std::puts("fastq_qual_sanitize: ok");
    return 0;
}
