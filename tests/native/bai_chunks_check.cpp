// bai_chunks_check.cpp -- npr_bai_chunks (csrc/npr_bam_host.cpp) on the host (tests/test_bai_chunks_host.py builds this with AddressSanitizer
// and UBSan and runs it on a case file it wrote).  The file: a uint32 count, then per case int32 tid, int64 beg, int64 end, uint32 n and the n
// bytes of one BAI image.  Every image is loaded into a heap buffer of exactly n bytes, so a read one byte outside it stops the program.
// Per case the function is called three times: for the count alone, with room for exactly that many chunks, and -- when there is a chunk --
// with room for one fewer, which must give NPR_ERR_CAPACITY; the arrays are filled with a pattern first and must keep it wherever the
// function says it wrote nothing.
// Printed per case: the case, the return value, n_ref (-1: not set), then the chunks as beg end pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "nprealign.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    const uint64_t pattern = 0xA5A5A5A5A5A5A5A5ull;
    for (uint32_t c = 0; c < cases; ++c) {
        int32_t tid;
        int64_t beg, end;
        uint32_t n;
        if (std::fread(&tid, 4, 1, f) != 1 || std::fread(&beg, 8, 1, f) != 1 || std::fread(&end, 8, 1, f) != 1 || std::fread(&n, 4, 1, f) != 1) return 2;
        std::unique_ptr<uint8_t[]> bai(new uint8_t[n ? n : 1]);
        if (n && std::fread(bai.get(), 1, n, f) != n) return 2;
        int64_t n_ref = -1;
        const int64_t count = npr_bai_chunks(bai.get(), n, tid, beg, end, nullptr, nullptr, 0, &n_ref);
        std::printf("%u %lld %lld", c, static_cast<long long>(count), static_cast<long long>(n_ref));
        const size_t room = count > 0 ? static_cast<size_t>(count) : 0;
        std::vector<uint64_t> cb(room + 1, pattern), ce(room + 1, pattern);
        int64_t again = -1;
        const int64_t filled = npr_bai_chunks(bai.get(), n, tid, beg, end, cb.data(), ce.data(), static_cast<int64_t>(room), &again);
        if (filled != count || again != n_ref || cb[room] != pattern || ce[room] != pattern) {
            std::printf("\nbai_chunks_check: case %u: the filling call gives %lld after %lld, or writes past its room\n", c, static_cast<long long>(filled), static_cast<long long>(count));
            return 1;
        }
        for (size_t k = 0; k < room; ++k) std::printf(" %llu %llu", static_cast<unsigned long long>(cb[k]), static_cast<unsigned long long>(ce[k]));
        std::printf("\n");
        if (room) {
            std::vector<uint64_t> sb(room, pattern), se(room, pattern);
            const int64_t small = npr_bai_chunks(bai.get(), n, tid, beg, end, sb.data(), se.data(), static_cast<int64_t>(room) - 1, &again);
            bool untouched = true;
            for (size_t k = 0; k < room; ++k) untouched = untouched && sb[k] == pattern && se[k] == pattern;
            if (small != NPR_ERR_CAPACITY || !untouched) {
                std::printf("bai_chunks_check: case %u: room for one chunk fewer gives %lld, or something was written\n", c, static_cast<long long>(small));
                return 1;
            }
        }
    }
    std::fclose(f);
    std::printf("bai_chunks_check ok\n");
    return 0;
}
