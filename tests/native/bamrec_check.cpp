// bamrec_check.cpp -- csrc/npr_bamrec.h on the host (tests/test_bam_pileup_host.py builds this with AddressSanitizer and UBSan and runs it on
// a case file it wrote).  The file: a uint32 count, then per case int32 flag_mask, uint32 n_ref, n_ref int64 reference lengths, uint32 n and
// the n bytes of one record (block_size included).  Every record is loaded into a heap buffer of exactly n bytes, so a read one byte outside
// it stops the program, and checked with the n bytes as what is available; a record that ends with its bytes (block_size + 4 = n) is
// checked again as a record cut short by the stream's end, with n - 1, which must be refused for its parts without a byte past n - 1 being
// read (the buffer then has n - 1 bytes).
// Printed per case: the verdict, why, whether the operations are a CG field's, their number, the reference and read bases they consume.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "npr_bamrec.h"

using namespace npr;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < cases; ++c) {
        int32_t flag_mask;
        uint32_t n_ref, n;
        if (std::fread(&flag_mask, 4, 1, f) != 1 || std::fread(&n_ref, 4, 1, f) != 1) return 2;
        std::vector<int64_t> ref_len(n_ref);
        if (n_ref && std::fread(ref_len.data(), 8, n_ref, f) != n_ref) return 2;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        std::unique_ptr<uint8_t[]> rec(new uint8_t[n]);
        if (n && std::fread(rec.get(), 1, n, f) != n) return 2;
        BamRecVerdict v;
        std::memset(&v, 0xEE, sizeof(v));
        bamrec_check(rec.get(), n, ref_len.data(), n_ref, flag_mask, v);
        int32_t size = -1;
        if (n >= 4) std::memcpy(&size, rec.get(), 4);
        if (n >= 4 && size >= 0 && 4 + static_cast<int64_t>(size) == n) {  // (the record ends with its bytes)
            std::unique_ptr<uint8_t[]> cut(new uint8_t[n - 1]);
            std::memcpy(cut.get(), rec.get(), n - 1);
            BamRecVerdict w;
            bamrec_check(cut.get(), n - 1, ref_len.data(), n_ref, flag_mask, w);
            if (w.verdict != BR_REFUSED || w.why != BR_WHY_PARTS) {
                std::printf("bamrec_check: case %u: a record cut by one byte is not refused for its parts: %d %d\n", c, w.verdict, w.why);
                return 1;
            }
        }
        std::printf("%u %d %d %d %lld %lld %lld\n", c, v.verdict, v.why, v.from_cg, static_cast<long long>(v.n_ops), static_cast<long long>(v.ref_sum),
                    static_cast<long long>(v.read_sum));
    }
    std::fclose(f);
    std::printf("bamrec_check ok\n");
    return 0;
}
