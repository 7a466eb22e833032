// bammerge_check.cpp -- the measure body and the virtual-offset search of csrc/npr_bamrec.h on the host (tests/test_bam_merge_host.py builds this
// with AddressSanitizer and UBSan and runs it on a case file it wrote).  The file: a uint32 count, then per record a uint32 n and the n bytes
// of one record (block_size included), each loaded into a heap buffer of exactly n bytes, so a read one byte outside it stops the program;
// then a uint32 number of block tables, per table a uint32 `blocks`, blocks + 1 int64 block offsets, blocks + 1 int64 stream offsets (both in
// heap buffers of exactly that size), a uint32 number of queries and that many int64 stream bytes u.
// Printed per record: its number, end, bin, size, refused; per query: "v", the table, the query, v(u).
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "npr_bamrec.h"

using namespace npr;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t records = 0, tables = 0;
    if (std::fread(&records, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < records; ++c) {
        uint32_t n;
        if (std::fread(&n, 4, 1, f) != 1 || n < 36) return 2;
        std::unique_ptr<uint8_t[]> rec(new uint8_t[n]);
        if (std::fread(rec.get(), 1, n, f) != n) return 2;
        BamRecMeasure m;
        bamrec_measure(rec.get(), m);
        std::printf("%u %lld %u %lld %d\n", c, static_cast<long long>(m.end), m.bin, static_cast<long long>(m.size), m.refused);
    }
    if (std::fread(&tables, 4, 1, f) != 1) return 2;
    for (uint32_t t = 0; t < tables; ++t) {
        uint32_t blocks, queries;
        if (std::fread(&blocks, 4, 1, f) != 1) return 2;
        std::unique_ptr<int64_t[]> block_off(new int64_t[blocks + 1]), stream_off(new int64_t[blocks + 1]);
        if (std::fread(block_off.get(), 8, blocks + 1, f) != blocks + 1 || std::fread(stream_off.get(), 8, blocks + 1, f) != blocks + 1) return 2;
        if (std::fread(&queries, 4, 1, f) != 1) return 2;
        for (uint32_t q = 0; q < queries; ++q) {
            int64_t u;
            if (std::fread(&u, 8, 1, f) != 1) return 2;
            std::printf("v %u %u %llu\n", t, q, bgzf_voffset_search(stream_off.get(), block_off.get(), blocks, u));
        }
    }
    std::fclose(f);
    std::printf("bammerge_check ok\n");
    return 0;
}
