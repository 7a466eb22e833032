// inflate_check.cpp -- csrc/npr_inflate.h on the host (tests/test_inflate_host.py builds this with AddressSanitizer and UBSan and runs it on
// a case file it wrote).  The file: a uint32 count, then per case uint32 n, isize, crc and n bytes of deflate data.  Every case is loaded
// into heap buffers of exactly n and isize bytes, so a read or write one byte outside either stops the program, and is decoded twice through
// the loop the kernel runs (inflate_member, one lane): with the whole data as its window, and with a window of 2 048 bytes that has to be
// refilled.  Printed per case: the status (INF_CRC when the decode is fine and the output's CRC-32 is not the case's), the bytes produced
// and the CRC-32 of the output.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "npr_inflate.h"

using namespace npr;

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

struct NoSync {
    void operator()() const {}
};

struct Result {
    int status;
    uint32_t produced, crc;
};

static Result run(const uint8_t *body, uint32_t n, uint32_t isize, uint32_t want_crc, uint32_t window) {
    std::unique_ptr<uint8_t[]> out(new uint8_t[isize]), win(new uint8_t[window]);
    std::memset(out.get(), 0xA5, isize);
    std::unique_ptr<Inflate> s(new Inflate);
    std::memset(s.get(), 0xEE, sizeof(Inflate));
    inflate_member(*s, body, n, out.get(), isize, win.get(), window, 0, 1, NoSync());
    Result r{s->status, s->produced, 0};
    if (r.produced > isize) {
        std::printf("inflate_check: produced %u of %u\n", r.produced, isize);
        std::exit(1);
    }
    r.crc = crc32_of(out.get(), r.produced);
    if (r.status == INF_OK && r.crc != want_crc) r.status = INF_CRC;
    return r;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t head[3];
        if (std::fread(head, 4, 3, f) != 3) return 2;
        const uint32_t n = head[0], isize = head[1], crc = head[2];
        std::unique_ptr<uint8_t[]> body(new uint8_t[n]);
        if (n && std::fread(body.get(), 1, n, f) != n) return 2;
        const Result whole = run(body.get(), n, isize, crc, n > 2 * INF_MARGIN ? n : 2 * INF_MARGIN);
        const Result small = run(body.get(), n, isize, crc, 2 * INF_MARGIN);
        if (whole.status != small.status || whole.produced != small.produced || whole.crc != small.crc) {
            std::printf("inflate_check: case %u: the two windows disagree: %d %u %08x / %d %u %08x\n", c, whole.status, whole.produced, whole.crc, small.status,
                        small.produced, small.crc);
            return 1;
        }
        std::printf("%u %d %u %u\n", c, whole.status, whole.produced, whole.crc);
    }
    std::fclose(f);
    std::printf("inflate_check ok\n");
    return 0;
}
