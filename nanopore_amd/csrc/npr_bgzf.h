// npr_bgzf.h -- what the two BGZF kernels share on the device (k_bgzf_frame in npr_bam.hip: stored blocks; k_bgzf_deflate in
// npr_deflate.hip: compressed blocks): little-endian stores, the block header, and the CRC-32 of a block's payload by a workgroup of 256
// threads (the method: the head of npr_bam.hip).
#ifndef NPR_BGZF_H
#define NPR_BGZF_H
#include <hip/hip_runtime.h>

#include "npr_device.h"

namespace npr {

constexpr int BGZF_THREADS = 256;
constexpr uint32_t BGZF_CRC_POLY = 0xEDB88320u;

__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {  // a * b modulo the polynomial, reflected: bit 31 is x^0
    uint32_t p = 0;
#pragma unroll 4
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ BGZF_CRC_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t x_pow_bytes(const uint32_t *x2n, uint32_t bytes) {  // x^(8 * bytes)
    uint32_t p = 0x80000000u;
    for (int k = 3; bytes; bytes >>= 1, ++k)
        if (bytes & 1) p = gf_mul(x2n[k & 31], p);
    return p;
}
__device__ __forceinline__ void put16(uint8_t *p, uint32_t v) { p[0] = static_cast<uint8_t>(v), p[1] = static_cast<uint8_t>(v >> 8); }
__device__ __forceinline__ void put32(uint8_t *p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v), p[1] = static_cast<uint8_t>(v >> 8), p[2] = static_cast<uint8_t>(v >> 16), p[3] = static_cast<uint8_t>(v >> 24);
}

// the 18 bytes before a block's deflate data; block_len = the whole block's length
__device__ __forceinline__ void bgzf_put_header(uint8_t *out, uint32_t block_len) {
    const uint8_t head[12] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0};
    for (int k = 0; k < 12; ++k) out[k] = head[k];
    out[12] = 'B', out[13] = 'C', out[14] = 2, out[15] = 0;
    put16(out + 16, block_len - 1);
}

__device__ __forceinline__ void bgzf_put_eof(uint8_t *out, int thread) {
    if (thread < BGZF_EOF) {
        const uint8_t eof[BGZF_EOF] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        out[thread] = eof[thread];
    }
}

// CRC-32 of in[0, L), L <= BGZF_PAYLOAD, by the whole workgroup (every thread calls; the value comes back to every thread).  LDS: table[256],
// t_crc[256], t_len[256]; they are free again on return.
__device__ __forceinline__ uint32_t bgzf_crc(const uint8_t *in, uint32_t L, const BgzfArgs &a, uint32_t *table, uint32_t *t_crc, uint32_t *t_len) {
    {
        uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BGZF_CRC_POLY : c >> 1;
        table[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t lo = min(L, threadIdx.x * BGZF_SLICE), hi = min(L, lo + BGZF_SLICE);
    uint32_t c = threadIdx.x == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t k = lo; k < hi; ++k) c = table[(c ^ in[k]) & 0xff] ^ (c >> 8);
    t_crc[threadIdx.x] = c, t_len[threadIdx.x] = hi - lo;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        const uint32_t step = 1u << k;
        if ((threadIdx.x & (2 * step - 1)) == 0) {
            const uint32_t rl = t_len[threadIdx.x + step];
            if (rl) {
                const uint32_t m = rl == BGZF_SLICE * step ? a.level[k] : x_pow_bytes(a.x2n, rl);
                t_crc[threadIdx.x] = gf_mul(t_crc[threadIdx.x], m) ^ t_crc[threadIdx.x + step];
                t_len[threadIdx.x] += rl;
            }
        }
        __syncthreads();
    }
    const uint32_t crc = ~t_crc[0];
    __syncthreads();
    return crc;
}

}  // namespace npr
#endif
