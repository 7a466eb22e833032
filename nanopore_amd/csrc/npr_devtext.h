// npr_devtext.h -- the digit helpers of the device text writers (npr_cigtext.hip: cigar text of packed cigars; npr_bamread.hip: the SAM lines of
// BAM records).  Included by .hip units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace npr {

__device__ __forceinline__ int digits30(uint32_t v) {  // decimal digits of v < 2^30
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ int digits32(uint32_t v) { return v >= 1000000000u ? 10 : digits30(v); }  // of any uint32 (digits30 counts to ten already)
// the k = digits32(v) digits of v at p[0 .. k)
__device__ __forceinline__ void put_digits(uint8_t *p, uint32_t v, int k) {
    for (int j = k - 1; j >= 0; --j) p[j] = static_cast<uint8_t>('0' + v % 10u), v /= 10u;
}
// a signed 32-bit number as text: its length, and the text at p
__device__ __forceinline__ int signed_len(int32_t v) { return v < 0 ? 1 + digits32(0u - static_cast<uint32_t>(v)) : digits32(static_cast<uint32_t>(v)); }
__device__ __forceinline__ int put_signed(uint8_t *p, int32_t v) {
    const uint32_t m = v < 0 ? 0u - static_cast<uint32_t>(v) : static_cast<uint32_t>(v);
    const int k = digits32(m);
    if (v < 0) *p++ = '-';
    put_digits(p, m, k);
    return k + (v < 0 ? 1 : 0);
}

}  // namespace npr
