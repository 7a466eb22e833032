// npr_inflate.hip -- the BGZF blocks of a file inflated on the device (the ABI: include/nprealign.h, npr_bgzf_inflate; the host side: npr_bam_api.cpp;
// the block table comes from npr_bgzf_scan, host code).  Integers only.
//   k_bgzf_inflate   one workgroup of BGZF_THREADS threads inflates one BGZF block (a workgroup takes every gridDim.x-th block), in these steps:
//     header         every thread reads the block's XLEN, CRC-32 and ISIZE; the deflate data is what lies between the extra field and the
//                    trailer.  ISIZE must be at most 65 536 and what the block table says (INF_ISIZE), the parts must fit the block (INF_INPUT).
//     decode         inflate_member (npr_inflate.h, the loop the host test runs under AddressSanitizer): lane 0 decodes headers and symbols
//                    from a window of the deflate data in LDS that all threads refill from global memory; all threads clear and fill the two
//                    look-up tables of a block's codes and copy stored blocks.  The payload is built in LDS: a match reads LDS.  Symbol
//                    decoding is serial by the format's nature; the blocks of the file are the parallelism.
//     CRC            bgzf_crc (npr_bgzf.h, shared with the writers) over the first BGZF_PAYLOAD bytes; a block of up to 65 536 bytes (other
//                    writers make them) has at most 256 more, which thread 0 adds with the same byte table.
//     store          only when the block's status is INF_OK: the payload to stream + stream_off[b], four bytes a thread where stream_off[b] is a
//                    multiple of four (it is, for full blocks of BGZF_PAYLOAD bytes), else byte by byte; consecutive threads, consecutive addresses.
//     status         status[b] = the block's INF_ status.  Every read of the file is checked against the block and every write against ISIZE
//                    before it happens (npr_inflate.h); a corrupt block costs bounded time and changes nothing but its status.
// LDS of k_bgzf_inflate (two workgroups a CU): the payload 65 536 + the window 8 192 (after the decode: the CRC's three tables of 1 KiB) + the
// decoder's state (npr_inflate.h Inflate: bit buffer, code lengths, per code the counts, canonical order and a look-up table of 1 024 entries).
#include <hip/hip_runtime.h>

#include "npr_bgzf.h"
#include "npr_device.h"
#include "npr_inflate.h"

namespace npr {
namespace {

constexpr int THREADS = BGZF_THREADS;
constexpr int O_PAY = 0, O_WIN = O_PAY + static_cast<int>(INF_MAX_ISIZE), WIN_BYTES = 8192, O_STATE = O_WIN + WIN_BYTES;
constexpr int LDS_BYTES = O_STATE + static_cast<int>(sizeof(Inflate));
static_assert(LDS_BYTES <= 80 * 1024, "two workgroups share a CU's LDS");
static_assert(O_STATE % 8 == 0 && alignof(Inflate) <= 8 && WIN_BYTES >= 3 * 1024 && WIN_BYTES >= 2 * static_cast<int>(INF_MARGIN), "the layout");

struct GroupSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

__device__ __forceinline__ uint32_t get32(const uint8_t *p) {
    return p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}

__global__ void __launch_bounds__(THREADS) k_bgzf_inflate(InflateArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    uint8_t *const pay = lds + O_PAY;
    uint8_t *const win = lds + O_WIN;
    uint32_t *const tab = reinterpret_cast<uint32_t *>(lds + O_WIN);
    Inflate &s = *reinterpret_cast<Inflate *>(lds + O_STATE);
    const uint32_t t = threadIdx.x;
    for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        __syncthreads();  // the block before is done with the LDS
        const uint8_t *const blk = a.file + a.block_off[b];
        const int64_t size = a.block_off[b + 1] - a.block_off[b], want = a.stream_off[b + 1] - a.stream_off[b];
        int status = INF_OK;
        uint32_t n = 0, isize = 0, crc_want = 0;
        const uint8_t *body = blk;
        if (size < 12 + 8 || size > 65536) {
            status = INF_INPUT;
        } else {
            const int64_t xlen = blk[10] | static_cast<int64_t>(blk[11]) << 8;
            if (12 + xlen + 8 > size) {
                status = INF_INPUT;
            } else {
                body = blk + 12 + xlen, n = static_cast<uint32_t>(size - 12 - xlen - 8);
                crc_want = get32(blk + size - 8), isize = get32(blk + size - 4);
                if (isize > INF_MAX_ISIZE || static_cast<int64_t>(isize) != want) status = INF_ISIZE;
            }
        }
        // (status is the same in every thread from here on: it comes from the arguments, then from LDS after a barrier)
        if (status == INF_OK) {
            inflate_member(s, body, n, pay, isize, win, static_cast<uint32_t>(WIN_BYTES), t, static_cast<uint32_t>(THREADS), GroupSync());
            status = s.status;
        }
        if (status == INF_OK) {
            const uint32_t head = min(isize, static_cast<uint32_t>(BGZF_PAYLOAD));
            uint32_t crc = bgzf_crc(pay, head, a.z, tab, tab + 256, tab + 512);
            if (isize > head) {  // (bgzf_crc leaves its byte table in tab[0 .. 256) and is done with the rest)
                if (t == 0) {
                    uint32_t c = ~crc;
                    for (uint32_t k = head; k < isize; ++k) c = tab[(c ^ pay[k]) & 0xff] ^ (c >> 8);
                    tab[256] = ~c;
                }
                __syncthreads();
                crc = tab[256];
            }
            if (crc != crc_want) status = INF_CRC;
        }
        if (status == INF_OK) {
            const int64_t at = a.stream_off[b];
            uint8_t *const to = a.stream + at;
            if ((at & 3) == 0) {  // (the stream's buffer is aligned as hipMalloc aligns, the payload in LDS to 16 bytes)
                const uint32_t words = isize / 4;
                for (uint32_t k = t; k < words; k += THREADS) reinterpret_cast<uint32_t *>(to)[k] = reinterpret_cast<const uint32_t *>(pay)[k];
                for (uint32_t k = 4 * words + t; k < isize; k += THREADS) to[k] = pay[k];
            } else {
                for (uint32_t k = t; k < isize; k += THREADS) to[k] = pay[k];
            }
        }
        if (t == 0) a.status[b] = status;
    }
}

}  // namespace

int launch_bgzf_inflate(const InflateArgs &a, void *stream) {
    if (a.blocks <= 0) return 0;
    const int64_t groups = a.blocks < INFLATE_MAX_GROUPS ? a.blocks : INFLATE_MAX_GROUPS;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(static_cast<unsigned>(groups)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
