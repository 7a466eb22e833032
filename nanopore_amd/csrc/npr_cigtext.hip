// npr_cigtext.hip -- k_cigtext_len, the scan of the lengths (npr_scan.h), k_cigtext_write: the SAM CIGAR text of packed
// cigars (one word per operation, length << 2 | op) where the words lie in HBM -- the per-record text work of the reference's writer loop
// (nanopore/analyses/utils.py:597-605: `aR.cigar = ...; outputSam.write(aR)`, pysam's cigarstring grammar: decimal length, then M / I / D, "*" for
// an empty cigar).  Byte for byte what npr_format_cigars_packed (npr_text.cpp) writes on the host; include/nprealign.h: npr_cigar_text_packed,
// npr_batch_cigar_text, NPR_OPT_FINISH_TEXT.
//
// Three steps, all integer work, ordinary vector stores only, no atomics: the output does not depend on the order anything runs in.
//   lengths  k_cigtext_len: one wavefront per list, a lane per operation 64 at a time; the list's length is the sum of (decimal digits + 1), 1 for an
//            empty list.  An operation code 3 sets *bad (every writer stores the same 1).
//   offsets  the exclusive running sum of the n lengths, in place, as int64 (a batch's text can pass 2^31 bytes): the tiled scan of
//            npr_scan.h (tile sums; their running sum in one workgroup with a carry; every tile on top of its offset).  On the device and
//            not on the host: the host has to wait for the total before it can size the text's buffers whichever side scans, and with the scan
//            here that wait fetches what the caller is given anyway (the offsets, 8 bytes per list) and nothing goes back up -- a host scan would
//            fetch the lengths and upload the offsets before the write pass could start.  The two were not timed against each other.
//   write    k_cigtext_write: one wavefront (a workgroup of its own) per list, tiles of 256 operations, four consecutive ones per lane.  A lane
//            counts its operations' digits by comparison with the powers of ten (lengths go up to 2^30 - 1: one to ten digits), one wavefront prefix
//            sum places the lanes in the tile, a running pointer joins the tiles.  The digits come from divisions by the constant ten (a multiply
//            and a shift).  The tile's bytes are put together in LDS, shifted by the destination's misalignment so that LDS dword j is the j-th
//            aligned dword of the destination, and leave as whole dwords, lane after lane (256 B per store instruction); only the up to three
//            bytes before the first and after the last whole dword of a tile go out as single bytes -- bytes of a dword two tiles or two lists
//            share are never written by a dword store.  2.8 KiB of LDS per workgroup: the wavefront slots, not the LDS, bound the occupancy.
//            A list of 10^5 operations is 400 tiles on one wavefront; a batch has thousands of lists, so the chip is full without cutting lists up.
// NOT MEASURED on hardware yet (tools/cigar_text_time.py -> profiles/cigar_text_time.json is the tool): the kernels' times, the bytes written per second
// against the 6.3 TB/s an MI355X streams, whether NPR_OPT_FINISH_TEXT pays; ds_write_b8 per output byte is the first thing to look at if the write pass
// turns out to be bound by the LDS and not by HBM.
#include <hip/hip_runtime.h>

#include "npr_device.h"
#include "npr_devtext.h"

namespace npr {
namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int OPS_PER_LANE = 4;
constexpr int TILE_OPS = WAVE * OPS_PER_LANE;
constexpr int TILE_BYTES = 3 + 11 * TILE_OPS;  // up to three bytes of misalignment, ten digits and a letter per operation

__device__ __forceinline__ int wave_scan(int v, int lane) {  // inclusive
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ int64_t list_ops(const CigTextArgs &a, int64_t i) { return a.n_ops ? a.n_ops[i] : a.word_off[i + 1] - a.word_off[i]; }

__global__ void __launch_bounds__(THREADS) k_cigtext_len(CigTextArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * WAVES + wv; i < a.n; i += static_cast<int64_t>(gridDim.x) * WAVES) {
        const int64_t m = list_ops(a, i);
        const uint32_t *src = a.words + a.word_off[i];
        int64_t k = 0;
        int other = 0;
        for (int64_t q = lane; q < m; q += WAVE) {
            const uint32_t w = src[q];
            other |= (w & 3u) == 3u;
            k += digits30(w >> 2) + 1;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) k += __shfl_xor(k, o, WAVE), other |= __shfl_xor(other, o, WAVE);
        if (lane == 0) {
            a.str_off[i] = k ? k : 1;  // an empty cigar is "*"
            if (other) *a.bad = 1;
        }
    }
}

// ---- the text ----
__global__ void __launch_bounds__(WAVE) k_cigtext_write(CigTextArgs a) {
    __shared__ uint32_t buf[(TILE_BYTES + 3) / 4];
    uint8_t *const bytes = reinterpret_cast<uint8_t *>(buf);
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const int64_t m = list_ops(a, i);
        char *dst = a.out + a.str_off[i];
        if (m <= 0) {
            if (lane == 0) *dst = '*';
            continue;
        }
        const uint32_t *src = a.words + a.word_off[i];
        for (int64_t base = 0; base < m; base += TILE_OPS) {
            uint32_t w[OPS_PER_LANE];
            int k[OPS_PER_LANE], s = 0;
#pragma unroll
            for (int q = 0; q < OPS_PER_LANE; ++q) {
                const int64_t at = base + OPS_PER_LANE * lane + q;
                w[q] = at < m ? src[at] : 0u;
                k[q] = at < m ? digits30(w[q] >> 2) + 1 : 0;
                s += k[q];
            }
            const int inc = wave_scan(s, lane);
            const int total = __shfl(inc, WAVE - 1, WAVE);
            const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 3u);  // LDS byte p is destination byte p - mis
            int p = mis + inc - s;
#pragma unroll
            for (int q = 0; q < OPS_PER_LANE; ++q) {
                if (k[q] == 0) continue;
                uint32_t v = w[q] >> 2;
                for (int j = k[q] - 2; j >= 0; --j) bytes[p + j] = static_cast<uint8_t>('0' + v % 10u), v /= 10u;
                const uint32_t op = w[q] & 3u;
                bytes[p + k[q] - 1] = op == 0u ? 'M' : (op == 1u ? 'I' : 'D');
                p += k[q];
            }
            __syncthreads();
            const int end = mis + total;
            char *const g0 = dst - mis;  // 4-byte aligned
            const int head_end = mis ? min(4, end) : 0, last_full = end >> 2;
            for (int j = (mis ? 1 : 0) + lane; j < last_full; j += WAVE) reinterpret_cast<uint32_t *>(g0)[j] = buf[j];
            if (mis + lane < head_end) g0[mis + lane] = static_cast<char>(bytes[mis + lane]);
            const int tail = max(4 * last_full, head_end) + lane;
            if (lane < 3 && tail < end) g0[tail] = static_cast<char>(bytes[tail]);
            dst += total;
            __syncthreads();  // (the next tile overwrites the buffer)
        }
    }
}

}  // namespace

int launch_cigtext_offsets(const CigTextArgs &a, void *stream) {
    if (a.n < 0) return static_cast<int>(hipErrorInvalidValue);
    const int64_t groups = (a.n + WAVES - 1) / WAVES;
    const int grid = static_cast<int>(groups < 1 ? 1 : (groups < (1 << 20) ? groups : (1 << 20)));
    hipLaunchKernelGGL(k_cigtext_len, dim3(grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launch_scan_tiled<int64_t, int64_t>(a.str_off, a.str_off, a.n, a.tile, stream);
}

int launch_cigtext_write(const CigTextArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    const int grid = static_cast<int>(a.n < (1 << 20) ? a.n : (1 << 20));
    hipLaunchKernelGGL(k_cigtext_write, dim3(grid), dim3(WAVE), 0, static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
