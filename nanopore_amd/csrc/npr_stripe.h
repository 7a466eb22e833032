// npr_stripe.h -- device helpers shared by the column-stripe kernels (npr_kernel_tile.hip: k_dp_tile, k_em_tile;
// npr_kernel_tile_cs.hip: k_dp_tile_cs): the stripe table entry through the scalar cache, the lane masks of a row from
// its packed word, the progress words in LDS, the buffer descriptor of a stripe, and the one-lane DPP shift of a cell
// across the wavefront.  Everything lives in an anonymous namespace of the including translation unit, as in npr_frame.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "npr_cell.h"
#include "npr_device.h"
#include "npr_frame.h"

namespace npr {

namespace {

typedef const __attribute__((address_space(4))) int32_t *cptr_i32;

struct UStripe {
    int X, K, df, dl;
    uint32_t row0;
};
__device__ __forceinline__ UStripe load_stripe(const Stripe *tab, int s) {
    cptr_i32 p = (cptr_i32)(tab + s);
    return UStripe{p[0], p[1], p[2], p[3], static_cast<uint32_t>(p[4])};
}

// lane masks of a row from its packed word (npr_sched.h tile_row_word): mask_r = (~0 << lo_r) & (~0 >> sh_r), six-bit
// fields -- the 64-bit shifts take six bits of their count, so the fields need no masking
__device__ __forceinline__ Masks<2> row_masks(uint32_t w) {
    Masks<2> m;
    m.cell[0] = (~0ull << (w & 63u)) & (~0ull >> ((w >> 6) & 63u));
    m.cell[1] = (~0ull << ((w >> 12) & 63u)) & (~0ull >> ((w >> 18) & 63u));
    m.lanes = m.cell[0] | m.cell[1];
    m.l0 = 0;
    return m;
}

// progress words: volatile LDS accesses (the pointer has to say LDS, or the compiler emits flat loads)
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ int lds_peek(const int *p) { return *(const volatile lds_int *)(p); }
__device__ __forceinline__ void lds_poke(int *p, int v) { *(volatile lds_int *)(p) = v; }

// The descriptor of a stripe's rows in one of the task's scratch areas: base = the stripe's first row.  A row is then
// addressed by a vector offset alone: nothing per row on the scalar unit, and no scalar offset operand (npr_frame.h
// store_row explains why).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stripe_rsrc(char *base, uint32_t row0, int row_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(base + static_cast<int64_t>(row0) * row_bytes, 0, -1, 0x00020000);
}

// every vector store of this wavefront has reached memory: what comes before a progress word is published
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// lane l <- lane l-1 (lane 0 takes `edge`);  lane l <- lane l+1 (lane 63 takes `edge`)
__device__ __forceinline__ float dppf_from_below(float v, float edge) { return bitsf(dpp_from_below(fbits(v), fbits(edge))); }
__device__ __forceinline__ float dppf_from_above(float v, float edge) { return bitsf(dpp_from_above(fbits(v), fbits(edge))); }
// ... of a whole cell: Cell (npr_cell.h, with its exponent) or RCell (npr_rs.h, five plain values)
template <class C>
__device__ __forceinline__ C cell_from_below(const C &v, const C &edge) {
    C o;
    o.m = dppf_from_below(v.m, edge.m), o.sx = dppf_from_below(v.sx, edge.sx), o.sy = dppf_from_below(v.sy, edge.sy);
    o.lx = dppf_from_below(v.lx, edge.lx), o.ly = dppf_from_below(v.ly, edge.ly);
    if constexpr (std::is_same_v<C, Cell>) o.e = dpp_from_below(v.e, edge.e);
    return o;
}
template <class C>
__device__ __forceinline__ C cell_from_above(const C &v, const C &edge) {
    C o;
    o.m = dppf_from_above(v.m, edge.m), o.sx = dppf_from_above(v.sx, edge.sx), o.sy = dppf_from_above(v.sy, edge.sy);
    o.lx = dppf_from_above(v.lx, edge.lx), o.ly = dppf_from_above(v.ly, edge.ly);
    if constexpr (std::is_same_v<C, Cell>) o.e = dpp_from_above(v.e, edge.e);
    return o;
}

}  // namespace

}  // namespace npr
