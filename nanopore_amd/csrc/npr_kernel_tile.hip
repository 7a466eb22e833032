// npr_kernel_tile.hip -- k_dp_tile<R>: the register-resident DP kernel for WIDE bands.
//
// Same recurrences and the same per-cell arithmetic (npr_cell.h) as k_dp_stair / k_dp_generic -- cactus_realign's banded
// five-state forward / backward / posterior pass, SURVEY.md 8a rows a5.3-a5.5, reference call site
// nanopore/analyses/utils.py:587 -- for the band the reference's own parameters give (anchors +- diagonalExpansion 10,
// 14 trimmed columns, splitMatrixBiggerThanThis 3000): a chain of unanchored rectangles hundreds to 3000 cells across,
// joined by 21-cell stripes.  97 % of its cells lie on anti-diagonals wider than one wavefront can hold.
//
// A frame that follows the anti-diagonal (k_dp_stair, k_dp_wide) needs the neighbour on BOTH sides, so a band spread
// over several wavefronts has to synchronise all of them after every anti-diagonal.  In lattice coordinates the
// dependencies of a cell, (x-1, y), (x, y-1), (x-1, y-1), point one way only.  So here the lattice COLUMNS of a task
// are cut into stripes of 64*R columns and one wavefront sweeps one stripe:
//   * slot j of the wavefront is lattice column X + j for the whole life of the stripe; on anti-diagonal d it holds the
//     cell (X + j, d - X - j).  (x, y-1) is the same slot on d-1, (x-1, y) the slot below on d-1, (x-1, y-1) the slot
//     below on d-2: one DPP shift per anti-diagonal (the shifted copy of d-1 is kept for the next step, where it is the
//     shifted d-2), no frame rebases, no reference stream -- a slot's reference base never changes; the read streams
//     through the wavefront one slot per step;
//   * the only thing a stripe needs from outside is the last column of the stripe to its left (forward) or the first
//     column of the stripe to its right (backward): one cell per anti-diagonal.  The producer writes it to the task's
//     scratch, the consumer stages 16 of them at a time into LDS; a per-wavefront progress word in LDS says how far a
//     stripe has got.  Wavefronts of a workgroup take the stripes of ONE task round-robin and run as a pipeline, each a
//     stripe width behind its left neighbour -- no barrier inside the sweep;
//   * forward match values stream to HBM one fixed-stride row per anti-diagonal of a stripe and stream back one row
//     ahead of use (every stripe is 64*R columns wide -- the last one may reach past lX --, so the right neighbour's
//     column always enters at lane 63 and a row is read by the lanes that wrote it);
//   * which lanes of a row hold band cells is read from a table the planner made (one packed word per row, k_plan_rowmask),
//     rows and neighbour cells are addressed by one buffer descriptor per stripe plus a vector offset: next to nothing
//     per step on the scalar unit, which the CU's four SIMDs share.
// Any band shape and width goes: what is outside the band is masked per anti-diagonal from the band arrays.
// Bit-identical to the other kernels and to the fp32 mirror (same cell arithmetic, order of evaluation is irrelevant to
// a cell's value).
//
// Layout: what the three stripe kernels share with k_dp_tile_cs (stripe table entries, row masks, progress words, stripe
// descriptors, the DPP shift of a cell) is npr_stripe.h.  Here: rows and neighbour cells in memory, the two steps, then the
// pieces k_dp_tile and k_em_tile are both built from, each written once -- the task and its LDS preamble (TileTask), the
// hand-over between neighbour stripes (TileEdge: the one polling loop and the one edge_stage call), the forward sweep
// (tile_forward_sweep), corner cells, totals, the task epilogue --, then the two kernels, which differ in their backward sweeps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "npr_cell.h"
#include "npr_device.h"
#include "npr_frame.h"
#include "npr_stripe.h"

namespace npr {

namespace {

constexpr int TILE_MAX_NW = 8;  // wavefronts per workgroup (launch bound)
constexpr int TILE_BLOCK = 16;  // neighbour cells staged / published at a time
constexpr int EDGE_FLOATS = 8;  // one neighbour cell in memory: m, sx, sy, lx, ly, e, -, -
constexpr int EDGE_ST_AUX = 0, EDGE_LD_AUX = 16;  // cache policy of the neighbour cells' stores and loads (16: sc1, edge_stage)

// One row per anti-diagonal of a stripe: 64*R cells of 8 bytes, lane l at 8*R*l.  The descriptor is the stripe's (its
// first row, stripe_rsrc); `vo` = this lane's byte offset in the row + 8 * 64 * R * (row - first row), in a VGPR.
template <int R>
__device__ __forceinline__ void tile_store_row(__amdgpu_buffer_rsrc_t rs, int vo, const Diag<R> &C, const Masks<R> &mk) {
    static_assert(R == 2, "k_dp_tile: two slots per lane");
    if (__builtin_amdgcn_inverse_ballot_w64(mk.lanes))
        __builtin_amdgcn_raw_buffer_store_b128(v4i{fbits(C.c[0].m), C.c[0].e, fbits(C.c[1].m), C.c[1].e}, rs, vo, 0, 0);
}
template <int R>
__device__ __forceinline__ void tile_load_row(__amdgpu_buffer_rsrc_t rs, int vo, FRow<R> &f, const Masks<R> &mk) {
    if (__builtin_amdgcn_inverse_ballot_w64(mk.lanes)) {
        const v4i q = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0);
        f.v[0] = bitsf(q.x), f.e[0] = q.y, f.v[1] = bitsf(q.z), f.e[1] = q.w;
    }
}
// the other four states of a row (k_em_tile): a second row of 16 bytes per cell
template <int R>
__device__ __forceinline__ void tile_store_planes(__amdgpu_buffer_rsrc_t rs, int vo, const Diag<R> &C, const Masks<R> &mk) {
    static_assert(R == 2, "k_em_tile: two slots per lane");
    if (__builtin_amdgcn_inverse_ballot_w64(mk.lanes)) {
        __builtin_amdgcn_raw_buffer_store_b128(v4i{fbits(C.c[0].sx), fbits(C.c[0].sy), fbits(C.c[0].lx), fbits(C.c[0].ly)}, rs, vo, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(v4i{fbits(C.c[1].sx), fbits(C.c[1].sy), fbits(C.c[1].lx), fbits(C.c[1].ly)}, rs, vo + 16, 0, 0);
    }
}

// the neighbour cell of a row: 32 bytes at (stripe's first) + 32 * (row - first row), written by the one lane that holds it
__device__ __forceinline__ void edge_store(__amdgpu_buffer_rsrc_t rs, int k, const Cell &c, uint64_t lane_mask) {
    if (__builtin_amdgcn_inverse_ballot_w64(lane_mask)) {
        const int vo = 4 * EDGE_FLOATS * k;
        __builtin_amdgcn_raw_buffer_store_b128(v4i{fbits(c.m), fbits(c.sx), fbits(c.sy), fbits(c.lx)}, rs, vo, 0, EDGE_ST_AUX);
        __builtin_amdgcn_raw_buffer_store_b64(v2i{fbits(c.ly), c.e}, rs, vo + 16, 0, EDGE_ST_AUX);
    }
}
// `cnt` neighbour cells starting at row `row` into this wavefront's LDS staging (lane l takes cell l).  The loads bypass
// the vector L1 (sc1: agent scope): the producer is another wavefront of this workgroup and its stores went through that cache.
__device__ __forceinline__ void edge_stage(char *Eb, uint32_t row, int cnt, float *stage, int lane) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Eb + static_cast<int64_t>(row) * (4 * EDGE_FLOATS), 0, -1, 0x00020000);
    if (__builtin_amdgcn_inverse_ballot_w64(low_lanes(cnt))) {
        const v4i q = __builtin_amdgcn_raw_buffer_load_b128(rs, 32 * lane, 0, EDGE_LD_AUX);
        const v2i g = __builtin_amdgcn_raw_buffer_load_b64(rs, 32 * lane + 16, 0, EDGE_LD_AUX);
        *reinterpret_cast<v4i *>(stage + EDGE_FLOATS * lane) = q;
        *reinterpret_cast<v2i *>(stage + EDGE_FLOATS * lane + 4) = g;
    }
}
__device__ __forceinline__ Cell edge_get(const float *stage, int k) {
    const float4 q = *reinterpret_cast<const float4 *>(stage + EDGE_FLOATS * k);
    const float2 g = *reinterpret_cast<const float2 *>(stage + EDGE_FLOATS * k + 4);
    return Cell{q.x, q.y, q.z, q.w, g.x, fbits(g.y)};
}

// One forward anti-diagonal of a stripe.  `io`: d-2 on entry, d on exit; `p1`: d-1; `carry`: the slot-below copy of
// d-2's top register (made by the step before) on entry, that of d-1 on exit; `edge`: the left stripe's last column on
// d-1 (every lane holds it, lane 0 uses it).  bx / by: X[x-1]*4 and Y[y-1]*4 of every slot.
// FLAT: every loaded model emits every base from every gap state with probability exactly 2^-2 (the shipped ones do; npr_rs.h rs_cell_emissions has
// the same switch): the four gap emissions are the constant, one LDS look-up per cell and direction instead of five.  The same factor in the same
// products: no bit changes.
template <int R, bool FLAT>
__device__ __forceinline__ void tile_emissions(const StepEnv &E, const Bases<R> &bx, const Bases<R> &by, int r, float &em, float &exs, float &exl, float &eys, float &eyl) {
    if constexpr (FLAT) {
        em = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, em) + 5 * bx.b[r] + by.b[r]);
        exs = exl = eys = eyl = 0.25f;
    } else {
        emissions<R>(E, bx, by, r, em, exs, exl, eys, eyl);
    }
}
template <int R, bool FLAT = false>
__device__ __forceinline__ void tile_fwd_step(int d, const StepEnv &E, Diag<R> &io, const Diag<R> &p1, Cell &carry, const Cell &edge,
                                              const Bases<R> &bx, const Bases<R> &by, const Masks<R> &mk) {
    const Cell Le = cell_from_below(p1.c[R - 1], edge);  // (x-1, y) of every lane's register 0
    Diag<R> o;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float em, exs, exl, eys, eyl;
        tile_emissions<R, FLAT>(E, bx, by, r, em, exs, exl, eys, eyl);
        o.c[r] = fwd_cell<false>(E.tr, r ? p1.c[r - 1] : Le, r ? io.c[r - 1] : carry, p1.c[r], em, exs, exl, eys, eyl);
    }
    settle_diag<R>(d, o, mk);
    io = o;
    carry = Le;
}
// One backward anti-diagonal.  `io`: d+2 -> d; `s1`: d+1; `carry`: the slot-above copy of d+2's register 0 -> that of
// d+1; `edge`: the right stripe's first column on d+1 (lane 63 uses it).  bx / by: X[x]*4 and Y[y]*4 of every slot.
template <int R, bool FLAT = false>
__device__ __forceinline__ void tile_bwd_step(int d, const StepEnv &E, Diag<R> &io, const Diag<R> &s1, Cell &carry, const Cell &edge,
                                              const Bases<R> &bx, const Bases<R> &by, const Masks<R> &mk) {
    const Cell Xe = cell_from_above(s1.c[0], edge);  // (x+1, y) of every lane's top register
    Diag<R> o;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float em, exs, exl, eys, eyl;
        tile_emissions<R, FLAT>(E, bx, by, r, em, exs, exl, eys, eyl);
        o.c[r] = bwd_cell<false>(E.tr, r + 1 < R ? io.c[r + 1] : carry, r + 1 < R ? s1.c[r + 1] : Xe, s1.c[r], em, exs, exl, eys, eyl);
    }
    settle_diag<R>(d, o, mk);
    io = o;
    carry = Xe;
}

// =====================================================================================================================
// What k_dp_tile and k_em_tile share: the task, the hand-over between neighbour stripes, the forward sweep, the totals.

// The dynamic LDS of a workgroup: the model, then misc ([0..3] totals, [4] pair counter, [5] next task), one progress word per
// wavefront, one staging block of neighbour cells per wavefront (k_em_tile: its bins behind those, em_tile_lds_bytes)
struct TileLds {
    float *model;
    int *misc, *prog;
    float *stage;  // this wavefront's
};
__device__ __forceinline__ TileLds tile_lds(char *smem, int wv) {
    TileLds L;
    L.model = reinterpret_cast<float *>(smem);
    L.misc = reinterpret_cast<int *>(L.model + MODEL_FLOATS);
    L.prog = L.misc + 8;
    L.stage = reinterpret_cast<float *>(L.prog + TILE_MAX_NW) + wv * (TILE_BLOCK * EDGE_FLOATS);
    return L;
}

// One task, everything wave-uniform.
struct TileTask {
    const uint8_t *X, *Y;
    int64_t pair_off;
    int lX, lY, D, pair_cap, model, xs, ys;
    int rs, re;          // rows of the model's start / end vectors
    cptr32 rowmask;      // one packed word per row, through the scalar cache
    const Stripe *tab;   // stripe s of S
    int S;
    char *Ef, *Eb;       // neighbour cells of the forward / the backward sweep, behind the rows in the task's scratch
};
template <int R>
__device__ __forceinline__ TileTask tile_task(const KernelArgs &a, int t, char *F) {
    const Task *tp = a.tasks + t;
    const int64_t tile_off = uni64(tp->tile_off), rowmask_off = uni64(tp->rowmask_off);
    const int flags = uni(tp->flags);
    TileTask T;
    T.X = a.seq + uni64(tp->x_off), T.Y = a.seq + uni64(tp->y_off), T.pair_off = uni64(tp->pair_off);
    T.lX = uni(tp->lX), T.lY = uni(tp->lY), T.D = uni(tp->D), T.pair_cap = uni(tp->pair_cap), T.model = uni(tp->model);
    T.xs = uni(tp->xs), T.ys = uni(tp->ys);
    T.rs = flags & 1, T.re = (flags >> 1) & 1;
    T.rowmask = (cptr32)(a.rowmask + rowmask_off);
    const Stripe *tab = a.stripes + tile_off;
    const UStripe hd = load_stripe(tab, 0);  // the table's header: stripes, rows
    T.S = hd.X;
    T.tab = tab + 1;
    const uint32_t rows = static_cast<uint32_t>(hd.K);
    T.Ef = F + static_cast<int64_t>(rows) * (64 * R * 8);
    T.Eb = T.Ef + static_cast<int64_t>(rows) * (4 * EDGE_FLOATS);
    return T;
}
// The workgroup takes the task up: the model into LDS, totals / pair counter / progress words reset (and BIN_ROWS rows of this
// wavefront's `lbins`, k_em_tile), between two barriers.  Returns the step environment with the transitions in VGPRs.
template <int BIN_ROWS>
__device__ __forceinline__ StepEnv tile_task_begin(const KernelArgs &a, const TileTask &T, const TileLds &L, int lane, float *lbins) {
    __syncthreads();
    {
        const float *gm = reinterpret_cast<const float *>(a.models + T.model);
        for (int i = threadIdx.x; i < MODEL_FLOATS; i += blockDim.x) L.model[i] = gm[i];
        if (threadIdx.x == 0) L.misc[0] = 0, L.misc[1] = E_DEAD, L.misc[2] = 0, L.misc[3] = E_DEAD, L.misc[4] = 0;
        if (threadIdx.x < TILE_MAX_NW) L.prog[threadIdx.x] = 0;
        if constexpr (BIN_ROWS > 0)
            for (int i = 0; i < BIN_ROWS; ++i) lbins[i * WAVE + lane] = 0.f;
    }
    __syncthreads();
    StepEnv E;
    E.mdl = reinterpret_cast<const DevModel *>(L.model);
    E.ltab = reinterpret_cast<const char *>(L.model);
    E.X = T.X, E.Y = T.Y, E.lX = T.lX, E.lY = T.lY, E.lane = lane;
    E.tr = load_trans(E.mdl->T);
    return E;
}

// The start cell (0, 0) / the end cell (lX, lY) from the model's start / end vector
__device__ __forceinline__ Cell corner_cell(const float *v) {
    Cell c;
    c.m = v[0], c.sx = v[1], c.sy = v[2], c.lx = v[3], c.ly = v[4];
    normalise(c, 0);
    return c;
}
// A sweep's total, <v, c> at its last corner, as (mantissa, exponent) into misc[slot], misc[slot + 1] (by the one lane that holds c)
__device__ __forceinline__ void capture_total(int *misc, int slot, const float *v, const Cell &c) {
    const float raw = dot5(v, c);
    if (raw > 0.f) {
        int k;
        reinterpret_cast<float *>(misc)[slot] = __builtin_frexpf(raw, &k);
        misc[slot + 1] = c.e + k;
    }
}
// A stripe's neighbour cells up to here are in memory: tell the wavefront that sweeps the neighbour stripe
__device__ __forceinline__ void publish_progress(int *word, int v, int lane) {
    wait_vm();
    if (lane == 0) lds_poke(word, v);
}

// The stripe next to the one a wavefront sweeps and the block of its neighbour cells this wavefront has staged in LDS.
// DIR = +1, the forward sweep: the stripe to the LEFT, whose last column slot 0 needs; its wavefront's progress word counts the rows
// whose neighbour cells are out.  DIR = -1, the backward sweep: the stripe to the RIGHT, whose first column the top slot needs; the
// progress word is the LOWEST row whose cell is out.  Entry q of the neighbour is its anti-diagonal df + q, row row0 + q.
// THE hand-over: a consumer never reads a cell before the producer's progress word covers it (the wait has no bound: the planner's
// stripe tables promise every row a wavefront that writes it), and the loads that follow bypass the vector L1 (edge_stage).
template <int DIR>
struct TileEdge {
    int df, len;         // the neighbour's first anti-diagonal and how many it has (0: no neighbour)
    uint32_t row0;
    const int *prog;     // the progress word of the wavefront that sweeps it
    char *cells;         // its neighbour cells in the task's scratch (Ef / Eb)
    float *stage;
    int lane;
    int blk_lo, blk_hi;  // staged: entries [blk_lo, blk_hi)
};
template <int DIR>
__device__ __forceinline__ TileEdge<DIR> edge_open(const TileTask &T, const TileLds &L, int s, int NW, int lane) {
    TileEdge<DIR> e;
    int df = 1, dl = 0, w = 0;
    e.row0 = 0;
    if (DIR > 0 ? s > 0 : s + 1 < T.S) {
        const UStripe n = load_stripe(T.tab, s - DIR);
        df = n.df, dl = n.dl, e.row0 = n.row0;
        w = (s - DIR) % NW;
    }
    e.df = df, e.len = dl - df + 1;
    e.prog = L.prog + w, e.cells = DIR > 0 ? T.Ef : T.Eb, e.stage = L.stage, e.lane = lane;
    e.blk_lo = e.blk_hi = DIR > 0 ? 0 : e.len;
    return e;
}
// wait for the block of TILE_BLOCK entries that begins (forward) / ends (backward) with entry q, and stage it
template <int DIR>
__device__ __forceinline__ void edge_fetch(TileEdge<DIR> &e, int q) {
    const int lo = DIR > 0 ? q : max(q - TILE_BLOCK + 1, 0), hi = DIR > 0 ? min(q + TILE_BLOCK, e.len) : q + 1;
    const int need = static_cast<int>(e.row0) + (DIR > 0 ? hi : lo);
    while (DIR > 0 ? uni(lds_peek(e.prog)) < need : uni(lds_peek(e.prog)) > need) __builtin_amdgcn_s_sleep(2);
    asm volatile("" ::: "memory");
    edge_stage(e.cells, e.row0 + lo, hi - lo, e.stage, e.lane);
    e.blk_lo = lo, e.blk_hi = hi;
}
// `carry` for a stripe's first anti-diagonal d0: (x-1, y-1) of slot 0 / (x+1, y+1) of the top slot is the neighbour's cell on d0 -+ 2
template <int DIR>
__device__ __forceinline__ void edge_seed(TileEdge<DIR> &e, int d0, Cell &carry) {
    const int q0 = d0 - 2 * DIR - e.df;
    if (q0 >= 0 && q0 < e.len) {
        edge_fetch(e, q0);
        const Cell c0 = edge_get(e.stage, q0 - e.blk_lo);
        if (e.lane == (DIR > 0 ? 0 : WAVE - 1)) carry = c0;
    }
}
// the neighbour's cell that the step of anti-diagonal d needs (its cell on d -+ 1; dead where it has none), in every lane
template <int DIR>
__device__ __forceinline__ Cell edge_at(TileEdge<DIR> &e, int d) {
    Cell c = dead_cell();
    const int q = d - DIR - e.df;
    if (static_cast<unsigned>(q) < static_cast<unsigned>(e.len)) {  // uniform; 0 <= q < len (len >= 0)
        if (DIR > 0 ? q >= e.blk_hi : q < e.blk_lo) edge_fetch(e, q);
        c = edge_get(e.stage, q - e.blk_lo);
    }
    return c;
}

// The forward sweep over this wavefront's stripes (s == wv mod NW).  PLANES: the other four states of every cell go to Fx too
// (k_em_tile, tile_store_planes).  Leaves the total in misc[0..1].
template <int R, bool FLAT, bool PLANES>
__device__ __forceinline__ void tile_forward_sweep(const TileTask &T, const StepEnv &E, const TileLds &L, int wv, int NW, char *F, char *Fx) {
    constexpr int K = 64 * R;
    const int lane = E.lane, lX = T.lX, lY = T.lY;
    const int voff = 8 * R * lane;
    int jr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) jr[r] = R * lane + r;
    for (int s = wv; s < T.S; s += NW) {
        const UStripe st = load_stripe(T.tab, s);
        if (st.dl < st.df) continue;
        TileEdge<+1> left = edge_open<+1>(T, L, s, NW, lane);
        Bases<R> bx, by;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            bx.b[r] = base4(E.X, lX, st.X + jr[r] - 1);
            by.b[r] = base4(E.Y, lY, (st.df - 1) - st.X - jr[r] - 1);  // as of anti-diagonal df - 1
        }
        Feed fy;
        feed_init<+1>(fy, E.Y, lY, st.df - st.X - 1, lane);
        Diag<R> A = dead_diag<R>(), B = dead_diag<R>();
        Cell carry = dead_cell();
        const uint64_t out_lane = 1ull << (st.K / R - 1);  // holds the stripe's last column in its top register
        cptr32 rm = T.rowmask + st.row0;                    // walked by pointer: the word of the row in hand
        uint32_t w_n = rm[0];                               // mask word one row ahead
        const __amdgpu_buffer_rsrc_t rsF = stripe_rsrc(F, st.row0, K * 8), rsE = stripe_rsrc(T.Ef, st.row0, 4 * EDGE_FLOATS);
        [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsX = PLANES ? stripe_rsrc(Fx, st.row0, K * 16) : rsF;
        edge_seed(left, st.df, carry);

        auto step = [&](int d, Diag<R> &io, const Diag<R> &p1) {
            const int k = d - st.df;
            const Masks<R> mk = row_masks(w_n);
            if (d < st.dl) w_n = rm[1];
            rm += 1;
            const Cell edge = edge_at(left, d);
            bases_down<R>(by, feed_get<+1>(fy, E.Y, lY, d - st.X - 1, lane));
            tile_fwd_step<R, FLAT>(d, E, io, p1, carry, edge, bx, by, mk);
            if (d == 0) {  // the start cell (0, 0): slot 0 of the first stripe
                if (lane == 0) io.c[0] = corner_cell(E.mdl->start + T.rs * 5);
            }
            tile_store_row<R>(rsF, voff + k * (K * 8), io, mk);
            if constexpr (PLANES) tile_store_planes<R>(rsX, 2 * voff + k * (K * 16), io, mk);
            edge_store(rsE, k, io.c[R - 1], out_lane);
            if ((k & (TILE_BLOCK - 1)) == TILE_BLOCK - 1 || d == st.dl) publish_progress(L.prog + wv, static_cast<int>(st.row0) + k + 1, lane);
        };
        int d = st.df;
        for (; d + 1 <= st.dl; d += 2) {
            step(d, B, A);
            step(d + 1, A, B);
        }
        if (d <= st.dl) step(d, B, A);
        if (s == T.S - 1) {  // total probability at the end corner (lX, lY), anti-diagonal D = this stripe's last row
            const bool inB = ((st.dl - st.df) & 1) == 0;
            const int je = lX - st.X;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (jr[r] == je) capture_total(L.misc, 0, E.mdl->end + T.re * 5, inB ? B.c[r] : A.c[r]);
        }
    }
}
// Every wavefront is through its forward sweep: what the task reports so far (the backward total and the pairs come later)
__device__ __forceinline__ TaskOut tile_forward_out(const int *misc) {
    __syncthreads();
    TaskOut out;
    out.tot_m = unif(reinterpret_cast<const float *>(misc)[0]), out.tot_e = uni(misc[1]);
    out.btot_m = 0.f, out.btot_e = E_DEAD, out.npairs = 0;
    out.status = out.tot_m > 0.f ? NPR_OK : NPR_ERR_ZERO_PROB;
    return out;
}
// Before the backward sweep: the progress words now mean the LOWEST row whose neighbour cell is out.  Returns the last stripe of
// this wavefront (s == wv mod NW).
__device__ __forceinline__ int tile_backward_begin(const TileLds &L, int S, int wv, int NW) {
    if (threadIdx.x < TILE_MAX_NW) L.prog[threadIdx.x] = 0x7fffffff;
    __syncthreads();
    return S - 1 - ((S - 1 - wv) % NW + NW) % NW;
}
// ... and after it: the total from the backward side, which the sweep of stripe 0 left in misc[2..3]
__device__ __forceinline__ void tile_backward_out(TaskOut &out, const int *misc) {
    __syncthreads();
    out.btot_m = unif(reinterpret_cast<const float *>(misc)[2]);
    out.btot_e = uni(misc[3]);
}
// The task's result out, the next task in: returns its index (uniform over the workgroup)
__device__ __forceinline__ int tile_task_end(const KernelArgs &a, int t, const TaskOut &out, int *misc) {
    if (threadIdx.x == 0) {
        a.outs[t] = out;
        misc[5] = atomicAdd(a.queue, 1);
    }
    __syncthreads();
    return uni(misc[5]) + static_cast<int>(gridDim.x);
}

template <int R, bool FLAT>
__global__ void __launch_bounds__(WAVE *TILE_MAX_NW) __attribute__((amdgpu_waves_per_eu(R == 2 ? 6 : 1))) k_dp_tile(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int K = 64 * R;

    const int lane = threadIdx.x & (WAVE - 1);
    const int wv = uni(static_cast<int>(threadIdx.x) >> 6);
    const int NW = static_cast<int>(blockDim.x) >> 6;
    const TileLds L = tile_lds(smem, wv);
    char *const F = a.F + uni64(a.region[blockIdx.x]) * 8;
    const int voff = 8 * R * lane;
    int jr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) jr[r] = R * lane + r;

    int t = blockIdx.x;
    while (t < a.ntasks) {
        const TileTask T = tile_task<R>(a, t, F);
        StepEnv E = tile_task_begin<0>(a, T, L, lane, nullptr);
        if constexpr (R >= T_SGPR_MIN_R) {
            Trans &tr = E.tr;
            tr.mm = unif(tr.mm), tr.sxm = unif(tr.sxm), tr.sym = unif(tr.sym), tr.lxm = unif(tr.lxm), tr.lym = unif(tr.lym);
            tr.msx = unif(tr.msx), tr.sxsx = unif(tr.sxsx), tr.sysx = unif(tr.sysx);
            tr.msy = unif(tr.msy), tr.sysy = unif(tr.sysy), tr.sxsy = unif(tr.sxsy);
            tr.mlx = unif(tr.mlx), tr.lxlx = unif(tr.lxlx), tr.mly = unif(tr.mly), tr.lyly = unif(tr.lyly);
        }
        const int lX = T.lX, lY = T.lY;

        tile_forward_sweep<R, FLAT, false>(T, E, L, wv, NW, F, nullptr);
        TaskOut out = tile_forward_out(L.misc);

        // =============================== backward + posteriors ===============================
        if (out.tot_m > 0.f) {
            const int tot_e = out.tot_e;
            const float inv_tot = 1.0f / out.tot_m;
            const PairSink sink{a.px, a.py, a.pp, T.pair_off, T.pair_cap, T.xs, T.ys, a.threshold};
            const int s_top = tile_backward_begin(L, T.S, wv, NW);
            for (int s = s_top; s >= 0; s -= NW) {
                const UStripe st = load_stripe(T.tab, s);
                if (st.dl < st.df) continue;
                TileEdge<-1> right = edge_open<-1>(T, L, s, NW, lane);
                const int X0 = st.X;  // every stripe is 64*R columns wide (npr_sched.h stripe_fill): slot j is column X0 + j
                Bases<R> bx, by;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    bx.b[r] = base4(E.X, lX, X0 + jr[r]);
                    by.b[r] = base4(E.Y, lY, (st.dl + 1) - X0 - jr[r]);  // as of anti-diagonal dl + 1
                }
                Feed fy;
                feed_init<-1>(fy, E.Y, lY, st.dl - X0 - (K - 1), lane);
                Diag<R> A = dead_diag<R>(), B = dead_diag<R>();
                Cell carry = dead_cell();
                const uint64_t out_lane = 1ull;  // lane 0 holds the stripe's first column in its register 0
                FRow<R> fa, fb;
#pragma unroll
                for (int r = 0; r < R; ++r) fa.v[r] = fb.v[r] = 0.f, fa.e[r] = fb.e[r] = E_DEAD;
                cptr32 rm = T.rowmask + st.row0 + static_cast<uint32_t>(st.dl - st.df);  // walked by pointer: the word of the row in hand
                const __amdgpu_buffer_rsrc_t rsF = stripe_rsrc(F, st.row0, K * 8), rsE = stripe_rsrc(T.Eb, st.row0, 4 * EDGE_FLOATS);
                // forward row of the first anti-diagonal (the later ones are loaded one step ahead, with their masks)
                Masks<R> mk_n = row_masks(rm[0]);
                tile_load_row<R>(rsF, voff + (st.dl - st.df) * (K * 8), fb, mk_n);
                edge_seed(right, st.dl, carry);

                // f: the forward row of d (loaded a step ago); fnext: where the row of d-1 goes
                auto step = [&](int d, Diag<R> &io, const Diag<R> &s1, FRow<R> &f, FRow<R> &fnext) {
                    const int k = d - st.df;
                    const Masks<R> mk = mk_n;
                    if (d > st.df) {
                        rm -= 1;
                        mk_n = row_masks(rm[0]);
                        tile_load_row<R>(rsF, voff + (k - 1) * (K * 8), fnext, mk_n);
                    }
                    const Cell edge = edge_at(right, d);
                    bases_up<R>(by, feed_get<-1>(fy, E.Y, lY, d - X0 - (K - 1), lane));
                    tile_bwd_step<R, FLAT>(d, E, io, s1, carry, edge, bx, by, mk);
                    if (d == T.D) {  // the end corner (lX, lY)
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (X0 + jr[r] == lX) io.c[r] = corner_cell(E.mdl->end + T.re * 5);
                    }
                    edge_store(rsE, k, io.c[0], out_lane);
                    // posteriors of this anti-diagonal, slots claimed from the workgroup's LDS counter
                    {
                        float p[R];
                        uint64_t hit[R];
                        int total = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            p[r] = posterior(f.v[r], f.e[r], io.c[r].m, io.c[r].e, tot_e, inv_tot);
                            hit[r] = __ballot(p[r] >= sink.threshold) & mk.cell[r];
                            total += __popcll(hit[r]);
                        }
                        if (d >= 2 && total) {
                            int base = 0;
                            if (lane == 0) base = atomicAdd(L.misc + 4, total);
                            base = uni(base);
                            const int y0 = d - X0;
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                if (hit[r]) {
                                    const int before = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(hit[r] >> 32),
                                                                                 __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(hit[r]), 0));
                                    const int slot = base + before;
                                    if (__builtin_amdgcn_inverse_ballot_w64(hit[r]) && slot < sink.cap) {
                                        sink.px[sink.off + slot] = X0 + jr[r] - 1 + sink.xs;
                                        sink.py[sink.off + slot] = y0 - jr[r] - 1 + sink.ys;
                                        sink.pp[sink.off + slot] = p[r];
                                    }
                                    base += __popcll(hit[r]);
                                }
                            }
                        }
                    }
                    if (((st.dl - d) & (TILE_BLOCK - 1)) == TILE_BLOCK - 1 || d == st.df) publish_progress(L.prog + wv, static_cast<int>(st.row0) + k, lane);
                };
                int d = st.dl;
                for (; d - 1 >= st.df; d -= 2) {
                    step(d, B, A, fb, fa);
                    step(d - 1, A, B, fa, fb);
                }
                if (d >= st.df) step(d, B, A, fb, fa);
                if (s == 0) {  // total from the backward side: the lattice point (0, 0) is the stripe's first slot on d = 0
                    const bool inB = ((st.dl - st.df) & 1) == 0;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (X0 + jr[r] == 0) capture_total(L.misc, 2, E.mdl->start + T.rs * 5, inB ? B.c[r] : A.c[r]);
                }
            }
            tile_backward_out(out, L.misc);
        }
        if (threadIdx.x == 0) {
            out.npairs = L.misc[4];
            if (out.npairs > T.pair_cap) out.status = NPR_ERR_CAPACITY;
        }
        t = tile_task_end(a, t, out, L.misc);
    }
}

// =====================================================================================================================
// k_em_tile<2>: the Baum-Welch E-step on column stripes -- the trainer's own band (anchors, splitMatrixBiggerThanThis 300,
// nanopore/analyses/utils.py:511) is 256-310 cells across at its widest and 87 on average: too wide for one wavefront's
// frame, and on the workgroup-wide frame of k_dp_wide<2, NW, EM> one wavefront in four works.  Same sweeps as k_dp_tile; the
// forward sweep also keeps the other four states of every cell (a second row of 16 bytes per cell), and the backward
// sweep, after the cells of anti-diagonal d, adds the posterior of every transition into them to 15 per-lane accumulators
// and of every emitted symbol to per-lane bins in LDS, as k_em_stair does.  In stripe coordinates the three predecessors
// of (x, y) are the same slot on d-1, the slot below on d-1 and the slot below on d-2: the rows of d-1 and d-2 stay in
// registers (one row is loaded per step, none twice), the slot below is one DPP shift, and lane 0's comes from the left
// stripe's last column, which the forward sweep left in the task's scratch for its neighbour.
constexpr int EM_TILE_NW = 4;

// all five states of a row back into registers; lanes outside the row keep what they held (every use is masked)
template <int R>
__device__ __forceinline__ void tile_load_full(__amdgpu_buffer_rsrc_t rsF, __amdgpu_buffer_rsrc_t rsX, int voF, int voX, Diag<R> &G,
                                               const Masks<R> &mk) {
    if (__builtin_amdgcn_inverse_ballot_w64(mk.lanes)) {
        const v4i q = __builtin_amdgcn_raw_buffer_load_b128(rsF, voF, 0, 0);
        const v4i u = __builtin_amdgcn_raw_buffer_load_b128(rsX, voX, 0, 0);
        const v4i w = __builtin_amdgcn_raw_buffer_load_b128(rsX, voX + 16, 0, 0);
        G.c[0] = Cell{bitsf(q.x), bitsf(u.x), bitsf(u.y), bitsf(u.z), bitsf(u.w), q.y};
        G.c[1] = Cell{bitsf(q.z), bitsf(w.x), bitsf(w.y), bitsf(w.z), bitsf(w.w), q.w};
    }
}
// one neighbour cell (32 bytes, the same address for every lane)
__device__ __forceinline__ Cell edge_load(char *Eb, uint32_t row) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Eb + static_cast<int64_t>(row) * (4 * EDGE_FLOATS), 0, -1, 0x00020000);
    const v4i q = __builtin_amdgcn_raw_buffer_load_b128(rs, 0, 0, 0);
    const v2i g = __builtin_amdgcn_raw_buffer_load_b64(rs, 16, 0, 0);
    return Cell{bitsf(q.x), bitsf(q.y), bitsf(q.z), bitsf(q.w), bitsf(g.x), g.y};
}

constexpr int EM_SKIP = -40;
__device__ __forceinline__ float &tile_bin_at(float *lbins, int byte_off) {
    return *reinterpret_cast<float *>(reinterpret_cast<char *>(lbins) + byte_off);
}

// Expected counts of the transitions into the cells `io` of one row: Gm = (x-1, y-1), Gl = (x-1, y), Gu = (x, y-1), each with
// the lanes on which that predecessor is a band cell; eX / eY: 4 * the bases consumed into the cell (X[x-1], Y[y-1]).
// (The accumulation of k_em_stair's em_cells, npr_kernel_stair.hip, on this kernel's neighbours.)
template <int R>
__device__ __forceinline__ void tile_em_cells(const StepEnv &E, const Diag<R> &io, const Masks<R> &mk, const Diag<R> &Gm, const uint64_t (&vm)[R],
                                              const Diag<R> &Gl, const uint64_t (&vl)[R], const Diag<R> &Gu, const uint64_t (&vu)[R],
                                              const Bases<R> &eX, const Bases<R> &eY, int tot_e, float inv_tot, float (&acc)[15], float *lbins,
                                              int lane) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const Cell c = io.c[r];
        const uint64_t here = __ballot(c.e != E_DEAD) & mk.cell[r];
        const int ex4 = eX.b[r], ey4 = eY.b[r];
        const int lane4 = 4 * lane;
        float bM = 0.f, bXs = 0.f, bXl = 0.f, bYs = 0.f, bYl = 0.f;  // this cell's emission posteriors
        // (round 6) A region whose every lane's F * B / total is below 2^EM_SKIP contributes nothing a count can see (2.7e8 terms of 2^-40 each are
        // 2.4e-4 of a count): the wavefront steps over it -- a stripe row that lies off the alignment's path, a third of the rows of the trainer's band.
        const int s_m = Gm.c[r].e + c.e - tot_e, s_l = Gl.c[r].e + c.e - tot_e, s_u = Gu.c[r].e + c.e - tot_e;
        const uint64_t live_m = here & vm[r] & __ballot(s_m > EM_SKIP), live_l = here & vl[r] & __ballot(s_l > EM_SKIP), live_u = here & vu[r] & __ballot(s_u > EM_SKIP);
        if (lanes_of(live_m)) {
            const Cell &Fm = Gm.c[r];
            const int s = min(max(Fm.e + c.e - tot_e, -200), 200);
            const float em = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, em) + 5 * ex4 + ey4);
            const float w = __builtin_ldexpf(em * c.m * inv_tot, s);
            const float t0 = Fm.m * E.tr.mm * w, t1 = Fm.sx * E.tr.sxm * w, t2 = Fm.sy * E.tr.sym * w, t3 = Fm.lx * E.tr.lxm * w,
                        t4 = Fm.ly * E.tr.lym * w;
            acc[0] += t0, acc[1] += t1, acc[2] += t2, acc[3] += t3, acc[4] += t4;
            bM = (t0 + t1) + (t2 + t3) + t4;
        }
        if (lanes_of(live_l)) {
            const Cell &Fl = Gl.c[r];
            const int s = min(max(Fl.e + c.e - tot_e, -200), 200);
            const float g = __builtin_ldexpf(inv_tot, s);
            const float exs = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, ex) + 20 + ex4);
            const float exl = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, ex) + 60 + ex4);
            const float ws = exs * c.sx * g, wl = exl * c.lx * g;
            const float t0 = Fl.m * E.tr.msx * ws, t1 = Fl.sx * E.tr.sxsx * ws, t2 = Fl.sy * E.tr.sysx * ws;
            const float u0 = Fl.m * E.tr.mlx * wl, u1 = Fl.lx * E.tr.lxlx * wl;
            acc[5] += t0, acc[6] += t1, acc[7] += t2, acc[8] += u0, acc[9] += u1;
            bXs = (t0 + t1) + t2, bXl = u0 + u1;
        }
        if (lanes_of(live_u)) {
            const Cell &Fu = Gu.c[r];
            const int s = min(max(Fu.e + c.e - tot_e, -200), 200);
            const float g = __builtin_ldexpf(inv_tot, s);
            const float eys = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, ey) + 40 + ey4);
            const float eyl = *reinterpret_cast<const float *>(E.ltab + offsetof(DevModel, ey) + 80 + ey4);
            const float ws = eys * c.sy * g, wl = eyl * c.ly * g;
            const float t0 = Fu.m * E.tr.msy * ws, t1 = Fu.sy * E.tr.sysy * ws, t2 = Fu.sx * E.tr.sxsy * ws;
            const float u0 = Fu.m * E.tr.mly * wl, u1 = Fu.ly * E.tr.lyly * wl;
            acc[10] += t0, acc[11] += t1, acc[12] += t2, acc[13] += u0, acc[14] += u1;
            bYs = (t0 + t1) + t2, bYl = u0 + u1;
        }
        if (lanes_of(live_m | live_l | live_u)) {  // the five bins of this cell (disjoint tables): all reads, then all writes; an N base goes to the scratch row
            constexpr int TRASH = EM_BINS * 256;
            const bool nx = ex4 >= 16, ny = ey4 >= 16;
            const int aM = ((nx || ny) ? TRASH : ex4 * 256 + ey4 * 64) + lane4;
            const int aXs = (nx ? TRASH : 16 * 256 + ex4 * 64) + lane4, aXl = (nx ? TRASH : 20 * 256 + ex4 * 64) + lane4;
            const int aYs = (ny ? TRASH : 24 * 256 + ey4 * 64) + lane4, aYl = (ny ? TRASH : 28 * 256 + ey4 * 64) + lane4;
            const float v0 = tile_bin_at(lbins, aM), v1 = tile_bin_at(lbins, aXs), v2 = tile_bin_at(lbins, aXl), v3 = tile_bin_at(lbins, aYs),
                        v4 = tile_bin_at(lbins, aYl);
            tile_bin_at(lbins, aM) = v0 + bM;
            tile_bin_at(lbins, aXs) = v1 + bXs;
            tile_bin_at(lbins, aXl) = v2 + bXl;
            tile_bin_at(lbins, aYs) = v3 + bYs;
            tile_bin_at(lbins, aYl) = v4 + bYl;
        }
    }
}

constexpr int EM_TILE_WPE = 3;  // wavefronts per SIMD the register allocation aims at (164 VGPRs unconstrained: 3)
template <int R>
__global__ void __launch_bounds__(WAVE *EM_TILE_NW) __attribute__((amdgpu_waves_per_eu(EM_TILE_WPE))) k_em_tile(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int K = 64 * R;

    const int lane = threadIdx.x & (WAVE - 1);
    const int wv = uni(static_cast<int>(threadIdx.x) >> 6);
    const int NW = static_cast<int>(blockDim.x) >> 6;
    const TileLds L = tile_lds(smem, wv);
    float *const lbins = reinterpret_cast<float *>(L.prog + TILE_MAX_NW) + NW * (TILE_BLOCK * EDGE_FLOATS) + wv * ((EM_BINS + 1) * WAVE);
    char *const F = a.F + uni64(a.region[blockIdx.x]) * 8;
    char *const Fx = reinterpret_cast<char *>(a.Fx) + uni64(a.region[blockIdx.x]) * 16;  // the other four states: 16 bytes per cell
    const int voff = 8 * R * lane;
    int jr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) jr[r] = R * lane + r;

    int t = blockIdx.x;
    while (t < a.ntasks) {
        const TileTask T = tile_task<R>(a, t, F);
        const StepEnv E = tile_task_begin<EM_BINS + 1>(a, T, L, lane, lbins);  // transitions in VGPRs, as in k_em_stair: every count multiplies by one
        const int lX = T.lX, lY = T.lY, model = T.model;

        // forward: as k_dp_tile, all five states stored
        tile_forward_sweep<R, false, true>(T, E, L, wv, NW, F, Fx);
        TaskOut out = tile_forward_out(L.misc);

        // =============================== backward + expected counts ===============================
        float acc[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) acc[i] = 0.f;
        if (out.tot_m > 0.f) {
            const int tot_e = out.tot_e;
            const float inv_tot = 1.0f / out.tot_m;
            const int s_top = tile_backward_begin(L, T.S, wv, NW);
            for (int s = s_top; s >= 0; s -= NW) {
                const UStripe st = load_stripe(T.tab, s);
                if (st.dl < st.df) continue;
                TileEdge<-1> right = edge_open<-1>(T, L, s, NW, lane);
                const TileEdge<+1> left = edge_open<+1>(T, L, s, NW, lane);  // its cells are all out: read straight from memory (edge_load)
                const int X0 = st.X;
                Bases<R> bx, by, bxm, bym;  // X[x], Y[y] of every slot (the backward cell) and X[x-1], Y[y-1] (the symbols emitted INTO it)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    bx.b[r] = base4(E.X, lX, X0 + jr[r]);
                    bxm.b[r] = base4(E.X, lX, X0 + jr[r] - 1);
                    by.b[r] = base4(E.Y, lY, (st.dl + 1) - X0 - jr[r]);
                    bym.b[r] = base4(E.Y, lY, (st.dl + 1) - X0 - jr[r] - 1);
                }
                Feed fy, fym;
                feed_init<-1>(fy, E.Y, lY, st.dl - X0 - (K - 1), lane);
                feed_init<-1>(fym, E.Y, lY, st.dl - X0 - (K - 1) - 1, lane);
                Diag<R> A = dead_diag<R>(), B = dead_diag<R>();
                Cell carry = dead_cell();
                const uint64_t out_lane = 1ull;
                cptr32 rm0 = T.rowmask + st.row0;
                const __amdgpu_buffer_rsrc_t rsF = stripe_rsrc(F, st.row0, K * 8), rsE = stripe_rsrc(T.Eb, st.row0, 4 * EDGE_FLOATS),
                                             rsX = stripe_rsrc(Fx, st.row0, K * 16);
                // forward rows of d-1 and d-2 (all five states), the masks of their lanes, and the left stripe's last column on them
                Diag<R> G1 = dead_diag<R>(), G2 = dead_diag<R>();
                Masks<R> m1{}, m2{};
                Cell eL1 = dead_cell(), eL2 = dead_cell();
                auto fetch_row = [&](int dd, Diag<R> &G, Masks<R> &m, Cell &eL) {
                    m.cell[0] = m.cell[1] = m.lanes = 0, m.l0 = 0;
                    if (dd >= st.df && dd <= st.dl) {  // uniform
                        const int k = dd - st.df;
                        m = row_masks(rm0[k]);
                        tile_load_full<R>(rsF, rsX, voff + k * (K * 8), 2 * voff + k * (K * 16), G, m);
                    }
                    eL = dead_cell();
                    const int q = dd - left.df;
                    if (static_cast<unsigned>(q) < static_cast<unsigned>(left.len)) eL = edge_load(T.Ef, left.row0 + static_cast<uint32_t>(q));
                };
                fetch_row(st.dl - 1, G1, m1, eL1);
                fetch_row(st.dl - 2, G2, m2, eL2);
                Masks<R> mk_n = row_masks(rm0[st.dl - st.df]);
                edge_seed(right, st.dl, carry);
                auto step = [&](int d, Diag<R> &io, const Diag<R> &s1) {
                    const int k = d - st.df;
                    const Masks<R> mk = mk_n;
                    if (d > st.df) mk_n = row_masks(rm0[k - 1]);
                    const Cell edge = edge_at(right, d);
                    bases_up<R>(by, feed_get<-1>(fy, E.Y, lY, d - X0 - (K - 1), lane));
                    bases_up<R>(bym, feed_get<-1>(fym, E.Y, lY, d - X0 - (K - 1) - 1, lane));
                    tile_bwd_step<R>(d, E, io, s1, carry, edge, bx, by, mk);
                    if (d == T.D) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (X0 + jr[r] == lX) io.c[r] = corner_cell(E.mdl->end + T.re * 5);
                    }
                    edge_store(rsE, k, io.c[0], out_lane);
                    if (d >= 1) {  // expected counts of the transitions into the cells of d
                        Diag<R> Gl, Gm;
                        Gl.c[1] = G1.c[0], Gl.c[0] = cell_from_below(G1.c[1], eL1);
                        Gm.c[1] = G2.c[0], Gm.c[0] = cell_from_below(G2.c[1], eL2);
                        const uint64_t vu[R] = {m1.cell[0], m1.cell[1]};
                        const uint64_t vl[R] = {(m1.cell[1] << 1) | (uni(eL1.e) != E_DEAD ? 1ull : 0ull), m1.cell[0]};
                        const uint64_t vm[R] = {(m2.cell[1] << 1) | (uni(eL2.e) != E_DEAD ? 1ull : 0ull), m2.cell[0]};
                        tile_em_cells<R>(E, io, mk, Gm, vm, Gl, vl, G1, vu, bxm, bym, tot_e, inv_tot, acc, lbins, lane);
                    }
                    // the rows the next anti-diagonal needs: d-2 moves up, d-3 comes from memory
                    G1 = G2, m1 = m2, eL1 = eL2;
                    fetch_row(d - 3, G2, m2, eL2);
                    if (((st.dl - d) & (TILE_BLOCK - 1)) == TILE_BLOCK - 1 || d == st.df) publish_progress(L.prog + wv, static_cast<int>(st.row0) + k, lane);
                };
                int d = st.dl;
                for (; d - 1 >= st.df; d -= 2) {
                    step(d, B, A);
                    step(d - 1, A, B);
                }
                if (d >= st.df) step(d, B, A);
                if (s == 0) {
                    const bool inB = ((st.dl - st.df) & 1) == 0;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (X0 + jr[r] == 0) capture_total(L.misc, 2, E.mdl->start + T.rs * 5, inB ? B.c[r] : A.c[r]);
                }
            }
            tile_backward_out(out, L.misc);
            // every wavefront adds up its own bins, then its transition accumulators through the same rows
            if (lane < EM_BINS) {
                double sum = 0.0;
                for (int q = 0; q < WAVE; ++q) sum += static_cast<double>(lbins[lane * WAVE + q]);
                atomicAdd(a.em_E + model * EM_BINS + lane, sum);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 15; ++i) lbins[i * WAVE + lane] = acc[i];
            __syncthreads();
            if (lane < 15) {
                double sum = 0.0;
                for (int q = 0; q < WAVE; ++q) sum += static_cast<double>(lbins[lane * WAVE + q]);
                const int map[15] = {0, 5, 10, 15, 20, 1, 6, 11, 3, 18, 2, 12, 7, 4, 24};  // accumulator order -> T[from*5+to]
                atomicAdd(a.em_T + model * 25 + map[lane], sum);
            }
        }
        t = tile_task_end(a, t, out, L.misc);
    }
}

}  // namespace

size_t tile_lds_bytes(int nw) { return sizeof(float) * (MODEL_FLOATS + 8 + TILE_MAX_NW + static_cast<size_t>(nw) * TILE_BLOCK * EDGE_FLOATS); }

// rows of 64*R cells plus one 32-byte neighbour cell per row for each sweep direction
int64_t tile_scratch_cells(int64_t rows, int R) { return rows * (64 * R + 2 * EDGE_FLOATS / 2); }

size_t em_tile_lds_bytes(int nw) { return tile_lds_bytes(nw) + sizeof(float) * static_cast<size_t>(nw) * (EM_BINS + 1) * WAVE; }
int em_tile_waves_per_cu() { return 4 * EM_TILE_WPE; }
int em_tile_waves() {  // wavefronts per task
    return 2;  // trainer's band 2.24 / 2.53 / 2.40 / 2.16e10 cells/s on 1 / 2 / 3 / 4 wavefronts per task, a 560-cell band 2.6 / 3.3 / 3.1 / 3.3e10
}

int launch_em_tile(const KernelArgs &a, int R, int grid, void *stream) {
    if (R != 2) return static_cast<int>(hipErrorInvalidValue);
    const int nw = em_tile_waves();
    hipLaunchKernelGGL((k_em_tile<2>), dim3(grid), dim3(WAVE * nw), em_tile_lds_bytes(nw), static_cast<hipStream_t>(stream), a);
    return static_cast<int>(hipGetLastError());
}

int launch_tile(const KernelArgs &a, int R, int NW, int grid, void *stream, bool flat) {  // flat: every loaded model's gap emissions are exactly 2^-2
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (NW < 1 || NW > TILE_MAX_NW) return static_cast<int>(hipErrorInvalidValue);
    const size_t lds = tile_lds_bytes(NW);
    if (R == 2 && flat)
        hipLaunchKernelGGL((k_dp_tile<2, true>), dim3(grid), dim3(WAVE * NW), lds, s, a);
    else if (R == 2)
        hipLaunchKernelGGL((k_dp_tile<2, false>), dim3(grid), dim3(WAVE * NW), lds, s, a);
    else
        return static_cast<int>(hipErrorInvalidValue);
    return static_cast<int>(hipGetLastError());
}

}  // namespace npr
