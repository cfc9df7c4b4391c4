// kernels_brick3d.hip -- small 3-D grids: SEVERAL iterations per launch on bricks that live in LDS (gfx950).
//
// The 3-D counterpart of kernels_tile2d.hip.  A workgroup loads a brick of the field -- S0 planes x S1 rows of 64 cells along x2, one
// lane per cell -- into LDS, with H ghost shells on every side of every axis THAT NEEDS THEM, performs K <= H iterations on it without
// leaving the CU (one workgroup barrier per iteration) and writes the cells it owns into the other global buffer (ping-pong in global
// memory for red-black too: a neighbouring brick must still find the old ghost values).  Ghost cells are swept like owned ones and go
// stale one shell per iteration from the outside in, so after K <= H iterations every owned cell holds exactly what K whole-grid
// iterations give it.  The arithmetic of a cell is cell_update.h's 3-D update on the same values in the same operand order as
// kernels_3d.hip (x0 - 1, x0 + 1, x1 - 1, x1 + 1, x2 - 1, x2 + 1): bit-identical to the per-iteration kernels
// (tests/test_gpu_brick3d.py).
//
// An axis that fits carries no ghosts.  The faces of the grid are locked, so on an axis whose whole extent fits inside the brick the
// brick covers the axis, starts at the face and spends nothing on shells; m[2] <= 64 is the common case, and a grid of up to
// brick_3d_max_rows() rows is ONE brick.  Three ghosted axes at H = 4 recompute about 6 cells per owned cell, two about 2.5.
//
// Geometry.  A row of the brick is one bank-conflict-free LDS access (64 lanes, 64 banks); the six neighbours of a cell are six LDS
// reads at fixed distances (+-1, +-64, +-64 S1).  Red-black: the colour is (x0 + x1 + x2 + iteration) even -- the opposite phase to
// 2-D --, so of a PAIR of rows (x0, x1), (x0, x1 + 1) the active cells are exactly one per column: a wave takes a row pair per pass, each
// lane the row that has its column's active cell, all 64 lanes busy.  Jacobi: a wave takes a row per pass and the brick ping-pongs
// between two LDS arrays.  Pairs (rows) are dealt to the sixteen waves of the workgroup in turn.  A row that has gone stale, lies on a
// face or outside the grid is skipped (wave-uniform): every row that IS updated has its x0 and x1 neighbours inside the brick, so the
// brick needs no padding.  Stale columns idle.  The locks of the rows a wave owns stay with it for the whole launch -- one bit per pass
// in a register of every lane: a brick has up to 18 passes per wave, too many for a lane mask each in scalar registers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "cell_update.h"
#include "kernels.h"

namespace epic_hip {

namespace {

#ifndef EPIC_BRICK_WAVES  // build knob (A/B): waves per workgroup (the 2-D tile's dependent chain measured best at 16)
#define EPIC_BRICK_WAVES 16
#endif
constexpr int kBrickWaves = EPIC_BRICK_WAVES;
constexpr int kBrickThreads = 64 * kBrickWaves;

struct Brick3dArgs {
    const float *in;
    float *out;
    const uint32_t *maskw;   // lane masks (kernels.h), 1 = locked; faces and padding are locked
    int m0, m1, pitch;
    int halo;
    int s0, s1;              // the brick in LDS: planes and rows (s1 even)
    int t0, t1, tc;          // cells a brick owns along each axis
    int nb1, nbc;            // bricks along x1 and x2
    int ghost0, ghost1, ghostc;   // whether the axis carries ghost shells (else the brick starts at the face and covers the axis)
    int steps;               // iterations of this launch, <= halo
    int parity;              // red-black: number of the first iteration & 1
};

// ROWS: rows of 64 cells the LDS arrays hold (s0 * s1 <= ROWS): brick_3d_max_rows() of the instantiation.
template <int MATH, bool RB, int ROWS>
__global__ __launch_bounds__(kBrickThreads) void brick3d_kernel(Brick3dArgs a)
{
    constexpr bool TOL = MATH == kMathTol;
    constexpr int kBufs = RB ? 1 : 2;
    constexpr int kCells = ROWS * 64;
    static_assert((ROWS / (RB ? 2 : 1) + kBrickWaves - 1) / kBrickWaves <= 32, "one lock bit per pass in a 32-bit register");
    __shared__ float u_lds[kBufs * kCells];
    __shared__ float q_lds[TOL ? kBufs * kCells : 1];
    __shared__ uint32_t n_lds[TOL ? kBufs * kCells : 1];
    __shared__ __attribute__((aligned(16))) char math_lds_bytes[TOL ? TolLn<5>::kLdsBytes : kMathLdsDoubles * (int)sizeof(double)];
    const TolLnEntry *const tl = reinterpret_cast<const TolLnEntry *>(math_lds_bytes);
    const MathTab tab = math_tables_at(reinterpret_cast<double *>(math_lds_bytes), kConstsPlain);
    MathTabRegs tab_regs = {};
    if (MATH == kMathPrecise) tab_regs = math_tables_fetch();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H = a.halo, S0 = a.s0, S1 = a.s1;
    const int bc = blockIdx.x % a.nbc, b1 = (blockIdx.x / a.nbc) % a.nb1, b0 = blockIdx.x / (a.nbc * a.nb1);
    // global position of local cell (0, 0, 0)
    const int G0 = a.ghost0 ? b0 * a.t0 - H : 0, G1 = a.ghost1 ? b1 * a.t1 - H : 0, C0 = a.ghostc ? bc * a.tc - H : 0;
    const int plane = S1 * 64;   // LDS distance of the x0 neighbours
    // units = row pairs (red-black) or rows (Jacobi), hp per plane; pass i of this wave is unit wave + W i
    const int hp = RB ? S1 >> 1 : S1, nunits = S0 * hp;
    const int l0_first = wave / hp, k_first = wave % hp;
    auto next_unit = [&](int &l0, int &k) {
        k += kBrickWaves;
        while (k >= hp) { k -= hp; ++l0; }   // (scalar)
    };

    // ---- load: the brick with its ghost shells, by the wave that will update the rows; cells outside the grid never change and
    // are never read by a cell that does (the faces are locked).  Jacobi: both arrays -- a row that is never updated is never copied.
    uint32_t lock_a = 0, lock_b = 0;   // bit i: this lane's cell of pass i is locked -- a: the row (Jacobi) or first row of the pair, b: its second
    const int gc = C0 + lane;
    {
        int l0 = l0_first, k = k_first;
        for (int i = 0, unit = wave; unit < nunits; ++i, unit += kBrickWaves) {
#pragma unroll
            for (int h = 0; h < (RB ? 2 : 1); ++h) {
                const int l1 = RB ? 2 * k + h : k;
                const int g0 = G0 + l0, g1 = G1 + l1;
                const bool inside = g0 >= 0 && g0 < a.m0 && g1 >= 0 && g1 < a.m1 && gc >= 0 && gc < a.pitch;
                float v = -1e6f;
                uint32_t lk = 1;
                if (inside) {
                    const size_t row = (size_t)g0 * a.m1 + g1;
                    v = a.in[row * a.pitch + gc];
                    lk = (a.maskw[mask_word_2d((unsigned)row, (unsigned)gc, (unsigned)a.pitch)] >> mask_bit_2d((unsigned)gc)) & 1u;
                }
                if (h == 0) lock_a |= lk << i;
                else lock_b |= lk << i;
                const int p = (l0 * S1 + l1) * 64 + lane;
                Split1 sp = {};
                if (TOL) sp = tol_split1(v);
#pragma unroll
                for (int b = 0; b < kBufs; ++b) {
                    u_lds[b * kCells + p] = v;
                    if (TOL) { q_lds[b * kCells + p] = sp.q; n_lds[b * kCells + p] = f2u(sp.zm); }
                }
            }
            next_unit(l0, k);
        }
    }
    if (MATH == kMathPrecise) math_tables_commit(tab_regs, reinterpret_cast<double *>(math_lds_bytes));
    if (TOL) TolLn<5>::stage(reinterpret_cast<TolLnEntry *>(math_lds_bytes));   // ends with a workgroup barrier
    else __syncthreads();

    // ---- K iterations on the brick
    // owned local cells [own_lo, own_hi) per axis (clipped to the grid): what the launch stores
    const int own0_lo = a.ghost0 ? H : 0, own0_hi = min(a.ghost0 ? S0 - H : S0, a.m0 - G0);
    const int own1_lo = a.ghost1 ? H : 0, own1_hi = min(a.ghost1 ? H + a.t1 : S1, a.m1 - G1);
    const bool own_col = (a.ghostc ? lane >= H && lane < 64 - H : true) && gc < a.pitch;
    for (int j = 0; j < a.steps; ++j) {
        // cells that still have six valid neighbours, off the faces of the grid: local [lo, hi] per axis
        const int lo0 = max(a.ghost0 ? j + 1 : 0, 1 - G0), hi0 = min(a.ghost0 ? S0 - 2 - j : S0 - 1, a.m0 - 2 - G0);
        const int lo1 = max(a.ghost1 ? j + 1 : 0, 1 - G1), hi1 = min(a.ghost1 ? S1 - 2 - j : S1 - 1, a.m1 - 2 - G1);
        const bool col_ok = a.ghostc ? lane >= j + 1 && lane <= 62 - j : true;   // (the faces along x2 are locked)
        const int src = RB ? 0 : (j & 1) * kCells, dst = RB ? 0 : ((j & 1) ^ 1) * kCells;
        int l0 = l0_first, k = k_first;
#pragma unroll 1
        for (int i = 0, unit = wave; unit < nunits; ++i, unit += kBrickWaves, next_unit(l0, k)) {
            if (l0 < lo0 || l0 > hi0) continue;   // wave-uniform
            bool upd;
            int p;
            if (RB) {
                const int r = 2 * k;
                const bool v0 = r >= lo1 && r <= hi1, v1 = r + 1 >= lo1 && r + 1 <= hi1;
                if (!(v0 || v1)) continue;   // wave-uniform: the pair has gone stale, lies on a face or outside the grid
                // the active cell of column gc in row (g0, g1) has (g0 + g1 + gc + iteration) even: of a pair that starts at an even
                // local row the lanes with (lane + bit) even take the first row, the others the second
                const int bit = (G0 + l0 + G1 + C0 + a.parity + j) & 1;
                const bool first = ((lane + bit) & 1) == 0;
                upd = (first ? v0 : v1) && col_ok && (((first ? lock_a : lock_b) >> i) & 1u) == 0;
                p = (l0 * S1 + r + (first ? 0 : 1)) * 64 + lane;
            } else {
                if (k < lo1 || k > hi1) continue;   // wave-uniform
                upd = col_ok && ((lock_a >> i) & 1u) == 0;
                p = (l0 * S1 + k) * 64 + lane;
            }
            const float c = u_lds[src + p];
            const float ua = u_lds[src + p - plane], ub = u_lds[src + p + plane], uu = u_lds[src + p - 64], ud = u_lds[src + p + 64],
                        ul = u_lds[src + p - 1], ur = u_lds[src + p + 1];
            float nv;
            if (TOL) {
                nv = tol_update_3d(ua, ub, uu, ud, ul, ur, q_lds[src + p - plane], n_lds[src + p - plane], q_lds[src + p + plane],
                                   n_lds[src + p + plane], q_lds[src + p - 64], n_lds[src + p - 64], q_lds[src + p + 64], n_lds[src + p + 64],
                                   q_lds[src + p - 1], n_lds[src + p - 1], q_lds[src + p + 1], n_lds[src + p + 1], tl);
            } else {
                nv = cell_update_3d<MATH>(ua, ub, uu, ud, ul, ur, tab);
            }
            const float o = upd ? nv : c;
            u_lds[dst + p] = o;
            if (TOL) {
                const Split1 sp = tol_split1(o);
                q_lds[dst + p] = sp.q;
                n_lds[dst + p] = f2u(sp.zm);
            }
        }
        __syncthreads();
    }

    // ---- store the owned cells (locked ones included: `out` is the other buffer)
    const int fin = RB ? 0 : (a.steps & 1) * kCells;
    const int n1 = max(own1_hi - own1_lo, 0), nrows = max(own0_hi - own0_lo, 0) * n1;   // (0: a brick beyond the grid)
    for (int r = wave; r < nrows; r += kBrickWaves) {
        const int l0 = own0_lo + r / n1, l1 = own1_lo + r % n1;
        if (own_col) a.out[((size_t)(G0 + l0) * a.m1 + (G1 + l1)) * a.pitch + gc] = u_lds[fin + (l0 * S1 + l1) * 64 + lane];
    }
}

}  // namespace

hipError_t launch_brick_3d(const float *in, float *out, const uint32_t *maskw, int m0, int m1, int pitch, const BrickPlan &plan, int steps,
                           int math, int parity, hipStream_t stream)
{
    if (steps <= 0) return hipSuccess;
    if (!in || !out || in == out || !maskw || pitch <= 0 || (pitch % 256) != 0 || m0 < 3 || m1 < 3) return hipErrorInvalidValue;
    if (math != kMathPrecise && math != kMathFast && math != kMathTol) return hipErrorInvalidValue;
    const bool rb = parity >= 0;
    const int max_rows = brick_3d_max_rows(math, rb);
    const int H = plan.halo;
    // everything the kernel's indexing relies on: the brick fits the LDS arrays, s1 is even, and per axis either the brick covers
    // the axis from its face or it owns t = s - 2 H >= 1 cells and the bricks together cover the axis
    if (H < 1 || steps > H || plan.s0 < 1 || plan.s1 < 2 || (plan.s1 & 1) || (long long)plan.s0 * plan.s1 > max_rows) return hipErrorInvalidValue;
    if (plan.nb0 < 1 || plan.nb1 < 1 || plan.nbc < 1 || (long long)plan.nb0 * plan.nb1 * plan.nbc > 0x7fffffffLL) return hipErrorInvalidValue;
    if (plan.ghost0 ? (plan.t0 < 1 || plan.t0 + 2 * H != plan.s0 || (long long)plan.nb0 * plan.t0 < m0) : (plan.nb0 != 1 || plan.s0 < m0)) return hipErrorInvalidValue;
    if (plan.ghost1 ? (plan.t1 < 1 || plan.t1 + 2 * H > plan.s1 || (long long)plan.nb1 * plan.t1 < m1) : (plan.nb1 != 1 || plan.s1 < m1)) return hipErrorInvalidValue;
    if (plan.ghostc ? (plan.tc != 64 - 2 * H || plan.tc < 1 || (long long)plan.nbc * plan.tc < plan.m2) : (plan.nbc != 1 || plan.m2 > 64)) return hipErrorInvalidValue;
    if (plan.m2 < 3 || plan.m2 > pitch) return hipErrorInvalidValue;
    Brick3dArgs a;
    a.in = in;
    a.out = out;
    a.maskw = maskw;
    a.m0 = m0;
    a.m1 = m1;
    a.pitch = pitch;
    a.halo = H;
    a.s0 = plan.s0;
    a.s1 = plan.s1;
    a.t0 = plan.t0;
    a.t1 = plan.t1;
    a.tc = plan.tc;
    a.nb1 = plan.nb1;
    a.nbc = plan.nbc;
    a.ghost0 = plan.ghost0;
    a.ghost1 = plan.ghost1;
    a.ghostc = plan.ghostc;
    a.steps = steps;
    a.parity = parity < 0 ? 0 : (parity & 1);
    void (*kernel)(Brick3dArgs);
    kernel = math == kMathTol    ? (rb ? brick3d_kernel<kMathTol, true, kBrickRowsTolRb> : brick3d_kernel<kMathTol, false, kBrickRowsTolJacobi>)
             : math == kMathFast ? (rb ? brick3d_kernel<kMathFast, true, kBrickRowsRb> : brick3d_kernel<kMathFast, false, kBrickRowsJacobi>)
                                 : (rb ? brick3d_kernel<kMathPrecise, true, kBrickRowsRb> : brick3d_kernel<kMathPrecise, false, kBrickRowsJacobi>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(plan.nb0 * plan.nb1 * plan.nbc)), dim3(kBrickThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace epic_hip
