// kernels_tile2d_batch_modes.hip -- SEVERAL 2-D fields of one grid shape per launch, in the modes kernels_tile2d_batch.hip does not
// have: the tol arithmetic (red-black and Jacobi), Jacobi with the precise arithmetic, and the fast arithmetic (gfx950).
//
// kernels_tile2d_batch.hip is the library's default mode -- precise, red-black -- and stays as it is, instruction for instruction.
// The callers that chose EPIC_HIP_MATH=tol for speed (the arithmetic bench.py times) or EPIC_HIP_SCHEME=jacobi, and hold a field
// per robot or per candidate goal, have the same independent work: this kernel is tile2d_kernel<MATH, RB, CW, RMAX> of
// kernels_tile2d.hip with the batch's field table, F fields of a group side by side in one workgroup of sixteen waves.
//
//   * blockIdx.x is the tile, blockIdx.y a group of F fields (BatchField entries, bufs[0] == nullptr: an empty slot, skipped
//     wave-uniformly).  The scalar stream of a step -- valid rows, owned lanes, colour, LDS offset -- is computed once per pass;
//     behind it come the LDS reads of all F fields, then F independent update chains, then F writes.  Lock masks are per field.
//   * tol: the split e^u = q 2^n of a cell is computed ONCE, by the lane that writes the cell, and kept in LDS beside u (q_lds,
//     n_lds) for the four cells it is a neighbour of -- as the single-field kernel does; recomputing it per step would be four
//     splits per cell update instead of one.  That triples a field's LDS.  The ln table (TolLn<4>, 16 KiB) is staged once per
//     workgroup and shared by its F fields.
//   * Jacobi: two copies of every plane, ping-pong per step (a register-held row window would tie a wave to consecutive rows; the
//     rows of a tile are dealt to the sixteen waves in turn so that the four waves of a SIMD cover each other's latencies).
//     Red-black runs in place.
//   * LDS per workgroup (a plane is (RMAX + 2) x 64 CW floats: 16.5 KiB narrow, 33 KiB wide at 64 rows, 65 KiB wide at 128 rows;
//     tables: 3 KiB precise, 16 KiB tol, none fast), and workgroups a CU's 160 KiB hold (sixteen waves each: two at the most):
//         tol red-black     narrow  F=1  49.5 + 16 =  65.5 KiB (2)   F=2  115 KiB (1)      wide (64 rows)  F=1  115 KiB (1)
//         tol Jacobi        narrow  F=1  99 + 16   = 115 KiB (1)     -- no F=2, and no wide tile (as the single-field kernel)
//         precise Jacobi    narrow  F=1  36 KiB (2)   F=2  69 KiB (2)   F=4  135 KiB (1)   wide (128 rows) F=1  133 KiB (1)
//         fast red-black    narrow  F=1  16.5 (2)     F=2  33 (2)       F=4  66 KiB (2)    wide (128 rows) F=1  65 (2)  F=2  130 KiB (1)
//         fast Jacobi       as precise Jacobi without the tables
//   * A check launch leaves max |du| of its LAST step over the owned cells per field and per tile, one plain store each into pinned
//     host memory, as the precise batch does.  A Jacobi check is a full sweep; EPIC_HIP_JACOBI_CHECKS=reference makes the check a
//     launch of its own through the red-black instantiation of the same arithmetic (batch2d_driver.hip).
//
// The cell update is cell_update.h's, the same function on the same values as tile2d_kernel: every field ends with the bits its own
// single call gives it (tests/test_gpu_batch2d_modes.py, tolerance 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_update.h"
#include "kernels.h"

namespace epic_hip {

namespace {

constexpr int kWaves = 16;   // as tile2d_kernel: the rows of a tile over sixteen waves, four per SIMD
constexpr int kThreads = 64 * kWaves;
constexpr lmask kOddLanes = 0xaaaaaaaaaaaaaaaaull;

struct TileModesArgs {
    const BatchField *fields;   // groups x F entries (the launcher's grid: blockIdx.y < groups)
    int src, dst;               // which of a field's three buffers this launch reads and writes (src != dst)
    int rows, pitch;
    int halo, tile_rows;        // H, T_r; owned columns per tile = LDS tile width - 2 H
    int tiles_c;
    int steps;                  // iterations of this launch, <= halo
    int parity;                 // red-black: number of the first iteration & 1
    int check;                  // the last step's max |du| per tile goes to BatchField::tile_delta[tile]
};

template <int MATH, bool RB, int F, int CW, int RMAX>
__global__ __launch_bounds__(kThreads) void tile2d_batch_modes_kernel(TileModesArgs a)
{
    constexpr bool TOL = MATH == kMathTol;
    constexpr int kBufs = RB ? 1 : 2;
    constexpr int kTileCols = 64 * CW;
    constexpr int kUnits = (RB ? RMAX / 2 : RMAX) * CW;       // (row pair | row) x column block
    constexpr int kPasses = (kUnits + kWaves - 1) / kWaves;   // units per wave
    constexpr int kSlots = RB ? 2 * kPasses : kPasses;        // rows a lane may update
    constexpr int kPlane = (RMAX + 2) * kTileCols;   // one pad row above and below: the neighbours of a stale edge cell stay inside
    constexpr int kField = kBufs * kPlane;           // floats of one field: its plane, twice for Jacobi
    constexpr int kTableBytes = TOL ? TolLn<4>::kLdsBytes : kMathLdsDoubles * (int)sizeof(double);
    static_assert((size_t)F * kField * sizeof(float) * (TOL ? 3 : 1) + kTableBytes <= 160 * 1024 - 256, "the tiles of F fields fit the LDS of a CU");
    __shared__ float u_lds[F * kField];
    __shared__ float q_lds[TOL ? F * kField : 1];
    __shared__ uint32_t n_lds[TOL ? F * kField : 1];
    __shared__ unsigned wg_delta[F];
    __shared__ __attribute__((aligned(16))) char math_lds_bytes[kTableBytes];
    const TolLnEntry *const tl = reinterpret_cast<const TolLnEntry *>(math_lds_bytes);
    const MathTab tab = math_tables_at(reinterpret_cast<double *>(math_lds_bytes), kConstsPlain);
    MathTabRegs tab_regs = {};
    if (MATH == kMathPrecise) tab_regs = math_tables_fetch();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tr = blockIdx.x / a.tiles_c, tc = blockIdx.x % a.tiles_c;
    const int H = a.halo, Sr = a.tile_rows + 2 * H, Tc = kTileCols - 2 * H;
    const int R0 = tr * a.tile_rows - H, C0 = tc * Tc - H;   // global position of local cell (0, 0)
    auto at = [](int lr, int lc) { return (lr + 1) * kTileCols + lc; };
    auto unit_row = [&](int i) { return (wave + kWaves * i) / CW; };   // row pair (red-black) or row (Jacobi) of pass i of this wave
    auto unit_blk = [&](int i) { return (wave + kWaves * i) % CW; };   // column block: local columns 64 blk .. 64 blk + 63
    auto slot_row = [&](int k) { return RB ? 2 * unit_row(k >> 1) + (k & 1) : unit_row(k); };
    auto slot_blk = [&](int k) { return unit_blk(RB ? k >> 1 : k); };

    // ---- the fields of this group (wave-uniform)
    const float *in[F];
    float *out[F];
    const uint32_t *maskw[F];
    float *tile_delta[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const BatchField &bf = a.fields[blockIdx.y * F + f];
        in[f] = bf.bufs[0] ? bf.bufs[a.src] : nullptr;
        out[f] = bf.bufs[a.dst];
        maskw[f] = bf.maskw;
        tile_delta[f] = bf.tile_delta;
    }

    // ---- load: the tile of every field with its ghost ring (cells outside the grid never change and are never read by a cell
    // that does), tol: with the split of every cell; the locks of the rows a wave will update stay with it as lane masks, per field
    lmask lockm[F][kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int lr = slot_row(k), lc = 64 * slot_blk(k) + lane;
        const int gr = R0 + lr, gc = C0 + lc;
        const bool inside = lr < Sr && gc >= 0 && gc < a.pitch && gr >= 0 && gr < a.rows;
        const size_t cell = (size_t)gr * a.pitch + gc;
        const size_t word = mask_word_2d((unsigned)gr, (unsigned)gc, (unsigned)a.pitch);
        const unsigned bit = mask_bit_2d((unsigned)gc);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            lockm[f][k] = ~0ull;
            if (lr >= Sr || in[f] == nullptr) continue;   // wave-uniform
            float v = -1e6f;
            uint32_t lk = 1;
            if (inside) {
                v = in[f][cell];
                lk = (maskw[f][word] >> bit) & 1u;
            }
            lockm[f][k] = __builtin_amdgcn_ballot_w64(lk != 0);
            u_lds[f * kField + at(lr, lc)] = v;
            if (TOL) {
                const Split1 sp = tol_split1(v);
                q_lds[f * kField + at(lr, lc)] = sp.q;
                n_lds[f * kField + at(lr, lc)] = f2u(sp.zm);
            }
        }
    }
    if (threadIdx.x < 2 * kTileCols) {   // the pad rows: read by the (discarded) updates of the outermost ring only
        const int lr = threadIdx.x < kTileCols ? -1 : Sr, lc = threadIdx.x % kTileCols;
#pragma unroll
        for (int fb = 0; fb < F * kBufs; ++fb) {   // (every plane of every field)
            u_lds[fb * kPlane + at(lr, lc)] = -1e6f;
            if (TOL) { q_lds[fb * kPlane + at(lr, lc)] = 1.0f; n_lds[fb * kPlane + at(lr, lc)] = kTolMagicBits; }
        }
    }
    if (threadIdx.x < F) wg_delta[threadIdx.x] = 0;
    if (MATH == kMathPrecise) math_tables_commit(tab_regs, reinterpret_cast<double *>(math_lds_bytes));
    if (TOL) TolLn<4>::stage(reinterpret_cast<TolLnEntry *>(math_lds_bytes));   // once for the F fields; ends with a workgroup barrier
    else __syncthreads();

    // ---- K iterations on the tiles
    const int own_r0 = H, own_r1 = H + a.tile_rows;   // owned local rows [own_r0, own_r1), columns [H, width - H)
    // lanes of column block blk whose local column lies in [lo, width - lo)
    auto cols_from = [&](int blk, int lo) -> lmask { return (blk == 0 ? ~0ull << lo : ~0ull) & (blk == CW - 1 ? ~0ull >> lo : ~0ull); };
    const int odd_lane = lane & 1;
    float dmax[F];
#pragma unroll
    for (int f = 0; f < F; ++f) dmax[f] = 0.0f;
    for (int j = 0; j < a.steps; ++j) {
        // cells that still have four valid neighbours: local rows [lo, hi_r], columns [lo, width - 1 - lo]
        const int lo = j + 1, hi_r = Sr - 2 - j;
        const bool check = a.check && j == a.steps - 1;
        const int src = RB ? 0 : (j & 1) * kPlane, dst = RB ? 0 : ((j & 1) ^ 1) * kPlane;
        // red-black: the active cell of column gc in global row gr has (gr + gc + iteration) odd (harmonic_cpu.cpp:46-51); in a row
        // pair that starts at an even local row the lanes with (lane + b) odd take the first row, the others the second
        const int b = (R0 + C0 + a.parity + j) & 1;
        const lmask first_row = b ? ~kOddLanes : kOddLanes;
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            // the scalar stream, once for all fields
            lmask valid, own;
            int p;
            const int blk = unit_blk(i);
            if (RB) {
                const int r2 = 2 * unit_row(i);
                const bool v0 = r2 >= lo && r2 <= hi_r, v1 = r2 + 1 >= lo && r2 + 1 <= hi_r;
                if (!(v0 || v1)) continue;   // wave-uniform: the pair has gone stale (or lies beyond the tile)
                valid = ((v0 ? first_row : 0ull) | (v1 ? ~first_row : 0ull)) & cols_from(blk, lo);
                own = ((r2 >= own_r0 && r2 < own_r1 ? first_row : 0ull) | (r2 + 1 >= own_r0 && r2 + 1 < own_r1 ? ~first_row : 0ull)) & cols_from(blk, H);
                p = at(r2, 64 * blk + lane) + ((odd_lane ^ b) ? 0 : kTileCols);
            } else {
                const int lr = unit_row(i);
                if (lr < lo || lr > hi_r) continue;   // wave-uniform
                valid = cols_from(blk, lo);
                own = lr >= own_r0 && lr < own_r1 ? cols_from(blk, H) : 0ull;
                p = at(lr, 64 * blk + lane);
            }
            // F vector chains behind it: all the reads, then the updates, then the writes
            float c[F], uu[F], ud[F], ul[F], ur[F], qu[F], qd[F], ql[F], qr[F];
            uint32_t nu[F], nd[F], nl[F], nr[F];
#pragma unroll
            for (int f = 0; f < F; ++f) {
                if (in[f] == nullptr) continue;   // wave-uniform
                const int s = f * kField + src + p;
                c[f] = u_lds[s];
                uu[f] = u_lds[s - kTileCols];
                ud[f] = u_lds[s + kTileCols];
                ul[f] = u_lds[s - 1];
                ur[f] = u_lds[s + 1];
                if (TOL) {
                    qu[f] = q_lds[s - kTileCols]; nu[f] = n_lds[s - kTileCols];
                    qd[f] = q_lds[s + kTileCols]; nd[f] = n_lds[s + kTileCols];
                    ql[f] = q_lds[s - 1];         nl[f] = n_lds[s - 1];
                    qr[f] = q_lds[s + 1];         nr[f] = n_lds[s + 1];
                }
            }
#pragma unroll
            for (int f = 0; f < F; ++f) {
                if (in[f] == nullptr) continue;
                const lmask lock = RB ? (lockm[f][2 * i] & first_row) | (lockm[f][2 * i + 1] & ~first_row) : lockm[f][i];
                float nv;
                if (TOL) nv = tol_update_2d(uu[f], ud[f], ul[f], ur[f], qu[f], nu[f], qd[f], nd[f], ql[f], nl[f], qr[f], nr[f], tl);
                else nv = cell_update_2d<MATH>(uu[f], ud[f], ul[f], ur[f], tab);
                const float o = sel(valid & ~lock, nv, c[f]);
                const int d = f * kField + dst + p;
                u_lds[d] = o;
                if (TOL) {
                    const Split1 sp = tol_split1(o);
                    q_lds[d] = sp.q;
                    n_lds[d] = f2u(sp.zm);
                }
                if (check) dmax[f] = max2(dmax[f], sel(own, fabsf(c[f] - o), 0.0f));   // (wave-uniform branch)
            }
        }
        __syncthreads();
    }

    // ---- store the owned cells (locked ones included: `out` is another buffer)
    const int fin = RB ? 0 : (a.steps & 1) * kPlane;
    for (int unit = own_r0 * CW + wave; unit < own_r1 * CW; unit += kWaves) {   // (row, column block) units of the owned rows
        const int lr = unit / CW, lc = 64 * (unit % CW) + lane;
        const int gr = R0 + lr, gc = C0 + lc;
        if (gr >= a.rows) break;   // wave-uniform
        if (lc >= H && lc < kTileCols - H && gc < a.pitch) {
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (in[f] != nullptr) out[f][(size_t)gr * a.pitch + gc] = u_lds[f * kField + fin + at(lr, lc)];
        }
    }
    if (a.check) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if (in[f] == nullptr) continue;
            const float d = wave_max(dmax[f]);
            if (lane == 0 && d > 0.0f) atomicMax(&wg_delta[f], __float_as_uint(d));
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < F; ++f)
            if (threadIdx.x == f && in[f] != nullptr) tile_delta[f][blockIdx.x] = __uint_as_float(wg_delta[f]);
    }
}

using Kernel = void (*)(TileModesArgs);

// the instantiations of one arithmetic and scheme: narrow tile F = 1, 2, 4 and wide tile (WR rows) F = 1, 2, as far as they fit the LDS
template <int MATH, bool RB, int NF, int WR, int WF> Kernel pick(int width, int F)
{
    if (width == kTile2dCols) {
        if (F == 1) return tile2d_batch_modes_kernel<MATH, RB, 1, 1, 64>;
        if constexpr (NF >= 2) if (F == 2) return tile2d_batch_modes_kernel<MATH, RB, 2, 1, 64>;
        if constexpr (NF >= 4) if (F == 4) return tile2d_batch_modes_kernel<MATH, RB, 4, 1, 64>;
    } else if constexpr (WF >= 1) {
        if (F == 1) return tile2d_batch_modes_kernel<MATH, RB, 1, 2, WR>;
        if constexpr (WF >= 2) if (F == 2) return tile2d_batch_modes_kernel<MATH, RB, 2, 2, WR>;
    }
    return nullptr;
}

}  // namespace

int tile_2d_batch_modes_max_fields(int math, bool redblack, int width)
{
    const bool narrow = width == kTile2dCols;
    if (!narrow && width != kTile2dWideCols) return 0;
    if (math == kMathTol) return redblack ? (narrow ? 2 : 1) : (narrow ? 1 : 0);
    if (math == kMathFast) return redblack ? (narrow ? 4 : 2) : (narrow ? 4 : 1);
    if (math == kMathPrecise && !redblack) return narrow ? 4 : 1;
    return 0;   // (precise red-black: kernels_tile2d_batch.hip)
}

hipError_t launch_tile_2d_batch_modes(const BatchField *d_fields, int groups, int fields_per_group, int src, int dst, int rows, int pitch,
                                      const TilePlan &plan, int steps, int math, int parity, bool check, hipStream_t stream)
{
    if (steps <= 0) return hipSuccess;
    if (!d_fields || groups < 1 || groups > 65535 || src == dst || src < 0 || src > 2 || dst < 0 || dst > 2 || pitch <= 0 ||
        (pitch % 256) != 0 || rows <= 0)
        return hipErrorInvalidValue;
    const bool rb = parity >= 0;
    const int width = plan.tile_cols + 2 * plan.halo, max_rows = tile_2d_max_rows(math, rb, width);
    const int F = fields_per_group;
    if (plan.halo < 1 || steps > plan.halo || plan.tile_rows < 2 || max_rows == 0 || plan.tile_rows + 2 * plan.halo > max_rows ||
        plan.tile_cols < 8 || plan.tiles_r < 1 || plan.tiles_c < 1 || (long long)plan.tiles_r * plan.tile_rows < rows ||
        (F != 1 && F != 2 && F != 4) || F > tile_2d_batch_modes_max_fields(math, rb, width))
        return hipErrorInvalidValue;
    TileModesArgs a;
    a.fields = d_fields;
    a.src = src;
    a.dst = dst;
    a.rows = rows;
    a.pitch = pitch;
    a.halo = plan.halo;
    a.tile_rows = plan.tile_rows;
    a.tiles_c = plan.tiles_c;
    a.steps = steps;
    a.parity = rb ? (parity & 1) : 0;
    a.check = check ? 1 : 0;
    Kernel kernel = nullptr;
    if (math == kMathTol) kernel = rb ? pick<kMathTol, true, 2, 64, 1>(width, F) : pick<kMathTol, false, 1, 64, 0>(width, F);
    else if (math == kMathFast) kernel = rb ? pick<kMathFast, true, 4, 128, 2>(width, F) : pick<kMathFast, false, 4, 128, 1>(width, F);
    else if (math == kMathPrecise && !rb) kernel = pick<kMathPrecise, false, 4, 128, 1>(width, F);
    if (!kernel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(plan.tiles_r * plan.tiles_c), (unsigned)groups), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace epic_hip
