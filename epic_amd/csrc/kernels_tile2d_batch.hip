// kernels_tile2d_batch.hip -- SEVERAL 2-D fields on one grid shape: the LDS tiles of kernels_tile2d.hip, batched (gfx950).
//
// One field of 0.06-1 Mcell leaves the chip mostly idle: a few dozen tiles for 256 CUs, and the sixteen waves of a tile wait at
// s_waitcnt for half their cycles.  A caller with several goals on one map -- a field per robot, per candidate
// goal, per hypothesis of a door being open -- has independent work: the fields share the grid's shape and nothing else (goals are
// locked cells, so even the masks differ).  This kernel relaxes them side by side:
//
//   * blockIdx.x is the tile (as in tile2d_kernel), blockIdx.y a GROUP of F fields.  A workgroup of sixteen waves holds the same
//     tile of its F fields in LDS, (RMAX + 2) x 64 CW floats per field (narrow tile: 16.9 KB, F <= 4; wide tile: 66.5 KB, F <= 2 of
//     the 160 KB), and the precise routines' tables once.
//   * The geometry of a step -- which rows are still valid, which lanes own a cell, the colour of a lane, the LDS offset of the
//     lane's cell -- is the same for every field of the group: the scalar stream of lane masks is computed ONCE per pass, and behind
//     it the wave reads the neighbours of all F fields, runs F independent update chains and writes F results.  Only the lock
//     masks are per field (lockm[F][kSlots], wave-uniform).  They do not all fit the scalar file: no instantiation uses scratch,
//     but the compiler parks 14 (F = 2 narrow), 56 (F = 4 narrow), 54 (F = 1 wide) and 167 (F = 2 wide) scalar registers in lanes
//     of vector registers, so part of the "scalar" stream is v_readlane / v_writelane traffic.
//   * The fields of a launch come from a table in device memory, one entry per field slot (BatchField: the context's three u
//     buffers, its lane masks, where its per-tile maxima go); the launch says which buffer is read and which written.  The pointers
//     are wave-uniform plain loads.  The last group may have empty slots (bufs[0] == nullptr): skipped wave-uniformly -- no
//     loads, no stores, no delta.
//   * A check launch leaves max |du| of its LAST step over the owned cells per field and per tile, one plain store each into
//     pinned host memory: nothing to zero, no atomics on one word, the host reduces per field.
//
// Red-black with the precise arithmetic only (the library's default mode, the one that is harmonic_complete_cpu bit for bit); the
// cell update is cell_update.h's cell_update_2d<kMathPrecise>, the same function on the same values as tile2d_kernel: every field
// ends with the bits the single-field kernels give it (tests/test_gpu_batch2d.py, tolerance 0).  F = 1 is the plain instantiation:
// a field per blockIdx.y, nothing interleaved.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_update.h"
#include "kernels.h"

namespace epic_hip {

namespace {

constexpr int kBatchWaves = 16;   // as tile2d_kernel: the row pairs of a tile over sixteen waves, four per SIMD
constexpr int kBatchThreads = 64 * kBatchWaves;
constexpr lmask kOddLanes = 0xaaaaaaaaaaaaaaaaull;

struct TileBatchArgs {
    const BatchField *fields;   // groups x F entries (the launcher's grid: blockIdx.y < groups)
    int src, dst;               // which of a field's three buffers this launch reads and writes (src != dst)
    int rows, pitch;
    int halo, tile_rows;        // H, T_r; owned columns per tile = LDS tile width - 2 H
    int tiles_c;
    int steps;                  // iterations of this launch, <= halo
    int parity;                 // number of the first iteration & 1
    int check;                  // the last step's max |du| per tile goes to BatchField::tile_delta[tile]
};

// CW, RMAX: the LDS tile is 64 CW columns wide and at most RMAX rows tall, as in tile2d_kernel.
template <int F, int CW, int RMAX>
__global__ __launch_bounds__(kBatchThreads) void tile2d_batch_kernel(TileBatchArgs a)
{
    constexpr int kTileCols = 64 * CW;
    constexpr int kUnits = RMAX / 2 * CW;                               // row pair x column block
    constexpr int kPasses = (kUnits + kBatchWaves - 1) / kBatchWaves;   // units per wave
    constexpr int kSlots = 2 * kPasses;                                 // rows a lane may update
    constexpr int kPlane = (RMAX + 2) * kTileCols;   // one pad row above and below: the neighbours of a stale edge cell stay inside
    static_assert((size_t)F * kPlane * sizeof(float) + kMathLdsDoubles * sizeof(double) <= 160 * 1024 - 256, "the tiles of F fields fit the LDS of a CU");
    __shared__ float u_lds[F * kPlane];
    __shared__ unsigned wg_delta[F];
    __shared__ __attribute__((aligned(16))) double math_lds[kMathLdsDoubles];
    const MathTab tab = math_tables_at(math_lds, kConstsPlain);
    const MathTabRegs tab_regs = math_tables_fetch();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tr = blockIdx.x / a.tiles_c, tc = blockIdx.x % a.tiles_c;
    const int H = a.halo, Sr = a.tile_rows + 2 * H, Tc = kTileCols - 2 * H;
    const int R0 = tr * a.tile_rows - H, C0 = tc * Tc - H;   // global position of local cell (0, 0)
    auto at = [](int lr, int lc) { return (lr + 1) * kTileCols + lc; };
    auto unit_row = [&](int i) { return (wave + kBatchWaves * i) / CW; };   // row pair of pass i of this wave
    auto unit_blk = [&](int i) { return (wave + kBatchWaves * i) % CW; };   // column block: local columns 64 blk .. 64 blk + 63
    auto slot_row = [&](int k) { return 2 * unit_row(k >> 1) + (k & 1); };   // the two rows of pass i's pair are slots 2 i, 2 i + 1

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
    // that does); the locks of the rows a wave will update stay with it as lane masks in scalar registers, per field
    lmask lockm[F][kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int lr = slot_row(k), lc = 64 * unit_blk(k >> 1) + lane;
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
            u_lds[f * kPlane + at(lr, lc)] = v;
        }
    }
    if (threadIdx.x < 2 * kTileCols) {   // the pad rows: read by the (discarded) updates of the outermost ring only
        const int lr = threadIdx.x < kTileCols ? -1 : Sr, lc = threadIdx.x % kTileCols;
#pragma unroll
        for (int f = 0; f < F; ++f) u_lds[f * kPlane + at(lr, lc)] = -1e6f;
    }
    if (threadIdx.x < F) wg_delta[threadIdx.x] = 0;
    math_tables_commit(tab_regs, math_lds);
    __syncthreads();

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
        // the active cell of column gc in global row gr has (gr + gc + iteration) odd (harmonic_cpu.cpp:46-51); in a row pair that
        // starts at an even local row the lanes with (lane + b) odd take the first row, the others the second
        const int b = (R0 + C0 + a.parity + j) & 1;
        const lmask first_row = b ? ~kOddLanes : kOddLanes;
#pragma unroll
        for (int i = 0; i < kPasses; ++i) {
            // the scalar stream, once for all fields
            const int blk = unit_blk(i), r2 = 2 * unit_row(i);
            const bool v0 = r2 >= lo && r2 <= hi_r, v1 = r2 + 1 >= lo && r2 + 1 <= hi_r;
            if (!(v0 || v1)) continue;   // wave-uniform: the pair has gone stale (or lies beyond the tile)
            const lmask valid = ((v0 ? first_row : 0ull) | (v1 ? ~first_row : 0ull)) & cols_from(blk, lo);
            const lmask own = ((r2 >= own_r0 && r2 < own_r1 ? first_row : 0ull) | (r2 + 1 >= own_r0 && r2 + 1 < own_r1 ? ~first_row : 0ull)) & cols_from(blk, H);
            const int p = at(r2, 64 * blk + lane) + ((odd_lane ^ b) ? 0 : kTileCols);
            // F vector chains behind it: all the reads, then the updates, then the writes
            float c[F], uu[F], ud[F], ul[F], ur[F];
#pragma unroll
            for (int f = 0; f < F; ++f) {
                if (in[f] == nullptr) continue;   // wave-uniform
                const float *u = u_lds + f * kPlane + p;
                c[f] = u[0];
                uu[f] = u[-kTileCols];
                ud[f] = u[kTileCols];
                ul[f] = u[-1];
                ur[f] = u[1];
            }
#pragma unroll
            for (int f = 0; f < F; ++f) {
                if (in[f] == nullptr) continue;
                const lmask lock = (lockm[f][2 * i] & first_row) | (lockm[f][2 * i + 1] & ~first_row);
                const float nv = cell_update_2d<kMathPrecise>(uu[f], ud[f], ul[f], ur[f], tab);
                const float o = sel(valid & ~lock, nv, c[f]);
                u_lds[f * kPlane + p] = o;
                if (check) dmax[f] = max2(dmax[f], sel(own, fabsf(c[f] - o), 0.0f));   // (wave-uniform branch)
            }
        }
        __syncthreads();
    }

    // ---- store the owned cells (locked ones included: `out` is another buffer)
    for (int unit = own_r0 * CW + wave; unit < own_r1 * CW; unit += kBatchWaves) {   // (row, column block) units of the owned rows
        const int lr = unit / CW, lc = 64 * (unit % CW) + lane;
        const int gr = R0 + lr, gc = C0 + lc;
        if (gr >= a.rows) break;   // wave-uniform
        if (lc >= H && lc < kTileCols - H && gc < a.pitch) {
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (in[f] != nullptr) out[f][(size_t)gr * a.pitch + gc] = u_lds[f * kPlane + at(lr, lc)];
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

}  // namespace

int tile_2d_batch_max_fields(int width) { return width == kTile2dCols ? 4 : width == kTile2dWideCols ? 2 : 0; }

hipError_t launch_tile_2d_batch(const BatchField *d_fields, int groups, int fields_per_group, int src, int dst, int rows, int pitch,
                                const TilePlan &plan, int steps, int parity, bool check, hipStream_t stream)
{
    if (steps <= 0) return hipSuccess;
    if (!d_fields || groups < 1 || groups > 65535 || src == dst || src < 0 || src > 2 || dst < 0 || dst > 2 || pitch <= 0 ||
        (pitch % 256) != 0 || rows <= 0)
        return hipErrorInvalidValue;
    const int width = plan.tile_cols + 2 * plan.halo, max_rows = tile_2d_max_rows(0, true, width);
    const int F = fields_per_group;
    if (plan.halo < 1 || steps > plan.halo || plan.tile_rows < 2 || max_rows == 0 || plan.tile_rows + 2 * plan.halo > max_rows ||
        plan.tile_cols < 8 || plan.tiles_r < 1 || plan.tiles_c < 1 || (long long)plan.tiles_r * plan.tile_rows < rows ||
        (F != 1 && F != 2 && F != 4) || F > tile_2d_batch_max_fields(width))
        return hipErrorInvalidValue;
    TileBatchArgs a;
    a.fields = d_fields;
    a.src = src;
    a.dst = dst;
    a.rows = rows;
    a.pitch = pitch;
    a.halo = plan.halo;
    a.tile_rows = plan.tile_rows;
    a.tiles_c = plan.tiles_c;
    a.steps = steps;
    a.parity = parity & 1;
    a.check = check ? 1 : 0;
    void (*kernel)(TileBatchArgs);
    if (width == kTile2dCols) kernel = F == 1 ? tile2d_batch_kernel<1, 1, 64> : F == 2 ? tile2d_batch_kernel<2, 1, 64> : tile2d_batch_kernel<4, 1, 64>;
    else kernel = F == 1 ? tile2d_batch_kernel<1, 2, 128> : tile2d_batch_kernel<2, 2, 128>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(plan.tiles_r * plan.tiles_c), (unsigned)groups), dim3(kBatchThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace epic_hip
