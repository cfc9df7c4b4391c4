// kernels_brick3d_batch.hip -- SEVERAL 3-D fields on one grid shape: the LDS bricks of kernels_brick3d.hip, batched (gfx950).
//
// One voxel field of 32^3 ... 96^3 is a handful of bricks for 256 CUs (brick3d_kernel's 150 KB of LDS leave a CU room for one
// workgroup), and its callers -- a field per candidate goal, per robot -- have many such fields on one box.  They share the grid's
// shape and nothing else: goals are locked cells, so even the masks differ.  This kernel relaxes them side by side, the 3-D
// counterpart of kernels_tile2d_batch.hip:
//
//   * blockIdx.x is the brick (decoded as in brick3d_kernel), blockIdx.y a slot of a field table in device memory (BatchField: the
//     context's three u buffers, its lane masks, where its per-brick maxima go); the launch says which buffer is read and which
//     written.  ONE field per workgroup: interleaving fields in a workgroup bought nothing in 2-D.  An empty
//     slot (bufs[0] == nullptr) is left by the whole workgroup before its first barrier.
//   * The geometry of a launch -- brick shape, shells, owned ranges, the validity that shrinks by one shell per step, the colour of a
//     lane, LDS offsets -- comes from the launch arguments and is the same for every field; only the loaded values and the lock bits
//     (one bit per pass in two registers of every lane, as in brick3d_kernel) are the field's.
//   * The LDS capacity is a template parameter: 576 rows of 64 cells (147 KB: the single-field kernel's brick, one workgroup per CU)
//     and 288 rows (74 KB + 3 KB of tables: TWO workgroups per CU, so one's barrier and LDS latency hide behind the other's issue).
//     Which serves a launch is the plan's decision (batch2d_driver.hip: batch_brick_plan).
//   * A check launch leaves max |du| of its LAST step per field and per brick, over the cells the brick owns and updated: reduced in
//     the wave, the sixteen wave maxima combined through LDS, one plain store by wave 0 into pinned host memory -- nothing to zero,
//     no atomics, the host reduces per field.  Ghost cells never count: their owner recomputes them, and the outermost are stale.
//
// Red-black with the precise arithmetic only (the library's default mode, harmonic_complete_cpu bit for bit): cell_update.h's
// cell_update_3d<kMathPrecise> on the same values in the same operand order as kernels_3d.hip and kernels_brick3d.hip (x0 - 1,
// x0 + 1, x1 - 1, x1 + 1, x2 - 1, x2 + 1), so every field ends with the bits the single-field kernels give it, and the maximum over
// a field's bricks is sweep3d_kernel<CHECK>'s delta (tests/test_gpu_batch3d.py, tolerance 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_update.h"
#include "kernels.h"

namespace epic_hip {

namespace {

constexpr int kWaves = 16;   // as brick3d_kernel: the row pairs of a brick dealt to sixteen waves in turn, four per SIMD
constexpr int kThreads = 64 * kWaves;

struct BrickBatchArgs {
    const BatchField *fields;   // one entry per blockIdx.y
    int src, dst;               // which of a field's three buffers this launch reads and writes (src != dst)
    int m0, m1, pitch;
    int halo;
    int s0, s1;                 // the brick in LDS: planes and rows (s1 even)
    int t0, t1, tc;             // cells a brick owns along each axis
    int nb1, nbc;               // bricks along x1 and x2
    int ghost0, ghost1, ghostc; // whether the axis carries ghost shells (else the brick starts at the face and covers the axis)
    int steps;                  // iterations of this launch, <= halo
    int parity;                 // number of the first iteration & 1
    int check;                  // the last step's max |du| per brick goes to BatchField::tile_delta[brick]
};

// ROWS: rows of 64 cells the LDS array holds (s0 * s1 <= ROWS).
template <int ROWS>
__global__ __launch_bounds__(kThreads) void brick3d_batch_kernel(BrickBatchArgs a)
{
    static_assert((ROWS / 2 + kWaves - 1) / kWaves <= 32, "one lock bit per pass in a 32-bit register");
    static_assert((size_t)ROWS * 64 * sizeof(float) + kMathLdsDoubles * sizeof(double) + kWaves * sizeof(float) <= 160 * 1024, "the brick fits the LDS of a CU");
    __shared__ float u_lds[ROWS * 64];
    __shared__ float wave_delta[kWaves];
    __shared__ __attribute__((aligned(16))) double math_lds[kMathLdsDoubles];

    // ---- the field of this workgroup (wave-uniform plain loads); an empty slot is left before the first barrier
    const BatchField &bf = a.fields[blockIdx.y];
    if (bf.bufs[0] == nullptr) return;
    const float *const in = bf.bufs[a.src];
    float *const out = bf.bufs[a.dst];
    const uint32_t *const maskw = bf.maskw;

    const MathTab tab = math_tables_at(math_lds, kConstsPlain);
    const MathTabRegs tab_regs = math_tables_fetch();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H = a.halo, S0 = a.s0, S1 = a.s1;
    const int bc = blockIdx.x % a.nbc, b1 = (blockIdx.x / a.nbc) % a.nb1, b0 = blockIdx.x / (a.nbc * a.nb1);
    // global position of local cell (0, 0, 0)
    const int G0 = a.ghost0 ? b0 * a.t0 - H : 0, G1 = a.ghost1 ? b1 * a.t1 - H : 0, C0 = a.ghostc ? bc * a.tc - H : 0;
    const int plane = S1 * 64;   // LDS distance of the x0 neighbours
    // units = row pairs, hp per plane; pass i of this wave is unit wave + 16 i
    const int hp = S1 >> 1, nunits = S0 * hp;
    const int l0_first = wave / hp, k_first = wave % hp;
    auto next_unit = [&](int &l0, int &k) {
        k += kWaves;
        while (k >= hp) { k -= hp; ++l0; }   // (scalar)
    };

    // ---- load: the brick with its ghost shells, by the wave that will update the rows; cells outside the grid never change and are
    // never read by a cell that does (the faces are locked)
    uint32_t lock_a = 0, lock_b = 0;   // bit i: this lane's cell of pass i is locked -- a: the first row of the pair, b: the second
    const int gc = C0 + lane;
    {
        int l0 = l0_first, k = k_first;
        for (int i = 0, unit = wave; unit < nunits; ++i, unit += kWaves) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int l1 = 2 * k + h;
                const int g0 = G0 + l0, g1 = G1 + l1;
                const bool inside = g0 >= 0 && g0 < a.m0 && g1 >= 0 && g1 < a.m1 && gc >= 0 && gc < a.pitch;
                float v = -1e6f;
                uint32_t lk = 1;
                if (inside) {
                    const size_t row = (size_t)g0 * a.m1 + g1;
                    v = in[row * a.pitch + gc];
                    lk = (maskw[mask_word_2d((unsigned)row, (unsigned)gc, (unsigned)a.pitch)] >> mask_bit_2d((unsigned)gc)) & 1u;
                }
                if (h == 0) lock_a |= lk << i;
                else lock_b |= lk << i;
                u_lds[(l0 * S1 + l1) * 64 + lane] = v;
            }
            next_unit(l0, k);
        }
    }
    math_tables_commit(tab_regs, math_lds);
    __syncthreads();

    // ---- K iterations on the brick
    // owned local cells [own_lo, own_hi) per axis (clipped to the grid): what the launch stores, and what a check counts
    const int own0_lo = a.ghost0 ? H : 0, own0_hi = min(a.ghost0 ? S0 - H : S0, a.m0 - G0);
    const int own1_lo = a.ghost1 ? H : 0, own1_hi = min(a.ghost1 ? H + a.t1 : S1, a.m1 - G1);
    const bool own_col = (a.ghostc ? lane >= H && lane < 64 - H : true) && gc < a.pitch;
    float dmax = 0.0f;
    for (int j = 0; j < a.steps; ++j) {
        // cells that still have six valid neighbours, off the faces of the grid: local [lo, hi] per axis
        const int lo0 = max(a.ghost0 ? j + 1 : 0, 1 - G0), hi0 = min(a.ghost0 ? S0 - 2 - j : S0 - 1, a.m0 - 2 - G0);
        const int lo1 = max(a.ghost1 ? j + 1 : 0, 1 - G1), hi1 = min(a.ghost1 ? S1 - 2 - j : S1 - 1, a.m1 - 2 - G1);
        const bool col_ok = a.ghostc ? lane >= j + 1 && lane <= 62 - j : true;   // (the faces along x2 are locked)
        const bool check = a.check && j == a.steps - 1;   // (wave-uniform)
        int l0 = l0_first, k = k_first;
#pragma unroll 1
        for (int i = 0, unit = wave; unit < nunits; ++i, unit += kWaves, next_unit(l0, k)) {
            if (l0 < lo0 || l0 > hi0) continue;   // wave-uniform
            const int r = 2 * k;
            const bool v0 = r >= lo1 && r <= hi1, v1 = r + 1 >= lo1 && r + 1 <= hi1;
            if (!(v0 || v1)) continue;   // wave-uniform: the pair has gone stale, lies on a face or outside the grid
            // the active cell of column gc in row (g0, g1) has (g0 + g1 + gc + iteration) even: of a pair that starts at an even local
            // row the lanes with (lane + bit) even take the first row, the others the second
            const int bit = (G0 + l0 + G1 + C0 + a.parity + j) & 1;
            const bool first = ((lane + bit) & 1) == 0;
            const bool upd = (first ? v0 : v1) && col_ok && (((first ? lock_a : lock_b) >> i) & 1u) == 0;
            // every row that IS updated has its x0 and x1 neighbours inside the brick (lo >= 1, hi <= S - 2); the lanes of an
            // invalid row of the pair read inside the array too (l0 >= 1, l0 <= S0 - 2) and discard what they compute
            const int p = (l0 * S1 + r + (first ? 0 : 1)) * 64 + lane;
            const float c = u_lds[p];
            const float nv = cell_update_3d<kMathPrecise>(u_lds[p - plane], u_lds[p + plane], u_lds[p - 64], u_lds[p + 64], u_lds[p - 1], u_lds[p + 1], tab);
            const float o = upd ? nv : c;
            u_lds[p] = o;
            if (check) {
                // owned cells only: a cell that is not updated contributes |c - c| = 0
                const int l1 = r + (first ? 0 : 1);
                const bool own = l0 >= own0_lo && l0 < own0_hi && l1 >= own1_lo && l1 < own1_hi && own_col;
                dmax = max2(dmax, own ? fabsf(c - o) : 0.0f);
            }
        }
        __syncthreads();
    }

    // ---- store the owned cells (locked ones included: `out` is another buffer)
    const int n1 = max(own1_hi - own1_lo, 0), nrows = max(own0_hi - own0_lo, 0) * n1;   // (0: a brick beyond the grid)
    for (int r = wave; r < nrows; r += kWaves) {
        const int l0 = own0_lo + r / n1, l1 = own1_lo + r % n1;
        if (own_col) out[((size_t)(G0 + l0) * a.m1 + (G1 + l1)) * a.pitch + gc] = u_lds[(l0 * S1 + l1) * 64 + lane];
    }

    // ---- the check: wave maxima through LDS, one float per brick by wave 0 (0 from a brick that updated nothing)
    if (a.check) {
        dmax = wave_max(dmax);
        if (lane == 0) wave_delta[wave] = dmax;
        __syncthreads();
        if (wave == 0) {
            const float d = wave_max(lane < kWaves ? wave_delta[lane] : 0.0f);
            if (lane == 0) bf.tile_delta[blockIdx.x] = d;
        }
    }
}

}  // namespace

hipError_t launch_brick_3d_batch(const BatchField *d_fields, int nfields, int src, int dst, int m0, int m1, int pitch, const BrickPlan &plan,
                                 int capacity_rows, int steps, int parity, bool check, hipStream_t stream)
{
    if (steps <= 0) return hipSuccess;
    if (!d_fields || nfields < 1 || nfields > 65535 || src == dst || src < 0 || src > 2 || dst < 0 || dst > 2 || pitch <= 0 ||
        (pitch % 256) != 0 || m0 < 3 || m1 < 3 || parity < 0)
        return hipErrorInvalidValue;
    if (capacity_rows != kBrickBatchRows && capacity_rows != kBrickBatchRowsHalf) return hipErrorInvalidValue;
    const int H = plan.halo;
    // everything the kernel's indexing relies on (as launch_brick_3d): the brick fits the LDS array, s1 is even, and per axis either
    // the brick covers the axis from its face or it owns t = s - 2 H >= 1 cells and the bricks together cover the axis
    if (H < 1 || steps > H || plan.s0 < 1 || plan.s1 < 2 || (plan.s1 & 1) || (long long)plan.s0 * plan.s1 > capacity_rows) return hipErrorInvalidValue;
    if (plan.nb0 < 1 || plan.nb1 < 1 || plan.nbc < 1 || (long long)plan.nb0 * plan.nb1 * plan.nbc > 0x7fffffffLL) return hipErrorInvalidValue;
    if (plan.ghost0 ? (plan.t0 < 1 || plan.t0 + 2 * H != plan.s0 || (long long)plan.nb0 * plan.t0 < m0) : (plan.nb0 != 1 || plan.s0 < m0)) return hipErrorInvalidValue;
    if (plan.ghost1 ? (plan.t1 < 1 || plan.t1 + 2 * H > plan.s1 || (long long)plan.nb1 * plan.t1 < m1) : (plan.nb1 != 1 || plan.s1 < m1)) return hipErrorInvalidValue;
    if (plan.ghostc ? (plan.tc != 64 - 2 * H || plan.tc < 1 || (long long)plan.nbc * plan.tc < plan.m2) : (plan.nbc != 1 || plan.m2 > 64)) return hipErrorInvalidValue;
    if (plan.m2 < 3 || plan.m2 > pitch) return hipErrorInvalidValue;
    BrickBatchArgs a;
    a.fields = d_fields;
    a.src = src;
    a.dst = dst;
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
    a.parity = parity & 1;
    a.check = check ? 1 : 0;
    void (*kernel)(BrickBatchArgs) = capacity_rows == kBrickBatchRows ? brick3d_batch_kernel<kBrickBatchRows> : brick3d_batch_kernel<kBrickBatchRowsHalf>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(plan.nb0 * plan.nb1 * plan.nbc), (unsigned)nfields), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace epic_hip
