// field_query.hip -- queries of the DEVICE-RESIDENT field (gfx950): potential and gradient at a batch of points, the flow field of a
// region, cells and regions read back.  2-D and 3-D; the launchers are called from field_query_driver.hip only.
//
// Until these a caller who wanted one value, a gradient at each of its particles or the descent direction of the cells round a robot
// had to copy the whole field to the host first (268 MB at 8192^2).  Nothing here writes the field or the masks.
//
// The per-point rule is field_query_rule.h, shared with the host twins (field_query_cpu.cpp), so results are bit-identical to them
// (tests/test_gpu_field_query.py).  Field access goes through the solver's private layout as in field_3d.hip: pitched u with rows of
// m2 cells, row = z * m1 + y; the lane masks over those rows (kernels.h: mask_word_2d / mask_bit_2d), every face cell locked.
// Indices are clamped, so no read can leave the allocation, and all loads of a point -- 24 for a 2-D gradient, 60 for a 3-D one,
// 2 + 4 / 2 + 8 for a potential -- depend on the point only and are issued unconditionally and together.
//
// Built with IEEE NaN comparisons (Makefile: the filter-out -fno-honor-nans line): a point may be NaN and a norm 0 / 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_query_rule.h"
#include "kernels.h"

namespace epic_hip {
namespace {

constexpr int kWave = 64;
constexpr int kTrips = 4;                      // a wave walks its strip in four trips of 64 consecutive cells
constexpr int kStripCols = kWave * kTrips;     // 256
constexpr int kWavesPerBlock = 4;

struct DevField {
    const float *u;
    const uint32_t *maskw;
    unsigned nx, ny, nz;  // columns (m2), rows (m1), planes (m0; 1: a 2-D field)
    unsigned pitch;
    __device__ __forceinline__ float at(unsigned x, unsigned y, unsigned z) const
    {
        x = min(x, nx - 1u);
        y = min(y, ny - 1u);
        z = min(z, nz - 1u);
        return u[((size_t)z * ny + y) * pitch + x];
    }
    __device__ __forceinline__ bool locked(unsigned x, unsigned y, unsigned z) const
    {
        x = min(x, nx - 1u);
        y = min(y, ny - 1u);
        z = min(z, nz - 1u);
        return (maskw[mask_word_2d(z * ny + y, x, pitch)] >> mask_bit_2d(x)) & 1u;
    }
};

struct Box {
    unsigned origin[3], extent[3];  // planes, rows, columns (the order of m; 2-D: origin[0] = 0, extent[0] = 1)
};

// One lane per point.  points: n_points x N floats; out: n_points x N floats (GRAD) or n_points floats; status may be null.
template <bool N3, bool GRAD>
__global__ __launch_bounds__(256) void sample_points_kernel(DevField f, unsigned n_points, const float *points, float cd, float *out,
                                                            unsigned char *status)
{
    constexpr unsigned N = N3 ? 3 : 2;
    const unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_points) return;
    const float *p = points + (size_t)N * id;
    const float x = p[0], y = p[1], z = N3 ? p[2] : 0.0f;
    unsigned char st;
    if (GRAD) {
        float g[3];
        st = fq::gradient<N3>(f, x, y, z, cd, g);
        float *o = out + (size_t)N * id;
        o[0] = g[0];
        o[1] = g[1];
        if (N3) o[2] = g[2];
    } else {
        float v;
        st = fq::potential<N3>(f, x, y, z, v);
        out[id] = v;
    }
    if (status) status[id] = st;
}

// The (row, strip) pair of a wave: pairs are numbered through the box's rows and its 256-column strips (strips are counted from
// the box's first column), four to a block, as in occupancy_region.hip.  False: no such pair (wave-uniform).
__device__ __forceinline__ bool pair_of_wave(const Box &b, unsigned nst, unsigned pairs, unsigned &row, unsigned &strip, unsigned &y,
                                             unsigned &z)
{
    const unsigned pair = blockIdx.x * (unsigned)kWavesPerBlock + (threadIdx.x >> 6);
    if (pair >= pairs) return false;
    row = pair / nst;
    strip = pair - row * nst;
    z = b.origin[0] + row / b.extent[1];
    y = b.origin[1] + row % b.extent[1];
    return true;
}

// The flow field of a box: a wave handles one (row, strip) -- in 3-D one (plane * row, strip) -- in four trips; in a trip lane L has
// cell 64 trip + L of the strip, so a lane's N floats go to consecutive lanes' consecutive addresses (one dwordx2 per lane in 2-D
// where `grad` is 8-byte aligned: VEC2) and the loads of neighbouring lanes hit the same lines.  Each cell computes its own sample
// indices: with an arbitrary cd, x - cd is not translation invariant in f32.  PACK (the box's width is a multiple of 4 and `status`
// is dword aligned): every fourth lane collects the bytes of its three neighbours and stores one dword.
template <bool N3, bool PACK, bool VEC2>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void flow_field_kernel(DevField f, Box b, unsigned nst, unsigned pairs, float cd,
                                                                            float *grad, unsigned char *status)
{
    constexpr unsigned N = N3 ? 3 : 2;
    const unsigned lane = threadIdx.x & (kWave - 1);
    unsigned row, strip, y, z;
    if (!pair_of_wave(b, nst, pairs, row, strip, y, z)) return;
    const size_t row_base = (size_t)row * b.extent[2];
#pragma unroll 1
    for (int t = 0; t < kTrips; ++t) {
        const unsigned c = strip * (unsigned)kStripCols + (unsigned)t * kWave + lane;   // column inside the box
        if (c - lane >= b.extent[2]) break;                                             // wave-uniform: the trip is past the box
        const bool in = c < b.extent[2];
        const unsigned x = b.origin[2] + min(c, b.extent[2] - 1u);   // lanes past the box redo its last cell and store nothing
        float g[3];
        const unsigned char st = fq::flow_cell<N3>(f, x, y, z, cd, g);
        if (in) {
            float *o = grad + (row_base + c) * N;
            if (VEC2) {
                *reinterpret_cast<float2 *>(o) = make_float2(g[0], g[1]);
            } else {
                o[0] = g[0];
                o[1] = g[1];
                if (N3) o[2] = g[2];
            }
        }
        if (status != nullptr) {
            if (PACK) {
                const unsigned s0 = st;
                const unsigned w = s0 | ((unsigned)__shfl_down(s0, 1) << 8) | ((unsigned)__shfl_down(s0, 2) << 16) |
                                   ((unsigned)__shfl_down(s0, 3) << 24);
                if (in && (lane & 3u) == 0) *reinterpret_cast<uint32_t *>(status + row_base + c) = w;
            } else if (in) {
                status[row_base + c] = st;
            }
        }
    }
}

// A box of the field as the device holds it, unpitched: values and the unpacked lock bits (0 / 1).  Same geometry as the flow field.
__global__ __launch_bounds__(kWave * kWavesPerBlock) void gather_region_kernel(DevField f, Box b, unsigned nst, unsigned pairs, float *u_out,
                                                                               unsigned *locked_out)
{
    const unsigned lane = threadIdx.x & (kWave - 1);
    unsigned row, strip, y, z;
    if (!pair_of_wave(b, nst, pairs, row, strip, y, z)) return;
    const size_t row_base = (size_t)row * b.extent[2];
#pragma unroll
    for (int t = 0; t < kTrips; ++t) {
        const unsigned c = strip * (unsigned)kStripCols + (unsigned)t * kWave + lane;
        if (c < b.extent[2]) {
            const unsigned x = b.origin[2] + c;
            if (u_out) u_out[row_base + c] = f.at(x, y, z);
            if (locked_out) locked_out[row_base + c] = f.locked(x, y, z) ? 1u : 0u;
        }
    }
}

// k cells, (x, y[, z]) each, all inside the grid (the driver has checked the list)
template <bool N3>
__global__ __launch_bounds__(256) void gather_cells_kernel(DevField f, unsigned k, const unsigned *v, float *u_out, unsigned *locked_out)
{
    constexpr unsigned N = N3 ? 3 : 2;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const unsigned x = v[(size_t)N * i], y = v[(size_t)N * i + 1], z = N3 ? v[(size_t)N * i + 2] : 0u;
    u_out[i] = f.at(x, y, z);
    locked_out[i] = f.locked(x, y, z) ? 1u : 0u;
}

bool field_ok(const QueryField &q)
{
    return q.u && q.maskw && (q.n == 2 || q.n == 3) && q.m0 >= 1 && (q.n == 3 || q.m0 == 1) && q.m1 >= 1 && q.m2 >= 1 && q.pitch >= q.m2 &&
           q.pitch % 256 == 0;
}

DevField dev_field(const QueryField &q)
{
    return DevField{q.u, q.maskw, (unsigned)q.m2, (unsigned)q.m1, (unsigned)q.m0, (unsigned)q.pitch};
}

// the box lies inside the grid (nothing is clipped) and its (row, strip) pairs fit a launch
bool box_of(const QueryField &q, const unsigned origin[3], const unsigned extent[3], Box &b, unsigned &nst, unsigned &pairs)
{
    const unsigned m[3] = {(unsigned)q.m0, (unsigned)q.m1, (unsigned)q.m2};
    for (int a = 0; a < 3; a++) {
        if (extent[a] < 1 || origin[a] > m[a] || extent[a] > m[a] - origin[a]) return false;
        b.origin[a] = origin[a];
        b.extent[a] = extent[a];
    }
    const unsigned long long strips = ((unsigned long long)extent[2] + kStripCols - 1) / kStripCols;
    const unsigned long long n = (unsigned long long)extent[0] * extent[1] * strips;
    if (n > 0x7fffffffull) return false;
    nst = (unsigned)strips;
    pairs = (unsigned)n;
    return true;
}

}  // namespace

hipError_t launch_sample_points(const QueryField &q, unsigned n_points, const float *d_points, bool gradient, float cd, float *d_out,
                                unsigned char *d_status, hipStream_t stream)
{
    if (n_points == 0) return hipSuccess;
    if (!field_ok(q) || !d_points || !d_out) return hipErrorInvalidValue;
    const DevField f = dev_field(q);
    const dim3 grid((n_points + 255u) / 256u), block(256);
    if (q.n == 3) {
        if (gradient) hipLaunchKernelGGL((sample_points_kernel<true, true>), grid, block, 0, stream, f, n_points, d_points, cd, d_out, d_status);
        else hipLaunchKernelGGL((sample_points_kernel<true, false>), grid, block, 0, stream, f, n_points, d_points, cd, d_out, d_status);
    } else {
        if (gradient) hipLaunchKernelGGL((sample_points_kernel<false, true>), grid, block, 0, stream, f, n_points, d_points, cd, d_out, d_status);
        else hipLaunchKernelGGL((sample_points_kernel<false, false>), grid, block, 0, stream, f, n_points, d_points, cd, d_out, d_status);
    }
    return hipGetLastError();
}

hipError_t launch_flow_field(const QueryField &q, const unsigned origin[3], const unsigned extent[3], float cd, float *d_gradient,
                             unsigned char *d_status, hipStream_t stream)
{
    Box b;
    unsigned nst = 0, pairs = 0;
    if (!field_ok(q) || !d_gradient || !box_of(q, origin, extent, b, nst, pairs)) return hipErrorInvalidValue;
    const DevField f = dev_field(q);
    const dim3 grid((pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    const bool pack = d_status != nullptr && extent[2] % 4 == 0 && reinterpret_cast<uintptr_t>(d_status) % 4 == 0;
    const bool vec2 = reinterpret_cast<uintptr_t>(d_gradient) % 8 == 0;
#define EPIC_FLOW_LAUNCH(N3, PACK, VEC2) \
    hipLaunchKernelGGL((flow_field_kernel<N3, PACK, VEC2>), grid, block, 0, stream, f, b, nst, pairs, cd, d_gradient, d_status)
    if (q.n == 3) {
        if (pack) EPIC_FLOW_LAUNCH(true, true, false);
        else EPIC_FLOW_LAUNCH(true, false, false);
    } else if (vec2) {
        if (pack) EPIC_FLOW_LAUNCH(false, true, true);
        else EPIC_FLOW_LAUNCH(false, false, true);
    } else {
        if (pack) EPIC_FLOW_LAUNCH(false, true, false);
        else EPIC_FLOW_LAUNCH(false, false, false);
    }
#undef EPIC_FLOW_LAUNCH
    return hipGetLastError();
}

hipError_t launch_gather_region(const QueryField &q, const unsigned origin[3], const unsigned extent[3], float *d_u, unsigned *d_locked,
                                hipStream_t stream)
{
    Box b;
    unsigned nst = 0, pairs = 0;
    if (!field_ok(q) || (!d_u && !d_locked) || !box_of(q, origin, extent, b, nst, pairs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_region_kernel, dim3((pairs + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, stream,
                       dev_field(q), b, nst, pairs, d_u, d_locked);
    return hipGetLastError();
}

hipError_t launch_gather_cells(const QueryField &q, unsigned k, const unsigned *d_v, float *d_u, unsigned *d_locked, hipStream_t stream)
{
    if (k == 0) return hipSuccess;
    if (!field_ok(q) || !d_v || !d_u || !d_locked) return hipErrorInvalidValue;
    const dim3 grid((k + 255u) / 256u), block(256);
    if (q.n == 3) hipLaunchKernelGGL(gather_cells_kernel<true>, grid, block, 0, stream, dev_field(q), k, d_v, d_u, d_locked);
    else hipLaunchKernelGGL(gather_cells_kernel<false>, grid, block, 0, stream, dev_field(q), k, d_v, d_u, d_locked);
    return hipGetLastError();
}

}  // namespace epic_hip
