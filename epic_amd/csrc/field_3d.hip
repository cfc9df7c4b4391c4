// field_3d.hip -- consumers and sparse edits of the DEVICE-RESIDENT 3-D field (gfx950): streamlines and set_cells.
//
// A relaxed 3-D field used to be a dead end on the device: a caller had to copy the whole field to the host (512 MB at 512^3)
// to walk it, and upload two whole arrays again to add one goal.  Here the walk runs where the field lives, as path_2d.hip does
// for 2-D grids -- one lane per start point, any number of start points per launch, only the way-points come back -- and a
// list of edits goes straight into the current u buffer and the lane masks.
//
// The walk restates harmonic_path3d_cpu.cpp operation by operation (f32 products and sums uncontracted, correctly rounded f32
// division, the norm and the stuck distance in f64 summed left to right and narrowed), so way-points are bit-identical to
// epic_hip_compute_path_3d_cpu on the same field (tests/test_gpu_field3d.py).  Field access goes through the solver's private
// layout: pitched u with rows of m2 cells, row = z * m1 + y; the lane masks of launch_pack_mask_3d, which are the 2-D lane
// masks over those m0 * m1 rows (kernels.h: mask_word_2d / mask_bit_2d) with every face of the grid locked.
//
// A walk is one chain of dependent memory round trips, so the measures of path_2d.hip are kept: indices are clamped so that no
// read can leave the allocation, and all 61 loads of a step -- six usability tests (lock bit + value), six samples of eight
// cells, the lock of the current cell -- depend on the current point only and are issued unconditionally and together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace epic_hip {
namespace {

struct Field3 {
    const float *u;
    const uint32_t *maskw;
    unsigned nx, ny, nz;  // columns (m2), rows (m1), planes (m0) of the caller's grid
    unsigned pitch;
};

// x86-64 converts float -> unsigned through a 64-bit signed truncation and keeps the low word (path_2d.hip: to_index)
__device__ __forceinline__ unsigned to_index(float v) { return (unsigned)(long long)v; }

// clamped: where the host code would not read at all (it tests usability first), the device reads the nearest cell
__device__ __forceinline__ float at(const Field3 &f, unsigned x, unsigned y, unsigned z)
{
    x = min(x, f.nx - 1u);
    y = min(y, f.ny - 1u);
    z = min(z, f.nz - 1u);
    return f.u[((size_t)z * f.ny + y) * f.pitch + x];
}

__device__ __forceinline__ bool locked(const Field3 &f, unsigned x, unsigned y, unsigned z)
{
    x = min(x, f.nx - 1u);
    y = min(y, f.ny - 1u);
    z = min(z, f.nz - 1u);
    return (f.maskw[mask_word_2d(z * f.ny + y, x, f.pitch)] >> mask_bit_2d(x)) & 1u;
}

__device__ __forceinline__ bool usable(const Field3 &f, float x, float y, float z)
{
    const unsigned cx = to_index(x + 0.5f), cy = to_index(y + 0.5f), cz = to_index(z + 0.5f);
    const bool lk = locked(f, cx, cy, cz);
    const float v = at(f, cx, cy, cz);
    return (cx < f.nx) & (cy < f.ny) & (cz < f.nz) & (!lk | !(v < 0.0f));
}

__device__ __forceinline__ float trilinear(const Field3 &f, float x, float y, float z)
{
    const unsigned x0 = to_index(x - 0.5f), x1 = to_index(x + 0.5f);
    const unsigned y0 = to_index(y - 0.5f), y1 = to_index(y + 0.5f);
    const unsigned z0 = to_index(z - 0.5f), z1 = to_index(z + 0.5f);
    const float alpha = x - (float)x0, beta = y - (float)y0, gamma = z - (float)z0;
    const float top0 = (1.0f - alpha) * at(f, x0, y0, z0) + alpha * at(f, x1, y0, z0);
    const float bottom0 = (1.0f - alpha) * at(f, x0, y1, z0) + alpha * at(f, x1, y1, z0);
    const float front = (1.0f - beta) * top0 + beta * bottom0;
    const float top1 = (1.0f - alpha) * at(f, x0, y0, z1) + alpha * at(f, x1, y0, z1);
    const float bottom1 = (1.0f - alpha) * at(f, x0, y1, z1) + alpha * at(f, x1, y1, z1);
    const float back = (1.0f - beta) * top1 + beta * bottom1;
    return (1.0f - gamma) * front + gamma * back;
}

// Returns false where the host returns EPIC_ERROR_INVALID_GRADIENT.
__device__ __forceinline__ bool gradient(const Field3 &f, float x, float y, float z, float cd, float &gx, float &gy, float &gz)
{
    const float xl = x - cd, xr = x + cd, yu = y - cd, yd = y + cd, zn = z - cd, zf = z + cd;
    const bool ok = usable(f, xl, y, z) & usable(f, xr, y, z) & usable(f, x, yu, z) & usable(f, x, yd, z) & usable(f, x, y, zn) &
                    usable(f, x, y, zf);
    const float v0 = trilinear(f, xl, y, z), v1 = trilinear(f, xr, y, z), v2 = trilinear(f, x, yu, z), v3 = trilinear(f, x, yd, z),
                v4 = trilinear(f, x, y, zn), v5 = trilinear(f, x, y, zf);
    if (!ok) return false;
    gx = (v1 - v0) / (2.0f * cd);
    gy = (v3 - v2) / (2.0f * cd);
    gz = (v5 - v4) / (2.0f * cd);
    const double dx = (double)gx, dy = (double)gy, dz = (double)gz;
    const float norm = (float)sqrt(dx * dx + dy * dy + dz * dz);
    gx /= norm;
    gy /= norm;
    gz /= norm;
    return true;
}

struct P3 { float x, y, z; };

// One lane per path.  pts: n_paths x 3 * max_points floats; k / rc: per path.
__global__ void follow_paths_3d_kernel(Field3 f, unsigned n_paths, const float *starts, float step, float cd, unsigned max_points,
                                       float *pts_all, unsigned *k_out, int *rc_out)
{
    const unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_paths) return;
    float x = starts[3 * (size_t)id], y = starts[3 * (size_t)id + 1], z = starts[3 * (size_t)id + 2];
    float *pts = pts_all + (size_t)id * 3 * max_points;
    k_out[id] = 0;
    if (!usable(f, x, y, z)) {
        rc_out[id] = 10;  // EPIC_ERROR_INVALID_LOCATION
        return;
    }
    unsigned n = 1;  // points so far
    const float half = step / 2.0f;
    if (max_points > 0) { pts[0] = x; pts[1] = y; pts[2] = z; }
    // the (up to) five points before the newest one, newest first, in registers
    P3 h0 = {0.0f, 0.0f, 0.0f}, h1 = h0, h2 = h0, h3 = h0, h4 = h0;
    auto near = [&](const P3 &q) {
        const double dx = (double)(x - q.x), dy = (double)(y - q.y), dz = (double)(z - q.z);
        return (float)sqrt(dx * dx + dy * dy + dz * dz) < half;
    };
    // the host loop runs while it holds fewer than max_points points
    for (;;) {
        const unsigned cx = to_index(x + 0.5f), cy = to_index(y + 0.5f), cz = to_index(z + 0.5f);
        // everything this step reads depends on (x, y, z) only: the lock of the current cell and the gradient samples
        const bool lk = locked(f, cx, cy, cz);
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        const bool grad_ok = gradient(f, x, y, z, cd, gx, gy, gz);
        if (!(n < max_points && cx < f.nx && cy < f.ny && cz < f.nz && !lk)) break;
        const unsigned back = n - 1 < 5u ? n - 1 : 5u;
        const bool is_stuck = (back >= 1 && near(h0)) | (back >= 2 && near(h1)) | (back >= 3 && near(h2)) | (back >= 4 && near(h3)) |
                              (back >= 5 && near(h4));
        if (is_stuck) break;
        if (!grad_ok) {
            rc_out[id] = 12;  // EPIC_ERROR_INVALID_GRADIENT
            return;
        }
        h4 = h3; h3 = h2; h2 = h1; h1 = h0; h0 = P3{x, y, z};
        x += gx * step;
        y += gy * step;
        z += gz * step;
        pts[3 * (size_t)n] = x;
        pts[3 * (size_t)n + 1] = y;
        pts[3 * (size_t)n + 2] = z;
        n++;
    }
    if (n <= 2) {
        rc_out[id] = 13;  // EPIC_ERROR_INVALID_PATH
        return;
    }
    k_out[id] = n;
    rc_out[id] = 0;
}

// The way-points that exist, packed: path i's 3 * k[i] floats go to packed + 3 * offset[i] (offset = the running sum of k, made on
// the host).  A batch of thousands of paths then comes back in ONE copy; a copy per path costs about 10 us each, 37 ms of the 51
// a batch of 4096 walks on 512^3 took before (profiles/paths_3d.txt).  One block per path.
__global__ void pack_paths_3d_kernel(const float *pts_all, size_t row, unsigned n_paths, const unsigned *k,
                                     const unsigned long long *offset, float *packed)
{
    for (unsigned i = blockIdx.x; i < n_paths; i += gridDim.x) {
        const size_t n = 3 * (size_t)k[i];
        const float *src = pts_all + (size_t)i * row;
        float *dst = packed + 3 * (size_t)offset[i];
        for (size_t j = threadIdx.x; j < n; j += blockDim.x) dst[j] = src[j];
    }
}

// Sparse edits, one thread per (x, y, z) triple, into the CURRENT buffer and the lane masks: set_cells_2d_kernel with a third
// coordinate.  Cells on a face of the grid stay locked in the mask whatever the edit says (the sweep never updates them).  Two
// entries naming the same cell race, as in the 2-D kernel: the caller must not repeat a cell within one list.
__global__ void set_cells_3d_kernel(float *u, uint32_t *maskw, unsigned m0, unsigned m1, unsigned m2, unsigned pitch, unsigned k,
                                    const unsigned *v, const unsigned *types)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const unsigned x = v[3 * (size_t)i], y = v[3 * (size_t)i + 1], z = v[3 * (size_t)i + 2];
    if (x >= m2 || y >= m1 || z >= m0) return;
    const unsigned t = types[i];
    if (t > 2u) return;
    const float val = (t == 0u) ? 0.0f : -1e6f;
    const bool lock = (t != 2u) || x == 0 || y == 0 || z == 0 || x == m2 - 1 || y == m1 - 1 || z == m0 - 1;
    const unsigned row = z * m1 + y;
    u[(size_t)row * pitch + x] = val;
    uint32_t *w = maskw + mask_word_2d(row, x, pitch);
    const uint32_t bit = 1u << mask_bit_2d(x);
    if (lock) atomicOr(w, bit);
    else atomicAnd(w, ~bit);
}

}  // namespace

hipError_t launch_follow_paths_3d(const float *u, const uint32_t *maskw, int m0, int m1, int m2, int pitch, unsigned n_paths,
                                  const float *d_starts, float step, float cd, unsigned max_points, float *d_pts, unsigned *d_k,
                                  int *d_rc, hipStream_t stream)
{
    if (n_paths == 0) return hipSuccess;
    if (m0 < 1 || m1 < 1 || m2 < 1 || pitch < m2 || pitch % 256 != 0) return hipErrorInvalidValue;
    Field3 f{u, maskw, (unsigned)m2, (unsigned)m1, (unsigned)m0, (unsigned)pitch};
    hipLaunchKernelGGL(follow_paths_3d_kernel, dim3((n_paths + 63) / 64), dim3(64), 0, stream, f, n_paths, d_starts, step, cd,
                       max_points, d_pts, d_k, d_rc);
    return hipGetLastError();
}

hipError_t launch_pack_paths_3d(const float *d_pts, size_t row, unsigned n_paths, const unsigned *d_k, const unsigned long long *d_offset,
                                float *d_packed, hipStream_t stream)
{
    if (n_paths == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_paths_3d_kernel, dim3(n_paths < 4096u ? n_paths : 4096u), dim3(64), 0, stream, d_pts, row, n_paths, d_k, d_offset,
                       d_packed);
    return hipGetLastError();
}

hipError_t launch_set_cells_3d(float *u, uint32_t *maskw, int m0, int m1, int m2, int pitch, unsigned k, const unsigned *v,
                               const unsigned *types, hipStream_t stream)
{
    if (k == 0) return hipSuccess;
    if (m0 < 1 || m1 < 1 || m2 < 1 || pitch < m2 || pitch % 256 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_cells_3d_kernel, dim3((k + 255) / 256), dim3(256), 0, stream, u, maskw, (unsigned)m0, (unsigned)m1,
                       (unsigned)m2, (unsigned)pitch, k, v, types);
    return hipGetLastError();
}

}  // namespace epic_hip
