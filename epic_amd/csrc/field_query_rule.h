// field_query_rule.h -- the per-point rule of the field queries (include/epic_hip.h, "Field queries"), stated once for the host twins
// (field_query_cpu.cpp) and the kernels (field_query.hip).
//
// The arithmetic is that of the host consumers, operation for operation: harmonic_path_cpu.cpp (usable / bilinear / gradient, itself
// the reference's libepic/src/harmonic/harmonic_path_cpu.cpp:41-118) for 2-D fields and harmonic_path3d_cpu.cpp for 3-D ones -- f32
// products and sums uncontracted (both sides are built with -ffp-contract=off), the two or three f32 divisions, the norm summed left
// to right in double and narrowed (std::pow(x, 2) of a float promoted to double is x * x exactly: 48 bits of product).  F is the
// field as one side holds it:
//   unsigned nx, ny, nz                   columns (last axis of m), rows, planes (1 for a 2-D field)
//   float at(x, y, z), bool locked(x, y, z)   the cell's value and lock, indices CLAMPED to the nearest cell
// so every load of a point is safe whatever the point is and none waits for a test: the functions below issue all of them first and
// select afterwards (path_2d.hip and field_3d.hip do the same; on the host it costs nothing).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define EPIC_FQ_HD __host__ __device__ __forceinline__
#else
#define EPIC_FQ_HD inline
#endif

namespace epic_hip {
namespace fq {

// EPIC_HIP_QUERY_* of include/epic_hip.h
constexpr unsigned char kOk = 0, kInvalidLocation = 1, kInvalidGradient = 2, kFlat = 3;

// float -> index as x86-64 compiles the reference's (unsigned)(float): a 64-bit signed truncation whose low word is kept, so a value
// below -1 wraps to a huge index and fails the bounds test.  NaN, +-inf and |v| >= 2^63 have no 64-bit truncation (hosts and devices
// disagree on what the conversion leaves): they are "outside the grid" here, on every side.
EPIC_FQ_HD unsigned to_index(float v)
{
    return (v > -9223372036854775808.0f && v < 9223372036854775808.0f) ? (unsigned)(long long)v : 0xffffffffu;
}

// inside the grid, and not a locked cell with u < 0 (an obstacle; goals are locked with u == 0)
template <bool N3, class F>
EPIC_FQ_HD bool usable(const F &f, float x, float y, float z)
{
    const unsigned cx = to_index(x + 0.5f), cy = to_index(y + 0.5f), cz = N3 ? to_index(z + 0.5f) : 0u;
    const bool lk = f.locked(cx, cy, cz);
    const float v = f.at(cx, cy, cz);
    return (cx < f.nx) & (cy < f.ny) & (cz < f.nz) & (!lk | !(v < 0.0f));
}

// between the four (eight) cell centres around the point; alpha, beta, gamma in [0.5, 1.5) as in the reference
template <bool N3, class F>
EPIC_FQ_HD float interpolate(const F &f, float x, float y, float z)
{
    const unsigned x0 = to_index(x - 0.5f), x1 = to_index(x + 0.5f);
    const unsigned y0 = to_index(y - 0.5f), y1 = to_index(y + 0.5f);
    const unsigned z0 = N3 ? to_index(z - 0.5f) : 0u, z1 = N3 ? to_index(z + 0.5f) : 0u;
    const float alpha = x - (float)x0, beta = y - (float)y0;
    const float top0 = (1.0f - alpha) * f.at(x0, y0, z0) + alpha * f.at(x1, y0, z0);
    const float bottom0 = (1.0f - alpha) * f.at(x0, y1, z0) + alpha * f.at(x1, y1, z0);
    const float front = (1.0f - beta) * top0 + beta * bottom0;
    if (!N3) return front;
    const float gamma = z - (float)z0;
    const float top1 = (1.0f - alpha) * f.at(x0, y0, z1) + alpha * f.at(x1, y0, z1);
    const float bottom1 = (1.0f - alpha) * f.at(x0, y1, z1) + alpha * f.at(x1, y1, z1);
    const float back = (1.0f - beta) * top1 + beta * bottom1;
    return (1.0f - gamma) * front + gamma * back;
}

// harmonic_compute_potential_2d_cpu / epic_hip_compute_potential_3d_cpu: 2 + 4 (2 + 8) loads
template <bool N3, class F>
EPIC_FQ_HD unsigned char potential(const F &f, float x, float y, float z, float &out)
{
    const bool ok = usable<N3>(f, x, y, z);
    const float v = interpolate<N3>(f, x, y, z);
    out = ok ? v : 0.0f;
    return ok ? kOk : kInvalidLocation;
}

// harmonic_compute_gradient_2d_cpu / epic_hip_compute_gradient_3d_cpu: central differences at +-cd (samples x-, x+, y-, y+, z-, z+),
// normalised; 4 x (2 + 4) = 24 loads, 6 x (2 + 8) = 60 in 3-D.  The point's own cell is not tested.  Where the norm is not a positive
// finite number the reference divides by it (0 / 0 on a flat field): that is kFlat and zeros here.  g: three floats (g[2] = 0 in 2-D).
template <bool N3, class F>
EPIC_FQ_HD unsigned char gradient(const F &f, float x, float y, float z, float cd, float *g)
{
    const float xl = x - cd, xr = x + cd, yu = y - cd, yd = y + cd, zn = z - cd, zf = z + cd;
    bool ok = usable<N3>(f, xl, y, z) & usable<N3>(f, xr, y, z) & usable<N3>(f, x, yu, z) & usable<N3>(f, x, yd, z);
    if (N3) ok = ok & usable<N3>(f, x, y, zn) & usable<N3>(f, x, y, zf);
    const float v0 = interpolate<N3>(f, xl, y, z), v1 = interpolate<N3>(f, xr, y, z);
    const float v2 = interpolate<N3>(f, x, yu, z), v3 = interpolate<N3>(f, x, yd, z);
    const float v4 = N3 ? interpolate<N3>(f, x, y, zn) : 0.0f, v5 = N3 ? interpolate<N3>(f, x, y, zf) : 0.0f;
    g[0] = g[1] = g[2] = 0.0f;
    if (!ok) return kInvalidGradient;
    const float gx = (v1 - v0) / (2.0f * cd);
    const float gy = (v3 - v2) / (2.0f * cd);
    const float gz = N3 ? (v5 - v4) / (2.0f * cd) : 0.0f;
    const double dx = (double)gx, dy = (double)gy, dz = (double)gz;
    double sum = dx * dx + dy * dy;
    if (N3) sum = sum + dz * dz;
    const float norm = (float)sqrt(sum);
    if (!(norm > 0.0f) || !(norm <= 3.402823466e+38f)) return kFlat;   // zero, NaN or infinite
    g[0] = gx / norm;
    g[1] = gy / norm;
    if (N3) g[2] = gz / norm;
    return kOk;
}

// The flow field's cell (cx, cy, cz): the sample point is the cell's own index as floats -- where potential() returns the cell's
// value.  A cell that is not usable is kInvalidLocation and zeros; every other cell, goals included, is gradient() at that point.
template <bool N3, class F>
EPIC_FQ_HD unsigned char flow_cell(const F &f, unsigned cx, unsigned cy, unsigned cz, float cd, float *g)
{
    const float x = (float)cx, y = (float)cy, z = (float)cz;
    const bool own = usable<N3>(f, x, y, z);
    const unsigned char st = gradient<N3>(f, x, y, z, cd, g);
    if (!own) {
        g[0] = g[1] = g[2] = 0.0f;
        return kInvalidLocation;
    }
    return st;
}

}  // namespace fq
}  // namespace epic_hip
