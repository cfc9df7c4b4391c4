// occupancy_points_rule.h -- the rule of epic_hip_set_occupancy_points_* (include/epic_hip.h), stated once for the host twin
// (occupancy_points_cpu.cpp), the multi-device route (occupancy_driver.hip) and the kernels (occupancy_points.hip): a point's cell, the
// ray a point casts from the sensor, and -- host only -- the block B the calls are defined by.
//
// Axes are the three of occupancy_rule.h (occupancy_region): the order of m, a 2-D grid being one plane.  A point is (x, y[, z]) with
// x along the LAST axis of m (the order of epic_hip_sample_potential_*): axis a of the box reads component 2 - a of the point, for
// n == 2 and n == 3 alike; axis 0 of a 2-D grid has no component and stays at cell 0.
//
// The ray, operation by operation (f32 throughout; no product is followed by a sum, so nothing can contract; both sides are built
// with -ffp-contract=off all the same).  With s the sensor, p the point, per axis:
//   cs = floor(s), ce = floor(p)                 the cells; |p| >= 2^31 has none: the axis never runs out of steps
//   steps = |ce - cs| (an integer), dir = sign(ce - cs) (of p where it has no cell)
//   where steps > 0:  d = p - s  (non-zero: the cells differ)
//                     dist = dir > 0 ? (float)(cs + 1) - s : s - (float)cs        the way to the first cell boundary, 0 <= dist <= 1
//                     tMax = dist / |d|,  tDelta = 1.0f / |d|                     two IEEE divisions
// The walk takes sum(steps) single-axis steps.  Each step clears the cell it stands in, then moves along the axis with the smallest
// tMax among the axes with steps still to go (ties: the lowest axis, compared with <), counts the step off and adds tDelta to that
// tMax.  It stops early when the move leaves the box.  So the start cell and every cell entered before the end cell are cleared and
// the end cell is not; a ray of zero steps clears nothing.  tMax may reach +inf (a d below 2^-126); it is never NaN.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#include "../../include/epic_hip.h"

#if defined(__HIPCC__)
#define EPIC_PTS_HD __host__ __device__ __forceinline__
#else
#define EPIC_PTS_HD inline
#endif

namespace epic_hip {
namespace pts {

struct Box {
    int o[3], e[3];   // origin and extent in the order of m; o + e <= 2^31 - 1
};

// floor of a coordinate as an integer; false: NaN, +-inf or 2^31 and more in magnitude (outside every box)
EPIC_PTS_HD bool cell_of(float v, int &c)
{
    const bool ok = v > -2147483648.0f && v < 2147483648.0f;
    c = ok ? (int)floorf(v) : 0;
    return ok;
}

EPIC_PTS_HD bool finite(float v) { return v >= -3.402823466e+38f && v <= 3.402823466e+38f; }

// p: the n components of a point.  cell / has: per axis, its cell and whether it has one.  Returns: the point is finite.
EPIC_PTS_HD bool classify(const float *p, unsigned n, int cell[3], bool has[3])
{
    bool fin = true;
    cell[0] = 0;
    has[0] = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++) {
        if (a < (int)(3u - n)) continue;
        const float v = p[2 - a];
        fin = fin && finite(v);
        has[a] = cell_of(v, cell[a]);
    }
    return fin;
}

EPIC_PTS_HD bool inside(const Box &b, const int cell[3], const bool has[3])
{
    bool in = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++) in = in && has[a] && cell[a] >= b.o[a] && cell[a] < b.o[a] + b.e[a];
    return in;
}

struct Ray {
    int cur[3], dir[3];
    unsigned rem[3];           // steps still to go; 0xffffffff: the point has no cell on this axis
    float tmax[3], tdelta[3];
    unsigned bound;            // iterations of the walk: min(sum of the steps, what the box can hold)
};

// s: the sensor, finite and inside the box; p: a finite point; n components each
EPIC_PTS_HD void ray_setup(const Box &b, const float *s, const float *p, unsigned n, Ray &r)
{
    unsigned long long total = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++) {
        r.cur[a] = 0;
        r.dir[a] = 0;
        r.rem[a] = 0u;
        r.tmax[a] = 0.0f;
        r.tdelta[a] = 0.0f;
        if (a < (int)(3u - n)) continue;
        const float sv = s[2 - a], pv = p[2 - a];
        int cs, ce;
        (void)cell_of(sv, cs);
        const bool has = cell_of(pv, ce);
        r.cur[a] = cs;
        if (has) {
            const long long diff = (long long)ce - (long long)cs;
            r.dir[a] = diff > 0 ? 1 : (diff < 0 ? -1 : 0);
            r.rem[a] = (unsigned)(diff < 0 ? -diff : diff);
        } else {
            r.dir[a] = pv > 0.0f ? 1 : -1;
            r.rem[a] = 0xffffffffu;
        }
        if (r.rem[a] != 0u) {
            const float d = pv - sv;
            const float dist = r.dir[a] > 0 ? (float)(cs + 1) - sv : sv - (float)cs;
            r.tmax[a] = dist / fabsf(d);
            r.tdelta[a] = 1.0f / fabsf(d);
        }
        total += r.rem[a];
    }
    const unsigned long long room = (unsigned long long)b.e[0] + (unsigned long long)b.e[1] + (unsigned long long)b.e[2];
    r.bound = (unsigned)(total < room ? total : room);   // inside the box a walk takes fewer than e[0] + e[1] + e[2] steps
}

// one step from r.cur (which the caller has cleared); false: the move left the box
EPIC_PTS_HD bool ray_step(const Box &b, Ray &r)
{
    int axis = -1;
    float best = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++)
        if (r.rem[a] != 0u && (axis < 0 || r.tmax[a] < best)) {
            axis = a;
            best = r.tmax[a];
        }
    bool in = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++)
        if (a == axis) {
            r.cur[a] += r.dir[a];
            r.rem[a] -= 1u;
            r.tmax[a] = r.tmax[a] + r.tdelta[a];
            in = r.cur[a] >= b.o[a] && r.cur[a] < b.o[a] + b.e[a];
        }
    return in;
}

// X of the inflation rule: the largest byte that is not no_change
inline int obstacle_byte(int no_change, unsigned flags)
{
    const int top = (flags & EPIC_HIP_OCC_UNSIGNED) ? 255 : 127;
    return top == no_change ? top - 1 : top;
}

// What both variants test before they touch anything (o / e: occupancy_region's): the box fits an int, points with a count, a
// no_change the byte type holds, 0 < obstacle_threshold <= X, and a sensor that is finite and inside the box.
inline bool args_ok(unsigned n, const size_t o[3], const size_t e[3], unsigned n_points, const float *points, const float *sensor,
                    int obstacle_threshold, int no_change, unsigned flags, Box &box)
{
    for (int a = 0; a < 3; a++) {
        if (o[a] + e[a] > 0x7fffffffull) return false;
        box.o[a] = (int)o[a];
        box.e[a] = (int)e[a];
    }
    if (n_points > 0 && points == nullptr) return false;
    const bool is_unsigned = (flags & EPIC_HIP_OCC_UNSIGNED) != 0;
    if (no_change < (is_unsigned ? 0 : -128) || no_change > (is_unsigned ? 255 : 127)) return false;
    if (obstacle_threshold <= 0 || obstacle_threshold > obstacle_byte(no_change, flags)) return false;
    if (sensor) {
        int cell[3];
        bool has[3];
        if (!classify(sensor, n, cell, has) || !inside(box, cell, has)) return false;
    }
    return true;
}

// The block B by its definition (box.e[0] * box.e[1] * box.e[2] bytes): clearing first, hits over it.
inline void rasterize(const Box &box, unsigned n, unsigned n_points, const float *points, const float *sensor, int no_change, unsigned flags,
                      unsigned char *out)
{
    const size_t e1 = (size_t)box.e[1], e2 = (size_t)box.e[2];
    const size_t cells = (size_t)box.e[0] * e1 * e2;
    const auto at = [&](const int c[3]) { return ((size_t)(c[0] - box.o[0]) * e1 + (size_t)(c[1] - box.o[1])) * e2 + (size_t)(c[2] - box.o[2]); };
    for (size_t i = 0; i < cells; i++) out[i] = (unsigned char)no_change;
    int cell[3];
    bool has[3];
    if (sensor)
        for (size_t i = 0; i < n_points; i++) {
            if (!classify(points + i * n, n, cell, has)) continue;
            Ray r;
            ray_setup(box, sensor, points + i * n, n, r);
            for (unsigned k = 0; k < r.bound; k++) {
                out[at(r.cur)] = 0;
                if (!ray_step(box, r)) break;
            }
        }
    for (size_t i = 0; i < n_points; i++)
        if (classify(points + i * n, n, cell, has) && inside(box, cell, has)) out[at(cell)] = (unsigned char)obstacle_byte(no_change, flags);
}

}  // namespace pts
}  // namespace epic_hip
