// occupancy_rule.h -- the per-cell rule of the dense occupancy ingestion (include/epic_hip.h: epic_hip_set_occupancy_2d_*), stated
// once for the host walk (occupancy_cpu.cpp) and the kernels (occupancy_2d.hip, occupancy_region.hip).  Interior cells only: the
// callers never hand a border cell in.  Below it, host only: the region's geometry, and the inflated block B' of
// epic_hip_set_occupancy_inflated_* by its definition (the CPU twin's and the multi-device route's; the kernel of occupancy_inflate.hip
// is held to it).
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"

#if defined(__HIPCC__)
#define EPIC_OCC_HD __host__ __device__
#else
#define EPIC_OCC_HD
#endif

namespace epic_hip {

struct OccCell {
    float u;
    bool locked;
    bool touched;   // false: the rule left the cell alone (u and locked are the values handed in)
};

// byte: the cell's byte of the message; u / was_locked: the cell as it is.  In the order of the header:
//   1. v == no_change                         untouched
//   2. a goal (locked, u == 0), no OVER_GOALS untouched
//   3. v >= obstacle_threshold                obstacle, locked
//   4. otherwise                              unlocked; free -- with KEEP_FREE a cell that was unlocked keeps its value
EPIC_OCC_HD inline OccCell occupancy_cell(unsigned char byte, float u, bool was_locked, int obstacle_threshold, int no_change,
                                          unsigned flags)
{
    const int v = (flags & EPIC_HIP_OCC_UNSIGNED) ? (int)byte : (int)(signed char)byte;
    OccCell c = {u, was_locked, false};
    if (v == no_change) return c;
    if (was_locked && u == (float)EPIC_LOG_SPACE_GOAL && !(flags & EPIC_HIP_OCC_OVER_GOALS)) return c;
    c.touched = true;
    if (v >= obstacle_threshold) {
        c.u = (float)EPIC_LOG_SPACE_OBSTACLE;
        c.locked = true;
    } else {
        c.locked = false;
        if (was_locked || !(flags & EPIC_HIP_OCC_KEEP_FREE)) c.u = (float)EPIC_LOG_SPACE_FREE;
    }
    return c;
}

EPIC_OCC_HD inline unsigned occupancy_float_bits(float f)
{
    unsigned b;
    memcpy(&b, &f, sizeof(b));
    return b;
}

// what `changed` counts: the locked flag changed, or the cell stayed locked and its value changed (goal <-> obstacle)
EPIC_OCC_HD inline bool occupancy_changed(float u, bool was_locked, const OccCell &after)
{
    return after.locked != was_locked || (was_locked && occupancy_float_bits(after.u) != occupancy_float_bits(u));
}

// The region of epic_hip_set_occupancy_region_* as three axes, for the host walk and the driver: origin / extent have n entries in
// the order of m (both null: the grid); a 2-D grid is one plane, {1, rows, cols}.  False: n is not 2 or 3, exactly one of the two
// pointers is null, or the region does not lie inside the grid (extent >= 1, origin + extent <= m, tested without overflow).
inline bool occupancy_region(unsigned n, const unsigned *m, const unsigned *origin, const unsigned *extent, size_t grid[3], size_t o[3],
                             size_t e[3])
{
    if ((n != 2 && n != 3) || (origin == nullptr) != (extent == nullptr)) return false;
    const unsigned lead = 3 - n;
    grid[0] = 1;
    o[0] = 0;
    e[0] = 1;
    for (unsigned i = 0; i < n; i++) {
        const unsigned mi = m[i], oi = origin ? origin[i] : 0u, ei = extent ? extent[i] : mi;
        if (ei < 1 || oi > mi || ei > mi - oi) return false;
        grid[lead + i] = mi;
        o[lead + i] = oi;
        e[lead + i] = ei;
    }
    return true;
}

// The inflated block B' of epic_hip_set_occupancy_inflated_* by its definition, on the host: `out` (e[0] * e[1] * e[2] bytes) is the
// block with every cell within sqrt(radius_sq) of a source, and not a source itself, set to X.  The squared distance to the nearest
// source of the block is the minimum over the sources of a sum of three squares, taken axis by axis: along the fastest axis first
// (a walk up and a walk down every row), then the minimum over the rows dy away of that plus dy^2, then over the planes.  Integers;
// everything above radius_sq is held at radius_sq + 1 ("far"), so 16 bits hold it (radius_sq <= 256).
inline void occupancy_inflate_block(const unsigned char *block, const size_t e[3], int obstacle_threshold, int no_change, unsigned flags,
                                    unsigned radius_sq, unsigned char *out)
{
    const size_t cells = e[0] * e[1] * e[2];
    const unsigned far = radius_sq + 1;
    const int top = (flags & EPIC_HIP_OCC_UNSIGNED) ? 255 : 127;
    const unsigned char fill = (unsigned char)(top == no_change ? top - 1 : top);
    long reach = 0;
    while ((reach + 1) * (reach + 1) <= (long)radius_sq) reach++;
    auto source = [&](size_t i) {
        const int v = (flags & EPIC_HIP_OCC_UNSIGNED) ? (int)block[i] : (int)(signed char)block[i];
        return v != no_change && v >= obstacle_threshold;
    };
    std::vector<unsigned short> d(cells), next(cells);
    for (size_t row = 0; row < e[0] * e[1]; row++) {   // along a row: the distance to the nearest source on either side, squared
        unsigned short *dr = d.data() + row * e[2];
        unsigned gap = far;   // cells since the last source; far: none yet (far * far > radius_sq)
        for (size_t x = 0; x < e[2]; x++) {
            gap = source(row * e[2] + x) ? 0u : std::min(gap + 1u, far);
            dr[x] = (unsigned short)std::min(gap * gap, far);
        }
        gap = far;
        for (size_t x = e[2]; x-- > 0;) {
            gap = source(row * e[2] + x) ? 0u : std::min(gap + 1u, far);
            dr[x] = (unsigned short)std::min<unsigned>(dr[x], std::min(gap * gap, far));
        }
    }
    for (int axis = 1; axis >= 0; axis--) {   // then across the rows of a plane, then across the planes
        const size_t count = e[axis], stride = axis == 1 ? e[2] : e[1] * e[2];
        if (count == 1) continue;
        for (size_t i = 0; i < cells; i++) {
            const long at = (long)((i / stride) % count);
            unsigned best = far;
            for (long k = std::max(-reach, -at); k <= reach && at + k < (long)count; k++)
                best = std::min(best, (unsigned)d[(size_t)((long)i + k * (long)stride)] + (unsigned)(k * k));
            next[i] = (unsigned short)std::min(best, far);
        }
        d.swap(next);
    }
    for (size_t i = 0; i < cells; i++) out[i] = (d[i] <= radius_sq && !source(i)) ? fill : block[i];
}

}  // namespace epic_hip
