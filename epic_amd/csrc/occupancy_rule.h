// occupancy_rule.h -- the per-cell rule of the dense occupancy ingestion (include/epic_hip.h: epic_hip_set_occupancy_2d_*), stated
// once for the host walk (occupancy_cpu.cpp) and the kernels (occupancy_2d.hip, occupancy_region.hip).  Interior cells only: the
// callers never hand a border cell in.
#pragma once
#include <string.h>

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

}  // namespace epic_hip
