// occupancy_points_cpu.cpp -- point clouds and laser scans applied to the host arrays (include/epic_hip.h:
// epic_hip_set_occupancy_points_cpu): the block B by its definition (occupancy_points_rule.h: rasterize), then the inflated call of
// occupancy_cpu.cpp on B.  This is the definition the device path (occupancy_points.hip) is held to.
#include <stdio.h>

#include <vector>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"
#include "occupancy_points_rule.h"
#include "occupancy_rule.h"

using epic::Harmonic;

extern "C" {

int epic_hip_set_occupancy_points_cpu(Harmonic *h, unsigned int n_points, const float *points, const float *sensor, const unsigned int *origin,
                                      const unsigned int *extent, int obstacle_threshold, int no_change, unsigned flags, unsigned int radius_sq,
                                      unsigned long long *changed)
{
    size_t m[3], o[3], e[3];
    epic_hip::pts::Box box;
    if (radius_sq > EPIC_HIP_OCC_MAX_RADIUS_SQ || h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr ||
        !epic_hip::occupancy_region(h->n, h->m, origin, extent, m, o, e) ||
        !epic_hip::pts::args_ok(h->n, o, e, n_points, points, sensor, obstacle_threshold, no_change, flags, box)) {
        fprintf(stderr, "Error[epic_hip_set_occupancy_points_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    std::vector<unsigned char> block(e[0] * e[1] * e[2]);
    epic_hip::pts::rasterize(box, h->n, n_points, points, sensor, no_change, flags, block.data());
    return epic_hip_set_occupancy_inflated_cpu(h, block.data(), origin, extent, obstacle_threshold, no_change, flags, radius_sq, changed);
}

}  // extern "C"
