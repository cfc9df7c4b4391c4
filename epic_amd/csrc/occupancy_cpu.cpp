// occupancy_cpu.cpp -- dense occupancy-grid ingestion on the host arrays (include/epic_hip.h: epic_hip_set_occupancy_2d_cpu,
// epic_hip_reset_free_cells_2d_cpu).
//
// The reference's callers turn a map message into a list of (x, y) pairs and a list of types, one entry per interior cell, and
// hand both to harmonic_utilities_set_cells_2d_cpu (src/epic_navigation_node_harmonic.cpp:383-426, :582-611;
// src/epic_nav_core_plugin.cpp:139-164).  These walk the message's bytes instead and apply the same per-cell rule where the cell
// lives.  The rule is stated once, in occupancy_rule.h, for this file and for the kernel (occupancy_2d.hip).
#include <stdio.h>
#include <string.h>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"
#include "occupancy_rule.h"

using epic::Harmonic;

extern "C" {

int epic_hip_set_occupancy_2d_cpu(Harmonic *h, const void *occ, int obstacle_threshold, int no_change, unsigned flags,
                                  unsigned long long *changed)
{
    if (h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr || occ == nullptr || h->n != 2) {
        fprintf(stderr, "Error[epic_hip_set_occupancy_2d_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const size_t rows = h->m[0], cols = h->m[1];
    const unsigned char *bytes = static_cast<const unsigned char *>(occ);
    unsigned long long count = 0;
    for (size_t y = 1; y + 1 < rows; y++)
        for (size_t x = 1; x + 1 < cols; x++) {
            const size_t cell = y * cols + x;
            const float before = h->u[cell];
            const bool was_locked = h->locked[cell] != 0;
            const epic_hip::OccCell after = epic_hip::occupancy_cell(bytes[cell], before, was_locked, obstacle_threshold, no_change, flags);
            if (!after.touched) continue;
            count += epic_hip::occupancy_changed(before, was_locked, after);
            h->u[cell] = after.u;
            h->locked[cell] = after.locked ? 1u : 0u;
        }
    if (changed) *changed = count;
    return EPIC_SUCCESS;
}

int epic_hip_reset_free_cells_2d_cpu(Harmonic *h)
{
    if (h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr || h->n != 2) {
        fprintf(stderr, "Error[epic_hip_reset_free_cells_2d_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const size_t rows = h->m[0], cols = h->m[1];
    for (size_t y = 1; y + 1 < rows; y++)
        for (size_t x = 1; x + 1 < cols; x++)
            if (h->locked[y * cols + x] == 0) h->u[y * cols + x] = (float)EPIC_LOG_SPACE_FREE;
    return EPIC_SUCCESS;
}

// The region forms (include/epic_hip.h: epic_hip_set_occupancy_region_*).  origin / extent in the order of m; both null: the grid.
// One walk for n in {2, 3}: a 2-D grid is walked as one plane without faces along the first axis.
int epic_hip_set_occupancy_region_cpu(Harmonic *h, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                      int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed)
{
    size_t m[3], o[3], e[3];
    if (h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr || occ == nullptr ||
        !epic_hip::occupancy_region(h->n, h->m, origin, extent, m, o, e)) {
        fprintf(stderr, "Error[epic_hip_set_occupancy_region_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const unsigned char *bytes = static_cast<const unsigned char *>(occ);
    const bool faces0 = h->n == 3;
    unsigned long long count = 0;
    for (size_t a = 0; a < e[0]; a++) {
        const size_t x0 = o[0] + a;
        if (faces0 && (x0 < 1 || x0 + 2 > m[0])) continue;
        for (size_t b = 0; b < e[1]; b++) {
            const size_t x1 = o[1] + b;
            if (x1 < 1 || x1 + 2 > m[1]) continue;
            for (size_t c = 0; c < e[2]; c++) {
                const size_t x2 = o[2] + c;
                if (x2 < 1 || x2 + 2 > m[2]) continue;
                const size_t cell = (x0 * m[1] + x1) * m[2] + x2;
                const float before = h->u[cell];
                const bool was_locked = h->locked[cell] != 0;
                const epic_hip::OccCell after =
                    epic_hip::occupancy_cell(bytes[(a * e[1] + b) * e[2] + c], before, was_locked, obstacle_threshold, no_change, flags);
                if (!after.touched) continue;
                count += epic_hip::occupancy_changed(before, was_locked, after);
                h->u[cell] = after.u;
                h->locked[cell] = after.locked ? 1u : 0u;
            }
        }
    }
    if (changed) *changed = count;
    return EPIC_SUCCESS;
}

int epic_hip_reset_free_cells_3d_cpu(Harmonic *h)
{
    if (h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr || h->n != 3) {
        fprintf(stderr, "Error[epic_hip_reset_free_cells_3d_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const size_t m0 = h->m[0], m1 = h->m[1], m2 = h->m[2];
    for (size_t x0 = 1; x0 + 1 < m0; x0++)
        for (size_t x1 = 1; x1 + 1 < m1; x1++)
            for (size_t x2 = 1; x2 + 1 < m2; x2++) {
                const size_t cell = (x0 * m1 + x1) * m2 + x2;
                if (h->locked[cell] == 0) h->u[cell] = (float)EPIC_LOG_SPACE_FREE;
            }
    return EPIC_SUCCESS;
}

}  // extern "C"
