// field_shift_cpu.cpp -- the rolling-window shift on the host arrays (include/epic_hip.h: epic_hip_shift_field_cpu).  This is the
// definition the device call (field_shift.hip, field_shift_driver.hip) is held to; the rule is field_shift_rule.h.
//
// A costmap with rolling_window or a voxel box centred on the robot moves with it by whole cells: the cells that stay inside keep
// their potential and their lock state, goals included, at their new indices; the strips that come in take the fill and are then
// ingested with epic_hip_set_occupancy_region_*.  One walk for n in {2, 3}: a 2-D grid is one plane without faces along the first axis.
#include <stdio.h>

#include <vector>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"
#include "field_shift_rule.h"

using epic::Harmonic;

extern "C" {

int epic_hip_shift_field_cpu(Harmonic *h, const int *shift, unsigned int fill_type, unsigned long long *kept)
{
    epic_hip::ShiftPlan p;
    if (h == nullptr || h->m == nullptr || h->u == nullptr || h->locked == nullptr || shift == nullptr ||
        !epic_hip::shift_plan(h->n, h->m, shift, fill_type, p)) {
        fprintf(stderr, "Error[epic_hip_shift_field_cpu]: %s\n", "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (kept) *kept = p.kept;
    if (p.zero) return EPIC_SUCCESS;
    const size_t m0 = (size_t)p.m[0], m1 = (size_t)p.m[1], m2 = (size_t)p.m[2];
    // the old cells: a shifted cell may be read after the cell it lands on was written
    std::vector<uint32_t> old_u, old_locked;
    if (!p.none) {
        old_u.resize(m0 * m1 * m2);
        memcpy(old_u.data(), h->u, old_u.size() * sizeof(uint32_t));   // bit patterns, not floats: any payload survives
        old_locked.assign(h->locked, h->locked + m0 * m1 * m2);
    }
    for (size_t x0 = p.faces0 ? 1 : 0; x0 + (p.faces0 ? 1 : 0) < m0; x0++) {
        long long y0 = 0, y1, y2;
        const bool ok0 = !p.faces0 || epic_hip::shift_source((long long)x0, p.s[0], p.m[0], y0);
        for (size_t x1 = 1; x1 + 1 < m1; x1++) {
            const bool ok1 = epic_hip::shift_source((long long)x1, p.s[1], p.m[1], y1) && ok0 && !p.none;
            for (size_t x2 = 1; x2 + 1 < m2; x2++) {
                const size_t cell = (x0 * m1 + x1) * m2 + x2;
                if (ok1 && epic_hip::shift_source((long long)x2, p.s[2], p.m[2], y2)) {
                    const size_t from = ((size_t)y0 * m1 + (size_t)y1) * m2 + (size_t)y2;
                    memcpy(&h->u[cell], &old_u[from], sizeof(uint32_t));
                    h->locked[cell] = old_locked[from];
                } else {
                    memcpy(&h->u[cell], &p.fill_bits, sizeof(uint32_t));
                    h->locked[cell] = p.fill_locked ? 1u : 0u;
                }
            }
        }
    }
    return EPIC_SUCCESS;
}

}  // extern "C"
