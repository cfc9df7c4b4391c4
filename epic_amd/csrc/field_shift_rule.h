// field_shift_rule.h -- the rule of the rolling-window shift (include/epic_hip.h: epic_hip_shift_field_*), stated once for the host
// twin (field_shift_cpu.cpp), the kernel (field_shift.hip) and its driver (field_shift_driver.hip).
//
// new(x) = old(x + shift) for every interior cell x whose source is an interior cell; every other interior cell takes the fill;
// border and face cells are neither read nor written.  A 2-D grid is one plane, {1, rows, cols}, without faces along the first axis.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/epic/epic_abi.h"

#if defined(__HIPCC__)
#define EPIC_SHIFT_HD __host__ __device__
#else
#define EPIC_SHIFT_HD
#endif

namespace epic_hip {

// The source coordinate of cell x along an axis of m cells, in 64 bits; false: the source is not an interior cell of that axis.
EPIC_SHIFT_HD inline bool shift_source(long long x, long long shift, long long m, long long &src)
{
    src = x + shift;
    return src >= 1 && src <= m - 2;
}

// The columns (cells of an axis) [lo, hi] that are interior and whose source is interior too; empty when lo > hi.
EPIC_SHIFT_HD inline void shift_covered(long long shift, long long m, long long &lo, long long &hi)
{
    lo = shift < 0 ? 1 - shift : 1;
    hi = shift > 0 ? m - 2 - shift : m - 2;
}

// A call's geometry and fill, made on the host.  s[i] is shift[i] where the shift keeps anything and 0 otherwise: |s[i]| < m[i] - 2,
// so nothing derived from it overflows an int; `none` says that every interior cell is uncovered.
struct ShiftPlan {
    int m[3];             // {m0, m1, cols}; 2-D: m0 = 1
    int s[3];
    bool faces0;          // the first axis has faces (3-D)
    bool zero;            // an all-zero shift: nothing is to be done
    bool none;
    uint32_t fill_bits;   // bit pattern of the fill's u
    bool fill_locked;
    unsigned long long kept, interior;
};

// False: n is not 2 or 3, a dimension does not fit an int, or fill_type is neither FREE nor OBSTACLE.
inline bool shift_plan(unsigned n, const unsigned *m, const int *shift, unsigned fill_type, ShiftPlan &p)
{
    if ((n != 2 && n != 3) || (fill_type != EPIC_CELL_TYPE_FREE && fill_type != EPIC_CELL_TYPE_OBSTACLE)) return false;
    const float fill = fill_type == EPIC_CELL_TYPE_FREE ? (float)EPIC_LOG_SPACE_FREE : (float)EPIC_LOG_SPACE_OBSTACLE;
    memcpy(&p.fill_bits, &fill, sizeof(fill));
    p.fill_locked = fill_type == EPIC_CELL_TYPE_OBSTACLE;
    const unsigned lead = 3 - n;
    p.faces0 = n == 3;
    p.m[0] = 1;
    p.s[0] = 0;
    p.zero = true;
    p.none = false;
    p.kept = p.interior = 1;
    for (unsigned i = 0; i < n; i++) {
        if (m[i] > 0x7fffffffu) return false;
        const long long inner = m[i] >= 2 ? (long long)m[i] - 2 : 0, by = shift[i] < 0 ? -(long long)shift[i] : (long long)shift[i];
        p.m[lead + i] = (int)m[i];
        p.s[lead + i] = shift[i];
        p.zero = p.zero && shift[i] == 0;
        p.interior *= (unsigned long long)inner;
        p.kept *= (unsigned long long)(by >= inner ? 0 : inner - by);
    }
    p.none = p.kept == 0;
    if (p.none) p.s[0] = p.s[1] = p.s[2] = 0;
    return true;
}

}  // namespace epic_hip
