// Stand-alone caller of the points form of the occupancy ingestion (epic_amd/csrc/occupancy_points_cpu.cpp and occupancy_cpu.cpp, included
// as source; the rule is occupancy_points_rule.h), built with -fsanitize=address,undefined by tests/test_occupancy_points_cpu.py: exactly-sized
// heap arrays, so a ray that walks one cell past the box, or a point that is binned outside it, is an error; float-to-int conversions of
// NaN, +-inf and 3e9 would be undefined behaviour.  2-D and 3-D windows, with and without a sensor, a call without points, a sensor outside the box.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../epic_amd/csrc/occupancy_cpu.cpp"
#include "../../epic_amd/csrc/occupancy_points_cpu.cpp"

#define EXPECT(cond) ((cond) ? (void)0 : (fprintf(stderr, "EXPECT failed: %s (line %d)\n", #cond, __LINE__), exit(1)))

int main()
{
    unsigned long long total = 0;
    for (unsigned n = 2; n <= 3; n++) {
        const unsigned lead = 3 - n, grid[3] = {7, 23, 150}, org[3] = {1, 2, 5}, ext[3] = {5, 19, 129};
        std::vector<unsigned> m(grid + lead, grid + 3), o(org + lead, org + 3), e(ext + lead, ext + 3);
        const size_t cells = (n == 3 ? 7u : 1u) * 23u * 150u;
        std::vector<float> u(cells, -3.0f), pts, sensor(n);
        std::vector<unsigned> locked(cells, 0);
        Harmonic h = {};
        h.n = n;
        h.m = m.data();
        h.u = u.data();
        h.locked = locked.data();
        for (unsigned k = 0; k < n; k++) sensor[k] = (float)o[n - 1 - k] + 0.25f;
        unsigned s = 99u + n;
        for (unsigned i = 0; i < 400 * n; i++) {   // in and around the box, then the values without a cell
            s = s * 1664525u + 1013904223u;
            pts.push_back((float)o[n - 1 - i % n] - 3.0f + (float)(s >> 8) * (float)(e[n - 1 - i % n] + 6) / 16777216.0f);
        }
        for (float v : {NAN, INFINITY, -INFINITY, 3e9f, -3e9f, 3.4e38f, -0.0f})
            for (unsigned k = 0; k < n; k++) pts.push_back(k == 0 ? v : sensor[k] + 1.0f);
        const unsigned count = (unsigned)(pts.size() / n);
        for (unsigned variant = 0; variant < 4; variant++) {   // sensor or not, radius_sq 0 or 9
            unsigned long long changed = ~0ull;
            EXPECT(epic_hip_set_occupancy_points_cpu(&h, count, pts.data(), (variant & 1) ? sensor.data() : nullptr, o.data(), e.data(), 50, -2, 0,
                                                     (variant & 2) ? 9 : 0, &changed) == EPIC_SUCCESS);
            total += changed;
        }
        EXPECT(epic_hip_set_occupancy_points_cpu(&h, 0, nullptr, sensor.data(), nullptr, nullptr, 50, -2, 0, 1, nullptr) == EPIC_SUCCESS);
        sensor[0] -= 1.0f;   // outside the box
        EXPECT(epic_hip_set_occupancy_points_cpu(&h, count, pts.data(), sensor.data(), o.data(), e.data(), 50, -2, 0, 1, nullptr) == EPIC_ERROR_INVALID_DATA);
    }
    EXPECT(total > 0);
    printf("occupancy points host code: ok (%llu cells changed)\n", total);
    return 0;
}
