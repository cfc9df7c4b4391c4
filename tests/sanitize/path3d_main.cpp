// Stand-alone caller of the host statement of the 3-D consumers and edits (epic_amd/csrc/harmonic_path3d_cpu.cpp), built with
// -fsanitize=address,undefined by tests/test_path3d_sanitize.py: exactly-sized heap arrays, so a read one cell outside u or locked
// is an error.  A tiny field relaxed by formula (u falls with the distance to the goal), goals in the interior, on a face and in the
// far corner, starts on those goals with cdPrecision 1.5 -- the cases where indices come closest to the ends of the arrays.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "epic/epic_abi.h"
#include "epic_hip.h"

using epic::Harmonic;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "EXPECT failed: %s (line %d)\n", #cond, __LINE__); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

int main()
{
    const unsigned m0 = 7, m1 = 9, m2 = 11;   // planes (z), rows (y), columns (x)
    std::vector<unsigned> m = {m0, m1, m2};
    const size_t cells = (size_t)m0 * m1 * m2;
    std::vector<float> u(cells);
    std::vector<unsigned> locked(cells);
    const unsigned gx = 7, gy = 4, gz = 3;
    auto at = [&](unsigned x, unsigned y, unsigned z) { return ((size_t)z * m1 + y) * m2 + x; };
    for (unsigned z = 0; z < m0; z++)
        for (unsigned y = 0; y < m1; y++)
            for (unsigned x = 0; x < m2; x++) {
                const bool face = x == 0 || y == 0 || z == 0 || x == m2 - 1 || y == m1 - 1 || z == m0 - 1;
                const float dx = (float)x - gx, dy = (float)y - gy, dz = (float)z - gz;
                locked[at(x, y, z)] = face;
                u[at(x, y, z)] = face ? -1e6f : -0.3f * sqrtf(dx * dx + dy * dy + dz * dz);
            }
    locked[at(gx, gy, gz)] = 1;
    // goals on a face and in the far corner (locked, u == 0): usable points whose neighbours would lie outside
    u[at(0, 4, 3)] = 0.0f;
    u[at(m2 - 1, m1 - 1, m0 - 1)] = 0.0f;
    Harmonic h = {};
    h.n = 3;
    h.m = m.data();
    h.u = u.data();
    h.locked = locked.data();

    // walks from every interior cell, two step sizes
    unsigned walked = 0, reached = 0;
    for (unsigned z = 1; z + 1 < m0; z++)
        for (unsigned y = 1; y + 1 < m1; y++)
            for (unsigned x = 1; x + 1 < m2; x++)
                for (float step : {0.2f, 1.7f}) {
                    unsigned k = 0;
                    float *path = nullptr;
                    const int rc = epic_hip_compute_path_3d_cpu(&h, x + 0.1f, y - 0.2f, z + 0.3f, step, 0.5f, 500, &k, &path);
                    EXPECT(rc == EPIC_SUCCESS || rc == EPIC_ERROR_INVALID_GRADIENT || rc == EPIC_ERROR_INVALID_PATH);
                    if (rc != EPIC_SUCCESS) {
                        EXPECT(path == nullptr);
                        continue;
                    }
                    EXPECT(k >= 3 && k <= 500 && path != nullptr);
                    walked++;
                    const float *end = path + 3 * (size_t)(k - 1);
                    reached += (unsigned)(end[0] + 0.5f) == gx && (unsigned)(end[1] + 0.5f) == gy && (unsigned)(end[2] + 0.5f) == gz;
                    EXPECT(epic::harmonic_free_path_cpu(path) == EPIC_SUCCESS && path == nullptr);
                }
    EXPECT(walked > 50 && reached > 10);

    // starts on goal cells of a face and of the far corner, large cdPrecision
    const float spots[][3] = {{0.0f, 4.0f, 3.0f}, {-0.4f, 4.0f, 3.0f}, {0.4f, 4.4f, 3.4f}, {10.0f, 8.0f, 6.0f}, {10.4f, 8.4f, 6.4f}, {9.6f, 7.6f, 5.6f}};
    for (const auto &s : spots)
        for (float cd : {0.5f, 1.5f}) {
            unsigned k = 0;
            float *path = nullptr;
            float v = 1.0f, a = 0.0f, b = 0.0f, c = 0.0f;
            EXPECT(epic_hip_compute_path_3d_cpu(&h, s[0], s[1], s[2], 0.2f, cd, 100, &k, &path) == EPIC_ERROR_INVALID_PATH);   // one point: the start is locked
            EXPECT(path == nullptr);
            EXPECT(epic_hip_compute_potential_3d_cpu(&h, s[0], s[1], s[2], &v) == EPIC_SUCCESS);
            EXPECT(epic_hip_compute_gradient_3d_cpu(&h, s[0], s[1], s[2], cd, &a, &b, &c) == EPIC_ERROR_INVALID_GRADIENT);     // a sample outside or in an obstacle
        }
    float v = 0.0f, a = 0.0f, b = 0.0f, c = 0.0f;
    EXPECT(epic_hip_compute_potential_3d_cpu(&h, 7.0f, 4.0f, 3.0f, &v) == EPIC_SUCCESS);
    EXPECT(epic_hip_compute_gradient_3d_cpu(&h, 5.2f, 4.1f, 2.9f, 0.5f, &a, &b, &c) == EPIC_SUCCESS);
    EXPECT(fabsf(a * a + b * b + c * c - 1.0f) < 1e-5f && a > 0.5f);
    EXPECT(epic_hip_compute_potential_3d_cpu(&h, 11.0f, 4.0f, 3.0f, &v) == EPIC_ERROR_INVALID_LOCATION);
    EXPECT(epic_hip_compute_potential_3d_cpu(&h, 5.0f, 4.0f, -3.0f, &v) == EPIC_ERROR_INVALID_LOCATION);
    EXPECT(epic_hip_compute_potential_3d_cpu(&h, 5.0f, 4.0f, 3e9f, &v) == EPIC_ERROR_INVALID_LOCATION);

    // sparse edits: every cell of the grid once, then entries outside and invalid types
    std::vector<unsigned> list, types;
    for (unsigned z = 0; z < m0; z++)
        for (unsigned y = 0; y < m1; y++)
            for (unsigned x = 0; x < m2; x++) {
                list.insert(list.end(), {x, y, z});
                types.push_back((x + y + z) % 3);
            }
    const unsigned outside[][3] = {{m2, 0, 0}, {0, m1, 0}, {0, 0, m0}, {~0u, ~0u, ~0u}};
    for (const auto &e : outside) {
        list.insert(list.end(), {e[0], e[1], e[2]});
        types.push_back(EPIC_CELL_TYPE_GOAL);
    }
    list.insert(list.end(), {1u, 1u, 1u});
    types.push_back(3u);
    EXPECT(epic_hip_set_cells_3d_cpu(&h, (unsigned)types.size(), list.data(), types.data()) == EPIC_SUCCESS);
    for (unsigned z = 0; z < m0; z++)
        for (unsigned y = 0; y < m1; y++)
            for (unsigned x = 0; x < m2; x++) {
                const unsigned t = (x + y + z) % 3;
                EXPECT(locked[at(x, y, z)] == (t != EPIC_CELL_TYPE_FREE));
                EXPECT(u[at(x, y, z)] == (t == EPIC_CELL_TYPE_GOAL ? 0.0f : -1e6f));
            }

    // the error returns
    unsigned k = 0;
    float *path = nullptr;
    Harmonic bad = h;
    bad.n = 2;
    EXPECT(epic_hip_compute_path_3d_cpu(&bad, 5.0f, 4.0f, 3.0f, 0.2f, 0.5f, 10, &k, &path) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_compute_path_3d_cpu(nullptr, 5.0f, 4.0f, 3.0f, 0.2f, 0.5f, 10, &k, &path) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_compute_potential_3d_cpu(&bad, 5.0f, 4.0f, 3.0f, &v) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_compute_gradient_3d_cpu(&h, 5.0f, 4.0f, 3.0f, 0.5f, &a, nullptr, &c) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_cells_3d_cpu(&bad, 1, list.data(), types.data()) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_cells_3d_cpu(&h, 0, list.data(), types.data()) == EPIC_ERROR_INVALID_DATA);
    float junk[3] = {0.0f, 0.0f, 0.0f};
    path = junk;
    EXPECT(epic_hip_compute_path_3d_cpu(&h, 5.0f, 4.0f, 3.0f, 0.2f, 0.5f, 10, &k, &path) == EPIC_ERROR_INVALID_DATA && path == junk);
    printf("3-D path host code: ok (%u walks, %u reached the goal)\n", walked, reached);
    return 0;
}
