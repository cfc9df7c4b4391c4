// Stand-alone caller of the host twins of the field queries (epic_amd/csrc/field_query_cpu.cpp), built with
// -fsanitize=address,undefined by tests/test_field_query_sanitize.py: exactly-sized heap arrays, so a read one cell outside u or
// locked is an error.  A 2-D and a 3-D field relaxed by formula, goals in the interior, on a face and in the far corner (usable
// cells whose neighbours would lie outside), samples at every cell's own point and half a cell beside it with cdPrecision up to
// 1.5, the edge coordinates (NaN, +-inf, negative, |x| >= 2^63), and regions in both corners -- where indices come closest to the
// ends of the arrays.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
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

static void run(unsigned n)
{
    const unsigned m0 = n == 3 ? 6 : 1, m1 = 9, m2 = 11;   // planes (z), rows (y), columns (x)
    std::vector<unsigned> m;
    if (n == 3) m.push_back(m0);
    m.push_back(m1);
    m.push_back(m2);
    const size_t cells = (size_t)m0 * m1 * m2;
    std::vector<float> u(cells);
    std::vector<unsigned> locked(cells);
    auto at = [&](unsigned x, unsigned y, unsigned z) { return ((size_t)z * m1 + y) * m2 + x; };
    const unsigned gx = 7, gy = 4, gz = n == 3 ? 3 : 0;
    for (unsigned z = 0; z < m0; z++)
        for (unsigned y = 0; y < m1; y++)
            for (unsigned x = 0; x < m2; x++) {
                const bool face = x == 0 || y == 0 || x == m2 - 1 || y == m1 - 1 || (n == 3 && (z == 0 || z == m0 - 1));
                const float dx = (float)x - gx, dy = (float)y - gy, dz = (float)z - gz;
                locked[at(x, y, z)] = face;
                u[at(x, y, z)] = face ? -1e6f : -0.3f * sqrtf(dx * dx + dy * dy + dz * dz);
            }
    locked[at(gx, gy, gz)] = 1;
    u[at(0, 4, gz)] = 0.0f;                       // a goal on a face
    u[at(m2 - 1, m1 - 1, m0 - 1)] = 0.0f;         // ... and in the far corner
    u[at(0, 0, 0)] = 0.0f;                        // ... and in the near one
    Harmonic h = {};
    h.n = n;
    h.m = m.data();
    h.u = u.data();
    h.locked = locked.data();

    // every cell's own point and points half a cell off it, three precisions
    std::vector<float> pts;
    for (unsigned z = 0; z < m0; z++)
        for (unsigned y = 0; y < m1; y++)
            for (unsigned x = 0; x < m2; x++)
                for (float off : {0.0f, 0.5f, -0.5f, 0.49f}) {
                    pts.push_back(x + off);
                    pts.push_back(y - off);
                    if (n == 3) pts.push_back(z + off);
                }
    const unsigned count = (unsigned)(pts.size() / n);
    std::vector<float> pot(count), grad((size_t)n * count);
    std::vector<unsigned char> st(count);
    EXPECT(epic_hip_sample_potential_cpu(&h, count, pts.data(), pot.data(), st.data()) == EPIC_SUCCESS);
    unsigned ok = 0;
    for (unsigned i = 0; i < count; i++) {
        EXPECT(st[i] == EPIC_HIP_QUERY_OK || (st[i] == EPIC_HIP_QUERY_INVALID_LOCATION && pot[i] == 0.0f));
        ok += st[i] == EPIC_HIP_QUERY_OK;
    }
    EXPECT(ok > count / 4);
    for (float cd : {0.5f, 0.25f, 1.5f}) {
        EXPECT(epic_hip_sample_gradient_cpu(&h, count, pts.data(), cd, grad.data(), st.data()) == EPIC_SUCCESS);
        EXPECT(epic_hip_sample_gradient_cpu(&h, count, pts.data(), cd, grad.data(), nullptr) == EPIC_SUCCESS);
        for (unsigned i = 0; i < count; i++) EXPECT(st[i] <= EPIC_HIP_QUERY_FLAT);
    }

    // edge coordinates: never OK, outputs zero
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[] = {nan, inf, -inf, -0.2f, -0.7f, -3.0f, -1e9f, 9223372036854775808.0f, -9223372036854775808.0f, 1e19f, -1e19f,
                         3e38f, -3e38f, 4294967296.0f, (float)m2 + 7.5f};
    std::vector<float> edge;
    for (unsigned ax = 0; ax < n; ax++)
        for (float v : bad) {
            float p[3] = {5.25f, 3.25f, 2.25f};
            p[ax] = v;
            // (the near corner and the face hold goals here: keep the other coordinates off them)
            for (unsigned a = 0; a < n; a++) edge.push_back(p[a]);
        }
    const unsigned ecount = (unsigned)(edge.size() / n);
    std::vector<float> epot(ecount), egrad((size_t)n * ecount);
    std::vector<unsigned char> est(ecount);
    EXPECT(epic_hip_sample_potential_cpu(&h, ecount, edge.data(), epot.data(), est.data()) == EPIC_SUCCESS);
    for (unsigned i = 0; i < ecount; i++) EXPECT(est[i] == EPIC_HIP_QUERY_INVALID_LOCATION && epot[i] == 0.0f);
    for (float cd : {0.5f, 0.3f, 1.5f, nan, inf}) {
        EXPECT(epic_hip_sample_gradient_cpu(&h, ecount, edge.data(), cd, egrad.data(), est.data()) == EPIC_SUCCESS);
        for (unsigned i = 0; i < ecount; i++) {
            EXPECT(est[i] == EPIC_HIP_QUERY_INVALID_GRADIENT);
            for (unsigned a = 0; a < n; a++) EXPECT(egrad[(size_t)n * i + a] == 0.0f);
        }
    }

    // regions: the grid, both corners, a single cell; each equals its slice of the grid
    std::vector<float> whole((size_t)n * cells);
    std::vector<unsigned char> wst(cells);
    for (float cd : {0.5f, 1.5f}) {
        EXPECT(epic_hip_flow_field_cpu(&h, nullptr, nullptr, cd, 0, whole.data(), wst.data()) == EPIC_SUCCESS);
        const unsigned boxes[4][2][3] = {{{0, 0, 0}, {2, 3, 5}}, {{m0 - 1, m1 - 2, m2 - 4}, {1, 2, 4}}, {{m0 / 2, 4, 7}, {1, 1, 1}},
                                         {{0, 0, 0}, {m0, m1, m2}}};
        for (const auto &box : boxes) {
            unsigned o[3] = {box[0][0], box[0][1], box[0][2]}, e[3] = {box[1][0], box[1][1], box[1][2]};
            if (e[0] > m0) e[0] = m0;
            const unsigned lead = 3 - n;   // a 2-D region has no plane entry
            std::vector<float> g((size_t)n * e[0] * e[1] * e[2]);
            std::vector<unsigned char> s((size_t)e[0] * e[1] * e[2]);
            EXPECT(epic_hip_flow_field_cpu(&h, o + lead, e + lead, cd, 0, g.data(), s.data()) == EPIC_SUCCESS);
            size_t i = 0;
            for (unsigned z = o[0]; z < o[0] + e[0]; z++)
                for (unsigned y = o[1]; y < o[1] + e[1]; y++)
                    for (unsigned x = o[2]; x < o[2] + e[2]; x++, i++) {
                        EXPECT(s[i] == wst[at(x, y, z)]);
                        EXPECT(memcmp(&g[n * i], &whole[n * at(x, y, z)], n * sizeof(float)) == 0);
                    }
        }
        const unsigned o_bad[3] = {0, 0, 1}, e_bad[3] = {m0, m1, m2};
        EXPECT(epic_hip_flow_field_cpu(&h, o_bad + (3 - n), e_bad + (3 - n), cd, 0, whole.data(), wst.data()) == EPIC_ERROR_INVALID_DATA);
    }
    EXPECT(epic_hip_sample_potential_cpu(&h, 0, nullptr, nullptr, nullptr) == EPIC_SUCCESS);
    EXPECT(epic_hip_sample_potential_cpu(&h, 1, nullptr, pot.data(), nullptr) == EPIC_ERROR_INVALID_DATA);
}

int main()
{
    run(2);
    run(3);
    printf("field query host code: ok\n");
    return 0;
}
