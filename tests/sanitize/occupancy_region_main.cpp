// Stand-alone caller of the region walk of the dense occupancy ingestion (epic_amd/csrc/occupancy_cpu.cpp, included as source),
// built with -fsanitize=address,undefined by tests/test_occupancy_region_cpu.py: exactly-sized heap arrays -- the region's bytes
// too -- so a read or write one cell past the window, the image, u or locked is an error.  The windows and boxes are those of the
// CPU tests (tests/occupancy_region_cases.py): on the border and the faces, on the last row and column, across the strip
// boundaries, three different extents; then the error returns.  Every result is compared with a walk over the WHOLE grid that
// looks each cell's byte up in a full image.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../epic_amd/csrc/occupancy_cpu.cpp"

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "EXPECT failed: %s (line %d)\n", #cond, __LINE__); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

namespace {

struct Box {
    unsigned o[3], e[3];
};

unsigned long long total = 0;

// m: n entries; box: n entries used, in the order of m
void run(unsigned n, const std::vector<unsigned> &m, const Box &box, bool whole)
{
    size_t g[3] = {1, 1, 1}, o[3] = {0, 0, 0}, e[3] = {1, 1, 1};
    for (unsigned i = 0; i < n; i++) {
        g[3 - n + i] = m[i];
        o[3 - n + i] = whole ? 0 : box.o[i];
        e[3 - n + i] = whole ? m[i] : box.e[i];
    }
    const size_t cells = g[0] * g[1] * g[2];
    for (unsigned flags = 0; flags < 8; flags++) {
        std::vector<float> u(cells);
        std::vector<unsigned> locked(cells);
        std::vector<unsigned char> full(cells);
        unsigned s = 12345u + flags + (unsigned)cells;
        for (size_t i = 0; i < cells; i++) {
            s = s * 1664525u + 1013904223u;
            locked[i] = (s >> 28) < 3;
            u[i] = locked[i] ? ((s >> 20) & 1 ? 0.0f : -1e6f) : -(float)((s >> 8) & 1023);
            full[i] = (unsigned char)(s >> 12);
        }
        std::vector<unsigned char> occ(e[0] * e[1] * e[2]);   // the region's bytes, exactly
        for (size_t a = 0; a < e[0]; a++)
            for (size_t b = 0; b < e[1]; b++)
                for (size_t c = 0; c < e[2]; c++) occ[(a * e[1] + b) * e[2] + c] = full[((o[0] + a) * g[1] + o[1] + b) * g[2] + o[2] + c];
        std::vector<float> want_u = u;
        std::vector<unsigned> want_l = locked;
        unsigned long long want_changed = 0;
        for (size_t x0 = 0; x0 < g[0]; x0++)
            for (size_t x1 = 0; x1 < g[1]; x1++)
                for (size_t x2 = 0; x2 < g[2]; x2++) {
                    const bool in_box = x0 >= o[0] && x0 < o[0] + e[0] && x1 >= o[1] && x1 < o[1] + e[1] && x2 >= o[2] && x2 < o[2] + e[2];
                    const bool inner = (n == 2 || (x0 > 0 && x0 + 1 < g[0])) && x1 > 0 && x1 + 1 < g[1] && x2 > 0 && x2 + 1 < g[2];
                    if (!in_box || !inner) continue;
                    const size_t cell = (x0 * g[1] + x1) * g[2] + x2;
                    const epic_hip::OccCell after = epic_hip::occupancy_cell(full[cell], u[cell], locked[cell] != 0, 50, -2, flags);
                    want_changed += epic_hip::occupancy_changed(u[cell], locked[cell] != 0, after);
                    want_u[cell] = after.u;
                    want_l[cell] = after.locked;
                }
        std::vector<unsigned> dims = m;
        Harmonic h = {};
        h.n = n;
        h.m = dims.data();
        h.u = u.data();
        h.locked = locked.data();
        unsigned long long changed = ~0ull;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, occ.data(), whole ? nullptr : box.o, whole ? nullptr : box.e, 50, -2, flags, &changed) ==
               EPIC_SUCCESS);
        EXPECT(changed == want_changed);
        for (size_t i = 0; i < cells; i++) EXPECT(epic_hip::occupancy_float_bits(u[i]) == epic_hip::occupancy_float_bits(want_u[i]) && locked[i] == want_l[i]);
        total += changed;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, occ.data(), whole ? nullptr : box.o, whole ? nullptr : box.e, 250, 1000, flags, nullptr) ==
               EPIC_SUCCESS);
        if (n == 3) {
            EXPECT(epic_hip_reset_free_cells_3d_cpu(&h) == EPIC_SUCCESS);
            for (size_t x0 = 1; x0 + 1 < g[0]; x0++)
                for (size_t x1 = 1; x1 + 1 < g[1]; x1++)
                    for (size_t x2 = 1; x2 + 1 < g[2]; x2++) {
                        const size_t cell = (x0 * g[1] + x1) * g[2] + x2;
                        EXPECT(locked[cell] != 0 || u[cell] == -1e6f);
                    }
        }
    }
}

Box span(const std::vector<unsigned> &m, const int *lo, const int *hi)
{
    Box b = {};
    for (size_t i = 0; i < m.size(); i++) {
        const int l = std::min(lo[i], (int)m[i] - 1), h = std::max(std::min(hi[i], (int)m[i]), l + 1);
        b.o[i] = (unsigned)l;
        b.e[i] = (unsigned)(h - l);
    }
    return b;
}

}  // namespace

int main()
{
    // the 2-D windows
    for (const std::vector<unsigned> &m : std::vector<std::vector<unsigned>>{{3, 5}, {5, 257}, {37, 301}, {130, 515}}) {
        const int rows = (int)m[0], cols = (int)m[1], h = rows > 3 ? std::min(rows - 2, 5) : 1;
        run(2, m, Box{}, true);
        std::vector<Box> w;
        w.push_back(Box{{(unsigned)std::min(2, rows - 2), (unsigned)std::min(3, cols - 2)}, {1, 1}});
        w.push_back(Box{{0, 0}, {(unsigned)std::min(rows, 4), (unsigned)std::min(cols, 6)}});
        w.push_back(Box{{(unsigned)rows - 3, (unsigned)cols - 5}, {3, 5}});
        if (cols > 250) w.push_back(Box{{1, 120}, {(unsigned)h, (unsigned)std::min(140, cols - 120)}});
        if (cols >= 12) {
            w.push_back(Box{{1, 3}, {(unsigned)h, 7}});
            w.push_back(cols >= 264 ? Box{{1, 252}, {(unsigned)h, 12}} : Box{{1, 4}, {(unsigned)h, 8}});
        }
        for (const Box &b : w) run(2, m, b, false);
    }
    // the 3-D boxes
    for (const std::vector<unsigned> &m : std::vector<std::vector<unsigned>>{{3, 3, 5}, {4, 5, 257}, {6, 7, 300}, {5, 9, 515}}) {
        const int m0 = (int)m[0], m1 = (int)m[1], m2 = (int)m[2];
        run(3, m, Box{}, true);
        const int spans[][2][3] = {{{0, 1, 1}, {2, m1 - 1, m2 - 1}},           {{m0 - 2, 1, 1}, {m0, m1 - 1, m2 - 1}}, {{1, 0, 1}, {m0 - 1, 2, m2 - 1}},
                                   {{1, m1 - 2, 1}, {m0 - 1, m1, m2 - 1}},     {{1, 1, 0}, {m0 - 1, m1 - 1, 3}},       {{1, 1, m2 - 3}, {m0 - 1, m1 - 1, m2}},
                                   {{0, 1, 2}, {m0, m1 - 1, 40}},              {{1, 1, 250}, {m0 - 1, 3, 262}},        {{1, 1, 252}, {m0 - 1, m1 - 1, 264}},
                                   {{1, 1, 4}, {m0 - 1, m1 - 1, 12}}};
        for (const auto &sp : spans) run(3, m, span(m, sp[0], sp[1]), false);
        run(3, m, Box{{1, 1, (unsigned)std::min(2, m2 - 2)}, {1, 1, 1}}, false);
        run(3, m, m0 >= 4 && m1 >= 5 ? Box{{1, 1, 1}, {2, 3, 5}} : Box{{1, 1, 1}, {1, 2, 3}}, false);
    }
    EXPECT(total > 0);
    // the error returns: nothing is read or written
    std::vector<unsigned> m = {4, 5, 7};
    std::vector<float> u(140, -3.0f);
    std::vector<unsigned> locked(140, 0);
    unsigned char byte = 100;   // a one-byte image: a call that went on would read past it
    Harmonic h = {};
    h.n = 3;
    h.m = m.data();
    h.u = u.data();
    h.locked = locked.data();
    const unsigned zero[3] = {0, 0, 0}, one[3] = {1, 1, 1};
    for (unsigned axis = 0; axis < 3; axis++) {
        unsigned o[3] = {0, 0, 0}, e[3] = {1, 1, 1};
        e[axis] = 0;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, o, e, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
        e[axis] = 1;
        o[axis] = m[axis];
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, o, e, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
        o[axis] = m[axis] - 1;
        e[axis] = 2;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, o, e, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
        o[axis] = 0xffffffffu;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, o, e, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
        o[axis] = 2;
        e[axis] = 0xffffffffu;
        EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, o, e, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    }
    EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, zero, nullptr, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, nullptr, one, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_occupancy_region_cpu(&h, nullptr, nullptr, nullptr, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_occupancy_region_cpu(nullptr, &byte, nullptr, nullptr, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    h.n = 4;
    EXPECT(epic_hip_set_occupancy_region_cpu(&h, &byte, nullptr, nullptr, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_reset_free_cells_3d_cpu(&h) == EPIC_ERROR_INVALID_DATA);
    for (size_t i = 0; i < u.size(); i++) EXPECT(u[i] == -3.0f && locked[i] == 0);
    printf("occupancy region host code: ok (%llu cells changed)\n", total);
    return 0;
}
