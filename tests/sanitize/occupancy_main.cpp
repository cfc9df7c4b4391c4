// Stand-alone caller of the host half of the dense occupancy ingestion (epic_amd/csrc/occupancy_cpu.cpp), built with
// -fsanitize=address,undefined by tests/test_occupancy_sanitize.py: exactly-sized heap arrays, so a read or write one cell past the
// image, u or locked is an error; odd shapes; every flag combination; the error returns.
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
    const unsigned shapes[][2] = {{3, 3}, {3, 5}, {5, 257}, {37, 301}, {130, 515}};
    unsigned long long total = 0;
    for (const auto &shape : shapes) {
        const size_t rows = shape[0], cols = shape[1], cells = rows * cols;
        std::vector<unsigned> m = {shape[0], shape[1]};
        for (unsigned flags = 0; flags < 8; flags++) {
            std::vector<float> u(cells);
            std::vector<unsigned> locked(cells);
            std::vector<unsigned char> occ(cells);
            unsigned s = 12345u + flags;
            for (size_t i = 0; i < cells; i++) {
                s = s * 1664525u + 1013904223u;
                locked[i] = (s >> 28) < 3;
                u[i] = locked[i] ? ((s >> 20) & 1 ? 0.0f : -1e6f) : -(float)((s >> 8) & 1023);
                occ[i] = (unsigned char)(s >> 12);
            }
            const std::vector<float> u0 = u;
            const std::vector<unsigned> l0 = locked;
            Harmonic h = {};
            h.n = 2;
            h.m = m.data();
            h.u = u.data();
            h.locked = locked.data();
            unsigned long long changed = ~0ull;
            EXPECT(epic_hip_set_occupancy_2d_cpu(&h, occ.data(), 50, -2, flags, &changed) == EPIC_SUCCESS);
            EXPECT(changed <= (rows - 2) * (cols - 2));
            for (size_t y = 0; y < rows; y++)
                for (size_t x = 0; x < cols; x++)
                    if (y == 0 || x == 0 || y == rows - 1 || x == cols - 1) EXPECT(u[y * cols + x] == u0[y * cols + x] && locked[y * cols + x] == l0[y * cols + x]);
            total += changed;
            EXPECT(epic_hip_set_occupancy_2d_cpu(&h, occ.data(), 250, 1000, flags, nullptr) == EPIC_SUCCESS);
            EXPECT(epic_hip_reset_free_cells_2d_cpu(&h) == EPIC_SUCCESS);
            for (size_t i = 0; i < cells; i++) EXPECT(locked[i] != 0 || u[i] == -1e6f || i / cols == 0 || i / cols == rows - 1 || i % cols == 0 || i % cols == cols - 1);
        }
    }
    EXPECT(total > 0);
    Harmonic bad = {};
    unsigned char byte = 0;
    EXPECT(epic_hip_set_occupancy_2d_cpu(nullptr, &byte, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_set_occupancy_2d_cpu(&bad, &byte, 50, -2, 0, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(epic_hip_reset_free_cells_2d_cpu(&bad) == EPIC_ERROR_INVALID_DATA);
    printf("occupancy host code: ok (%llu cells changed)\n", total);
    return 0;
}
