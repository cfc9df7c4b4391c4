// Stand-alone caller of the rolling-window shift on the host arrays (epic_amd/csrc/field_shift_cpu.cpp, included as source), built with
// -fsanitize=address,undefined by tests/test_shift_cpu.py: exactly-sized heap arrays, so a source index one cell outside the grid is an
// error, and INT_MIN must not overflow anywhere.  The python test's shapes and shifts, both fills; kept against its closed form.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../epic_amd/csrc/field_shift_cpu.cpp"

#define EXPECT(cond) ((cond) ? (void)0 : (fprintf(stderr, "EXPECT failed: %s (line %d)\n", #cond, __LINE__), exit(1)))

int main()
{
    const unsigned shapes[3][3] = {{1, 5, 5}, {1, 37, 300}, {6, 7, 70}};
    const int diagonal[3][3] = {{1, 3, -33}, {-1, -2, 31}, {0, 1, 256}};
    unsigned long long calls = 0, total = 0;
    for (const auto &g : shapes) {
        const unsigned n = g[0] == 1 ? 2 : 3, lead = 3 - n;
        std::vector<unsigned> m(g + lead, g + 3);
        const size_t cells = (size_t)g[0] * g[1] * g[2];
        std::vector<std::vector<int>> shifts = {std::vector<int>(n, 0)};
        for (unsigned a = 0; a < n; a++)
            for (int s : {1, -1, INT_MIN, INT_MAX, (int)m[a] - 2, 2 - (int)m[a]}) {
                shifts.push_back(std::vector<int>(n, 0));
                shifts.back()[a] = s;
            }
        for (const auto &d : diagonal) shifts.push_back(std::vector<int>(d + lead, d + 3));
        for (const auto &shift : shifts)
            for (unsigned fill : {(unsigned)EPIC_CELL_TYPE_FREE, (unsigned)EPIC_CELL_TYPE_OBSTACLE}) {
                std::vector<float> u(cells);
                std::vector<unsigned> locked(cells);
                for (size_t i = 0; i < cells; i++) {
                    u[i] = -(float)(i % 977);
                    locked[i] = (unsigned)(i % 7 == 0);
                }
                Harmonic h = {};
                h.n = n;
                h.m = m.data();
                h.u = u.data();
                h.locked = locked.data();
                unsigned long long kept = ~0ull, want = 1;
                EXPECT(epic_hip_shift_field_cpu(&h, shift.data(), fill, &kept) == EPIC_SUCCESS);
                for (unsigned a = 0; a < n; a++) {
                    const long long inner = (long long)m[a] - 2, by = shift[a] < 0 ? -(long long)shift[a] : shift[a];
                    want *= (unsigned long long)(by >= inner ? 0 : inner - by);
                }
                EXPECT(kept == want && u[0] == 0.0f && u[cells - 1] == -(float)((cells - 1) % 977));   // the corners are never written
                calls++;
                total += kept;
            }
    }
    Harmonic none = {};
    int one[3] = {1, 1, 1};
    EXPECT(epic_hip_shift_field_cpu(&none, one, EPIC_CELL_TYPE_FREE, nullptr) == EPIC_ERROR_INVALID_DATA);
    EXPECT(total > 0);
    printf("field shift host code: ok (%llu calls, %llu cells kept)\n", calls, total);
    return 0;
}
