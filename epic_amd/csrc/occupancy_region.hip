// occupancy_region.hip -- dense occupancy ingestion into a rectangular region of a device-resident 2-D or 3-D field (gfx950).
//
// A costmap update is a window of a map, a depth sensor's refresh a box of voxels: one byte per cell of the box, unpitched.  The 3-D
// masks are the 2-D lane masks over the m0 * m1 rows of m2 cells (kernels.h), so the geometry of occupancy_2d_kernel carries over:
// one wave per (row, 256-column strip), lane L owning columns 256 strip + 4 L .. + 3; the lane reads its float4 of u and the
// strip's four 64-bit lane-mask words, decides its cells by the rule of occupancy_rule.h, four ballots are the four new words (a
// word is written only where it differs, by one lane), the float4 goes back where a value changed, `changed` falls out of the
// popcounts into the spread counters.  No atomics on the mask; every store is an ordinary vector store.
//
// What differs from occupancy_2d_kernel:
//   * only the rows and strips the box touches are launched, and the (row, strip) pairs are numbered through: wave w of block b
//     takes pair 4 b + w.  (Strips on grid.y, four to a block, would leave half of every block idle on a 512-column field.)
//   * a lane decides a cell only if the cell lies inside the box, its row is off the faces of the grid (3-D: x0 and x1 both; 2-D:
//     the row is not a border row) and its column is in [1, cols - 2].  Every other cell hands its mask bit and its value through,
//     which is what makes a strip that the box covers in part correct.
//   * the byte of cell (row, c) sits at occ[i * extent[2] + (c - origin[2])], i the row's number inside the box.  Where the box's
//     column origin and width are multiples of 4 and the copy on the device is aligned, a lane's four cells are all inside the box
//     or all outside it and its bytes are one aligned dword (DWORD = true); otherwise the lane loads the bytes of its cells inside
//     the box one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "occupancy_rule.h"

namespace epic_hip {

namespace {

constexpr int kWave = 64;
constexpr int kColsPerLane = 4;
constexpr int kStripCols = kWave * kColsPerLane;  // 256
constexpr int kWavesPerBlock = 4;

template <bool DWORD>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void occupancy_region_kernel(float *u, uint32_t *maskw, const unsigned char *occ,
                                                                                  OccRegion g, int pitch, int strip_lo, unsigned nst,
                                                                                  unsigned pairs, int obstacle_threshold, int no_change,
                                                                                  unsigned flags, unsigned long long *changed)
{
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned pair = blockIdx.x * (unsigned)kWavesPerBlock + (threadIdx.x >> 6);
    if (pair >= pairs) return;  // wave-uniform
    const unsigned i = pair / nst;  // row of the box
    const int strip = strip_lo + (int)(pair - i * nst);
    const int x0 = g.origin[0] + (int)(i / (unsigned)g.extent[1]), x1 = g.origin[1] + (int)(i % (unsigned)g.extent[1]);
    if ((g.faces0 && (x0 < 1 || x0 > g.m0 - 2)) || x1 < 1 || x1 > g.m1 - 2) return;  // wave-uniform; rows on a face are never touched
    const int nstrips = pitch >> 8;
    const size_t r = (size_t)x0 * g.m1 + x1;
    const int c0 = strip * kStripCols + lane * kColsPerLane;
    unsigned long long *mw = reinterpret_cast<unsigned long long *>(maskw) + (r * nstrips + strip) * 4;
    float4 *up = reinterpret_cast<float4 *>(u + r * pitch + c0);   // in bounds for every lane: rows are padded to whole strips
    const float4 uv = *up;
    const unsigned long long old[kColsPerLane] = {mw[0], mw[1], mw[2], mw[3]};
    const int lo = g.origin[2], hi = g.origin[2] + g.extent[2];   // the box's columns [lo, hi)
    const unsigned char *row = occ + (size_t)i * g.extent[2];     // the byte of column c: row[c - lo]
    unsigned char b[kColsPerLane];
    if (DWORD) {
        const uint32_t w = (c0 >= lo && c0 < hi) ? *reinterpret_cast<const uint32_t *>(row + (c0 - lo)) : 0u;
#pragma unroll
        for (int j = 0; j < kColsPerLane; ++j) b[j] = (unsigned char)(w >> (8 * j));
    } else {
#pragma unroll
        for (int j = 0; j < kColsPerLane; ++j) b[j] = (c0 + j >= lo && c0 + j < hi) ? row[c0 + j - lo] : (unsigned char)0;
    }
    float v[kColsPerLane] = {uv.x, uv.y, uv.z, uv.w};
    unsigned count = 0;
    bool store = false;
    // every lane of the wave stays active down to the last ballot
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
        const int c = c0 + j;
        const bool was_locked = (old[j] >> lane) & 1ull;
        OccCell cell = {v[j], was_locked, false};
        if (c >= lo && c < hi && c >= 1 && c <= g.cols - 2) cell = occupancy_cell(b[j], v[j], was_locked, obstacle_threshold, no_change, flags);
        const bool moved = occupancy_float_bits(cell.u) != occupancy_float_bits(v[j]);
        const unsigned long long now = __ballot(cell.locked);
        const unsigned long long relocked = __ballot(cell.locked && was_locked && moved);
        count += (unsigned)__popcll(old[j] ^ now) + (unsigned)__popcll(relocked);
        if (lane == j && now != old[j]) mw[j] = now;
        store |= moved;
        v[j] = cell.u;
    }
    if (store) *up = make_float4(v[0], v[1], v[2], v[3]);
    if (changed != nullptr && count != 0 && lane == 0)
        atomicAdd(changed + (size_t)(((unsigned)r + 37u * (unsigned)strip) & (unsigned)(kOccCounters - 1)) * kOccCounterStride,
                  (unsigned long long)count);
}

}  // namespace

hipError_t launch_occupancy_region(float *u, uint32_t *maskw, const unsigned char *d_occ, const OccRegion &g, int pitch,
                                   int obstacle_threshold, int no_change, unsigned flags, unsigned long long *d_changed, hipStream_t stream)
{
    if (!u || !maskw || !d_occ || g.m0 < (g.faces0 ? 3 : 1) || (!g.faces0 && g.m0 != 1) || g.m1 < 3 || g.cols < 3 || pitch < g.cols ||
        (pitch % kStripCols) != 0)
        return hipErrorInvalidValue;
    const int m[3] = {g.m0, g.m1, g.cols};
    for (int a = 0; a < 3; a++)   // the box lies inside the grid: the kernel clips nothing
        if (g.origin[a] < 0 || g.extent[a] < 1 || (long long)g.origin[a] + g.extent[a] > m[a]) return hipErrorInvalidValue;
    const int strip_lo = g.origin[2] / kStripCols, strip_hi = (g.origin[2] + g.extent[2] - 1) / kStripCols;
    const unsigned long long nst = (unsigned long long)(strip_hi - strip_lo + 1);
    const unsigned long long pairs = (unsigned long long)g.extent[0] * (unsigned long long)g.extent[1] * nst;
    if (pairs > 0x7fffffffull) return hipErrorInvalidValue;   // (2^31 pairs are 2^39 cells)
    const dim3 grid((unsigned)((pairs + kWavesPerBlock - 1) / kWavesPerBlock)), block(kWave * kWavesPerBlock);
    // a lane's four bytes as one dword: its four cells are inside the box together, at an aligned address
    const bool dword = (g.origin[2] % 4) == 0 && (g.extent[2] % 4) == 0 && (reinterpret_cast<uintptr_t>(d_occ) % 4) == 0;
    if (dword)
        hipLaunchKernelGGL(occupancy_region_kernel<true>, grid, block, 0, stream, u, maskw, d_occ, g, pitch, strip_lo, (unsigned)nst,
                           (unsigned)pairs, obstacle_threshold, no_change, flags, d_changed);
    else
        hipLaunchKernelGGL(occupancy_region_kernel<false>, grid, block, 0, stream, u, maskw, d_occ, g, pitch, strip_lo, (unsigned)nst,
                           (unsigned)pairs, obstacle_threshold, no_change, flags, d_changed);
    return hipGetLastError();
}

}  // namespace epic_hip
