// occupancy_2d.hip -- dense occupancy-grid ingestion on the device-resident 2-D state (gfx950).
//
// A map message is one byte per cell.  The reference's callers expand it into a list of (x, y, type) entries, 12 bytes per
// cell, and scatter that list (set_cells_2d_kernel: one atomic on a mask word per entry).  occupancy_2d_kernel reads the bytes
// themselves: one wave per (row, 256-column strip) -- the geometry of pack_mask_2d_kernel --, lane L owning columns
// 256 strip + 4 L .. + 3.  The lane reads its four bytes, its float4 of u and the strip's four 64-bit lane-mask words, decides
// its four cells by the rule of occupancy_rule.h, four ballots ARE the four new mask words (lanes 0-3 write one each, and only
// a word that differs), and the float4 goes back where a value changed.  No atomics on the mask.
//
// `changed` falls out of the ballots: popcount(old word ^ new word) cells changed their lock, a fifth ballot per word marks the
// cells that stayed locked and changed their value (goal <-> obstacle).  The count is wave-uniform: lane 0 adds it, once per wave
// and only when it is not zero, to one of kOccCounters words in lines of their own (kernels.h: one word for all serialises).
//
// Border rows, border columns and the padding beyond `cols` are never decided: their mask bits are handed through as they are
// (locked: pack_mask_2d_kernel forces them, set_cells_2d_kernel keeps them), their values are not stored.
//
// The image on the device: `occ_pitch` bytes per row.  Where occ_pitch is a multiple of 4 and at least the field's pitch (the
// driver copies the message as it is: where cols is a multiple of 256), a lane's four bytes are one aligned dword (DWORD = true);
// otherwise the lane loads the bytes of its columns below `cols` one by one.
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
__global__ __launch_bounds__(kWave * kWavesPerBlock) void occupancy_2d_kernel(float *u, uint32_t *maskw, const unsigned char *occ,
                                                                              size_t occ_pitch, int rows, int cols, int pitch,
                                                                              int obstacle_threshold, int no_change, unsigned flags,
                                                                              unsigned long long *changed)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int nstrips = pitch >> 8;
    const int strip = blockIdx.y * kWavesPerBlock + (threadIdx.x >> 6);
    const int r = blockIdx.x;  // rows ride on grid.x: grid.y stops at 65535
    if (strip >= nstrips || r < 1 || r >= rows - 1) return;  // wave-uniform; border rows are never touched
    const int c0 = strip * kStripCols + lane * kColsPerLane;
    unsigned long long *mw = reinterpret_cast<unsigned long long *>(maskw) + ((size_t)r * nstrips + strip) * 4;
    float4 *up = reinterpret_cast<float4 *>(u + (size_t)r * pitch + c0);   // in bounds for every lane: rows are padded to whole strips
    const float4 uv = *up;
    const unsigned long long old[kColsPerLane] = {mw[0], mw[1], mw[2], mw[3]};
    const unsigned char *row = occ + (size_t)r * occ_pitch;
    unsigned char b[kColsPerLane];
    if (DWORD) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(row + c0);
#pragma unroll
        for (int j = 0; j < kColsPerLane; ++j) b[j] = (unsigned char)(w >> (8 * j));
    } else {
#pragma unroll
        for (int j = 0; j < kColsPerLane; ++j) b[j] = c0 + j < cols ? row[c0 + j] : (unsigned char)0;
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
        if (c >= 1 && c <= cols - 2) cell = occupancy_cell(b[j], v[j], was_locked, obstacle_threshold, no_change, flags);
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
        atomicAdd(changed + (size_t)((r + 37 * strip) & (kOccCounters - 1)) * kOccCounterStride, (unsigned long long)count);
}

// srvResetFreeCells on the resident state: u = EPIC_LOG_SPACE_FREE wherever the mask bit is clear (unlocked cells are interior
// cells: the border and the padding are locked).  Same geometry.
__global__ __launch_bounds__(kWave * kWavesPerBlock) void reset_free_cells_2d_kernel(float *u, const uint32_t *maskw, int rows, int pitch)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int nstrips = pitch >> 8;
    const int strip = blockIdx.y * kWavesPerBlock + (threadIdx.x >> 6);
    const int r = blockIdx.x;
    if (strip >= nstrips || r >= rows) return;  // wave-uniform
    const unsigned long long *mw = reinterpret_cast<const unsigned long long *>(maskw) + ((size_t)r * nstrips + strip) * 4;
    if ((mw[0] & mw[1] & mw[2] & mw[3]) == ~0ull) return;  // wave-uniform: nothing unlocked in this strip of the row
    float4 *up = reinterpret_cast<float4 *>(u + (size_t)r * pitch + strip * kStripCols + lane * kColsPerLane);
    float4 uv = *up;
    const float free_value = (float)EPIC_LOG_SPACE_FREE;
    if (!((mw[0] >> lane) & 1ull)) uv.x = free_value;
    if (!((mw[1] >> lane) & 1ull)) uv.y = free_value;
    if (!((mw[2] >> lane) & 1ull)) uv.z = free_value;
    if (!((mw[3] >> lane) & 1ull)) uv.w = free_value;
    *up = uv;
}

bool geometry_ok(int rows, int cols, int pitch) { return rows >= 3 && cols >= 3 && pitch >= cols && (pitch % kStripCols) == 0; }

}  // namespace

hipError_t launch_occupancy_2d(float *u, uint32_t *maskw, const unsigned char *d_occ, size_t occ_pitch, int rows, int cols, int pitch,
                               int obstacle_threshold, int no_change, unsigned flags, unsigned long long *d_changed, hipStream_t stream)
{
    if (!u || !maskw || !d_occ || !geometry_ok(rows, cols, pitch) || occ_pitch < (size_t)cols) return hipErrorInvalidValue;
    const int nstrips = pitch / kStripCols;
    const dim3 grid(rows, (nstrips + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    // a lane's four bytes as one dword: aligned, and inside the row for the last lane of the last strip too
    const bool dword = (occ_pitch % 4) == 0 && occ_pitch >= (size_t)pitch && (reinterpret_cast<uintptr_t>(d_occ) % 4) == 0;
    if (dword)
        hipLaunchKernelGGL(occupancy_2d_kernel<true>, grid, block, 0, stream, u, maskw, d_occ, occ_pitch, rows, cols, pitch,
                           obstacle_threshold, no_change, flags, d_changed);
    else
        hipLaunchKernelGGL(occupancy_2d_kernel<false>, grid, block, 0, stream, u, maskw, d_occ, occ_pitch, rows, cols, pitch,
                           obstacle_threshold, no_change, flags, d_changed);
    return hipGetLastError();
}

hipError_t launch_reset_free_cells_2d(float *u, const uint32_t *maskw, int rows, int cols, int pitch, hipStream_t stream)
{
    if (!u || !maskw || !geometry_ok(rows, cols, pitch)) return hipErrorInvalidValue;
    const int nstrips = pitch / kStripCols;
    const dim3 grid(rows, (nstrips + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(reset_free_cells_2d_kernel, grid, dim3(kWave * kWavesPerBlock), 0, stream, u, maskw, rows, pitch);
    return hipGetLastError();
}

}  // namespace epic_hip
