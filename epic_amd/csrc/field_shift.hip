// field_shift.hip -- the rolling-window shift of a device-resident 2-D or 3-D field by whole cells (gfx950): values and lock bits in
// ONE launch.  The rule is field_shift_rule.h; the host twin is field_shift_cpu.cpp.
//
// Geometry: the one of the occupancy kernels.  One wave per (destination row, 256-column strip) -- the 3-D field is m0 * m1 rows of
// m2 cells --, lane L owning columns 256 strip + 4 L .. + 3 as one quad, the (row, strip) pairs numbered through, four to a block.
// Everything about a row is wave-uniform and lives in SGPRs: whether it is a border / face row, its source row x + shift (64-bit),
// whether that row is interior.
//
// Values.  u is read from the current buffer and the shifted field is written to the OTHER buffer, every cell of every row up to the
// pitch: no cell is read after it was overwritten, and the driver hands "current" over by flipping Ctx::cur.  Cells the rule does
// not write -- border and face cells, the padding columns -- are copied from the current buffer at their own index, so the
// destination is a complete field; only the lanes that hold such a cell load their own quad (a face row: all of them).
//   * The column shift s2 = 4 a + b, b = s2 mod 4: destination quad Q needs columns from the source quads Q + a and Q + a + 1.  A lane
//     loads ONE aligned quad, Q + a (clamped into the row; a clamped quad only ever feeds cells whose source is outside the grid, which
//     take the fill), and takes the first b floats of Q + a + 1 from its right neighbour's registers: b full-wave DPP moves
//     (v_mov_b32_dpp wave_shl:1, the sweeps' horizontal-neighbour move).  Lane 63's right neighbour is the first quad of the next
//     strip: wave-uniform, one more 16-byte load at a scalar address.  b is a template parameter: the picks are register renames and
//     b == 0 (every shift along the slower axes only, every column shift by a multiple of 4) moves nothing.  Every global access of u
//     is a 16-byte aligned dwordx4.
//     The alternatives read the same bytes from HBM: two overlapping quad loads per lane double the vector-memory instructions and
//     the L1 lookups of a kernel that does nothing else; an LDS row per wave costs a ds_write_b128, a wait and four ds_read_b32 at
//     bank-conflicting strides for b != 0.  The DPP form is at most 3 VALU moves per lane beside 9 v_cndmask.
//   * A row whose source row lies outside the interior is written from the fill constant without a load.
//   * Bit patterns move as uint32: no float instruction ever sees a value, so any payload survives.
//
// Lock bits.  The lane masks (kernels.h) hold, per row and strip, four 64-bit words, bit L of word j = cell 256 strip + 4 L + j.
// Along a row the words j of successive strips are one bit stream over the quads: stream_j[Q] = lock of cell 4 Q + j.  A column shift
// s2 maps stream j onto stream j' = (j + s2) mod 4, moved by q = floor((j + s2) / 4) quads -- so lane j (0 .. 3) of the wave produces
// destination word j: it funnel-shifts two words of stream j' of the SOURCE row by q mod 64, ANDs the range of lanes whose cell and
// source cell are both interior (closed form: two divisions by 4), ORs the fill's lock bit on the interior cells without a source and
// forces every other bit -- border, face, padding -- locked, as pack_mask_*_kernel does.  The new words go to a second mask block (no
// word is read after it was rewritten); the driver swaps the blocks.  The fused copy of a 2-D field is rebuilt by the caller.
//
// Plain vector stores only; no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_shift_rule.h"
#include "kernels.h"

namespace epic_hip {

namespace {

constexpr int kWave = 64;
constexpr int kColsPerLane = 4;
constexpr int kStripCols = kWave * kColsPerLane;  // 256
constexpr int kWavesPerBlock = 4;

typedef uint32_t quad __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

struct ShiftArgs {
    const uint32_t *src;   // the current buffer of u, as bit patterns
    uint32_t *dst;         // the other one
    const u64 *mask_in;    // lane masks (kernels.h)
    u64 *mask_out;         // a second block of the same size
    ShiftPlan p;
    int pitch, nstrips;
    unsigned pairs;        // rows x nstrips
};

// lane i receives lane i + 1's v; lane 63 keeps `edge`.  All 64 lanes are active wherever this is called.
__device__ __forceinline__ uint32_t from_next_lane(uint32_t v, uint32_t edge)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

// bit L set for every lane L in 0 .. 63 whose cell base + 4 L lies in [lo, hi]
__device__ __forceinline__ u64 lanes_in(long long lo, long long hi, long long base)
{
    long long first = (lo - base + 3) >> 2, last = (hi - base) >> 2;   // ceil and floor of a division by 4 (arithmetic shifts)
    if (first < 0) first = 0;
    if (last > kWave - 1) last = kWave - 1;
    if (first > last) return 0ull;
    const int n = (int)(last - first) + 1;
    return (n == kWave ? ~0ull : (1ull << n) - 1ull) << first;
}

template <int B>   // the column shift mod 4: floats a destination quad is off its first source quad
__global__ __launch_bounds__(kWave * kWavesPerBlock) void field_shift_kernel(ShiftArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned pair = blockIdx.x * (unsigned)kWavesPerBlock + (threadIdx.x >> 6);
    if (pair >= a.pairs) return;   // wave-uniform
    const ShiftPlan &p = a.p;
    const unsigned r = pair / (unsigned)a.nstrips;
    const int strip = (int)(pair - r * (unsigned)a.nstrips);
    const int x0 = (int)(r / (unsigned)p.m[1]), x1 = (int)(r % (unsigned)p.m[1]);
    const int cols = p.m[2];
    const bool face = x1 < 1 || x1 > p.m[1] - 2 || (p.faces0 && (x0 < 1 || x0 > p.m[0] - 2));
    long long y0 = 0, y1 = 0;
    const bool ok0 = !p.faces0 || shift_source(x0, p.s[0], p.m[0], y0);
    const bool row_ok = shift_source(x1, p.s[1], p.m[1], y1) && ok0 && !face && !p.none;   // the source row is an interior row
    const size_t srow = row_ok ? (size_t)y0 * (size_t)p.m[1] + (size_t)y1 : 0;
    const int c0 = strip * kStripCols + lane * kColsPerLane;
    const size_t at = (size_t)r * a.pitch + c0;   // in bounds for every lane: rows are padded to whole strips

    // ---- values
    quad own = {0u, 0u, 0u, 0u};   // the lane's cells as they are: only where one of them is not the rule's to write
    if (face || c0 == 0 || c0 + kColsPerLane > cols - 1) own = *reinterpret_cast<const quad *>(a.src + at);
    uint32_t v[kColsPerLane] = {p.fill_bits, p.fill_bits, p.fill_bits, p.fill_bits};
    if (row_ok) {   // wave-uniform
        const int nq = a.pitch >> 2, qa = (p.s[2] - B) / 4;   // s2 = 4 qa + B exactly
        const uint32_t *row = a.src + srow * a.pitch;
        const int q = (c0 >> 2) + qa;
        const quad q0 = *reinterpret_cast<const quad *>(row + 4 * (size_t)min(max(q, 0), nq - 1));
        if (B == 0) {
            v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
        } else {
            const int qe = strip * kWave + kWave + qa;   // the quad right of lane 63's
            const quad e = *reinterpret_cast<const quad *>(row + 4 * (size_t)min(max(qe, 0), nq - 1));
            const uint32_t nx = from_next_lane(q0.x, e.x);
            const uint32_t ny = B >= 2 ? from_next_lane(q0.y, e.y) : 0u;
            const uint32_t nz = B >= 3 ? from_next_lane(q0.z, e.z) : 0u;
            if (B == 1) { v[0] = q0.y; v[1] = q0.z; v[2] = q0.w; v[3] = nx; }
            if (B == 2) { v[0] = q0.z; v[1] = q0.w; v[2] = nx; v[3] = ny; }
            if (B == 3) { v[0] = q0.w; v[1] = nx; v[2] = ny; v[3] = nz; }
        }
    }
    long long lo, hi;   // the columns that are interior and have an interior source
    shift_covered(p.s[2], cols, lo, hi);
    const uint32_t mine[kColsPerLane] = {own.x, own.y, own.z, own.w};
    uint32_t o[kColsPerLane];
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
        const int c = c0 + j;
        const bool interior = !face && c >= 1 && c <= cols - 2;
        const bool covered = row_ok && c >= lo && c <= hi;
        o[j] = !interior ? mine[j] : covered ? v[j] : p.fill_bits;
    }
    *reinterpret_cast<quad *>(a.dst + at) = quad{o[0], o[1], o[2], o[3]};

    // ---- lock bits: lane j writes word j of this (row, strip)
    if (lane < kColsPerLane) {
        const int j = lane;
        u64 w = ~0ull;   // a border or face row: every bit locked
        if (!face) {
            const long long base = (long long)strip * kStripCols + j;   // the cell of bit 0
            const u64 inner = lanes_in(1, cols - 2, base);
            u64 covered = 0ull, moved = 0ull;
            if (row_ok) {
                covered = lanes_in(lo, hi, base);
                const int t = j + p.s[2], jp = t & 3;                       // the source stream, and
                const long long first = (long long)strip * kWave + (t >> 2);  // the quad of the row its bit 0 comes from
                const long long word = first >> 6;
                const int off = (int)(first & 63);
                const u64 *words = a.mask_in + srow * (size_t)a.nstrips * 4 + jp;   // stream jp of the source row: word k at [4 k]
                const u64 w0 = word >= 0 && word < a.nstrips ? words[4 * word] : 0ull;
                const u64 w1 = off != 0 && word + 1 >= 0 && word + 1 < a.nstrips ? words[4 * (word + 1)] : 0ull;
                moved = off ? (w0 >> off) | (w1 << (64 - off)) : w0;
            }
            w = (moved & covered) | (p.fill_locked ? inner & ~covered : 0ull) | ~inner;
        }
        a.mask_out[((size_t)r * a.nstrips + strip) * 4 + j] = w;
    }
}

}  // namespace

hipError_t launch_field_shift(const float *u_cur, float *u_other, const uint32_t *maskw, uint32_t *maskw_out, const ShiftPlan &plan, int pitch,
                              hipStream_t stream)
{
    if (!u_cur || !u_other || u_cur == u_other || !maskw || !maskw_out || maskw == maskw_out || plan.zero || plan.m[0] < (plan.faces0 ? 3 : 1) ||
        (!plan.faces0 && plan.m[0] != 1) || plan.m[1] < 3 || plan.m[2] < 3 || pitch < plan.m[2] || (pitch % kStripCols) != 0)
        return hipErrorInvalidValue;
    for (int i = 0; i < 3; i++) {   // what shift_plan() promises: a shift that keeps anything is shorter than the interior
        const long long by = plan.s[i] < 0 ? -(long long)plan.s[i] : plan.s[i];
        if (by != 0 && by >= (long long)plan.m[i] - 2) return hipErrorInvalidValue;
    }
    ShiftArgs a;
    a.src = reinterpret_cast<const uint32_t *>(u_cur);
    a.dst = reinterpret_cast<uint32_t *>(u_other);
    a.mask_in = reinterpret_cast<const u64 *>(maskw);
    a.mask_out = reinterpret_cast<u64 *>(maskw_out);
    a.p = plan;
    a.pitch = pitch;
    a.nstrips = pitch / kStripCols;
    const unsigned long long pairs = (unsigned long long)plan.m[0] * (unsigned long long)plan.m[1] * (unsigned long long)a.nstrips;
    if (pairs > 0x7fffffffull) return hipErrorInvalidValue;   // (2^31 pairs are 2^39 cells)
    a.pairs = (unsigned)pairs;
    const dim3 grid((unsigned)((pairs + kWavesPerBlock - 1) / kWavesPerBlock)), block(kWave * kWavesPerBlock);
    switch (plan.s[2] & 3) {
    case 0: hipLaunchKernelGGL(field_shift_kernel<0>, grid, block, 0, stream, a); break;
    case 1: hipLaunchKernelGGL(field_shift_kernel<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(field_shift_kernel<2>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(field_shift_kernel<3>, grid, block, 0, stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace epic_hip
