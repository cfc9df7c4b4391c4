// occupancy_inflate.hip -- exact Euclidean inflation of the obstacle bytes of a block on the device (gfx950), in front of the
// ingestion rule (include/epic_hip.h: epic_hip_set_occupancy_inflated_gpu).  The block is the region's bytes as uploaded, extent[0] *
// extent[1] rows of extent[2] bytes; a cell within sqrt(radius_sq) of a source (a byte that is not no_change and reaches the
// threshold) that is not a source itself gets the byte X.  The bytes are edited in place: occupancy_region_kernel then reads B'.
//
// Two kernels, bits all the way, no atomics:
//   1. occupancy_source_bits_kernel: one wave per (row, 64-cell word of the row, counted from the block's first column).  Lane L tests
//      the byte of column 64 word + L (one dword per four lanes where the row width and the copy are aligned, single bytes
//      otherwise), __ballot is the word of source bits, lane 0 stores it: rows x nwords words, cells past the row's end are 0.
//      The bytes are read once; the dilation works on a bit per cell, an eighth of the block's size.
//   2. occupancy_inflate_kernel: a workgroup owns a brick of tz planes x ty rows x kBrickWords words.  The brick's source words with
//      a halo of hz planes, hy rows and one word on each side along x go into LDS (a lane loads a word; outside the block: 0):
//      3-D, radius 16: 40 x 48 x 4 words = 60 KB.  Then one lane per output word: the offsets (dz, dy) with dz^2 + dy^2 <= radius_sq
//      allow a half-width w = isqrt(radius_sq - dz^2 - dy^2) along x.  The host's table lists them from the widest down, as the LDS
//      distance of the row and w.  The lane ORs the three-word windows (left, centre, right) of the rows of one width into its
//      accumulator, and dilates the accumulator by one cell (D1: shift left, shift right, carry the edge bits between the words)
//      on every step down in width: a row of width w is dilated w times, at most 16 D1 per word whatever the radius.  Each D1
//      costs the outer words one valid bit at their far ends; 16 < 64.  The table is read at wave-uniform addresses.
//      Last, the lanes walk the brick's cells (four to a lane where dwords are aligned): where the dilated bit is set and the
//      source bit is not, the byte becomes X.  Only such bytes are stored; a dword belongs to one lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/epic_hip.h"
#include "kernels.h"

namespace epic_hip {

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBrickWords = 2;              // words of output along x per brick
constexpr int kLdsWords = kBrickWords + 2;  // with one halo word on each side
constexpr int kBrickCols = kBrickWords * kWave;

template <bool DWORD>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void occupancy_source_bits_kernel(const unsigned char *__restrict__ occ,
                                                                                       unsigned long long *__restrict__ bits, int width,
                                                                                       unsigned nwords, unsigned pairs, int obstacle_threshold,
                                                                                       int no_change, unsigned flags)
{
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned pair = blockIdx.x * (unsigned)kWavesPerBlock + (threadIdx.x >> 6);
    if (pair >= pairs) return;  // wave-uniform
    const unsigned row = pair / nwords, word = pair - row * nwords;
    const int col = (int)word * kWave + lane;
    const unsigned char *rowp = occ + (size_t)row * width;
    unsigned char b = 0;
    if (col < width) {
        if (DWORD) b = (unsigned char)(*reinterpret_cast<const uint32_t *>(rowp + (col & ~3)) >> (8 * (col & 3)));   // width % 4 == 0
        else b = rowp[col];
    }
    const int v = (flags & EPIC_HIP_OCC_UNSIGNED) ? (int)b : (int)(signed char)b;
    const unsigned long long w = __ballot(col < width && v != no_change && v >= obstacle_threshold);
    if (lane == 0) bits[pair] = w;
}

struct InflateGeom {
    int e0, e1, e2;       // the block
    int nwords;           // words per row of `bits`
    int tz, ty;           // planes and rows of a brick
    int hz, hy;           // halo planes and rows
    int bricks_x, bricks_y;
    int entries;
    unsigned fill;        // X in every byte
};

// one-cell dilation of the 192 cells l | c | r along x; cells beyond the far ends of l and r count as 0
__device__ inline void dilate1(unsigned long long &l, unsigned long long &c, unsigned long long &r)
{
    const unsigned long long nl = l | (l << 1) | (l >> 1) | (c << 63);
    const unsigned long long nc = c | (c << 1) | (c >> 1) | (l >> 63) | (r << 63);
    const unsigned long long nr = r | (r << 1) | (r >> 1) | (c >> 63);
    l = nl;
    c = nc;
    r = nr;
}

template <bool DWORD>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void occupancy_inflate_kernel(unsigned char *__restrict__ occ,
                                                                                   const unsigned long long *__restrict__ bits,
                                                                                   const int *__restrict__ table, InflateGeom g)
{
    extern __shared__ unsigned long long lds[];
    const int P = g.tz + 2 * g.hz, Q = g.ty + 2 * g.hy;
    unsigned long long *dilated = lds + (size_t)P * Q * kLdsWords;   // tz * ty * kBrickWords words
    const int bx = (int)(blockIdx.x % (unsigned)g.bricks_x);
    const int by = (int)((blockIdx.x / (unsigned)g.bricks_x) % (unsigned)g.bricks_y);
    const int bz = (int)(blockIdx.x / ((unsigned)g.bricks_x * (unsigned)g.bricks_y));
    const int z0 = bz * g.tz, y0 = by * g.ty, w0 = bx * kBrickWords;

    // the brick's source words and their halo; outside the block: 0
    for (int i = threadIdx.x; i < P * Q * kLdsWords; i += blockDim.x) {
        const int k = i % kLdsWords, q = (i / kLdsWords) % Q, p = i / (kLdsWords * Q);
        const int z = z0 - g.hz + p, y = y0 - g.hy + q, w = w0 - 1 + k;
        unsigned long long s = 0;
        if (z >= 0 && z < g.e0 && y >= 0 && y < g.e1 && w >= 0 && w < g.nwords) s = bits[((size_t)z * g.e1 + y) * g.nwords + w];
        lds[i] = s;
    }
    __syncthreads();

    // one lane per output word
    for (int o = threadIdx.x; o < g.tz * g.ty * kBrickWords; o += blockDim.x) {
        const int k = o % kBrickWords, q = (o / kBrickWords) % g.ty, p = o / (kBrickWords * g.ty);
        unsigned long long l = 0, c = 0, r = 0;
        if (z0 + p < g.e0 && y0 + q < g.e1 && w0 + k < g.nwords) {
            const unsigned long long *centre = lds + ((size_t)(p + g.hz) * Q + (q + g.hy)) * kLdsWords + 1 + k;
            int width = g.entries > 0 ? (table[0] & 0xff) : 0;
            for (int e = 0; e < g.entries; ++e) {   // wave-uniform: the table is the same for every lane
                const int t = table[e], w = t & 0xff;
                for (; width > w; --width) dilate1(l, c, r);
                const unsigned long long *row = centre + (t >> 8);   // |dz| <= hz and |dy| <= hy: inside the staged words
                c |= row[0];
                if (w > 0) {
                    l |= row[-1];
                    r |= row[1];
                }
            }
            for (; width > 0; --width) dilate1(l, c, r);
        }
        dilated[o] = c;
    }
    __syncthreads();

    // the brick's cells: X where the dilated bit is set and the source bit is not
    constexpr int kCells = DWORD ? 4 : 1;
    for (int i = threadIdx.x; i < g.tz * g.ty * (kBrickCols / kCells); i += blockDim.x) {
        const int cell = i * kCells, col = cell % kBrickCols, rowi = cell / kBrickCols;
        const int q = rowi % g.ty, p = rowi / g.ty;
        const int z = z0 + p, y = y0 + q, x = w0 * kWave + col;
        if (z >= g.e0 || y >= g.e1 || x >= g.e2) continue;
        const int k = col / kWave;
        const unsigned long long src = lds[((size_t)(p + g.hz) * Q + (q + g.hy)) * kLdsWords + 1 + k];
        const unsigned long long mark = (dilated[rowi * kBrickWords + k] & ~src) >> (col % kWave);
        unsigned char *at = occ + ((size_t)z * g.e1 + y) * g.e2 + x;
        if (DWORD) {   // e2 % 4 == 0 and x % 4 == 0: the lane's four cells are inside the row, at an aligned address
            const unsigned nib = (unsigned)mark & 0xfu;
            if (nib != 0) {
                const uint32_t sel = ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) |
                                     ((nib & 8u) ? 0xff000000u : 0u);
                uint32_t *at4 = reinterpret_cast<uint32_t *>(at);
                *at4 = (*at4 & ~sel) | (g.fill & sel);
            }
        } else if (mark & 1ull) {
            *at = (unsigned char)g.fill;
        }
    }
}

unsigned isqrt(unsigned v)
{
    unsigned r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

}  // namespace

OccInflatePlan plan_occupancy_inflate(const int extent[3], unsigned radius_sq)
{
    OccInflatePlan p;
    const int reach = (int)isqrt(radius_sq);
    for (int a = 0; a < 3; a++) p.extent[a] = extent[a];
    p.radius_sq = radius_sq;
    p.nwords = (extent[2] + kWave - 1) / kWave;
    p.tz = extent[0] == 1 ? 1 : 8;   // a 2-D block (or one plane): 32 rows to a wave; boxes: 8 x 16 rows to four waves
    p.ty = extent[0] == 1 ? 32 : 16;
    p.hz = std::min(reach, extent[0] - 1);   // sources lie inside the block: no offset reaches further than the block is deep
    p.hy = std::min(reach, extent[1] - 1);
    const int Q = p.ty + 2 * p.hy;
    for (int dz = -p.hz; dz <= p.hz; dz++)
        for (int dy = -p.hy; dy <= p.hy; dy++) {
            const int rest = (int)radius_sq - dz * dz - dy * dy;
            if (rest < 0) continue;
            p.table.push_back((dz * Q + dy) * kLdsWords * 256 + (int)isqrt((unsigned)rest));   // (LDS distance of the row) << 8 | w
        }
    std::stable_sort(p.table.begin(), p.table.end(), [](int a, int b) { return (a & 0xff) > (b & 0xff); });   // the widest first
    p.bits_bytes = (size_t)extent[0] * extent[1] * p.nwords * sizeof(unsigned long long);
    return p;
}

hipError_t upload_occupancy_inflate(const OccInflatePlan &p, void *d_scratch, hipStream_t stream)
{
    if (!d_scratch || p.table.empty()) return hipErrorInvalidValue;
    return hipMemcpyAsync(static_cast<unsigned char *>(d_scratch) + p.bits_bytes, p.table.data(), p.table.size() * sizeof(int), hipMemcpyHostToDevice,
                          stream);
}

hipError_t launch_occupancy_inflate(const OccInflatePlan &p, unsigned char *d_occ, void *d_scratch, int obstacle_threshold, int no_change,
                                    unsigned flags, hipStream_t stream, bool bits_ready)
{
    if (!d_occ || !d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) % 8) != 0 || p.table.empty() || p.radius_sq > 256u) return hipErrorInvalidValue;
    for (int a = 0; a < 3; a++)
        if (p.extent[a] < 1) return hipErrorInvalidValue;
    unsigned long long *d_bits = static_cast<unsigned long long *>(d_scratch);
    int *d_table = reinterpret_cast<int *>(static_cast<unsigned char *>(d_scratch) + p.bits_bytes);
    const unsigned long long pairs = (unsigned long long)p.extent[0] * (unsigned long long)p.extent[1] * (unsigned long long)p.nwords;
    InflateGeom g;
    g.e0 = p.extent[0];
    g.e1 = p.extent[1];
    g.e2 = p.extent[2];
    g.nwords = p.nwords;
    g.tz = p.tz;
    g.ty = p.ty;
    g.hz = p.hz;
    g.hy = p.hy;
    g.bricks_x = (p.nwords + kBrickWords - 1) / kBrickWords;
    g.bricks_y = (p.extent[1] + p.ty - 1) / p.ty;
    g.entries = (int)p.table.size();
    const int top = (flags & EPIC_HIP_OCC_UNSIGNED) ? 255 : 127;
    g.fill = (unsigned)((top == no_change ? top - 1 : top) & 0xff) * 0x01010101u;
    const unsigned long long bricks = (unsigned long long)g.bricks_x * (unsigned long long)g.bricks_y * (unsigned long long)((p.extent[0] + p.tz - 1) / p.tz);
    if (pairs > 0x7fffffffull || bricks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds_bytes = ((size_t)(p.tz + 2 * p.hz) * (p.ty + 2 * p.hy) * kLdsWords + (size_t)p.tz * p.ty * kBrickWords) * sizeof(unsigned long long);
    if (lds_bytes > 65536) return hipErrorInvalidValue;   // 63 488 at the largest radius
    const bool dword = (p.extent[2] % 4) == 0 && (reinterpret_cast<uintptr_t>(d_occ) % 4) == 0;
    const dim3 grid1((unsigned)((pairs + kWavesPerBlock - 1) / kWavesPerBlock)), block1(kWave * kWavesPerBlock);
    const dim3 grid2((unsigned)bricks), block2((unsigned)(p.tz * p.ty * kBrickWords));   // one lane per output word: 64 or 256
    if (dword) {
        if (!bits_ready)
            hipLaunchKernelGGL(occupancy_source_bits_kernel<true>, grid1, block1, 0, stream, d_occ, d_bits, p.extent[2], (unsigned)p.nwords,
                               (unsigned)pairs, obstacle_threshold, no_change, flags);
        hipLaunchKernelGGL(occupancy_inflate_kernel<true>, grid2, block2, lds_bytes, stream, d_occ, d_bits, d_table, g);
    } else {
        if (!bits_ready)
            hipLaunchKernelGGL(occupancy_source_bits_kernel<false>, grid1, block1, 0, stream, d_occ, d_bits, p.extent[2], (unsigned)p.nwords,
                               (unsigned)pairs, obstacle_threshold, no_change, flags);
        hipLaunchKernelGGL(occupancy_inflate_kernel<false>, grid2, block2, lds_bytes, stream, d_occ, d_bits, d_table, g);
    }
    return hipGetLastError();
}

}  // namespace epic_hip
