// occupancy_points.hip -- a point cloud or a laser scan turned into the block of bytes of the inflated ingestion, on the device (gfx950;
// include/epic_hip.h: epic_hip_set_occupancy_points_gpu).  Only the points cross the bus.  The rule is occupancy_points_rule.h's, the
// same functions the host twin runs.
//
// Two bit planes, `hit` and `clear`, in the word layout of occupancy_source_bits_kernel (occupancy_inflate.hip): one 64-bit word per
// 64 cells along the block's fastest axis, nwords words per row, cells past the row's end 0.  The hit plane IS the source-bit plane of
// the block these kernels write, so occupancy_inflate_kernel takes it as it is and the ballot stage over the bytes is skipped.
//   1. occupancy_points_bin_kernel: a lane per point.  A hit computes its word and bit.  Clouds are coherent -- a scan line falls into a
//      handful of words --, so lanes that target one word merge in registers before memory sees them: the lowest pending lane's word
//      is broadcast, the lanes that match OR their bits together over six xor-shuffles and the leader issues one vector atomic-or.
//      kMergeRounds such rounds; what is still pending after them (a scattered cloud: 64 words to a wave) goes out lane by lane.
//   2. occupancy_points_ray_kernel (only with a sensor): a lane per point walks its ray, bounded by the integer step count.  Every ray
//      starts in the sensor's cell: the bits a lane sets in the sensor's word stay in a register of their own and leave through the
//      merge above after the walk, one atomic per wave where unmerged rays would send one per ray and step to a single word.  The
//      other words are accumulated along the walk -- a ray stays in a word for up to 64 steps along the fastest axis -- and flushed with
//      one atomic when the ray enters the next word.
//   3. occupancy_points_expand_kernel: planes to bytes.  A lane covers 16 cells of a word: a nibble of each plane is spread to four
//      byte masks (a multiply and a mask), X / 0 / no_change are selected with them, one 16-byte store (rows whose width is no multiple
//      of 16 take byte stores).
// Vector stores and vector atomics only.  An LDS-accumulating variant of kernel 1 was not built: nothing measured asks for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/epic_hip.h"
#include "kernels.h"
#include "occupancy_points_rule.h"

namespace epic_hip {

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kMergeRounds = 4;
#if defined(EPIC_OCC_POINTS_PLAIN_ATOMICS)   // the B side of the A/B of profiles/occupancy_points.txt
constexpr bool kMerge = false;
#else
constexpr bool kMerge = true;
#endif

struct PointsGeom {
    pts::Box box;
    unsigned nwords;     // words per row of a plane
    unsigned n;          // components of a point
    unsigned n_points;
    float sensor[3];     // n components; unused without a sensor
};

__device__ inline unsigned word_of(const PointsGeom &g, const int cell[3])
{
    const unsigned row = (unsigned)(cell[0] - g.box.o[0]) * (unsigned)g.box.e[1] + (unsigned)(cell[1] - g.box.o[1]);
    return row * g.nwords + ((unsigned)(cell[2] - g.box.o[2]) >> 6);
}

__device__ inline unsigned long long bit_of(const PointsGeom &g, const int cell[3]) { return 1ull << ((unsigned)(cell[2] - g.box.o[2]) & 63u); }

// plane[word] |= bits for every lane with `pending`; the whole wave calls it (the shuffles need every lane)
__device__ inline void wave_or(unsigned long long *__restrict__ plane, unsigned word, unsigned long long bits, bool pending)
{
    if (kMerge) {
        const int lane = threadIdx.x & (kWave - 1);
#pragma unroll 1
        for (int round = 0; round < kMergeRounds; ++round) {
            const unsigned long long todo = __ballot(pending);
            if (todo == 0) break;   // wave-uniform
            const int leader = __ffsll(todo) - 1;
            const unsigned key = __shfl(word, leader);
            const bool mine = pending && word == key;
            unsigned long long acc = mine ? bits : 0ull;
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) acc |= __shfl_xor(acc, d);
            if (lane == leader) atomicOr(&plane[key], acc);
            pending = pending && !mine;
        }
    }
    if (pending) atomicOr(&plane[word], bits);
}

__device__ inline bool load_point(const float *__restrict__ points, const PointsGeom &g, unsigned i, float p[3])
{
    p[0] = p[1] = p[2] = 0.0f;
    if (i >= g.n_points) return false;
    if (g.n == 2) {   // 8-byte aligned: the driver places the points on a 16-byte boundary
        const float2 v = reinterpret_cast<const float2 *>(points)[i];
        p[0] = v.x;
        p[1] = v.y;
    } else {
        const float *at = points + (size_t)i * 3u;
        p[0] = at[0];
        p[1] = at[1];
        p[2] = at[2];
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void occupancy_points_bin_kernel(const float *__restrict__ points, unsigned long long *__restrict__ hit,
                                                                      PointsGeom g)
{
    float p[3];
    int cell[3];
    bool has[3];
    const bool live = load_point(points, g, blockIdx.x * (unsigned)kBlock + threadIdx.x, p);
    const bool fin = pts::classify(p, g.n, cell, has);
    const bool is_hit = live && fin && pts::inside(g.box, cell, has);
    wave_or(hit, is_hit ? word_of(g, cell) : 0xffffffffu, is_hit ? bit_of(g, cell) : 0ull, is_hit);
}

__global__ __launch_bounds__(kBlock) void occupancy_points_ray_kernel(const float *__restrict__ points, unsigned long long *__restrict__ clear,
                                                                      PointsGeom g)
{
    float p[3];
    int cell[3];
    bool has[3];
    const bool live = load_point(points, g, blockIdx.x * (unsigned)kBlock + threadIdx.x, p);
    const bool cast = pts::classify(p, g.n, cell, has) && live;
    (void)pts::classify(g.sensor, g.n, cell, has);   // inside the box: the driver has tested it
    const unsigned home = word_of(g, cell);
    unsigned long long home_bits = 0ull;
    if (cast) {
        pts::Ray r;
        pts::ray_setup(g.box, g.sensor, p, g.n, r);
        unsigned at = home;              // the word `acc` belongs to, once the ray has left the sensor's word
        unsigned long long acc = 0ull;
        for (unsigned k = 0; k < r.bound; ++k) {   // r.cur is inside the box here
            const unsigned w = word_of(g, r.cur);
            const unsigned long long b = bit_of(g, r.cur);
            if (w == home) {
                home_bits |= b;
            } else {
                if (w != at) {
                    if (acc != 0ull) atomicOr(&clear[at], acc);
                    at = w;
                    acc = 0ull;
                }
                acc |= b;
            }
            if (!pts::ray_step(g.box, r)) break;
        }
        if (acc != 0ull) atomicOr(&clear[at], acc);
    }
    wave_or(clear, home, home_bits, home_bits != 0ull);
}

// four plane bits to four byte masks: bit k to 0xff in byte k
__device__ inline uint32_t spread4(unsigned nibble) { return ((nibble * 0x00204081u) & 0x01010101u) * 0xffu; }

template <bool VEC>
__global__ __launch_bounds__(kBlock) void occupancy_points_expand_kernel(const unsigned long long *__restrict__ hit,
                                                                         const unsigned long long *__restrict__ clear,
                                                                         unsigned char *__restrict__ occ, int width, unsigned nwords,
                                                                         unsigned quarters, uint32_t fill, uint32_t keep)
{
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= quarters) return;
    const unsigned pair = i >> 2, q = i & 3u;
    const unsigned row = pair / nwords, word = pair - row * nwords;
    const int col = (int)(word * 64u + q * 16u);
    if (col >= width) return;
    const unsigned h = (unsigned)(hit[pair] >> (16u * q)) & 0xffffu, c = (unsigned)(clear[pair] >> (16u * q)) & 0xffffu;
    unsigned char *at = occ + (size_t)row * (size_t)width + (size_t)col;
    if (VEC) {   // width % 16 == 0: the 16 cells are inside the row, at a 16-byte aligned address
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t hm = spread4((h >> (4 * k)) & 0xfu), cm = spread4((c >> (4 * k)) & 0xfu);
            v[k] = (hm & fill) | (~hm & ~cm & keep);
        }
        *reinterpret_cast<uint4 *>(at) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 16 && col + j < width; j++)
            at[j] = (unsigned char)(((h >> j) & 1u) ? fill : (((c >> j) & 1u) ? 0u : keep));
    }
}

}  // namespace

hipError_t launch_occupancy_points(const float *d_points, unsigned n_points, unsigned n, const float *sensor, const int origin[3],
                                   const int extent[3], unsigned long long *d_hit, unsigned long long *d_clear, unsigned char *d_occ,
                                   int no_change, unsigned flags, hipStream_t stream)
{
    if (!d_hit || !d_clear || !d_occ || (n != 2 && n != 3) || (n_points > 0 && !d_points) || (reinterpret_cast<uintptr_t>(d_points) % 8) != 0)
        return hipErrorInvalidValue;
    PointsGeom g;
    for (int a = 0; a < 3; a++) {
        if (extent[a] < 1 || origin[a] < 0 || (long long)origin[a] + extent[a] > 0x7fffffffll) return hipErrorInvalidValue;
        g.box.o[a] = origin[a];
        g.box.e[a] = extent[a];
        g.sensor[a] = (sensor && a < (int)n) ? sensor[a] : 0.0f;
    }
    g.nwords = occupancy_points_nwords(extent);
    g.n = n;
    g.n_points = n_points;
    const unsigned long long words = (unsigned long long)extent[0] * (unsigned long long)extent[1] * g.nwords;
    if (words > kOccPointsMaxWords) return hipErrorInvalidValue;
    const dim3 block(kBlock), grid((unsigned)(((unsigned long long)n_points + kBlock - 1) / kBlock));
    if (n_points > 0) {
        hipLaunchKernelGGL(occupancy_points_bin_kernel, grid, block, 0, stream, d_points, d_hit, g);
        if (sensor) hipLaunchKernelGGL(occupancy_points_ray_kernel, grid, block, 0, stream, d_points, d_clear, g);
    }
    const unsigned quarters = (unsigned)words * 4u;
    const uint32_t fill = (uint32_t)(pts::obstacle_byte(no_change, flags) & 0xff) * 0x01010101u, keep = (uint32_t)(no_change & 0xff) * 0x01010101u;
    const dim3 grid3((quarters + (unsigned)kBlock - 1u) / (unsigned)kBlock);
    if (extent[2] % 16 == 0 && (reinterpret_cast<uintptr_t>(d_occ) % 16) == 0)
        hipLaunchKernelGGL(occupancy_points_expand_kernel<true>, grid3, block, 0, stream, d_hit, d_clear, d_occ, extent[2], g.nwords, quarters, fill, keep);
    else
        hipLaunchKernelGGL(occupancy_points_expand_kernel<false>, grid3, block, 0, stream, d_hit, d_clear, d_occ, extent[2], g.nwords, quarters, fill,
                           keep);
    return hipGetLastError();
}

}  // namespace epic_hip
