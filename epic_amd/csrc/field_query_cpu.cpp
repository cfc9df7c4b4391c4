// field_query_cpu.cpp -- the host twins of the field queries (include/epic_hip.h, "Field queries"): batched potential and gradient
// samples and the flow field of a region, on harmonic->u / harmonic->locked.
//
// The rule is field_query_rule.h, shared with the kernels (field_query.hip); the arithmetic is that of
// harmonic_compute_potential_2d_cpu / harmonic_compute_gradient_2d_cpu (harmonic_path_cpu.cpp) and epic_hip_compute_potential_3d_cpu
// / epic_hip_compute_gradient_3d_cpu (harmonic_path3d_cpu.cpp), so wherever those succeed with a finite result the twins return their
// bits (tests/test_field_query_cpu.py).  Two deliberate differences from the 2-D functions, both where they read outside their
// arrays: reads are clamped to the nearest cell, and a coordinate that has no 64-bit truncation is outside the grid.  Per-item
// failures are statuses, not messages: a batch of a million samples must not write a million lines.
#include <cstddef>
#include <cstdio>

#include "../../include/epic/epic_abi.h"
#include "../../include/epic_hip.h"
#include "field_query_rule.h"
#include "occupancy_rule.h"

namespace {

using epic::Harmonic;
namespace fq = epic_hip::fq;

struct HostField {
    unsigned nx, ny, nz;  // columns (last axis of m), rows, planes (1: a 2-D field)
    const float *u;
    const unsigned *lock;
    size_t cell(unsigned x, unsigned y, unsigned z) const
    {
        x = x < nx ? x : nx - 1u;
        y = y < ny ? y : ny - 1u;
        z = z < nz ? z : nz - 1u;
        return ((size_t)z * ny + y) * nx + x;
    }
    float at(unsigned x, unsigned y, unsigned z) const { return u[cell(x, y, z)]; }
    bool locked(unsigned x, unsigned y, unsigned z) const { return lock[cell(x, y, z)] == 1; }
};

bool valid(const Harmonic *h)
{
    if (!h || !h->m || !h->u || !h->locked || (h->n != 2 && h->n != 3)) return false;
    for (unsigned i = 0; i < h->n; i++)
        if (h->m[i] < 1) return false;
    return true;
}

HostField field_of(const Harmonic *h)
{
    return h->n == 3 ? HostField{h->m[2], h->m[1], h->m[0], h->u, h->locked} : HostField{h->m[1], h->m[0], 1u, h->u, h->locked};
}

int invalid(const char *fn)
{
    fprintf(stderr, "Error[%s]: %s\n", fn, "Invalid data.");
    return EPIC_ERROR_INVALID_DATA;
}

template <bool N3>
void sample_potential(const HostField &f, unsigned n_points, const float *points, float *potential, unsigned char *status)
{
    constexpr unsigned N = N3 ? 3 : 2;
    for (size_t i = 0; i < n_points; i++) {
        const float *p = points + N * i;
        const unsigned char st = fq::potential<N3>(f, p[0], p[1], N3 ? p[2] : 0.0f, potential[i]);
        if (status) status[i] = st;
    }
}

template <bool N3>
void sample_gradient(const HostField &f, unsigned n_points, const float *points, float cd, float *gradient, unsigned char *status)
{
    constexpr unsigned N = N3 ? 3 : 2;
    for (size_t i = 0; i < n_points; i++) {
        const float *p = points + N * i;
        float g[3];
        const unsigned char st = fq::gradient<N3>(f, p[0], p[1], N3 ? p[2] : 0.0f, cd, g);
        for (unsigned a = 0; a < N; a++) gradient[N * i + a] = g[a];
        if (status) status[i] = st;
    }
}

template <bool N3>
void flow_field(const HostField &f, const size_t o[3], const size_t e[3], float cd, float *gradient, unsigned char *status)
{
    constexpr unsigned N = N3 ? 3 : 2;
    size_t i = 0;
    for (size_t z = o[0]; z < o[0] + e[0]; z++)
        for (size_t y = o[1]; y < o[1] + e[1]; y++)
            for (size_t x = o[2]; x < o[2] + e[2]; x++, i++) {
                float g[3];
                const unsigned char st = fq::flow_cell<N3>(f, (unsigned)x, (unsigned)y, (unsigned)z, cd, g);
                for (unsigned a = 0; a < N; a++) gradient[N * i + a] = g[a];
                if (status) status[i] = st;
            }
}

}  // namespace

extern "C" {

int epic_hip_sample_potential_cpu(Harmonic *harmonic, unsigned int n_points, const float *points, float *potential, unsigned char *status)
{
    static const char *fn = "epic_hip_sample_potential_cpu";
    if (!valid(harmonic)) return invalid(fn);
    if (n_points == 0) return EPIC_SUCCESS;
    if (!points || !potential) return invalid(fn);
    const HostField f = field_of(harmonic);
    if (harmonic->n == 3) sample_potential<true>(f, n_points, points, potential, status);
    else sample_potential<false>(f, n_points, points, potential, status);
    return EPIC_SUCCESS;
}

int epic_hip_sample_gradient_cpu(Harmonic *harmonic, unsigned int n_points, const float *points, float cdPrecision, float *gradient,
                                 unsigned char *status)
{
    static const char *fn = "epic_hip_sample_gradient_cpu";
    if (!valid(harmonic)) return invalid(fn);
    if (n_points == 0) return EPIC_SUCCESS;
    if (!points || !gradient) return invalid(fn);
    const HostField f = field_of(harmonic);
    if (harmonic->n == 3) sample_gradient<true>(f, n_points, points, cdPrecision, gradient, status);
    else sample_gradient<false>(f, n_points, points, cdPrecision, gradient, status);
    return EPIC_SUCCESS;
}

int epic_hip_flow_field_cpu(Harmonic *harmonic, const unsigned int *origin, const unsigned int *extent, float cdPrecision, unsigned flags,
                            float *gradient, unsigned char *status)
{
    static const char *fn = "epic_hip_flow_field_cpu";
    size_t m[3], o[3], e[3];
    if (!valid(harmonic) || !gradient || flags != 0 ||   // EPIC_HIP_QUERY_DEVICE_OUT is for the device calls
        !epic_hip::occupancy_region(harmonic->n, harmonic->m, origin, extent, m, o, e))
        return invalid(fn);
    const HostField f = field_of(harmonic);
    if (harmonic->n == 3) flow_field<true>(f, o, e, cdPrecision, gradient, status);
    else flow_field<false>(f, o, e, cdPrecision, gradient, status);
    return EPIC_SUCCESS;
}

}  // extern "C"
