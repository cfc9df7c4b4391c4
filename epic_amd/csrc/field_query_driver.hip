// field_query_driver.hip -- host driver of the queries of a device-resident field (include/epic_hip.h, "Field queries":
// epic_hip_sample_potential_gpu, epic_hip_sample_gradient_gpu, epic_hip_flow_field_gpu, epic_hip_get_cells_gpu,
// epic_hip_get_region_gpu).  Every call of the launchers of field_query.hip lives here; like occupancy_driver.hip and
// field3d_driver.hip this is not one of the driver_* units (driver.h), which are built against a fake runtime that knows only their
// launchers.
//
// Every call is an ordering point like the device walk (epic_hip_compute_paths_2d_gpu, driver_ext.hip): the iterations counted so far
// are flushed, the kernel reads c->buf[c->cur] on the context's stream, the call synchronises before it returns, every temporary is
// freed on every path.  Unlike the edits NOTHING is written to the field or the masks: no work list is invalidated, and a tracked
// relaxation goes on after a query as if it had not happened (tests/test_gpu_field_query_states.py).
//
// Multi-device mode: the field lives in slabs on several devices.  All five calls take the route the dense edits take there
// (occupancy_driver.hip): the owned units of every slab -- values and lock bits -- are read back, and the host twin
// (field_query_cpu.cpp), or a slice of the snapshot, answers.  Bit-identical to one device by construction; per-slab kernels are not
// built.
#include "driver.h"
#include "occupancy_rule.h"

using namespace epic_drv;

namespace {

// Two-output read-backs up to this size come back in ONE copy and are split on the host.  Not measured, reasoned: a copy of its own costs
// about 10 us whatever its size (profiles/paths_3d.txt), a pass over the bytes on the host about 0.1 us per KB -- they meet near 100 KB,
// and at hundreds of MB (a whole grid) the staging buffer and the pass would cost more than the copies do.
constexpr size_t kStagedCopyBytes = (size_t)1 << 20;

int invalid(const char *fn)
{
    report(fn, "Invalid data.");
    return EPIC_ERROR_INVALID_DATA;
}

// the context of a Harmonic whose n is 2 or 3 and whose device state is resident with the same dimensions; null otherwise
Ctx *context_of(Harmonic *h)
{
    if (!h || !h->m || (h->n != 2 && h->n != 3)) return nullptr;
    Ctx *c = find_ctx(h);
    return (c && ready(h, c) && c->n == (int)h->n && same_dims(h, c)) ? c : nullptr;
}

epic_hip::QueryField field_of(const Ctx *c)
{
    return c->n == 3 ? epic_hip::QueryField{c->buf[c->cur], c->maskw, 3, c->m[0], c->m[1], c->m[2], c->pitch}
                     : epic_hip::QueryField{c->buf[c->cur], c->maskw, 2, 1, c->m[0], c->m[1], c->pitch};
}

// The cells of a multi-device context as the devices hold them: values and lock flags (0 / 1) of every owned unit, behind a Harmonic
// that the host twins take.
struct Snapshot {
    std::vector<float> u;
    std::vector<unsigned> locked;
    Harmonic view;
};

int take_snapshot(Harmonic *h, Ctx *c, Snapshot &s, const char *fn)
{
    const size_t rows = (size_t)c->rows, cols = (size_t)c->cols, words_per_row = (size_t)(c->pitch / 256) * 8u, ur = unit_rows(c);
    s.u.resize(rows * cols);
    s.locked.assign(rows * cols, 1u);
    s.view = *h;
    s.view.u = s.u.data();
    s.view.locked = s.locked.data();
    const int rc = multi_get_values(&s.view, c, fn);   // (synchronises every slab)
    if (rc != EPIC_SUCCESS) return rc;
    DeviceGuard g;
    std::vector<uint32_t> words;
    for (auto &sl : c->slabs) {
        const size_t owned = (size_t)(sl.hi - sl.lo) * ur;   // rows
        words.resize(owned * words_per_row);
        if (hipSetDevice(sl.dev) != hipSuccess ||
            hipMemcpy(words.data(), sl.maskw + (size_t)sl.first() * ur * words_per_row, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) !=
                hipSuccess) {
            (void)hipGetLastError();
            report(fn, "Failed to copy memory from device to host for the locked cells.");
            return EPIC_ERROR_MEMCPY_TO_HOST;
        }
        for (size_t r = 0; r < owned; r++)
            for (size_t x = 0; x < cols; x++)
                s.locked[((size_t)sl.lo * ur + r) * cols + x] =
                    (words[epic_hip::mask_word_2d((unsigned)r, (unsigned)x, (unsigned)c->pitch)] >> epic_hip::mask_bit_2d((unsigned)x)) & 1u;
    }
    return EPIC_SUCCESS;
}

// synchronise, free, and turn a late failure into a code: the tail every call shares
int finish(Ctx *c, void *tmp, int rc, const char *fn)
{
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after the query kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    if (tmp) (void)hipFree(tmp);
    return rc;
}

int sample_points(Harmonic *harmonic, unsigned n_points, const float *points, bool gradient, float cd, float *out, unsigned char *status,
                  const char *fn)
{
    Ctx *c = context_of(harmonic);
    if (!c) return invalid(fn);
    if (n_points == 0) return EPIC_SUCCESS;
    if (!points || !out) return invalid(fn);
    if (const int frc = flush_pending(harmonic, c, fn)) return frc;   // the query reads the field of every iteration asked for
    if (c->multi()) {
        Snapshot s;
        if (const int src = take_snapshot(harmonic, c, s, fn)) return src;
        return gradient ? epic_hip_sample_gradient_cpu(&s.view, n_points, points, cd, out, status)
                        : epic_hip_sample_potential_cpu(&s.view, n_points, points, out, status);
    }
    const size_t in_bytes = (size_t)c->n * n_points * sizeof(float), out_bytes = (gradient ? (size_t)c->n : 1u) * n_points * sizeof(float);
    unsigned char *tmp = nullptr;   // the points, the results, the statuses
    int rc = EPIC_SUCCESS;
    if (hipMalloc((void **)&tmp, in_bytes + out_bytes + n_points) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the points.");
        return EPIC_ERROR_DEVICE_MALLOC;
    }
    float *d_points = reinterpret_cast<float *>(tmp), *d_out = reinterpret_cast<float *>(tmp + in_bytes);
    unsigned char *d_status = status ? tmp + in_bytes + out_bytes : nullptr;
    if (hipMemcpyAsync(d_points, points, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from host to device for the points.");
        rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
    } else if (epic_hip::launch_sample_points(field_of(c), n_points, d_points, gradient, cd, d_out, d_status, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'sample points' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    } else if (hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
               (status && hipMemcpyAsync(status, d_status, n_points, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) {
        report(fn, "Failed to copy memory from device to host for the samples.");
        rc = EPIC_ERROR_MEMCPY_TO_HOST;
    }
    return finish(c, tmp, rc, fn);
}

}  // namespace

extern "C" {

int epic_hip_sample_potential_gpu(Harmonic *harmonic, unsigned int n_points, const float *points, float *potential, unsigned char *status)
{
    return sample_points(harmonic, n_points, points, false, 0.0f, potential, status, "epic_hip_sample_potential_gpu");
}

int epic_hip_sample_gradient_gpu(Harmonic *harmonic, unsigned int n_points, const float *points, float cdPrecision, float *gradient,
                                 unsigned char *status)
{
    return sample_points(harmonic, n_points, points, true, cdPrecision, gradient, status, "epic_hip_sample_gradient_gpu");
}

int epic_hip_flow_field_gpu(Harmonic *harmonic, const unsigned int *origin, const unsigned int *extent, float cdPrecision, unsigned flags,
                            float *gradient, unsigned char *status)
{
    static const char *fn = "epic_hip_flow_field_gpu";
    Ctx *c = context_of(harmonic);
    size_t m[3], o[3], e[3];
    if (!c || !gradient || (flags & ~EPIC_HIP_QUERY_DEVICE_OUT) || !epic_hip::occupancy_region(harmonic->n, harmonic->m, origin, extent, m, o, e))
        return invalid(fn);
    const bool device_out = (flags & EPIC_HIP_QUERY_DEVICE_OUT) != 0;
    if (device_out && c->multi()) {
        report(fn, "Invalid data (EPIC_HIP_QUERY_DEVICE_OUT is not available in multi-device mode).");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (const int frc = flush_pending(harmonic, c, fn)) return frc;
    if (c->multi()) {
        Snapshot s;
        if (const int src = take_snapshot(harmonic, c, s, fn)) return src;
        return epic_hip_flow_field_cpu(&s.view, origin, extent, cdPrecision, 0, gradient, status);
    }
    const unsigned bo[3] = {(unsigned)o[0], (unsigned)o[1], (unsigned)o[2]}, be[3] = {(unsigned)e[0], (unsigned)e[1], (unsigned)e[2]};
    const size_t cells = e[0] * e[1] * e[2], grad_bytes = cells * (size_t)c->n * sizeof(float);
    unsigned char *tmp = nullptr;
    int rc = EPIC_SUCCESS;
    if (device_out) {   // the kernel writes straight into the caller's device memory
        if (epic_hip::launch_flow_field(field_of(c), bo, be, cdPrecision, gradient, status, c->stream) != hipSuccess) {
            report(fn, "Failed to execute the 'flow field' kernel.");
            rc = EPIC_ERROR_KERNEL_EXECUTION;
        }
        return finish(c, nullptr, rc, fn);
    }
    if (hipMalloc((void **)&tmp, grad_bytes + cells) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the flow field.");
        return EPIC_ERROR_DEVICE_MALLOC;
    }
    float *d_gradient = reinterpret_cast<float *>(tmp);
    unsigned char *d_status = status ? tmp + grad_bytes : nullptr;
    if (epic_hip::launch_flow_field(field_of(c), bo, be, cdPrecision, d_gradient, d_status, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'flow field' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    } else if (hipMemcpyAsync(gradient, d_gradient, grad_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
               (status && hipMemcpyAsync(status, d_status, cells, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) {
        report(fn, "Failed to copy memory from device to host for the flow field.");
        rc = EPIC_ERROR_MEMCPY_TO_HOST;
    }
    return finish(c, tmp, rc, fn);
}

int epic_hip_get_cells_gpu(Harmonic *harmonic, unsigned int k, const unsigned int *v, float *u_out, unsigned int *locked_out)
{
    static const char *fn = "epic_hip_get_cells_gpu";
    Ctx *c = context_of(harmonic);
    if (!c) return invalid(fn);
    if (k == 0) return EPIC_SUCCESS;
    if (!v || !u_out || !locked_out) return invalid(fn);
    const size_t n = (size_t)c->n;
    const unsigned nx = (unsigned)c->m[n - 1], ny = (unsigned)c->m[n - 2], nz = n == 3 ? (unsigned)c->m[0] : 1u;
    for (size_t i = 0; i < k; i++)   // the list is checked on the host first: one bad entry and nothing is touched
        if (v[n * i] >= nx || v[n * i + 1] >= ny || (n == 3 && v[n * i + 2] >= nz)) {
            report(fn, "Invalid location.");
            return EPIC_ERROR_INVALID_LOCATION;
        }
    if (const int frc = flush_pending(harmonic, c, fn)) return frc;
    if (c->multi()) {
        Snapshot s;
        if (const int src = take_snapshot(harmonic, c, s, fn)) return src;
        for (size_t i = 0; i < k; i++) {
            const size_t cell = ((n == 3 ? (size_t)v[n * i + 2] : 0u) * ny + v[n * i + 1]) * nx + v[n * i];
            u_out[i] = s.u[cell];
            locked_out[i] = s.locked[cell];
        }
        return EPIC_SUCCESS;
    }
    const size_t v_bytes = n * k * sizeof(unsigned), out_bytes = 2 * (size_t)k * sizeof(uint32_t);
    unsigned char *tmp = nullptr;   // the list; behind it k values and k flags, which come back in one copy
    std::vector<uint32_t> back(2 * (size_t)k);
    int rc = EPIC_SUCCESS;
    if (hipMalloc((void **)&tmp, v_bytes + out_bytes) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the cell locations.");
        return EPIC_ERROR_DEVICE_MALLOC;
    }
    unsigned *d_v = reinterpret_cast<unsigned *>(tmp);
    float *d_u = reinterpret_cast<float *>(tmp + v_bytes);
    unsigned *d_locked = reinterpret_cast<unsigned *>(tmp + v_bytes) + k;
    if (hipMemcpyAsync(d_v, v, v_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from host to device for the cell locations.");
        rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
    } else if (epic_hip::launch_gather_cells(field_of(c), k, d_v, d_u, d_locked, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'gather cells' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    } else if (hipMemcpyAsync(back.data(), d_u, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from device to host for the cells.");
        rc = EPIC_ERROR_MEMCPY_TO_HOST;
    }
    rc = finish(c, tmp, rc, fn);
    if (rc == EPIC_SUCCESS) {
        memcpy(u_out, back.data(), (size_t)k * sizeof(float));
        memcpy(locked_out, back.data() + k, (size_t)k * sizeof(unsigned));
    }
    return rc;
}

int epic_hip_get_region_gpu(Harmonic *harmonic, const unsigned int *origin, const unsigned int *extent, unsigned flags, float *u_out,
                            unsigned int *locked_out)
{
    static const char *fn = "epic_hip_get_region_gpu";
    Ctx *c = context_of(harmonic);
    size_t m[3], o[3], e[3];
    if (!c || (!u_out && !locked_out) || (flags & ~EPIC_HIP_QUERY_DEVICE_OUT) ||
        !epic_hip::occupancy_region(harmonic->n, harmonic->m, origin, extent, m, o, e))
        return invalid(fn);
    const bool device_out = (flags & EPIC_HIP_QUERY_DEVICE_OUT) != 0;
    if (device_out && c->multi()) {
        report(fn, "Invalid data (EPIC_HIP_QUERY_DEVICE_OUT is not available in multi-device mode).");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (const int frc = flush_pending(harmonic, c, fn)) return frc;
    const size_t cells = e[0] * e[1] * e[2];
    if (c->multi()) {
        Snapshot s;
        if (const int src = take_snapshot(harmonic, c, s, fn)) return src;
        size_t i = 0;
        for (size_t z = o[0]; z < o[0] + e[0]; z++)
            for (size_t y = o[1]; y < o[1] + e[1]; y++)
                for (size_t x = o[2]; x < o[2] + e[2]; x++, i++) {
                    const size_t cell = (z * m[1] + y) * m[2] + x;
                    if (u_out) u_out[i] = s.u[cell];
                    if (locked_out) locked_out[i] = s.locked[cell];
                }
        return EPIC_SUCCESS;
    }
    const unsigned bo[3] = {(unsigned)o[0], (unsigned)o[1], (unsigned)o[2]}, be[3] = {(unsigned)e[0], (unsigned)e[1], (unsigned)e[2]};
    int rc = EPIC_SUCCESS;
    if (device_out) {
        if (epic_hip::launch_gather_region(field_of(c), bo, be, u_out, locked_out, c->stream) != hipSuccess) {
            report(fn, "Failed to execute the 'gather region' kernel.");
            rc = EPIC_ERROR_KERNEL_EXECUTION;
        }
        return finish(c, nullptr, rc, fn);
    }
    const size_t part = cells * sizeof(uint32_t), bytes = part * ((u_out ? 1u : 0u) + (locked_out ? 1u : 0u));
    unsigned char *tmp = nullptr;   // the values and behind them the flags, whichever are asked for
    if (hipMalloc((void **)&tmp, bytes) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the region.");
        return EPIC_ERROR_DEVICE_MALLOC;
    }
    float *d_u = u_out ? reinterpret_cast<float *>(tmp) : nullptr;
    unsigned *d_locked = locked_out ? reinterpret_cast<unsigned *>(tmp + (u_out ? part : 0)) : nullptr;
    // one copy: a single output goes straight to the caller; two come back together and are split here -- up to kStagedCopyBytes,
    // beyond which a second pass over the bytes on the host costs more than a second copy's latency
    const bool staged = u_out && locked_out && bytes <= kStagedCopyBytes;
    std::vector<unsigned char> back(staged ? bytes : 0);
    if (epic_hip::launch_gather_region(field_of(c), bo, be, d_u, d_locked, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'gather region' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    } else if (staged ? hipMemcpyAsync(back.data(), tmp, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess
                      : ((u_out && hipMemcpyAsync(u_out, d_u, part, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
                         (locked_out && hipMemcpyAsync(locked_out, d_locked, part, hipMemcpyDeviceToHost, c->stream) != hipSuccess))) {
        report(fn, "Failed to copy memory from device to host for the region.");
        rc = EPIC_ERROR_MEMCPY_TO_HOST;
    }
    rc = finish(c, tmp, rc, fn);
    if (rc == EPIC_SUCCESS && staged) {
        memcpy(u_out, back.data(), part);
        memcpy(locked_out, back.data() + part, part);
    }
    return rc;
}

}  // extern "C"
