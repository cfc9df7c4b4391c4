// field3d_driver.hip -- host driver of the consumers and sparse edits of a device-resident 3-D field (include/epic_hip.h:
// epic_hip_compute_paths_3d_gpu, epic_hip_compute_path_3d_gpu, epic_hip_set_cells_3d_gpu).  Every call of the launchers of
// field_3d.hip lives here; like occupancy_driver.hip this is not one of the driver_* units (driver.h), which are built against a
// fake runtime that knows only their launchers.
//
// The path calls are epic_hip_compute_paths_2d_gpu / _path_2d_gpu (driver_ext.hip) step for step, the edit is
// harmonic_utilities_set_cells_2d_gpu (driver_loop.hip) step for step: the iterations counted so far are flushed first, the work
// goes onto the context's stream, every temporary is freed on every path, the same failing step gives the same code.  The 3-D
// sweeps derive nothing from the masks (the 2-D fused layout has no 3-D counterpart: driver_registry.hip, upload_locked), so an
// edit rebuilds nothing; it invalidates the work lists (force_all) so that a tracked relaxation reruns every tile.
//
// Multi-device mode: the field lives in plane slabs on several devices, and none of the three calls is available there --
// they say which host route takes their place.
#include "driver.h"

using namespace epic_drv;

namespace {

constexpr unsigned kDirectCopies = 8;   // up to this many paths, each path's way-points are copied back on their own

bool valid_host_side(const Harmonic *h) { return h != nullptr && h->m != nullptr && h->u != nullptr && h->locked != nullptr; }

}  // namespace

extern "C" {

// starts: n_paths (x, y, z) triples; k / rc: n_paths entries; paths: n_paths rows of 3 * maxLength floats (row i holds 3 * k[i]
// values).  All host pointers.
int epic_hip_compute_paths_3d_gpu(Harmonic *harmonic, unsigned int n_paths, const float *starts, float stepSize, float cdPrecision,
                                  unsigned int maxLength, unsigned int *k, int *rc_out, float *paths)
{
    static const char *fn = "epic_hip_compute_paths_3d_gpu";
    Ctx *c = harmonic ? find_ctx(harmonic) : nullptr;
    if (!harmonic || !ready(harmonic, c) || c->n != 3 || n_paths == 0 || !starts || !k || !rc_out || !paths) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (c->multi()) {  // the field lives on several devices: read it back and walk it with epic_hip_compute_path_3d_cpu
        report(fn, "Invalid data (not available in multi-device mode: use harmonic_get_potential_values_gpu and epic_hip_compute_path_3d_cpu).");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (const int frc = flush_pending(harmonic, c, fn)) return frc;   // the walk reads the field of every iteration asked for
    // the host walk stops at (2u * maxLength) / 2u points (the 2-D loop's unsigned product, harmonic_path3d_cpu.cpp)
    const unsigned max_points = (2u * maxLength) / 2u;
    const size_t row = 3 * (size_t)max_points;
    float *d_starts = nullptr, *d_pts = nullptr, *d_packed = nullptr;
    unsigned long long *d_offset = nullptr;
    unsigned *d_k = nullptr;
    int *d_rc = nullptr;
    int rc = EPIC_SUCCESS;
    if (hipMalloc((void **)&d_starts, 3 * (size_t)n_paths * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&d_pts, std::max<size_t>(row * n_paths, 1) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&d_k, (size_t)n_paths * sizeof(unsigned)) != hipSuccess ||
        hipMalloc((void **)&d_rc, (size_t)n_paths * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the paths.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else if (hipMemcpyAsync(d_starts, starts, 3 * (size_t)n_paths * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from host to device for the start points.");
        rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
    } else if (epic_hip::launch_follow_paths_3d(c->buf[c->cur], c->maskw, c->m[0], c->m[1], c->m[2], c->pitch, n_paths, d_starts, stepSize,
                                                cdPrecision, max_points, d_pts, d_k, d_rc, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'follow paths' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    } else if (hipMemcpyAsync(k, d_k, (size_t)n_paths * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
               hipMemcpyAsync(rc_out, d_rc, (size_t)n_paths * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
               hipStreamSynchronize(c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from device to host for the path lengths.");
        rc = EPIC_ERROR_MEMCPY_TO_HOST;
    } else if (n_paths <= kDirectCopies) {
        for (unsigned i = 0; i < n_paths; i++)  // only the way-points that exist come back
            if (k[i] > 0 && hipMemcpyAsync(paths + i * row, d_pts + i * row, 3 * (size_t)k[i] * sizeof(float), hipMemcpyDeviceToHost,
                                           c->stream) != hipSuccess)
                rc = EPIC_ERROR_MEMCPY_TO_HOST;
        if (hipStreamSynchronize(c->stream) != hipSuccess) rc = EPIC_ERROR_MEMCPY_TO_HOST;
        if (rc != EPIC_SUCCESS) report(fn, "Failed to copy memory from device to host for the paths.");
    } else {
        // a batch: the way-points that exist are packed on the device and come back in one copy (field_3d.hip: pack_paths_3d_kernel)
        std::vector<unsigned long long> offset(n_paths);
        unsigned long long total = 0;
        for (unsigned i = 0; i < n_paths; i++) {
            offset[i] = total;
            total += k[i];
        }
        if (total > 0) {
            std::vector<float> packed(3 * (size_t)total);
            if (hipMalloc((void **)&d_offset, (size_t)n_paths * sizeof(unsigned long long)) != hipSuccess ||
                hipMalloc((void **)&d_packed, packed.size() * sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                report(fn, "Failed to allocate device-side memory for the paths.");
                rc = EPIC_ERROR_DEVICE_MALLOC;
            } else if (hipMemcpyAsync(d_offset, offset.data(), (size_t)n_paths * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream) !=
                       hipSuccess) {
                report(fn, "Failed to copy memory from host to device for the start points.");
                rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
            } else if (epic_hip::launch_pack_paths_3d(d_pts, row, n_paths, d_k, d_offset, d_packed, c->stream) != hipSuccess) {
                report(fn, "Failed to execute the 'follow paths' kernel.");
                rc = EPIC_ERROR_KERNEL_EXECUTION;
            } else if (hipMemcpyAsync(packed.data(), d_packed, packed.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                       hipStreamSynchronize(c->stream) != hipSuccess) {
                report(fn, "Failed to copy memory from device to host for the paths.");
                rc = EPIC_ERROR_MEMCPY_TO_HOST;
            } else {
                for (unsigned i = 0; i < n_paths; i++)
                    if (k[i] > 0) memcpy(paths + i * row, packed.data() + 3 * (size_t)offset[i], 3 * (size_t)k[i] * sizeof(float));
            }
        }
    }
    if (rc != EPIC_SUCCESS) (void)hipStreamSynchronize(c->stream);
    for (void *p : {(void *)d_starts, (void *)d_pts, (void *)d_k, (void *)d_rc, (void *)d_offset, (void *)d_packed})
        if (p) (void)hipFree(p);
    return rc;
}

// epic_hip_compute_path_3d_cpu's contract on the resident field: *path must be null on entry and receives a new[] array of
// 3 * *k floats that harmonic_free_path_cpu (or delete[]) releases.
int epic_hip_compute_path_3d_gpu(Harmonic *harmonic, float x, float y, float z, float stepSize, float cdPrecision,
                                 unsigned int maxLength, unsigned int *k, float **path)
{
    static const char *fn = "epic_hip_compute_path_3d_gpu";
    if (!harmonic || !k || !path || *path != nullptr) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    const size_t row = 3 * (size_t)((2u * maxLength) / 2u);
    std::vector<float> pts(std::max<size_t>(row, 1));
    const float start[3] = {x, y, z};
    unsigned n = 0;
    int walk = EPIC_SUCCESS;
    int rc = epic_hip_compute_paths_3d_gpu(harmonic, 1, start, stepSize, cdPrecision, maxLength, &n, &walk, pts.data());
    if (rc != EPIC_SUCCESS) return rc;
    if (walk != EPIC_SUCCESS) {
        report(fn, walk == EPIC_ERROR_INVALID_LOCATION ? "Invalid location."
                   : walk == EPIC_ERROR_INVALID_GRADIENT ? "Could not compute gradient."
                                                         : "Could not compute a valid path.");
        return walk;
    }
    *k = n;
    *path = new float[3 * (size_t)n];
    std::copy(pts.begin(), pts.begin() + 3 * (size_t)n, *path);
    return EPIC_SUCCESS;
}

// v: k (x, y, z) triples, no cell twice; an ordering point that synchronises, like harmonic_utilities_set_cells_2d_gpu.
int epic_hip_set_cells_3d_gpu(Harmonic *harmonic, unsigned int k, const unsigned int *v, const unsigned int *types)
{
    static const char *fn = "epic_hip_set_cells_3d_gpu";
    if (!valid_host_side(harmonic) || harmonic->n == 0 || k == 0 || v == nullptr || types == nullptr) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    Ctx *c = find_ctx(harmonic);
    if (!ready(harmonic, c) || c->n != 3) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (c->multi()) {  // plane slabs: edit the host arrays and upload them again
        report(fn, "Invalid data (not available in multi-device mode: use epic_hip_set_cells_3d_cpu and harmonic_update_model_gpu).");
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);   // the iterations counted so far act on the cells as they were
        if (frc != EPIC_SUCCESS) return frc;
    }
    unsigned *d_v = nullptr, *d_types = nullptr;
    int rc = EPIC_SUCCESS;
    force_all(c);  // cells and mask bits change under the work lists
    if (hipMalloc((void **)&d_v, 3 * (size_t)k * sizeof(unsigned)) != hipSuccess ||
        hipMalloc((void **)&d_types, (size_t)k * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the cell locations and types.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else if (hipMemcpyAsync(d_v, v, 3 * (size_t)k * sizeof(unsigned), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
               hipMemcpyAsync(d_types, types, (size_t)k * sizeof(unsigned), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        report(fn, "Failed to copy memory from host to device for the cell locations and types.");
        rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
    } else if (epic_hip::launch_set_cells_3d(c->buf[c->cur], c->maskw, c->m[0], c->m[1], c->m[2], c->pitch, k, d_v, d_types, c->stream) !=
               hipSuccess) {
        report(fn, "Failed to execute the 'set cells' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after 'set cells' kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    if (d_v) (void)hipFree(d_v);
    if (d_types) (void)hipFree(d_types);
    return rc;
}

}  // extern "C"
