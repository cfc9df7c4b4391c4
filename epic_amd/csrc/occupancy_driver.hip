// occupancy_driver.hip -- host driver of the dense occupancy ingestion on the device-resident state (include/epic_hip.h:
// epic_hip_set_occupancy_2d_gpu, epic_hip_reset_free_cells_2d_gpu).  Every call of the launchers of occupancy_2d.hip lives here.
//
// An ordering point like harmonic_utilities_set_cells_2d_gpu (driver_loop.hip), step for step: the iterations counted so far are
// flushed (they act on the cells as they were; a block enqueued ahead is dropped), the work goes onto the context's stream into
// the current buffer, the call synchronises before it returns, every temporary is freed on every path.  The work lists are
// invalidated (force_all) as the sparse edit does -- except when EPIC_HIP_OCC_KEEP_FREE is set and the kernel reports that nothing
// changed: then the resident state is bit for bit what it was, nothing is woken, and a tracked relaxation goes on as if the call
// had not happened.
//
// Multi-device mode: the image is expanded to a list on the host and goes through multi_set_cells, the route the sparse edit
// takes on slabs.  The rule needs the cells as the devices hold them, so the field and the lock bits of the owned rows are read
// back first.  That is a whole field over the bus per message: the mode keeps its results bit-identical to one device, not the
// dense route's cost.
//
// The region forms (epic_hip_set_occupancy_region_gpu, epic_hip_timed_occupancy_region_gpu, epic_hip_reset_free_cells_3d_gpu) follow
// the same sequence on 2-D and 3-D fields with the launcher of occupancy_region.hip: only the region's bytes are copied.  The 3-D
// sweeps derive nothing from the masks, so a 3-D edit rebuilds nothing.  In multi-device mode a 2-D region takes the list route
// above, restricted to the window; a 3-D field lives in plane slabs there, for which no edit is built: the calls name the host route.
#include "driver.h"
#include "occupancy_rule.h"

namespace epic_drv {

namespace {

bool valid_host_side(const Harmonic *h) { return h != nullptr && h->m != nullptr && h->u != nullptr && h->locked != nullptr && h->n == 2; }

// the device-resident cells of a multi-device context on the host: values and lock bits of every owned row
int multi_snapshot(Harmonic *h, Ctx *c, std::vector<float> &u, std::vector<unsigned char> &locked, const char *fn)
{
    const size_t rows = (size_t)c->rows, cols = (size_t)c->cols, words_per_row = (size_t)(c->pitch / 256) * 8u;
    u.resize(rows * cols);
    locked.assign(rows * cols, 1);
    Harmonic view = *h;
    view.u = u.data();
    const int rc = multi_get_values(&view, c, fn);   // (synchronises every slab)
    if (rc != EPIC_SUCCESS) return rc;
    DeviceGuard g;
    std::vector<uint32_t> words;
    for (auto &sl : c->slabs) {
        const size_t owned = (size_t)(sl.hi - sl.lo);
        words.resize(owned * words_per_row);
        if (hipSetDevice(sl.dev) != hipSuccess ||
            hipMemcpy(words.data(), sl.maskw + (size_t)sl.first() * words_per_row, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            report(fn, "Failed to copy memory from device to host for the locked cells.");
            return EPIC_ERROR_MEMCPY_TO_HOST;
        }
        for (size_t r = 0; r < owned; r++)
            for (size_t x = 0; x < cols; x++)
                locked[((size_t)sl.lo + r) * cols + x] =
                    (words[epic_hip::mask_word_2d((unsigned)r, (unsigned)x, (unsigned)c->pitch)] >> epic_hip::mask_bit_2d((unsigned)x)) & 1u;
    }
    return EPIC_SUCCESS;
}

// occ == nullptr: reset_free_cells.  win (may be null: the grid): {y0, x0, height, width} of the window `occ` holds, unpitched.
int multi_dense_edit(Harmonic *h, Ctx *c, const unsigned char *occ, int obstacle_threshold, int no_change, unsigned flags,
                     unsigned long long *changed, const char *fn, const size_t *win = nullptr)
{
    std::vector<float> u;
    std::vector<unsigned char> locked;
    const int src = multi_snapshot(h, c, u, locked, fn);
    if (src != EPIC_SUCCESS) return src;
    std::vector<unsigned> v, types;
    unsigned long long count = 0;
    const size_t cols = (size_t)c->cols;
    const size_t y0 = win ? win[0] : 0, x0 = win ? win[1] : 0, height = win ? win[2] : (size_t)c->rows, width = win ? win[3] : cols;
    for (size_t y = std::max<size_t>(y0, 1); y < y0 + height && y + 1 < (size_t)c->rows; y++)
        for (size_t x = std::max<size_t>(x0, 1); x < x0 + width && x + 1 < cols; x++) {
            const size_t cell = y * cols + x;
            const bool was_locked = locked[cell] != 0;
            epic_hip::OccCell after = {u[cell], was_locked, false};
            if (occ) after = epic_hip::occupancy_cell(occ[(y - y0) * width + (x - x0)], u[cell], was_locked, obstacle_threshold, no_change, flags);
            else if (!was_locked) after.u = (float)EPIC_LOG_SPACE_FREE;
            count += epic_hip::occupancy_changed(u[cell], was_locked, after);
            if (after.locked == was_locked && epic_hip::occupancy_float_bits(after.u) == epic_hip::occupancy_float_bits(u[cell])) continue;
            v.push_back((unsigned)x);
            v.push_back((unsigned)y);
            types.push_back(after.locked ? EPIC_CELL_TYPE_OBSTACLE : EPIC_CELL_TYPE_FREE);
        }
    if (changed) *changed = count;
    if (types.empty()) {
        if (!(occ && (flags & EPIC_HIP_OCC_KEEP_FREE) && count == 0)) force_all(c);
        return EPIC_SUCCESS;
    }
    if (types.size() > 0xffffffffull) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    force_all(c);
    return multi_set_cells(c, (unsigned)types.size(), v.data(), types.data(), fn);
}

// The sequence both dense calls share, behind the ordering point: one temporary -- the counters of `changed` (kernels.h: kOccCounters
// words in lines of their own) and behind them the `bytes` bytes of the image or the region, copied as they are (staging an image with
// rows padded to the field's pitch was measured and gained nothing: profiles/occupancy_ingest.txt) --, launch(d_occ, d_changed), in 2-D
// the fused masks, the counters back, synchronise, free, and force_all unless KEEP_FREE is set and nothing changed.
// kernel_ms (may be null): the device time of the ingestion kernel alone, between two events on the context's stream
template <class Launch>
int staged_edit(Ctx *c, const void *occ, size_t bytes, unsigned flags, unsigned long long *changed, float *kernel_ms, const char *fn, Launch launch)
{
    const size_t slot = epic_hip::kOccCounterBytes;
    unsigned char *tmp = nullptr;
    unsigned long long count = 0;
    std::vector<unsigned long long> counters(epic_hip::kOccCounterBytes / sizeof(unsigned long long), 0);
    bool untouched = false;   // the kernel ran to its end and reported that nothing changed
    int rc = EPIC_SUCCESS;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (kernel_ms && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) {
        (void)hipGetLastError();
        report(fn, "Failed to create the timing events.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else if (hipMalloc((void **)&tmp, slot + bytes) != hipSuccess) {
        (void)hipGetLastError();
        report(fn, "Failed to allocate device-side memory for the occupancy image.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else {
        unsigned long long *d_changed = reinterpret_cast<unsigned long long *>(tmp);
        unsigned char *d_occ = tmp + slot;
        if (hipMemsetAsync(d_changed, 0, slot, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_occ, occ, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            report(fn, "Failed to copy memory from host to device for the occupancy image.");
            rc = EPIC_ERROR_MEMCPY_TO_DEVICE;
        } else if ((kernel_ms && hipEventRecord(ev[0], c->stream) != hipSuccess) ||
                   launch(d_occ, d_changed) != hipSuccess ||
                   (kernel_ms && hipEventRecord(ev[1], c->stream) != hipSuccess) ||
                   (c->n == 2 && epic_hip::launch_fuse_masks_2d(c->maskw, c->rows, c->pitch, c->maskf(), c->stream) != hipSuccess)) {
            report(fn, "Failed to execute the 'set occupancy' kernel.");
            rc = EPIC_ERROR_KERNEL_EXECUTION;
        } else if (hipMemcpyAsync(counters.data(), d_changed, slot, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
            report(fn, "Failed to copy memory from device to host for the number of changed cells.");
            rc = EPIC_ERROR_MEMCPY_TO_HOST;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after 'set occupancy' kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    if (rc == EPIC_SUCCESS && kernel_ms && hipEventElapsedTime(kernel_ms, ev[0], ev[1]) != hipSuccess) {
        report(fn, "Failed to read the timing events.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (tmp) (void)hipFree(tmp);
    if (rc == EPIC_SUCCESS) {
        for (int i = 0; i < epic_hip::kOccCounters; i++) count += counters[(size_t)i * epic_hip::kOccCounterStride];
        untouched = (flags & EPIC_HIP_OCC_KEEP_FREE) && count == 0;
        if (changed) *changed = count;
    }
    if (!untouched) force_all(c);   // cells and mask bits changed under the work lists (or a failure left that open)
    return rc;
}

int set_occupancy(Harmonic *harmonic, const void *occ, int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed,
                  float *kernel_ms, const char *fn)
{
    Ctx *c = valid_host_side(harmonic) && occ != nullptr ? find_ctx(harmonic) : nullptr;
    if (c == nullptr || !ready(harmonic, c) || c->n != 2) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);   // the iterations counted so far act on the cells as they were
        if (frc != EPIC_SUCCESS) return frc;
    }
    if (kernel_ms) *kernel_ms = 0.0f;
    if (c->multi()) return multi_dense_edit(harmonic, c, static_cast<const unsigned char *>(occ), obstacle_threshold, no_change, flags, changed, fn);

    const size_t cols = (size_t)c->cols;
    return staged_edit(c, occ, (size_t)c->rows * cols, flags, changed, kernel_ms, fn, [&](const unsigned char *d_occ, unsigned long long *d_changed) {
        return epic_hip::launch_occupancy_2d(c->buf[c->cur], c->maskw, d_occ, cols, c->rows, c->cols, c->pitch, obstacle_threshold, no_change, flags,
                                             d_changed, c->stream);
    });
}

const char *kMulti3dRegion = "Invalid data (not available in multi-device mode: use epic_hip_set_occupancy_region_cpu and harmonic_update_model_gpu).";
const char *kMulti3dReset = "Invalid data (not available in multi-device mode: use epic_hip_reset_free_cells_3d_cpu and harmonic_update_model_gpu).";

// The region form, n in {2, 3}: set_occupancy's ordering point and staged_edit, with only the region's bytes over the bus and only
// the region's rows and strips under the kernel (occupancy_region.hip).
int set_occupancy_region(Harmonic *harmonic, const void *occ, const unsigned *origin, const unsigned *extent, int obstacle_threshold,
                         int no_change, unsigned flags, unsigned long long *changed, float *kernel_ms, const char *fn)
{
    size_t m[3], o[3], e[3];
    const bool host_ok = harmonic != nullptr && harmonic->m != nullptr && harmonic->u != nullptr && harmonic->locked != nullptr &&
                         occ != nullptr && epic_hip::occupancy_region(harmonic->n, harmonic->m, origin, extent, m, o, e);
    Ctx *c = host_ok ? find_ctx(harmonic) : nullptr;
    if (c == nullptr || !ready(harmonic, c) || c->n != (int)harmonic->n || !same_dims(harmonic, c)) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (c->n == 3 && c->multi()) {  // plane slabs: edit the host arrays and upload them again
        report(fn, kMulti3dRegion);
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);   // the iterations counted so far act on the cells as they were
        if (frc != EPIC_SUCCESS) return frc;
    }
    if (kernel_ms) *kernel_ms = 0.0f;
    if (c->multi()) {
        const size_t win[4] = {o[1], o[2], e[1], e[2]};
        return multi_dense_edit(harmonic, c, static_cast<const unsigned char *>(occ), obstacle_threshold, no_change, flags, changed, fn, win);
    }

    epic_hip::OccRegion region;
    region.m0 = (int)m[0];
    region.m1 = (int)m[1];
    region.cols = (int)m[2];
    for (int a = 0; a < 3; a++) {
        region.origin[a] = (int)o[a];
        region.extent[a] = (int)e[a];
    }
    region.faces0 = c->n == 3;
    return staged_edit(c, occ, e[0] * e[1] * e[2], flags, changed, kernel_ms, fn, [&](const unsigned char *d_occ, unsigned long long *d_changed) {
        return epic_hip::launch_occupancy_region(c->buf[c->cur], c->maskw, d_occ, region, c->pitch, obstacle_threshold, no_change, flags, d_changed,
                                                 c->stream);
    });
}

}  // namespace

}  // namespace epic_drv

using namespace epic_drv;

extern "C" {

int epic_hip_set_occupancy_2d_gpu(Harmonic *harmonic, const void *occ, int obstacle_threshold, int no_change, unsigned flags,
                                  unsigned long long *changed)
{
    return set_occupancy(harmonic, occ, obstacle_threshold, no_change, flags, changed, nullptr, "epic_hip_set_occupancy_2d_gpu");
}

int epic_hip_timed_occupancy_2d_gpu(Harmonic *harmonic, const void *occ, int obstacle_threshold, int no_change, unsigned flags,
                                    unsigned long long *changed, float *kernel_ms)
{
    static const char *fn = "epic_hip_timed_occupancy_2d_gpu";
    if (kernel_ms == nullptr) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    return set_occupancy(harmonic, occ, obstacle_threshold, no_change, flags, changed, kernel_ms, fn);
}

int epic_hip_reset_free_cells_2d_gpu(Harmonic *harmonic)
{
    static const char *fn = "epic_hip_reset_free_cells_2d_gpu";
    Ctx *c = valid_host_side(harmonic) ? find_ctx(harmonic) : nullptr;
    if (c == nullptr || !ready(harmonic, c) || c->n != 2) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);
        if (frc != EPIC_SUCCESS) return frc;
    }
    if (c->multi()) return multi_dense_edit(harmonic, c, nullptr, 0, 0, 0, nullptr, fn);
    int rc = EPIC_SUCCESS;
    force_all(c);   // values change under the work lists
    if (epic_hip::launch_reset_free_cells_2d(c->buf[c->cur], c->maskw, c->rows, c->cols, c->pitch, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'reset free cells' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after 'reset free cells' kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    return rc;
}

int epic_hip_set_occupancy_region_gpu(Harmonic *harmonic, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                      int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed)
{
    return set_occupancy_region(harmonic, occ, origin, extent, obstacle_threshold, no_change, flags, changed, nullptr,
                                "epic_hip_set_occupancy_region_gpu");
}

int epic_hip_timed_occupancy_region_gpu(Harmonic *harmonic, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                        int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed, float *kernel_ms)
{
    static const char *fn = "epic_hip_timed_occupancy_region_gpu";
    if (kernel_ms == nullptr) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    return set_occupancy_region(harmonic, occ, origin, extent, obstacle_threshold, no_change, flags, changed, kernel_ms, fn);
}

// unlocked cells are interior cells (the faces and the padding are locked in the masks), and the 3-D masks are the 2-D lane masks
// over m0 * m1 rows: the 2-D kernel does the work
int epic_hip_reset_free_cells_3d_gpu(Harmonic *harmonic)
{
    static const char *fn = "epic_hip_reset_free_cells_3d_gpu";
    const bool host_ok = harmonic != nullptr && harmonic->m != nullptr && harmonic->u != nullptr && harmonic->locked != nullptr && harmonic->n == 3;
    Ctx *c = host_ok ? find_ctx(harmonic) : nullptr;
    if (c == nullptr || !ready(harmonic, c) || c->n != 3) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (c->multi()) {
        report(fn, kMulti3dReset);
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);
        if (frc != EPIC_SUCCESS) return frc;
    }
    int rc = EPIC_SUCCESS;
    force_all(c);   // values change under the work lists
    if (epic_hip::launch_reset_free_cells_2d(c->buf[c->cur], c->maskw, c->rows, c->cols, c->pitch, c->stream) != hipSuccess) {
        report(fn, "Failed to execute the 'reset free cells' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after 'reset free cells' kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    return rc;
}

}  // extern "C"
