// field_shift_driver.hip -- host driver of the rolling-window shift on the device-resident state (include/epic_hip.h:
// epic_hip_shift_field_gpu).  Every call of the launcher of field_shift.hip lives here; not one of the driver_* units, for the reason
// occupancy_driver.hip is none (driver.h).
//
// An ordering point with the sequence of occupancy_driver.hip: the iterations counted so far are flushed (they act on the cells as
// they were; a block enqueued ahead is dropped), the work goes onto the context's stream, the call synchronises before it returns,
// every temporary is freed on every path, and the work lists are invalidated (force_all) -- unless the shift is all-zero: then
// nothing is launched and the resident state is bit for bit what it was.
//
// How "current" is handed over.  The kernel reads the current buffer of u and the lane masks and writes the whole shifted field into
// the OTHER buffer and the new masks into a second mask block allocated here (2-D: with room for the fused copy, which
// launch_fuse_masks_2d derives behind the kernel).  When the stream has run both, Ctx::cur is flipped, the mask blocks change places
// (the old one is freed), the struct's d_u / d_locked follow, and the captured launch sequences, which hold the old mask's address,
// are dropped.  On any failure nothing is handed over: the state the caller had is untouched.
// What the stale buffer needs: nothing.  The solver never reads the non-current buffer before it has written it -- a Jacobi sweep, a
// fused pass, a tile or brick launch store every cell they own into it, locked ones included (their select copies those through),
// and red-black half-sweeps never look at it; a list-driven launch skips tiles on the strength of "both buffers agree here", and
// force_all makes the next two sweeps (the next fused pass) run every tile, which re-establishes exactly that.  The padding columns
// hold the obstacle seed in both buffers already and are copied through.
#include "driver.h"
#include "field_shift_rule.h"

namespace epic_drv {

namespace {

const char *kMultiShift = "Invalid data (not available in multi-device mode: use epic_hip_shift_field_cpu and harmonic_update_model_gpu).";

int shift_field(Harmonic *harmonic, const int *shift, unsigned fill_type, unsigned long long *kept, float *kernel_ms, const char *fn)
{
    epic_hip::ShiftPlan plan;
    const bool host_ok = harmonic != nullptr && harmonic->m != nullptr && shift != nullptr &&
                         epic_hip::shift_plan(harmonic->n, harmonic->m, shift, fill_type, plan);
    Ctx *c = host_ok ? find_ctx(harmonic) : nullptr;
    if (c == nullptr || !ready(harmonic, c) || c->n != (int)harmonic->n || !same_dims(harmonic, c)) {
        report(fn, "Invalid data.");
        return EPIC_ERROR_INVALID_DATA;
    }
    if (kernel_ms) *kernel_ms = 0.0f;
    if (c->multi()) {   // slabs: shift the host arrays and upload them again
        report(fn, kMultiShift);
        return EPIC_ERROR_INVALID_DATA;
    }
    {
        const int frc = flush_pending(harmonic, c, fn);   // the iterations counted so far act on the cells as they were
        if (frc != EPIC_SUCCESS) return frc;
    }
    if (kept) *kept = plan.kept;
    if (plan.zero) return EPIC_SUCCESS;   // nothing moves: no launch, no work list invalidated

    uint32_t *fresh = nullptr;   // the second mask block
    int rc = EPIC_SUCCESS;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (kernel_ms && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) {
        (void)hipGetLastError();
        report(fn, "Failed to create the timing events.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else if (hipMalloc((void **)&fresh, c->mask_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        fresh = nullptr;
        report(fn, "Failed to allocate device-side memory for the shifted locked cells.");
        rc = EPIC_ERROR_DEVICE_MALLOC;
    } else if ((kernel_ms && hipEventRecord(ev[0], c->stream) != hipSuccess) ||
               epic_hip::launch_field_shift(c->buf[c->cur], c->buf[c->cur ^ 1], c->maskw, fresh, plan, c->pitch, c->stream) != hipSuccess ||
               (kernel_ms && hipEventRecord(ev[1], c->stream) != hipSuccess) ||
               (c->n == 2 && epic_hip::launch_fuse_masks_2d(fresh, c->rows, c->pitch, fresh + epic_hip::mask_words_2d(c->rows, c->pitch),
                                                            c->stream) != hipSuccess)) {
        (void)hipGetLastError();
        report(fn, "Failed to execute the 'shift field' kernel.");
        rc = EPIC_ERROR_KERNEL_EXECUTION;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == EPIC_SUCCESS) {
        report(fn, "Failed to synchronize the device after 'shift field' kernel.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    if (rc == EPIC_SUCCESS && kernel_ms && hipEventElapsedTime(kernel_ms, ev[0], ev[1]) != hipSuccess) {
        report(fn, "Failed to read the timing events.");
        rc = EPIC_ERROR_DEVICE_SYNCHRONIZE;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc == EPIC_SUCCESS) {   // hand over: the other buffer and the second mask block are the field now
        std::swap(fresh, c->maskw);
        c->cur ^= 1;
        drop_graphs(c);         // (captured sequences hold the old mask's address)
        harmonic->d_u = current_u(c);
        harmonic->d_locked = c->maskw;
    }
    if (fresh) (void)hipFree(fresh);
    force_all(c);   // cells and mask bits moved under the work lists (or a failure left that open)
    return rc;
}

}  // namespace

}  // namespace epic_drv

using namespace epic_drv;

extern "C" {

int epic_hip_shift_field_gpu(Harmonic *harmonic, const int *shift, unsigned int fill_type, unsigned long long *kept, float *kernel_ms)
{
    return shift_field(harmonic, shift, fill_type, kept, kernel_ms, "epic_hip_shift_field_gpu");
}

}  // extern "C"
