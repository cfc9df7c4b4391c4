// batch2d_driver.hip -- host driver of the batched relaxation (include/epic_hip.h: epic_hip_execute_batch_gpu,
// epic_hip_complete_batch_gpu, epic_hip_batch_plan): SEVERAL fields of one grid shape per launch, 2-D maps on shared LDS tiles
// (kernels_tile2d_batch.hip) and -- the file has kept its name -- 3-D voxel fields on LDS bricks (kernels_brick3d_batch.hip).  Every
// call of those two launchers lives here; like occupancy_driver.hip this is not one of the driver_* units (driver.h), which are built
// against a fake runtime that knows only their launchers, and none of them calls into this one.
//
// What a batch call does with a field is what harmonic_execute_gpu does with it alone -- the same start (pending iterations flushed,
// currentIteration = 0, harmonic_initialize_gpu), the same iterations in the same order with the same arithmetic, the reference's exit
// rule (a converged check with currentIteration >= max(m)), the same end (harmonic_get_potential_values_gpu, harmonic_uninitialize_gpu)
// -- so u, currentIteration, delta and the released device state are the single call's bit for bit.  Only WHERE the iterations run
// differs: the fields that share a shape, a checking period and a mode (arithmetic, scheme, EPIC_HIP_JACOBI_CHECKS) on a grid the
// single-field tile path -- 3-D: the single-field brick path, default mode only -- takes advance together, one launch for all of them;
// every other field goes through harmonic_execute_gpu inside the same call.  A field whose check changes its mode (the tol mode's
// finishing phase, the Jacobi hand-over: driver_loop.hip) leaves its group AT THAT CHECK, in the state its single call has there, and
// goes on alone through harmonic_execute_gpu's own loop (relax_to_end).
#include "driver.h"

using namespace epic_drv;
using namespace epic;

namespace {

struct Member {
    Harmonic *h;
    Ctx *c;
    unsigned index;   // in the caller's array
    std::shared_ptr<Relaxation> rx;   // from the start of its relaxation (run_group) until it has left the group and ended
};
struct BatchPlan { epic_hip::TilePlan tp; int fields; };   // fields per workgroup; 0: no plan
struct BrickBatchPlan { epic_hip::BrickPlan bp; int capacity; };   // 3-D: the bricks and the LDS capacity (rows) of the instantiation; 0: no plan
constexpr long long kBrickDeltaCap = 4096;   // bricks of a launch (their maxima are read per field after every block)

// Fields one workgroup holds of a tile of this mode and width: the library's default mode is kernels_tile2d_batch.hip, every other
// arithmetic and scheme kernels_tile2d_batch_modes.hip; 0: no instantiation.
bool default_mode(const Ctx *c) { return c->math == 0 && c->redblack; }
int mode_max_fields(int math, bool redblack, int width)
{
    return math == 0 && redblack ? epic_hip::tile_2d_batch_max_fields(width) : epic_hip::tile_2d_batch_modes_max_fields(math, redblack, width);
}

// A field the batched kernel can take: everything harmonic_execute_gpu validates holds, and the context is in a mode that has a
// batched instantiation, on a grid the single-field tile path would take with its per-tile checks -- or, 3-D, in the library's default
// mode on a grid the single-field path would put on bricks (which leaves out tracked contexts and grids above brick_up_to_cells).
bool batchable(Harmonic *h, Ctx *c)
{
    if (!h || !h->m || !h->u || !h->locked || !(h->epsilon > 0.0f) || !h->d_m || !h->d_u || !h->d_locked || h->d_delta ||
        h->numIterationsToStaggerCheck == 0)
        return false;
    if (!ready(h, c) || (c->n != 2 && c->n != 3) || c->multi() || !c->devices.empty() || !c->cfg.batch || !c->cfg.tile_pipeline) return false;
    if (c->n == 3) return default_mode(c) && brick_plan(c).halo > 0;
    if (mode_max_fields(c->math, c->redblack, epic_hip::kTile2dCols) == 0) return false;
    return tile_checks(c, tile_plan(c));
}

// From how many fields of `cells` cells each the batched kernel is taken (fewer: the per-field loop); a lone field is never
// batched -- harmonic_execute_gpu's pipelined blocks are the better route for it.  Read from profiles/batch_2d.txt (batch / loop of
// harmonic_complete_gpu in one process, three alternating repetitions; the rows "F=1 ... 2" are the plan two fields get): two fields
// win about 1.4 x on basic.png (0.07 Mcell) and on maze.png (0.23 Mcell) and LOSE on umass.png (0.29 Mcell, about 0.9 x); from four
// fields every map wins, 1.4 x and more.  Between 0.23 and 0.29 Mcell nothing was measured: the bound sits under umass.
// The other modes, from profiles/batch_2d_modes.txt (the same tool and rule, the batch forced against a loop of harmonic_complete_gpu in
// the same mode, epsilon 1e-3: on only where a row beats the loop by more than its spread).  Two fields: maze.png wins in every mode
// (1.19-1.24 x), basic.png's 1.11-1.33 x lie inside spreads of 18-20 %, umass.png LOSES (0.95, 0.94, 0.78 x): not taken.  Four fields:
//   tol red-black    1.21 / 1.31 / 1.14 x on basic / maze / umass (spread <= 1.3 %), 1.15-1.53 x at 16 and 64
//   tol Jacobi       1.22 / 1.26 x on basic / maze; umass 1.02 x (spread 1.0 %) at four and 1.10-1.11 x from sixteen: above 0.25 Mcell from sixteen
//   precise Jacobi   1.68 / 1.29 / 1.18 x, 1.32-1.72 x at 16 and 64
//   fast             not measured: off (EPIC_HIP_BATCH=1 under EPIC_HIP_STUDY=1 takes it, as it takes any mode from two fields)
unsigned batch_from_fields(const Ctx *c)
{
    const long long cells = (long long)c->rows * c->cols;
    if (default_mode(c)) return cells > 250000 ? 4 : 2;
    if (c->math == 4) return !c->redblack && cells > 250000 ? 16 : 4;
    return c->math == 0 ? 4 : ~0u;
}

// Width, ring depth, tile height and fields per workgroup for `live` fields of rows x cols cells, by the cost model of the
// single-field tiles (driver_plan.hip: tile_plan): an iteration of ONE workgroup costs its share of the launch,
// (2.7 us + 0.06 us per 1000 LDS cells) / H, plus the step -- the larger of a latency chain, 0.84 us + 0.055 us per pass and SIMD,
// and the issue of the passes, 0.2 us + 0.21 us per pass and SIMD -- and 60 % more for every further workgroup a CU has to take.
// Two things differ.  The workgroups of a launch are tiles x ceil(live / F), laid over 256 CUs: with many fields one field no longer
// has to fill the chip, so taller tiles and the wide tile (1.3-1.5 ring cells per owned cell instead of 2.3) are considered for
// every count -- the tile height is what gives every CU one workgroup, where the LDS tile allows.  And a workgroup issues the
// passes of F fields per step: kStepOfFields is what that costs against F workgroups of one field, read from the forced rows of
// profiles/batch_2d.txt.  F = 2 at the SAME geometry and 32 fields is 3-4 % slower than F = 1 on both widths (basic 44x44 H=10,
// maze 100x100 H=14, umass 108x108 H=10): the interleave itself buys nothing, and F = 2 is taken only where half as many workgroups
// make a better geometry.  F = 4 against F = 1 on the same narrow tiles is 1.09 / 1.16 x at 32 fields of basic.png (44x44 H=10) and
// 1.23 / 1.27 x at 8 fields of umass.png, but 0.93 x and 0.96 x at 32 fields of maze.png and umass.png, where F = 1 needs many rounds:
// 1.12 is basic.png's figure, not fitted further, and the model never picks F = 4 on the measured maps.
// The bits do not depend on any of it.  Study knobs: EPIC_HIP_BATCH_FIELDS / _HALO / _ROWS / _WIDTH.
// The other modes (math, redblack) take the same model with what differs in tile_plan's: a Jacobi wave takes a row per pass, not a row
// pair, the tol passes issue in 0.17 us instead of 0.21, and the tile heights and fields per workgroup are what that mode's LDS holds
// (kernels_tile2d_batch_modes.hip).  kStepOfFields is the precise red-black figure there too; the forced rows of
// profiles/batch_2d_modes.txt say what F = 2 and F = 4 are worth with the tol table staged once for F fields.
constexpr double kStepOfFields[5] = {0.0, 1.0, 1.04, 0.0, 1.12};   // [F]: step of a workgroup of F fields / (F x the step of one)
BatchPlan batch_plan(int rows, int cols, unsigned live, const Config &cfg, int math = 0, bool redblack = true)
{
    BatchPlan best = {{0, 0, 0, 0, 0}, 0};
    double best_cost = 0.0;
    int widest_fields = 0;   // the most fields any allowed width holds in this mode: a forced F above it means that many
    for (int width : {epic_hip::kTile2dCols, epic_hip::kTile2dWideCols})
        if (!cfg.batch_width || width == cfg.batch_width) widest_fields = std::max(widest_fields, mode_max_fields(math, redblack, width));
    for (int width : {epic_hip::kTile2dCols, epic_hip::kTile2dWideCols}) {
        if (cfg.batch_width && width != cfg.batch_width) continue;
        const int max_rows = epic_hip::tile_2d_max_rows(math, redblack, width), max_fields = mode_max_fields(math, redblack, width);
        if (max_rows == 0) continue;
        for (int fields : {1, 2, 4}) {
            if (fields > max_fields) continue;
            // a forced F means F: a width that cannot hold it is left out, unless no allowed width holds it (then the largest F there is)
            if (cfg.batch_fields && fields != std::min(cfg.batch_fields, widest_fields)) continue;
            const int groups = (int)((live + fields - 1) / fields);
            for (int halo : {8, 10, 12, 14, 16}) {
                const int h = cfg.batch_halo ? cfg.batch_halo : halo;
                int tr = cfg.batch_rows;
                if (tr <= 0) {   // the height that gives every CU one workgroup (tile_2d_plan's rule, for tiles x groups)
                    if (2 * h >= width - 8) break;
                    const int tiles_c = (cols + width - 2 * h - 1) / (width - 2 * h);
                    const int tiles_r_max = std::max(1, 256 / (tiles_c * groups));
                    tr = std::max(8, ((rows + tiles_r_max - 1) / tiles_r_max + 1) / 2 * 2);
                }
                const epic_hip::TilePlan p = epic_hip::tile_2d_plan(rows, cols, h, tr, width, max_rows);
                if (p.halo > 0 && (size_t)p.tiles_r * p.tiles_c <= kTileDeltaCap) {
                    const int s_r = p.tile_rows + 2 * h;
                    const double per_simd = (redblack ? s_r / 2.0 : (double)s_r) * (width / 64) / 4.0 * fields;
                    const double rounds = std::max(1.0, (double)p.tiles_r * p.tiles_c * groups / 256.0);
                    const double step = std::max(0.84 + 0.055 * per_simd, 0.2 + (math == 4 ? 0.17 : 0.21) * per_simd) * kStepOfFields[fields];
                    const double cost = (rounds > 1.0 ? 1.6 * rounds / 2.0 + 0.2 : 1.0) * ((2.7 + 0.00006 * s_r * width * fields) / h + step);
                    if (best.fields == 0 || cost < best_cost) { best = BatchPlan{p, fields}; best_cost = cost; }
                }
                if (cfg.batch_halo) break;
            }
        }
    }
    return best;
}

// 3-D: from how many voxel fields of this shape the batched brick kernel is taken (fewer: the per-field loop; ~0u: never).  A lone field
// is never batched.  Read from profiles/batch_3d.txt (epic_hip_complete_batch_gpu / loop of harmonic_complete_gpu in one process, three
// alternating repetitions): the batch is taken only where a row shows it faster than the loop by more than that row's spread, and a
// size without a row keeps the loop.
//   16^3   loop: 1.08 x at four fields is the only row that passes; 16 and 32 fields LOSE (0.98, 0.97 x, spread <= 2.8 %)
//   32^3   from four: 1.05 x, 1.03 x, 1.02 x, 1.03 x, 1.03 x at 4 ... 64 fields (spread <= 1.4 %); two fields 1.05 x inside a spread of 5.1 %
//   64^3   from two: 1.02 x (spread 1.8 %), then 1.03 x;  64 x 64 x 200 (0.82 Mcell, shells along x2 too) from two: 1.04 x (1.3 %), 1.07-1.08 x
//   96^3   from four: 1.03-1.04 x (spread <= 1.4 %); two fields 1.00 x
// Sizes between two measured ones take the stricter neighbour; below 32^3 and above 96^3 nothing supports the batch.
unsigned batch3d_from_fields(const int *m)
{
    const long long cells = (long long)m[0] * m[1] * m[2];
    if (cells < 32 * 32 * 32 || cells > 96 * 96 * 96) return ~0u;
    return cells >= 64 * 64 * 64 && cells <= 64 * 64 * 200 ? 2u : 4u;   // (64^3 and 64 x 64 x 200 both take two; 32^3 ... 64^3 and up to 96^3 four)
}

// Shell depth, bricks per axis and LDS capacity for `live` voxel fields of m0 x m1 x m2 cells, in brick_plan's cost form
// (driver_plan.hip; DESIGN.md sections 4.12, 4.14): an iteration of ONE workgroup costs (launch + load and store of the brick) / H plus
// the step -- the larger of a latency chain and the issue of one SIMD's passes --, x 1.6 per further round.  Three things differ.
// The workgroups of a launch are bricks x live fields.  A round is 256 workgroups at capacity 576 and 512 at capacity 288, where a CU
// holds two -- and as soon as a CU does hold two they share its issue, so the issue term counts twice there while the latency chain
// of one hides behind the other: that is the whole case for the small capacity, and an ASSUMPTION of this model, not a fit.  And with
// many fields a field no longer has to fill the chip: larger bricks with less shell recomputation come into reach, as the wide tile
// did in 2-D.  The per-pass constants (0.004 per brick row, 1.0 + 0.07 per pass, 0.4 per pass) are brick_plan's PLACEHOLDERS,
// UNFITTED ESTIMATES, reused as they are.  The bits do not depend on any of it.  Study knobs: EPIC_HIP_BATCH_HALO (shell depth),
// EPIC_HIP_BRICK_DIMS (S0xS1), EPIC_HIP_BATCH_BRICK_ROWS (capacity).
BrickBatchPlan batch_brick_plan(const int *m, unsigned live, const Config &cfg)
{
    BrickBatchPlan best = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0};
    double best_cost = 0.0;
    for (int capacity : {epic_hip::kBrickBatchRows, epic_hip::kBrickBatchRowsHalf}) {
        if (cfg.batch_brick_rows && capacity != cfg.batch_brick_rows) continue;
        const bool half = capacity == epic_hip::kBrickBatchRowsHalf;
        auto consider = [&](const epic_hip::BrickPlan &p) {
            const long long bricks = (long long)p.nb0 * p.nb1 * p.nbc;
            if (p.halo == 0 || bricks > kBrickDeltaCap) return;
            const double wgs = (double)bricks * live;
            const double per_simd = std::ceil((p.s1 / 2) * (double)p.s0 / 16.0) * 4.0;
            const double rounds = std::ceil(wgs / (half ? 512.0 : 256.0));
            const double issue = (half && wgs > 256.0 ? 2.0 : 1.0) * 0.4 * per_simd;
            const double step = std::max(1.0 + 0.07 * per_simd, 0.2 + issue);
            const double cost = (rounds > 1.0 ? 1.6 * rounds / 2.0 + 0.2 : 1.0) * ((2.7 + 0.004 * p.s0 * p.s1) / p.halo + step);
            if (best.capacity == 0 || cost < best_cost) { best = BrickBatchPlan{p, capacity}; best_cost = cost; }
        };
        for (int halo : {2, 3, 4, 6, 8}) {
            const int h = cfg.batch_halo ? cfg.batch_halo : halo;
            if (cfg.brick_s0 > 0) {
                consider(epic_hip::brick_3d_plan(m[0], m[1], m[2], h, cfg.brick_s0, cfg.brick_s1, capacity));
            } else {
                for (int nb0 = 1; nb0 <= 64; ++nb0)
                    for (int nb1 = 1; nb1 <= 16; ++nb1) {
                        const int s0 = nb0 == 1 ? m[0] : (m[0] + nb0 - 1) / nb0 + 2 * h;
                        const int s1 = nb1 == 1 ? m[1] : (((m[1] + nb1 - 1) / nb1 + 2 * h + 1) & ~1);
                        if ((nb0 > 1 && s0 >= m[0]) || (nb1 > 1 && s1 >= m[1])) continue;   // (the shells would make it the whole axis again)
                        consider(epic_hip::brick_3d_plan(m[0], m[1], m[2], h, s0, s1, capacity));
                    }
            }
            if (cfg.batch_halo) break;
        }
    }
    return best;
}

// What a batch call does with the fields as they are now: rc[i] = -1 for a field that goes through harmonic_execute_gpu; the
// others in groups of one shape, one checking period and one mode, each at least batch_from_fields() strong, in the order of their
// first member (fields of different modes in one call form different groups; a lone field of its mode is never batched).
std::vector<std::vector<Member>> group_fields(EpicHarmonicT *const *fields, unsigned count)
{
    std::vector<std::vector<Member>> groups;
    for (unsigned i = 0; i < count; i++) {
        Harmonic *h = fields[i];
        Ctx *c = h ? find_ctx(h) : nullptr;
        if (!batchable(h, c)) continue;
        const Member m = {h, c, i, nullptr};
        auto same = [&](const std::vector<Member> &g) {   // (3-D: rows = m[0] m[1], so all three extents are compared)
            return g[0].c->n == c->n && g[0].c->m[0] == c->m[0] && g[0].c->rows == c->rows && g[0].c->cols == c->cols &&
                   g[0].h->numIterationsToStaggerCheck == h->numIterationsToStaggerCheck && g[0].c->math == c->math &&
                   g[0].c->redblack == c->redblack && jacobi_reference_checks(g[0].c) == jacobi_reference_checks(c);
        };
        auto it = std::find_if(groups.begin(), groups.end(), same);
        if (it == groups.end()) groups.push_back({m});
        else it->push_back(m);
    }
    groups.erase(std::remove_if(groups.begin(), groups.end(),
                                [](const std::vector<Member> &g) {
                                    // (a forced EPIC_HIP_BATCH_FIELDS batches from two fields: how the crossover is measured)
                                    const Ctx *c = g[0].c;
                                    if (c->n == 3)   // (a forced F, capacity or shell depth batches from two fields: how the crossover is measured)
                                        return g.size() < (c->cfg.batch_fields || c->cfg.batch_brick_rows || c->cfg.batch_halo ? 2u : batch3d_from_fields(c->m)) ||
                                               batch_brick_plan(c->m, (unsigned)g.size(), c->cfg).capacity == 0;
                                    // (so does EPIC_HIP_BATCH=1 under EPIC_HIP_STUDY=1: the modes that are off by default)
                                    return g.size() < (c->cfg.batch_fields || c->cfg.batch_forced ? 2u : batch_from_fields(c)) ||
                                           batch_plan(c->rows, c->cols, (unsigned)g.size(), c->cfg, c->math, c->redblack).fields == 0;
                                }),
                 groups.end());
    return groups;
}

// What a group shares for the length of a call: a stream, the field table (pinned staging and its device copy) and the pinned
// per-field, per-tile maxima of a check.
struct Shared {
    hipStream_t stream = nullptr;
    epic_hip::BatchField *h_table = nullptr, *d_table = nullptr;
    float *h_delta = nullptr;
    size_t delta_cap = 0;
    bool make(size_t slots)
    {
        return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess &&
               hipHostMalloc((void **)&h_table, slots * sizeof(epic_hip::BatchField), hipHostMallocDefault) == hipSuccess &&
               hipMalloc((void **)&d_table, slots * sizeof(epic_hip::BatchField)) == hipSuccess;
    }
    bool hold_deltas(size_t words)   // (only between blocks: nothing is in flight)
    {
        if (words <= delta_cap) return true;
        if (h_delta) (void)hipHostFree(h_delta);
        delta_cap = 0;
        if (hipHostMalloc((void **)&h_delta, words * sizeof(float), hipHostMallocDefault) != hipSuccess) { h_delta = nullptr; return false; }
        delta_cap = words;
        return true;
    }
    ~Shared()
    {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (h_table) (void)hipHostFree(h_table);
        if (d_table) (void)hipFree(d_table);
        if (h_delta) (void)hipHostFree(h_delta);
    }
};

// The relaxation of one group, harmonic_execute_gpu's loop for all its fields at once.  A block is the plain iterations up to the
// next check plus that check (iteration 0 is a check of its own), cut into launches of at most `halo` steps exactly like
// enqueue_block in driver_loop.hip; the parity comes from the iteration number.  Three buffers per field rotate, as there: a block
// never writes the buffer it started from, so whatever fails in it leaves every context in the state its last read check describes.
// After a block the per-field maxima are read and every field's check is followed by what follows it in the single call
// (Relaxation::after_check): a field that has ended -- or whose mode the check has changed: the tol mode's finishing phase, the Jacobi
// hand-over -- leaves with the buffer, iteration number and delta of that check and goes through relax_to_end, which continues it as
// harmonic_execute_gpu would (not at all, if it has ended) and reads it back; the table is repacked so that the workgroups stay full,
// and the plan is made again for the fields that are left.  (The next block is NOT enqueued ahead of the check's read, as the
// single-field loop does: DESIGN.md section 4.13.)  A Jacobi group under EPIC_HIP_JACOBI_CHECKS=reference runs its check as a launch
// of its own, ONE red-black step of the same arithmetic, as enqueue_block does.  A group of 3-D fields runs the same loop on bricks:
// only the plan and the launch differ (the third buffer of tiles_pipeline_ready is rows x pitch floats, and a 3-D context's rows are
// m[0] m[1]).
void run_group(std::vector<Member> &members, unsigned numThreads, int *rc, const char *fn)
{
    const Config cfg = members[0].c->cfg;
    const int rows = members[0].c->rows, cols = members[0].c->cols, pitch = members[0].c->pitch;
    const unsigned stagger = members[0].h->numIterationsToStaggerCheck;
    const bool voxels = members[0].c->n == 3;
    const int m3[3] = {members[0].c->m[0], members[0].c->m[1], members[0].c->m[2]};
    const int math = members[0].c->math;
    const bool redblack = members[0].c->redblack, ref_checks = jacobi_reference_checks(members[0].c);
    std::vector<Member> live;
    for (const Member &m : members) {
        // an ordering point for every field, and the start of its relaxation (harmonic_execute_gpu)
        int r = flush_pending(m.h, m.c, fn);
        if (r == EPIC_SUCCESS && !tiles_pipeline_ready(m.c)) {   // no third buffer to be had: this field alone
            rc[m.index] = harmonic_execute_gpu(m.h, numThreads);
            continue;
        }
        if (r == EPIC_SUCCESS && hipStreamSynchronize(m.c->stream) != hipSuccess) {
            report(fn, "Failed to synchronize the device before the batch.");
            r = EPIC_ERROR_DEVICE_SYNCHRONIZE;
        }
        if (r == EPIC_SUCCESS) {
            m.h->currentIteration = 0;
            fold_listed_work(m.c);
            m.c->work_full = 0.0;
            m.c->finish_from = 0;
            r = harmonic_initialize_gpu(m.h, numThreads);
            if (r != EPIC_SUCCESS) report(fn, "Failed to initialize GPU variables.");
        }
        rc[m.index] = r;
        if (r != EPIC_SUCCESS) continue;
        m.h->delta = m.h->epsilon + 1.0f;
        live.push_back(m);
        live.back().rx = std::make_shared<Relaxation>(m.h, m.c);
    }
    if (live.empty()) return;
    auto fail_all = [&](int code, const char *msg) {
        report(fn, msg);
        (void)hipGetLastError();
        for (const Member &m : live) rc[m.index] = code;
    };
    Shared sh;
    if (!sh.make(live.size() + 3)) return fail_all(EPIC_ERROR_DEVICE_MALLOC, "Failed to allocate the field table of the batch.");

    BatchPlan plan = {{0, 0, 0, 0, 0}, 0};
    BrickBatchPlan bplan = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0};
    size_t planned_for = 0;
    while (!live.empty()) {
        if (planned_for != live.size()) {   // (again whenever fields have retired)
            if (voxels) bplan = batch_brick_plan(m3, (unsigned)live.size(), cfg);
            else plan = batch_plan(rows, cols, (unsigned)live.size(), cfg, math, redblack);
            planned_for = live.size();
        }
        const int F = voxels ? (bplan.capacity ? 1 : 0) : plan.fields;
        const int tiles = voxels ? bplan.bp.nb0 * bplan.bp.nb1 * bplan.bp.nbc : plan.tp.tiles_r * plan.tp.tiles_c;
        const int halo = voxels ? bplan.bp.halo : plan.tp.halo;
        if (F == 0) return fail_all(EPIC_ERROR_KERNEL_EXECUTION, "No tile plan for the batch.");
        const int groups = ((int)live.size() + F - 1) / F;
        if (!sh.hold_deltas(live.size() * (size_t)tiles)) return fail_all(EPIC_ERROR_DEVICE_MALLOC, "Failed to allocate pinned memory for the batch's checks.");
        // the table of this block: slot s is live[s]; bufs[0] is the state the latest check describes and is only read
        for (int s = 0; s < groups * F; s++) {
            epic_hip::BatchField &bf = sh.h_table[s];
            bf = epic_hip::BatchField{{nullptr, nullptr, nullptr}, nullptr, nullptr};
            if (s >= (int)live.size()) continue;
            Ctx *c = live[s].c;
            bf = epic_hip::BatchField{{c->buf[c->cur], c->buf[c->cur ^ 1], c->spare}, c->maskw, sh.h_delta + (size_t)s * tiles};
        }
        if (hipMemcpyAsync(sh.d_table, sh.h_table, (size_t)groups * F * sizeof(epic_hip::BatchField), hipMemcpyHostToDevice, sh.stream) != hipSuccess)
            return fail_all(EPIC_ERROR_MEMCPY_TO_DEVICE, "Failed to copy the field table of the batch to the device.");
        const unsigned first = live[0].h->currentIteration;   // (the same for every live field: one checking period, one start)
        const unsigned total = first % stagger == 0 ? 1u : stagger - first % stagger + 1u;
        int src = 0;
        for (unsigned i = 0; i < total;) {
            unsigned k = std::min<unsigned>(total - i, (unsigned)halo);
            if (ref_checks && i + k == total && k > 1) k--;   // (the reference's half-sweep: a launch of its own)
            const bool half_sweep = redblack || (ref_checks && i + k == total);
            const int dst = src == 1 ? 2 : 1;
            const int parity = (int)((first + i) & 1u);
            hipError_t e;
            if (voxels)
                e = epic_hip::launch_brick_3d_batch(sh.d_table, groups, src, dst, m3[0], m3[1], pitch, bplan.bp, bplan.capacity, (int)k, parity, i + k == total, sh.stream);
            else if (math == 0 && half_sweep)
                e = epic_hip::launch_tile_2d_batch(sh.d_table, groups, F, src, dst, rows, pitch, plan.tp, (int)k, parity, i + k == total, sh.stream);
            else
                e = epic_hip::launch_tile_2d_batch_modes(sh.d_table, groups, F, src, dst, rows, pitch, plan.tp, (int)k, math, half_sweep ? parity : -1,
                                                         i + k == total, sh.stream);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(sh.stream);
                return fail_all(EPIC_ERROR_KERNEL_EXECUTION, "Failed to execute the batched 'Jacobi update' kernel.");
            }
            src = dst;
            i += k;
        }
        if (hipStreamSynchronize(sh.stream) != hipSuccess)
            return fail_all(EPIC_ERROR_DEVICE_SYNCHRONIZE, "Failed to synchronize the device after the batched 'update and check' kernel.");
        // the check of every field; the ones it ends, and the ones whose mode it changes, leave
        std::vector<Member> next;
        for (size_t s = 0; s < live.size(); s++) {
            const Member &m = live[s];
            Ctx *c = m.c;
            if (src == 2) { std::swap(c->spare, c->buf[c->cur]); drop_graphs(c); }   // (captured sequences hold addresses)
            else c->cur ^= 1;
            m.h->d_u = current_u(c);
            float d = 0.0f;
            for (int t = 0; t < tiles; ++t) d = std::max(d, sh.h_delta[s * (size_t)tiles + t]);
            m.h->delta = d;
            m.h->currentIteration = first + total;
            c->work_full += (double)total;
            m.rx->result = d < m.h->epsilon ? EPIC_SUCCESS_AND_CONVERGED : EPIC_SUCCESS;
            m.rx->after_check();
            if (!m.rx->over() && c->math == math && c->redblack == redblack) {
                next.push_back(m);
                continue;
            }
            rc[m.index] = relax_to_end(*m.rx, fn);
            live[s].rx.reset();   // (the context has its mode back, as after the single call)
        }
        live.swap(next);
    }
}

bool valid_call(EpicHarmonicT *const *fields, unsigned count, unsigned numThreads, const char *fn, int *code)
{
    bool twice = false;
    if (fields && count > 0) {
        std::vector<const void *> seen;
        for (unsigned i = 0; i < count; i++)
            if (fields[i]) seen.push_back(fields[i]);
        std::sort(seen.begin(), seen.end());
        twice = std::adjacent_find(seen.begin(), seen.end()) != seen.end();
    }
    if (!fields || count == 0 || twice) {
        report(fn, twice ? "Invalid data (a field appears twice in the batch)." : "Invalid data.");
        *code = EPIC_ERROR_INVALID_DATA;
        return false;
    }
    if (numThreads % 32 != 0) {
        report(fn, "Must specficy a number of threads divisible by 32 (the number of threads in a warp).");
        *code = EPIC_ERROR_INVALID_CUDA_PARAM;
        return false;
    }
    return true;
}

// rc[i] for every field with skip[i] == 0
void execute_fields(EpicHarmonicT *const *fields, unsigned count, unsigned numThreads, const std::vector<char> &skip, int *rc, const char *fn)
{
    std::vector<EpicHarmonicT *> taken(fields, fields + count);
    for (unsigned i = 0; i < count; i++)
        if (skip[i]) taken[i] = nullptr;   // (a null member is not batchable)
    std::vector<std::vector<Member>> groups = group_fields(taken.data(), count);
    std::vector<char> batched(count, 0);
    for (const auto &g : groups)
        for (const Member &m : g) batched[m.index] = 1;
    for (unsigned i = 0; i < count; i++)
        if (!skip[i] && !batched[i]) rc[i] = harmonic_execute_gpu(fields[i], numThreads);
    for (auto &g : groups) run_group(g, numThreads, rc, fn);
}

int first_failure(const int *rc, unsigned count, int *results)
{
    int all = EPIC_SUCCESS;
    for (unsigned i = 0; i < count; i++) {
        if (results) results[i] = rc[i];
        if (all == EPIC_SUCCESS && rc[i] != EPIC_SUCCESS) all = rc[i];
    }
    return all;
}

}  // namespace

extern "C" {

int epic_hip_execute_batch_gpu(EpicHarmonicT *const *fields, unsigned int count, unsigned int numThreads, int *results)
{
    static const char *fn = "epic_hip_execute_batch_gpu";
    int code = EPIC_SUCCESS;
    if (!valid_call(fields, count, numThreads, fn, &code)) return code;
    std::vector<int> rc(count, EPIC_SUCCESS);
    execute_fields(fields, count, numThreads, std::vector<char>(count, 0), rc.data(), fn);
    return first_failure(rc.data(), count, results);
}

int epic_hip_complete_batch_gpu(EpicHarmonicT *const *fields, unsigned int count, unsigned int numThreads, int *results)
{
    static const char *fn = "epic_hip_complete_batch_gpu";
    int code = EPIC_SUCCESS;
    if (!valid_call(fields, count, numThreads, fn, &code)) return code;
    // harmonic_complete_gpu per field (harmonic_gpu.cu:168-201): the three initialisations, the relaxation, the three releases --
    // a step that fails ends that field's sequence where the single call's would end
    std::vector<int> rc(count, EPIC_SUCCESS);
    std::vector<char> skip(count, 0);
    for (unsigned i = 0; i < count; i++) {
        rc[i] = harmonic_initialize_dimension_size_gpu(fields[i]);
        if (rc[i] == EPIC_SUCCESS) rc[i] = harmonic_initialize_potential_values_gpu(fields[i]);
        if (rc[i] == EPIC_SUCCESS) rc[i] = harmonic_initialize_locked_gpu(fields[i]);
        skip[i] = rc[i] != EPIC_SUCCESS;
    }
    execute_fields(fields, count, numThreads, skip, rc.data(), fn);
    for (unsigned i = 0; i < count; i++) {
        if (rc[i] != EPIC_SUCCESS) continue;
        if (harmonic_uninitialize_dimension_size_gpu(fields[i]) != EPIC_SUCCESS) rc[i] = EPIC_ERROR_DEVICE_FREE;
        if (harmonic_uninitialize_potential_values_gpu(fields[i]) != EPIC_SUCCESS) rc[i] = EPIC_ERROR_DEVICE_FREE;
        if (harmonic_uninitialize_locked_gpu(fields[i]) != EPIC_SUCCESS) rc[i] = EPIC_ERROR_DEVICE_FREE;
    }
    return first_failure(rc.data(), count, results);
}

int epic_hip_batch_plan(EpicHarmonicT *const *fields, unsigned int count, unsigned int *batched, int *fields_per_workgroup, int *halo,
                        int *tile_rows, int *tile_cols)
{
    static const char *fn = "epic_hip_batch_plan";
    int code = EPIC_SUCCESS;
    if (!valid_call(fields, count, 0, fn, &code)) return code;
    const std::vector<std::vector<Member>> groups = group_fields(fields, count);
    unsigned n = 0;
    for (const auto &g : groups) n += (unsigned)g.size();
    BatchPlan plan = {{0, 0, 0, 0, 0}, 0};
    if (!groups.empty() && groups[0][0].c->n == 3) {   // a 3-D group: one field per workgroup, shells, and the brick's planes and rows
        const BrickBatchPlan b = batch_brick_plan(groups[0][0].c->m, (unsigned)groups[0].size(), groups[0][0].c->cfg);
        plan = BatchPlan{{b.bp.halo, b.bp.s0, b.bp.s1, 0, 0}, b.capacity ? 1 : 0};
    } else if (!groups.empty()) {
        const Ctx *c = groups[0][0].c;
        plan = batch_plan(c->rows, c->cols, (unsigned)groups[0].size(), c->cfg, c->math, c->redblack);
    }
    if (batched) *batched = n;
    if (fields_per_workgroup) *fields_per_workgroup = plan.fields;
    if (halo) *halo = plan.tp.halo;
    if (tile_rows) *tile_rows = plan.tp.tile_rows;
    if (tile_cols) *tile_cols = plan.tp.tile_cols;
    return EPIC_SUCCESS;
}

}  // extern "C"
