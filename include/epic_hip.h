/*
 * epic_hip.h -- extension entry points of the MI355X-native libepic.so (plain C ABI).
 *
 * The reference ABI (include/epic/epic_abi.h) has no notion of streams, batches of sweeps, timing or
 * more than one GPU.  These additions sit beside it for callers that want them (bench.py, the slab
 * decomposition driver epic_amd/slab.py, a ROS node that wants "k sweeps" in one call); nothing in the
 * reference ABI depends on them.  All pointers named d_* are device pointers on the current HIP device;
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 */
#ifndef EPIC_HIP_H
#define EPIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
namespace epic { struct Harmonic; }
typedef epic::Harmonic EpicHarmonicT;
extern "C" {
#else
struct Harmonic;
typedef struct Harmonic EpicHarmonicT;
#endif

/* "epic-hip <semver> gfx950" */
const char *epic_hip_version(void);
/* Number of HIP devices visible (0 on a GPU-less host; never fails). */
int epic_hip_device_count(void);

/* ---- batches on an initialised Harmonic (device state created by harmonic_initialize_*_gpu) ----------
 * Enqueue `sweeps` iterations of the selected scheme without a host round-trip; currentIteration advances by `sweeps`.
 * If check_last != 0 the last sweep also reduces max|du| and the call synchronises, stores it in
 * harmonic->delta and returns EPIC_SUCCESS_AND_CONVERGED when delta < epsilon (needs harmonic_initialize_gpu).
 * Otherwise it returns after enqueueing (ordering points: any *_and_check, get_potential_values, update_model,
 * set_cells, uninitialize).  Replaces a loop over harmonic_update_gpu (libepic/src/harmonic/harmonic_gpu.cu:327-350),
 * e.g. the navigation node's update(num_steps) (src/epic_navigation_node_harmonic.cpp:165-189). */
int epic_hip_update_n_gpu(EpicHarmonicT *harmonic, unsigned int sweeps, int check_last);

/* Same, bracketed by HIP events on the library's own stream; *elapsed_ms = device time of the batch.
 * Synchronises.  check_every = 0: no checks; k > 0: every k-th sweep (counted by currentIteration % k == 0,
 * the reference's rule, harmonic_gpu.cu:268) is a check sweep. */
int epic_hip_timed_sweeps_gpu(EpicHarmonicT *harmonic, unsigned int sweeps, unsigned int check_every,
                              float *elapsed_ms);

/* How many iterations one kernel launch of a batch of PLAIN (unchecked) iterations advances in the current configuration:
 * 2 where pairs of iterations run as one fused pass over the data -- Jacobi with the tol math (two sweeps, 4 B of HBM
 * traffic per cell-update instead of 8) and red-black with any math (both colours), 2-D grids from the size at which the pass beats
 * the other kernel families (tol Jacobi 1.5 Mcell, tol red-black 2 Mcell, precise red-black 5.5 Mcell; EPIC_HIP_FUSE_MIN_CELLS) with activity tracking off (per device in multi-device mode, between exchanges); results are bit-identical to single iterations, an odd iteration and
 * every check iteration run singly -- 1 otherwise, 0 without device state.  EPIC_HIP_NO_FUSE=1 switches the fusion off. */
int epic_hip_iterations_per_pass(EpicHarmonicT *harmonic);

/* Small 2-D grids (at most 3 Mcell -- less where another family is faster: EPIC_HIP_TILE_MAX_CELLS --, one device, activity tracking off -- the maps the reference's callers relax): the plain
 * iterations between two checks run SEVERAL PER LAUNCH on tiles that stay in LDS with that many ghost rings
 * (epic_amd/csrc/kernels_tile2d.hip); bit-identical to single iterations.  Returns the iterations one such launch advances
 * (8, 10, 12, 14 or 16, chosen per grid by a cost model of the launch; 1 to 27 when EPIC_HIP_TILE_HALO fixes it), 0 where the path
 * is not used.  EPIC_HIP_TILE=0 switches it off; EPIC_HIP_TILE_HALO / _ROWS / _WIDTH / _MAX_CELLS tune it. */
int epic_hip_tile_iterations(EpicHarmonicT *harmonic);

/* Rows per task of that fused pass in the current configuration (0: no fused pass).  On grids of at least 4 Mcell on one
 * device the height is measured on the grid itself the first time a pair of plain iterations is enqueued (a few candidates,
 * three launches each, ~10 ms, once per grid and kind of pass; results do not depend on it): before that the call returns
 * the rule's value.  EPIC_HIP_TUNE=0 keeps the rule; EPIC_HIP_FUSED_ROWS / epic_hip_set_rows_per_task fix the height. */
int epic_hip_fused_rows_per_task(EpicHarmonicT *harmonic);

/* tol math, harmonic_execute_gpu / harmonic_complete_gpu: the loop leaves the tol arithmetic at the first check with
 * delta < 10 epsilon (100 epsilon for epsilon <= 1e-5) and FINISHES with the reference's own iteration (red-black half-sweeps, bit-exact expf / logf).  For
 * relaxations to stagnation (epsilon <= 1e-5) only a check of that phase may end the loop -- the converged field is then the end point of the
 * reference's iteration from a state within a few 1e-5 of it: maps/umass.png 1.4e-6 from harmonic_complete_cpu's field instead of 1.6e-5.  At the
 * callers' epsilons (> 1e-5) the hand-over check keeps its own verdict (round 6: on maps that converge within a few checks the reference stops at that
 * very check), and a first check that reports delta = 0 exactly (a run that has not moved yet) does not hand over.  Measured against the reference on
 * 720 generated cases (2-D and 3-D): tests/tol_campaign.py, DESIGN.md section 2.
 * EPIC_HIP_TOL_FINISH=0 in the environment keeps the tol iteration to the end (honoured for epsilon <= 1e-5 only: above, the
 * finishing phase is what makes the stop the reference's).  EPIC_HIP_TOL_FINISH_FACTOR=f replaces the 10 / 100 (a study knob:
 * tools/finish_study_gpu.py swept it over every map of the reference).
 * WHAT tol CANNOT PROMISE: on maps whose delta crosses epsilon in steps of single ulps (the reference's maps/trivial.png, an
 * almost empty 1024^2 room: delta falls 0.15 % per 100 iterations) the iteration at which the loop stops is decided by single
 * ulps of single cells; no hand-over factor is safe there (4e-3 from the reference for factors 10, 50, 300; inside the bar for
 * 20 and 100 -- by chance), and only the default precise math reproduces the reference.  The library says so once on stderr
 * when a tol relaxation reaches its hand-over on such a plateau (delta down by less than 0.3 % per check over the last 32 checks).
 * Returns the iteration number at which the finishing phase of the latest call began (0: it had none). */
unsigned int epic_hip_finish_iteration(EpicHarmonicT *harmonic);

/* Tuning knob: rows marched by one wave in the 2-D kernel (0 = automatic).  Also EPIC_HIP_ROWS_PER_TASK. */
int epic_hip_set_rows_per_task(EpicHarmonicT *harmonic, unsigned int rows_per_task);

/* Arithmetic of the sweep kernels (also EPIC_HIP_MATH=precise|tol|fast in the environment at initialisation):
 *   0 precise (default)  exp/log bit-identical to the host libm's expf/logf, evaluated in f64 -- the bit-exact parity mode;
 *   4 tol                one exp-class split e^u = q 2^n per CELL (packed f32 polynomial), shared by the cells it is a
 *                        neighbour of, one table-driven log per cell (256 intervals per binade, exact f32 reduction,
 *                        2^-33 accurate); every rounding stage of the reference kept.  2-D and 3-D,
 *                        Jacobi and red-black.  Jacobi stops by the reference's own test.  harmonic_execute_gpu /
 *                        harmonic_complete_gpu finish a tol relaxation with the reference's own iteration
 *                        (epic_hip_finish_iteration, above): converged fields within 1e-5 max(1, |u|) of the reference's
 *                        on every map and grid under test, 1.4e-6 on the ill-conditioned umass.png (the tol iteration
 *                        alone: 1.6e-5 there).  ~1.3x faster per sweep than precise, ~1.75x where pairs of
 *                        iterations run as one fused pass (epic_hip_iterations_per_pass); the benchmarked mode;
 *   1 fast               v_exp_f32 / v_log_f32: biased (one update: -0.25 to -0.6 f32 spacings against precise where |u| <~ 1
 *                        and next to a goal, nothing from |u| ~ 40 on), ~1e-4 relative drift on ill-conditioned maps; no
 *                        parity claim;
 *   2 traffic            diagnostic: same loads/stores, trivial arithmetic (2-D only).
 * (3 was round 1's df32 mode, removed: EPIC_ERROR_INVALID_DATA.) */
int epic_hip_set_math_mode(EpicHarmonicT *harmonic, int mode);

/* Iteration scheme: 1 = the reference's red-black Gauss-Seidel, in place (DEFAULT: one iteration = one colour,
 * libepic/src/harmonic/harmonic_cpu.cpp:46-51, :89-102; with the default precise math every half-sweep, the iteration count
 * and the converged field are bit-identical to harmonic_complete_cpu), 0 = Jacobi ping-pong (one iteration recomputes
 * every unlocked cell: what BASELINE.json's metric names and bench.py times; twice the arithmetic for the same answer).
 * Also EPIC_HIP_SCHEME=jacobi|redblack in the environment at initialisation.
 * EPIC_HIP_JACOBI_CHECKS=reference (environment, opt-in): every CHECK iteration of a Jacobi run is the reference's half-sweep of that
 * iteration's colour, in place -- the state after a check, and so the field a relaxation ends with, is the reference's own (with the
 * precise math bit for bit, iteration count included); INTEGRATION.md section 6. */
int epic_hip_set_scheme(EpicHarmonicT *harmonic, int scheme);

/* Activity tracking: 0 off, 1 on, 2 automatic (default: on for grids above 4 Mcell; also
 * EPIC_HIP_TRACK=0|1 in the environment at initialisation).  A tile (2-D: rows_per_task x 256 cells; 3-D: 32 x 256 cells
 * of one plane) is recomputed in an
 * iteration only if the previous iteration changed a value it reads (one of its own cells or the adjacent row / column of
 * an edge neighbour); otherwise the update would reproduce the values already held, so fields, delta and iteration counts
 * are bit-identical with tracking on or off.  Every iteration builds the work lists of its successor, which then runs as
 * a fixed-size launch of persistent waves over exactly those tiles.  Any upload, set_cells or mode change makes the next
 * two iterations run every tile.  bench.py times the kernel with tracking off. */
int epic_hip_set_activity_tracking(EpicHarmonicT *harmonic, int on);

/* Streamline extraction on the device-resident field (the path step that follows the relaxation).
 * The reference copies the whole field to the host for every request (src/epic_navigation_node_harmonic.cpp:621-626) and
 * walks it with harmonic_compute_path_2d_cpu (libepic/src/harmonic/harmonic_path_cpu.cpp:154-221); these walk it in HBM,
 * one lane per start point, and return only the way-points -- bit-identical to the host walk on the same field.
 *   starts  n_paths (x, y) pairs in cell units;  k / rc  n_paths entries (rc: EPIC_SUCCESS, EPIC_ERROR_INVALID_LOCATION,
 *   EPIC_ERROR_INVALID_GRADIENT or EPIC_ERROR_INVALID_PATH per path, k = 0 unless EPIC_SUCCESS);
 *   paths   n_paths rows of 2 * maxLength floats, row i holding k[i] (x, y) pairs.  All pointers are host pointers.
 * The device mask treats the grid border as locked (harmonic.h:35-37 makes that a precondition of the solver). */
int epic_hip_compute_paths_2d_gpu(EpicHarmonicT *harmonic, unsigned int n_paths, const float *starts, float stepSize,
                                  float cdPrecision, unsigned int maxLength, unsigned int *k, int *rc, float *paths);
/* One path, with harmonic_compute_path_2d_cpu's contract: *path must be NULL, receives a new[] array of 2 * *k floats
 * (release with harmonic_free_path_cpu), the return value is the walk's code. */
int epic_hip_compute_path_2d_gpu(EpicHarmonicT *harmonic, float x, float y, float stepSize, float cdPrecision,
                                 unsigned int maxLength, unsigned int *k, float **path);

/* ---- 3-D fields: potential, gradient, streamlines and sparse edits ---------------------------------------------------
 * The reference relaxes n-D grids but consumes and edits only 2-D ones; these close the caller's loop for n == 3.
 * Axes: cell (x0, x1, x2) of m = {m0, m1, m2} sits at u[(x0 * m1 + x1) * m2 + x2].  A point is (x, y, z) in cell units, x along
 * m[2] (columns), y along m[1] (rows), z along m[0] (planes): the 2-D convention (x along m[1], y along m[0]) with z added as
 * the slowest axis.  Way-points and cell lists are (x, y, z) triples in this order.
 * The rule is the reference's 2-D one (libepic/src/harmonic/harmonic_path_cpu.cpp:41-232) generalised operation by operation,
 * the third axis always the last operand: trilinear = (1 - gamma) * front + gamma * back with front / back the 2-D bilinear on
 * planes z0 / z1; six samples at +-cdPrecision in the order x-, x+, y-, y+, z-, z+; the norm and the stuck distance are
 * three-term sums in double, left to right.  A field that is constant along z, walked from an integer z with cdPrecision 0.5,
 * therefore reproduces harmonic_compute_path_2d_cpu bit for bit.  Codes and stderr texts are the 2-D ones under the new names;
 * a point that leaves the grid ends the walk.
 *   epic_hip_compute_path_3d_cpu  *path must be NULL, receives a new[] array of 3 * *k floats (release with harmonic_free_path_cpu).
 *   epic_hip_set_cells_3d_cpu     harmonic_utilities_set_cells_2d_cpu on k triples: same types, values, warnings and skipping.
 * EPIC_ERROR_INVALID_DATA: a null harmonic, m, u, locked or output pointer, n != 3, (set_cells) k == 0.
 * The _gpu calls work on the device-resident state of a 3-D Harmonic and have the contracts of their 2-D counterparts
 * (epic_hip_compute_paths_2d_gpu, epic_hip_compute_path_2d_gpu, harmonic_utilities_set_cells_2d_gpu): ordering points, host
 * pointers only, the same codes for the same failing steps.
 *   starts  n_paths (x, y, z) triples;  k / rc  n_paths entries (k = 0 unless rc is EPIC_SUCCESS);
 *   paths   n_paths rows of 3 * maxLength floats, row i holding k[i] triples -- bit-identical to epic_hip_compute_path_3d_cpu on
 *           the same field.
 * Border rule: the device mask treats every face of the grid as locked (a precondition of the solver), so a device walk ends on a
 * face cell and epic_hip_set_cells_3d_gpu leaves a face cell locked whatever type it is given (its value is still written).
 * Duplicate cells: the edits of one list are applied concurrently; a list must not name a cell twice (the result for that cell
 * would be either entry's).  Out-of-area entries and invalid types are skipped, silently on the device.
 * epic_hip_set_cells_3d_gpu edits the device state only (the current u buffer and the masks), synchronises, and makes the next two
 * iterations of a tracked relaxation run every tile.
 * Multi-device mode (EPIC_HIP_DEVICES): plane-slab versions are not built.  All three _gpu calls return EPIC_ERROR_INVALID_DATA
 * with a message naming the host route: harmonic_get_potential_values_gpu + epic_hip_compute_path_3d_cpu for paths,
 * epic_hip_set_cells_3d_cpu + harmonic_update_model_gpu for edits. */
int epic_hip_compute_potential_3d_cpu(EpicHarmonicT *h, float x, float y, float z, float *potential);
int epic_hip_compute_gradient_3d_cpu(EpicHarmonicT *h, float x, float y, float z, float cdPrecision, float *gx, float *gy,
                                     float *gz);
int epic_hip_compute_path_3d_cpu(EpicHarmonicT *h, float x, float y, float z, float stepSize, float cdPrecision,
                                 unsigned int maxLength, unsigned int *k, float **path);
int epic_hip_set_cells_3d_cpu(EpicHarmonicT *h, unsigned int k, const unsigned int *v, const unsigned int *types);
int epic_hip_compute_paths_3d_gpu(EpicHarmonicT *h, unsigned int n_paths, const float *starts, float stepSize, float cdPrecision,
                                  unsigned int maxLength, unsigned int *k, int *rc, float *paths);
int epic_hip_compute_path_3d_gpu(EpicHarmonicT *h, float x, float y, float z, float stepSize, float cdPrecision,
                                 unsigned int maxLength, unsigned int *k, float **path);
int epic_hip_set_cells_3d_gpu(EpicHarmonicT *h, unsigned int k, const unsigned int *v, const unsigned int *types);

/* ---- dense occupancy-grid ingestion (2-D) -------------------------------------------------------------------------
 * A map message applied where the state lives.  The reference's callers expand a message into a list of (x, y) pairs and a
 * list of types with one entry per interior cell and hand both to harmonic_utilities_set_cells_2d_cpu / _gpu
 * (src/epic_navigation_node_harmonic.cpp:383-426 subOccupancyGrid, :582-611 srvResetFreeCells; src/epic_nav_core_plugin.cpp:139-164
 * setCellsFromCostmap): 12 bytes per cell over the bus for a message of 1.  These take the message's bytes.
 *   occ   host pointer to m[0] x m[1] bytes, row-major and unpitched: msg->data / costmap->getCharMap().
 * For every INTERIOR cell (1 <= y <= m[0] - 2, 1 <= x <= m[1] - 2), with v = the cell's byte widened to int (signed char;
 * unsigned char with EPIC_HIP_OCC_UNSIGNED), in this order:
 *   1. v == no_change: the cell is untouched (a no_change outside the byte's range switches the test off);
 *   2. the cell is a goal (locked and u == 0.0f) and EPIC_HIP_OCC_OVER_GOALS is not set: untouched;
 *   3. v >= obstacle_threshold: u = EPIC_LOG_SPACE_OBSTACLE, locked;
 *   4. otherwise: unlocked, u = EPIC_LOG_SPACE_FREE -- except that with EPIC_HIP_OCC_KEEP_FREE a cell that was unlocked already
 *      keeps the value it has: a converged field survives a message that changed three cells (warm start).
 * Border cells are never touched.  flags 0, threshold 50, no_change -2 is subOccupancyGrid followed by setCells, cell for cell;
 * UNSIGNED | OVER_GOALS, threshold 250 and a no_change out of range is setCellsFromCostmap.
 *   *changed (may be NULL) receives the number of cells whose locked flag changed, or that stayed locked and changed their value
 *   (goal <-> obstacle).
 * The _cpu variants edit harmonic->u and harmonic->locked; the _gpu variants edit the device-resident state only (the current u
 * buffer and the masks; the goal test reads the device state) -- the split of the reference's set_cells pair: a node calls both.
 * The _gpu variants are ordering points like harmonic_utilities_set_cells_2d_gpu and synchronise.  With EPIC_HIP_OCC_KEEP_FREE
 * and *changed == 0 the resident state is bit for bit what it was and a tracked relaxation goes on undisturbed; every other call
 * makes the next two iterations run every tile.
 * epic_hip_reset_free_cells_2d_*: every unlocked interior cell back to EPIC_LOG_SPACE_FREE (srvResetFreeCells).
 * EPIC_ERROR_INVALID_DATA: a null harmonic, m, u, locked or occ, n != 2, (_gpu) no device state; HIP failures give the codes
 * harmonic_utilities_set_cells_2d_gpu gives for the same steps. */
#define EPIC_HIP_OCC_KEEP_FREE   1u  /* a cell that is unlocked before and free after keeps its potential (warm start) */
#define EPIC_HIP_OCC_UNSIGNED    2u  /* bytes are unsigned char (costmap_2d costs); default: signed char (nav_msgs/OccupancyGrid) */
#define EPIC_HIP_OCC_OVER_GOALS  4u  /* goal cells are overwritten like any other (the plugin's rule); default: goals are left alone (the node's rule) */
int epic_hip_set_occupancy_2d_cpu(EpicHarmonicT *h, const void *occ, int obstacle_threshold, int no_change,
                                  unsigned flags, unsigned long long *changed);
int epic_hip_set_occupancy_2d_gpu(EpicHarmonicT *h, const void *occ, int obstacle_threshold, int no_change,
                                  unsigned flags, unsigned long long *changed);
/* epic_hip_set_occupancy_2d_gpu bracketing its kernel with HIP events on the library's stream: *kernel_ms = the device time of
 * the ingestion kernel alone (not the copy of the image, not the rebuild of the fused masks; 0 in multi-device mode).  For
 * tools/bench_occupancy.py: the stream is the library's own, nothing outside can time a kernel on it. */
int epic_hip_timed_occupancy_2d_gpu(EpicHarmonicT *h, const void *occ, int obstacle_threshold, int no_change,
                                    unsigned flags, unsigned long long *changed, float *kernel_ms);
int epic_hip_reset_free_cells_2d_cpu(EpicHarmonicT *h);
int epic_hip_reset_free_cells_2d_gpu(EpicHarmonicT *h);

/* ---- dense occupancy ingestion into a region, 2-D and 3-D ----------------------------------------------------------
 * A costmap publishes rectangular updates, a depth sensor refreshes a box of voxels: these apply a block of bytes to a
 * rectangular region of a 2-D or 3-D field (harmonic->n is 2 or 3).  A whole voxel grid is the region "the grid".
 *   origin, extent   n entries each IN THE ORDER OF m, slowest axis first: {y0, x0} and {height, width} for n == 2 (m = {rows,
 *                    cols}); the indices along m[0], m[1], m[2] for n == 3 (cell (x0, x1, x2) at u[(x0 * m[1] + x1) * m[2] + x2]:
 *                    planes, rows, columns -- NOT the (x, y, z) order of the cell lists).  Both NULL: the whole grid.
 *   occ              host pointer to extent[0] * ... * extent[n - 1] bytes, row-major in the order of m and unpitched: the
 *                    `data` of a map_msgs/OccupancyGridUpdate as it comes, or a dense block of voxels.
 * The region must lie inside the grid: extent[i] >= 1 and origin[i] + extent[i] <= m[i] for every i (tested without overflow);
 * nothing is clipped.  The rule is the four-step rule of epic_hip_set_occupancy_2d_* above, with the same obstacle_threshold,
 * no_change and flags, applied to every cell of the region that is INTERIOR to the grid: not on the border in 2-D, not on any of
 * the six faces in 3-D.  Bytes that fall on border or face cells are ignored; cells outside the region are neither read nor
 * written.  *changed (may be NULL) counts what it counts there, over the region.
 * The _cpu variant edits harmonic->u and harmonic->locked.  The _gpu variant edits the device-resident state only and is an
 * ordering point with the sequence of epic_hip_set_occupancy_2d_gpu: pending iterations are flushed, only the region's bytes
 * cross the bus, the call synchronises, and the next two iterations run every tile -- unless EPIC_HIP_OCC_KEEP_FREE is set and
 * *changed == 0: then the resident state is bit for bit what it was.  With both pointers NULL on a 2-D field the result is that
 * of epic_hip_set_occupancy_2d_*.  epic_hip_timed_occupancy_region_gpu: the same call, *kernel_ms = the device time of the
 * ingestion kernel alone (0 in multi-device mode).
 * epic_hip_reset_free_cells_3d_*: every unlocked interior cell of a 3-D field back to EPIC_LOG_SPACE_FREE.
 * Multi-device mode (EPIC_HIP_DEVICES): a 2-D region takes the route of epic_hip_set_occupancy_2d_gpu there (the resident cells
 * are read back, the rule runs on the host over the window, the cells that change go through the sparse edit); results are
 * bit-identical to one device.  For n == 3 plane-slab edits are not built: epic_hip_set_occupancy_region_gpu, the timed call and
 * epic_hip_reset_free_cells_3d_gpu return EPIC_ERROR_INVALID_DATA with a message naming the host route,
 * epic_hip_set_occupancy_region_cpu (epic_hip_reset_free_cells_3d_cpu) followed by harmonic_update_model_gpu.
 * EPIC_ERROR_INVALID_DATA: a null harmonic, m, u, locked or occ; n not 2 or 3 (reset: n != 3); exactly one of origin and extent
 * NULL; a region that does not lie inside the grid; (_gpu) no device state; (timed) a null kernel_ms.  HIP failures give the
 * codes epic_hip_set_occupancy_2d_gpu gives for the same steps. */
int epic_hip_set_occupancy_region_cpu(EpicHarmonicT *h, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                      int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed);
int epic_hip_set_occupancy_region_gpu(EpicHarmonicT *h, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                      int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed);
int epic_hip_timed_occupancy_region_gpu(EpicHarmonicT *h, const void *occ, const unsigned int *origin, const unsigned int *extent,
                                        int obstacle_threshold, int no_change, unsigned flags, unsigned long long *changed,
                                        float *kernel_ms);
int epic_hip_reset_free_cells_3d_cpu(EpicHarmonicT *h);
int epic_hip_reset_free_cells_3d_gpu(EpicHarmonicT *h);

/* ---- Field queries: point samples, flow fields, cell read-back (2-D and 3-D) -----------------------------------------
 * Questions a caller asks of a relaxed field, answered where the field lives: harmonic->n is 2 or 3, and every call dispatches
 * on it.  The reference answers a request for one value by copying the whole field to the host
 * (src/epic_navigation_node_harmonic.cpp:522-542, srvGetCell -> harmonic_get_potential_values_gpu: 268 MB at 8192^2).
 *   points          n floats each, (x, y[, z]) in cell units, x along the LAST axis of m (the convention of the path functions);
 *   v               cell lists, n unsigned each in the same order, as for the set_cells calls;
 *   origin, extent  n entries each in the order of m, as for epic_hip_set_occupancy_region_*; both NULL: the whole grid.  The
 *                   region must lie inside the grid; nothing is clipped.
 * Per-item status, one unsigned char: */
#define EPIC_HIP_QUERY_OK                0  /* the value(s) are those of the host function */
#define EPIC_HIP_QUERY_INVALID_LOCATION  1  /* outside the grid, or an obstacle (locked with u < 0); outputs +0.0f */
#define EPIC_HIP_QUERY_INVALID_GRADIENT  2  /* one of the 2 n samples at +-cdPrecision is an invalid location; outputs +0.0f */
#define EPIC_HIP_QUERY_FLAT              3  /* the norm of the central differences is zero, NaN or infinite; outputs +0.0f */
#define EPIC_HIP_QUERY_DEVICE_OUT  1u  /* flags: the output pointers are device memory on the context's device */
/* The anchor is the existing host functions, bit for bit: harmonic_compute_potential_2d_cpu, harmonic_compute_gradient_2d_cpu,
 * epic_hip_compute_potential_3d_cpu, epic_hip_compute_gradient_3d_cpu.  Reads are clamped to the nearest cell and a coordinate
 * goes to an index through a 64-bit signed truncation whose low word is kept (NaN, +-inf and |x| >= 2^63, which have none, are
 * outside the grid), as the device walks do; the 2-D calls therefore differ from the reference's functions only where those read
 * outside their arrays.
 *   sample_potential  potential[i] and OK where the host function succeeds; INVALID_LOCATION and +0.0f where it returns
 *                     EPIC_ERROR_INVALID_LOCATION.
 *   sample_gradient   gradient holds n floats per point.  The point's own cell is not tested (the reference does not test it).
 *                     INVALID_GRADIENT and zeros where the host function returns that code; otherwise FLAT and zeros when the
 *                     norm (the same bits as the host's) is not a positive finite number -- !(norm > 0) || isinf(norm): the
 *                     reference returns success with 0 / 0 components there --; otherwise OK and the host function's bits.
 *   flow_field        for every cell of the region in row-major m order: the sample point is the cell's own index as floats
 *                     (where the potential function returns the cell's value).  A cell that is not usable (outside, or locked
 *                     with u < 0) gets INVALID_LOCATION and zeros; every other cell, goals included, gets what sample_gradient
 *                     gives at that point.  gradient: n floats per cell; status: one byte per cell.
 *   get_cells         value and lock state (0 / 1) of k cells as the device holds them.  The list is checked on the host first:
 *                     an entry outside the grid makes the call return EPIC_ERROR_INVALID_LOCATION with the outputs untouched.
 *   get_region        the same for a region, unpitched; either output may be NULL, not both.
 * status may be NULL in every call.  A call returns EPIC_SUCCESS when the batch ran, whatever the items' statuses; a count of 0 is
 * a success that touches nothing.  EPIC_ERROR_INVALID_DATA: a null harmonic, m or required pointer ((_cpu) u, locked), n not 2 or
 * 3, an invalid region, unknown flags, (_gpu) no device state or dimensions that are not the resident ones -- what
 * epic_hip_compute_paths_2d_gpu returns for a context that is not initialised.
 * The _cpu calls read harmonic->u / harmonic->locked.  The _gpu calls read the device-resident state and are ordering points like
 * the device walk: pending iterations are flushed, the kernel reads the current buffer on the library's stream, the call
 * synchronises before it returns and frees its temporaries on every path.  They write nothing to the field or the masks: no work
 * list is invalidated, and a tracked relaxation continues after a query with the bits and the iteration count of one that was never
 * queried.  All input pointers are host memory.
 * EPIC_HIP_QUERY_DEVICE_OUT (epic_hip_flow_field_gpu and epic_hip_get_region_gpu only): the output pointers are device memory on
 * the context's device (a torch tensor's data_ptr()); the kernels write straight into them, no temporary, no copy -- a whole-grid
 * flow field at 8192^2 is 537 MB + 67 MB, twice the field.  The call still synchronises the library's stream before it returns;
 * work of the caller's own streams on those buffers must have finished before the call.  EPIC_ERROR_INVALID_DATA in multi-device
 * mode and in the _cpu call.
 * Face cells: the device masks have every face cell of the grid locked, whatever harmonic->locked says.  Host and device agree
 * when the faces are locked obstacles in the host arrays -- what every caller of the reference and epic_amd.synthetic produce.
 * Multi-device mode (EPIC_HIP_DEVICES): all five _gpu calls read the owned units of every slab back (values and lock bits) and
 * answer from that snapshot with the host twin or a slice of it: results are bit-identical to one device, at the price of a whole
 * field over the bus per call.  Per-slab query kernels are not built. */
int epic_hip_sample_potential_cpu(EpicHarmonicT *h, unsigned int n_points, const float *points, float *potential,
                                  unsigned char *status);
int epic_hip_sample_potential_gpu(EpicHarmonicT *h, unsigned int n_points, const float *points, float *potential,
                                  unsigned char *status);
int epic_hip_sample_gradient_cpu(EpicHarmonicT *h, unsigned int n_points, const float *points, float cdPrecision, float *gradient,
                                 unsigned char *status);
int epic_hip_sample_gradient_gpu(EpicHarmonicT *h, unsigned int n_points, const float *points, float cdPrecision, float *gradient,
                                 unsigned char *status);
int epic_hip_flow_field_cpu(EpicHarmonicT *h, const unsigned int *origin, const unsigned int *extent, float cdPrecision,
                            unsigned flags, float *gradient, unsigned char *status);
int epic_hip_flow_field_gpu(EpicHarmonicT *h, const unsigned int *origin, const unsigned int *extent, float cdPrecision,
                            unsigned flags, float *gradient, unsigned char *status);
int epic_hip_get_cells_gpu(EpicHarmonicT *h, unsigned int k, const unsigned int *v, float *u_out, unsigned int *locked_out);
int epic_hip_get_region_gpu(EpicHarmonicT *h, const unsigned int *origin, const unsigned int *extent, unsigned flags, float *u_out,
                            unsigned int *locked_out);

/* Diagnostic: the number of tiles the next iteration will recompute and the number of tiles (both 0 when tracking is
 * off).  Synchronises the stream and copies the list counters to the host. */
int epic_hip_activity_stats(EpicHarmonicT *harmonic, unsigned long long *active_tiles, unsigned long long *tiles);
/* The same with a separate output for the tiles due in the next iteration (with work lists both outputs report that
 * number: the tiles a launch changed are the tiles it lists, apart from woken neighbours); due_tiles may be NULL. */
int epic_hip_activity_stats2(EpicHarmonicT *harmonic, unsigned long long *active_tiles, unsigned long long *due_tiles,
                             unsigned long long *tiles);

/* Work accounting: how many whole-grid iterations' worth of tiles the kernels have actually RUN since the last reset --
 * an iteration that runs every tile counts 1 (a fused pass over two iterations 2), a list-driven iteration of a tracked
 * run counts (tiles listed) / (tiles).  harmonic_execute_gpu resets it when it starts; reset != 0 resets it after reading.
 * currentIteration minus this number is what activity tracking skipped.  Synchronises the stream. */
int epic_hip_work_done(EpicHarmonicT *harmonic, double *grid_iterations, int reset);

/* Test hook: d_out[i] = (which & 1) ? ln(d_in[i]) : exp(d_in[i]) with the precise device routines; which & 2: in the form the red-black
 * kernels use (the first Horner addend kept in vector registers, cell_update.h: MathTab::consts) -- same operations, same bits. */
int epic_hip_eval_math(const float *d_in, float *d_out, size_t n, int which, void *stream);

/* ---- several GPUs behind the unchanged ABI ------------------------------------------------------------------------
 * EPIC_HIP_DEVICES=0,1,2,3 in the environment when a Harmonic's device state is created makes every harmonic_*_gpu entry
 * point work on ONE grid cut along its slowest axis into one slab per listed device (rows in 2-D, planes in 3-D), in this process: harmonic_complete_gpu(&h, 1024) --
 * the ROS plugin's only call, /root/reference/src/epic_nav_core_plugin.cpp:256 -- then uses the whole node.  The reference
 * has nothing like it (libepic/src/harmonic/harmonic_gpu.cu:168-201 drives one device).  A device may be listed more than
 * once ("0,0,0,0": four slabs on one GPU).  EPIC_HIP_HALO=G (default by slab height: 8 from 4096 rows per device up, 16 from
 * 2048, 32 below): ghost units per interior side, traded every G
 * iterations with hipMemcpyPeerAsync -- or, where peer access between two listed devices cannot be enabled (reported once on
 * stderr; EPIC_HIP_NO_PEER=1 forces it), through pinned host memory; results are bit-identical to the single-device path for
 * every list and every G.  One host thread per slab issues its launches (EPIC_HIP_THREADS=0: the calling thread does; between hand-overs a
 * thread spins for at most EPIC_HIP_SPIN_US microseconds, default 20, then sleeps: an idle Harmonic costs its host process nothing);
 * activity tracking works per slab.  Grids with fewer than 4 units per listed device and an unusable list fall back to one
 * device; path requests walk on the host in this mode.
 * epic_hip_device_layout: which device holds which units (rows of a 2-D grid, planes of a 3-D one) -- returns the number of slabs (1 in single-device mode) and
 * fills at most `cap` entries of each non-NULL array (owned rows [row_begin, row_end); ghost rows per interior side). */
int epic_hip_device_layout(EpicHarmonicT *harmonic, int cap, int *devices, unsigned int *row_begin, unsigned int *row_end,
                           unsigned int *ghost_rows);

/* Multi-device mode reporting on itself (the first run on real hardware cannot be rehearsed): one JSON object in buf -- per seam
 * the two devices, hipDeviceCanAccessPeer in both directions, the transport chosen (peer / staged / same-device), link type and
 * hops where the runtime reports them; then ONE exchange iteration under timing events: per slab the interior sweep (compute
 * stream) and the boundary bands + incoming halo copies (second stream), in microseconds from the earlier of the two starts,
 * the time both were running (overlap_us) and whether the copies ended before the interior did (copies_hidden).  Runs the iterations up to and including the next exchange (currentIteration advances).  Returns the
 * number of bytes written, 0 when the Harmonic is not in multi-device mode or buf is too small. */
int epic_hip_multi_report(EpicHarmonicT *harmonic, char *buf, size_t cap);

/* ---- configuration ---------------------------------------------------------------------------------------------------
 * The library reads its environment (the EPIC_HIP_* knobs of INTEGRATION.md section 6) ONCE per Harmonic, when the library-side
 * context of that Harmonic is created (the first harmonic_initialize_*_gpu), into one struct (epic_amd/csrc/driver_config.h);
 * nothing is read again behind the caller's back.  Two classes: PRODUCT knobs (EPIC_HIP_MATH, _SCHEME, _TRACK, _DEVICES with _HALO / _NO_PEER /
 * _THREADS / _SPIN_US, _TOL_FINISH, _DEFER) are always honoured; STUDY knobs (thresholds, task heights, tile plans, launch flags, the tuner: they
 * select a code path, never a result) are read only under EPIC_HIP_STUDY=1 -- one that is set without it is ignored and named once on stderr.
 * epic_hip_config_dump: one JSON object in buf -- "config": every knob as read then; "state": dimensions and the modes in force now
 * (epic_hip_set_* change them); "path": the kernel family a batch of plain iterations takes (LDS tiles / fused pairs / tracked
 * pairs / list-driven sweeps / single sweeps, replayed from a hipGraph or not), the tile plan, task heights, and in multi-device
 * mode the halo depth and the transport of every seam.  Returns the bytes written; 0 without a context or when buf is too small.
 * epic_hip_config_reload: re-reads the environment for this Harmonic's context (a knob that changed is applied; modes set through
 * epic_hip_set_* stay unless their variable changed; EPIC_HIP_DEVICES / EPIC_HIP_HALO are taken over when neither a field nor a
 * mask is resident, i.e. they shape the NEXT initialisation -- "state" of config_dump shows the slab layout in force) -- for a caller
 * that changes a variable on a live context (tests, bench.py).  It also refreshes the process-wide knobs: EPIC_HIP_FLAGS and
 * EPIC_HIP_LIST_WAVES are read by the 2-D launchers from those (speed only, never results), for every context of the process.
 * NULL: the process-wide knobs only (what the raw operators below go by). */
int epic_hip_config_dump(EpicHarmonicT *harmonic, char *buf, size_t cap);
int epic_hip_config_reload(EpicHarmonicT *harmonic);

/* Geometry of the device-resident state: pitch in floats, bytes of one u buffer, bytes of the packed mask. */
int epic_hip_get_layout(EpicHarmonicT *harmonic, unsigned int *pitch, size_t *u_bytes, size_t *mask_bytes);

/* ---- raw operators on caller-owned device memory (slab decomposition / multi-process drivers) ----------
 * 2-D grid of `rows` x `pitch` floats (pitch % 256 == 0, rows include any ghost rows); the mask is the private
 * bit layout produced by epic_hip_pack_mask_2d (epic_hip_mask_words_2d(rows, pitch) uint32 words, 1 bit per cell).
 * epic_hip_sweep_2d sweeps rows [row_begin, row_end) from d_in to d_out; if d_delta_bits != NULL the max |du|
 * of those rows is atomically max-ed into it as float bits (zero it first).  Asynchronous on `stream`. */
size_t epic_hip_mask_words_2d(unsigned int rows, unsigned int pitch);
unsigned int epic_hip_pitch_for_cols(unsigned int cols);
int epic_hip_pack_mask_2d(const uint32_t *d_locked, unsigned int rows, unsigned int cols, unsigned int pitch,
                          int ghost_top, int ghost_bottom, uint32_t *d_maskw, void *stream);
int epic_hip_sweep_2d(const float *d_in, float *d_out, const uint32_t *d_maskw, unsigned int rows,
                      unsigned int pitch, unsigned int row_begin, unsigned int row_end, unsigned int rows_per_task,
                      int math_mode, uint32_t *d_delta_bits, void *stream);
/* TWO Jacobi sweeps of the whole local grid in one pass (tol math only: math_mode 4): d_out receives what two calls of
 * epic_hip_sweep_2d over rows [0, rows) -- d_in -> tmp -> d_out -- would leave there, bit for bit, with the field moved
 * through HBM once.  No delta (check iterations run singly).  In a slab, two more ghost rows go stale.
 * rows_per_task = 0: the library's choice for this size. */
int epic_hip_sweep2_2d(const float *d_in, float *d_out, const uint32_t *d_maskw, unsigned int rows, unsigned int pitch,
                       unsigned int rows_per_task, int math_mode, void *stream);
/* The masks a second time, cut for the fused passes' lane -> column mapping (lane L of strip S holds columns 248 S + 4 L .. + 3; as
 * many strips as cover the row when the first strip owns its lane 0 and the last one the row's last quad): epic_hip_sweeps_2d takes
 * them as d_maskf and then skips a funnel shift of two mask words per row and wave (NULL: it shifts, as epic_hip_sweep2_2d,
 * which has no such parameter, always does -- a different instantiation of the pass: time and tune through the call you run).
 * epic_hip_mask_words_fused_2d(rows, pitch) uint32 words; derive after every epic_hip_pack_mask_2d. */
size_t epic_hip_mask_words_fused_2d(unsigned int rows, unsigned int pitch);
int epic_hip_fuse_masks_2d(const uint32_t *d_maskw, unsigned int rows, unsigned int pitch, uint32_t *d_maskf, void *stream);
/* `n` plain Jacobi sweeps of the whole local grid in ONE call (a driver in an interpreted language pays its per-call cost
 * once per stretch between two halo exchanges instead of once per launch): the field starts in d_a, the sweeps ping-pong
 * between d_a and d_b, *flips receives the PARITY of the number of buffer changes (1: the result is in d_b, 0: in d_a).  tol math (math_mode 4):
 * pairs of sweeps run as fused passes (rows_per_pair = 0: the library's choice), a last odd sweep singly; other modes: n single
 * sweeps.  Bit-identical to n calls of epic_hip_sweep_2d. */
int epic_hip_sweeps_2d(float *d_a, float *d_b, const uint32_t *d_maskw, const uint32_t *d_maskf, unsigned int rows,
                       unsigned int pitch, unsigned int n, unsigned int rows_per_task, unsigned int rows_per_pair, int math_mode,
                       int *flips, void *stream);
/* The same for the reference's red-black scheme: one in-place half-sweep of rows [row_begin, row_end) of d_u, updating
 * the unlocked cells with (local row + column + parity) odd (libepic/src/harmonic/harmonic_cpu.cpp:46-51 with
 * parity = currentIteration; a slab whose local row 0 is global row `top` passes (currentIteration + top) & 1). */
int epic_hip_sweep_rb_2d(float *d_u, const uint32_t *d_maskw, unsigned int rows, unsigned int pitch, unsigned int row_begin,
                         unsigned int row_end, unsigned int rows_per_task, int math_mode, int parity,
                         uint32_t *d_delta_bits, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EPIC_HIP_H */
