"""``Harmonic``: the solver object of the reference's python package (libepic/python/epic/harmonic.py:36-125),
bound to the MI355X-native library.

Same constructor defaults (epsilon 1e-2, stagger 100) and the same ``solve(algorithm, process, numThreads, epsilon)``
call sequence -- initialize x3 -> harmonic_complete_gpu -> uninitialize x3 (harmonic.py:67-92).  One deliberate
difference: the reference silently re-runs on the CPU when the GPU path fails (harmonic.py:76-86); here that is an
error unless the caller opts in with ``allow_cpu_fallback=True``, so a missing GPU can never masquerade as a GPU
result.
"""
import ctypes as ct
import time

import numpy as np

from . import epic_harmonic as eh


class Harmonic(eh.EpicHarmonic):
    """A log-space harmonic function over an n-D occupancy grid."""

    def __init__(self):
        self.n = 0
        self.m = ct.POINTER(ct.c_uint)()
        self.u = ct.POINTER(ct.c_float)()
        self.locked = ct.POINTER(ct.c_uint)()
        self.epsilon = 1e-2
        self.delta = self.epsilon + 1.0
        self.numIterationsToStaggerCheck = 100
        self.currentIteration = 0
        self.d_m = ct.POINTER(ct.c_uint)()
        self.d_u = ct.POINTER(ct.c_float)()
        self.d_locked = ct.POINTER(ct.c_uint)()
        self.d_delta = ct.POINTER(ct.c_float)()
        self._keep = {}

    # -- data ----------------------------------------------------------------------------------------------
    def set_grid(self, m, u, locked):
        """Attach host arrays (copied into numpy arrays this object keeps alive)."""
        m = np.ascontiguousarray(np.asarray(m, dtype=np.uint32))
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float32)).reshape(-1).copy()
        locked = np.ascontiguousarray(np.asarray(locked, dtype=np.uint32)).reshape(-1).copy()
        cells = int(np.prod(m.astype(np.int64)))
        if u.size != cells or locked.size != cells:
            raise ValueError("u and locked must have prod(m) = %d elements" % cells)
        self._keep = dict(m=m, u=u, locked=locked)
        self.n = len(m)
        self.m = m.ctypes.data_as(ct.POINTER(ct.c_uint))
        self.u = u.ctypes.data_as(ct.POINTER(ct.c_float))
        self.locked = locked.ctypes.data_as(ct.POINTER(ct.c_uint))

    @property
    def shape(self):
        return tuple(int(self.m[i]) for i in range(self.n))

    def u_array(self):
        """The host potential values as a numpy view of shape m."""
        if "u" in self._keep:
            return self._keep["u"].reshape(self.shape)
        cells = int(np.prod(self.shape))
        return np.ctypeslib.as_array(self.u, shape=(cells,)).reshape(self.shape)

    def locked_array(self):
        if "locked" in self._keep:
            return self._keep["locked"].reshape(self.shape)
        cells = int(np.prod(self.shape))
        return np.ctypeslib.as_array(self.locked, shape=(cells,)).reshape(self.shape)

    # -- solve ---------------------------------------------------------------------------------------------
    def solve(self, algorithm='gauss-seidel', process='gpu', numThreads=1024, epsilon=1e-2,
              allow_cpu_fallback=False):
        """Relax to ``epsilon``.  Returns (wall-time, cpu-time) of the solver call, excluding (un)initialisation,
        like the reference (harmonic.py:54-107).  ``process`` is 'gpu' (Jacobi sweeps on the MI355X) or 'cpu'
        (the exported red-black Gauss-Seidel)."""
        if algorithm != 'gauss-seidel':
            raise ValueError("the algorithm '%s' is undefined" % algorithm)
        self.epsilon = epsilon
        timing = None
        if process == 'gpu':
            result = eh._epic.harmonic_initialize_dimension_size_gpu(self)
            result += eh._epic.harmonic_initialize_potential_values_gpu(self)
            result += eh._epic.harmonic_initialize_locked_gpu(self)
            failed = result != 0
            if not failed:
                timing = (time.time(), time.process_time())
                result = eh._epic.harmonic_complete_gpu(self, int(numThreads))
                timing = (time.time() - timing[0], time.process_time() - timing[1])
                failed = result != 0
            # complete_gpu uninitialises on success; on failure (and for the re-entrant first set) do it here
            eh._epic.harmonic_uninitialize_dimension_size_gpu(self)
            eh._epic.harmonic_uninitialize_potential_values_gpu(self)
            eh._epic.harmonic_uninitialize_locked_gpu(self)
            eh._epic.harmonic_uninitialize_gpu(self)
            if failed:
                if not allow_cpu_fallback:
                    raise RuntimeError("epic_amd: the GPU solver failed with code %d and allow_cpu_fallback is off"
                                       % result)
                print("Failed to execute the 'epic' library's GPU solver; falling back to the CPU as requested.")
                process = 'cpu'
        if process == 'cpu':
            timing = (time.time(), time.process_time())
            result = eh._epic.harmonic_complete_cpu(self)
            timing = (time.time() - timing[0], time.process_time() - timing[1])
            if result != 0:
                raise RuntimeError("epic_amd: the CPU solver failed with code %d" % result)
        elif timing is None:
            raise ValueError("process must be 'gpu' or 'cpu'")
        return timing

    # -- map messages ---------------------------------------------------------------------------------------
    def set_occupancy(self, occ, obstacle_threshold=50, no_change=-2, keep_free=False, unsigned=False, over_goals=False,
                      process='gpu', origin=None):
        """Apply a map message (one byte per cell, shape m) by the rule of epic_hip_set_occupancy_2d_* (include/epic_hip.h):
        the defaults are the navigation node's /map callback; ``unsigned=True, over_goals=True, obstacle_threshold=250,
        no_change=-1`` is the nav_core plugin's costmap rule.  ``process``: 'cpu' edits the host arrays, 'gpu' the
        device-resident state, 'both' the host arrays and then the device state, as the node does.  ``keep_free``: cells
        that stay free keep their potential (warm start).  Returns ``changed`` (of the device call for 'both').

        The grid may be 2-D or 3-D.  ``origin`` (n entries in the order of m, slowest axis first) makes ``occ`` a window of
        a map or a box of voxels placed there, ``occ.shape`` being its extent (epic_hip_set_occupancy_region_*); the
        window must lie inside the grid."""
        if process not in ('gpu', 'cpu', 'both'):
            raise ValueError("process must be 'gpu', 'cpu' or 'both'")
        n = int(self.n)
        if n not in (2, 3):
            raise ValueError("map messages exist for 2-D and 3-D grids, not n = %d" % n)
        occ = np.ascontiguousarray(np.asarray(occ, dtype=np.uint8 if unsigned else np.int8))
        flags = ((eh.EPIC_HIP_OCC_KEEP_FREE if keep_free else 0) | (eh.EPIC_HIP_OCC_UNSIGNED if unsigned else 0)
                 | (eh.EPIC_HIP_OCC_OVER_GOALS if over_goals else 0))
        rule = (int(obstacle_threshold), int(no_change), flags)
        if origin is None:
            if occ.size != int(np.prod(self.shape)):
                raise ValueError("occ must have prod(m) = %d elements" % int(np.prod(self.shape)))
            if n == 2:
                variants = ((eh._epic.epic_hip_set_occupancy_2d_cpu, ()), (eh._epic.epic_hip_set_occupancy_2d_gpu, ()))
            else:
                variants = ((eh._epic.epic_hip_set_occupancy_region_cpu, (None, None)), (eh._epic.epic_hip_set_occupancy_region_gpu, (None, None)))
        else:
            origin = np.ascontiguousarray(np.asarray(origin, dtype=np.uint32)).reshape(-1)
            if occ.ndim != n or origin.size != n:
                raise ValueError("a window needs occ with %d axes and an origin of %d entries" % (n, n))
            extent = np.array(occ.shape, dtype=np.uint32)
            if np.any(extent < 1) or np.any(origin.astype(np.int64) + extent > np.array(self.shape, dtype=np.int64)):
                raise ValueError("the window must lie inside the grid")
            UP = ct.POINTER(ct.c_uint)
            window = (origin.ctypes.data_as(UP), extent.ctypes.data_as(UP))
            variants = ((eh._epic.epic_hip_set_occupancy_region_cpu, window), (eh._epic.epic_hip_set_occupancy_region_gpu, window))
        changed = ct.c_ulonglong(0)
        for (variant, where), wanted in zip(variants, (('cpu', 'both'), ('gpu', 'both'))):
            if process in wanted:
                rc = variant(self, occ.ctypes.data, *where, *rule, ct.byref(changed))
                if rc != 0:
                    raise RuntimeError("epic_amd: %s failed with code %d" % (variant.__name__, rc))
        return int(changed.value)

    def reset_free_cells(self, process='gpu'):
        """Every unlocked interior cell back to EPIC_LOG_SPACE_FREE (the node's reset_free_cells service), on a 2-D or a 3-D
        grid; ``process`` as in ``set_occupancy``."""
        if process not in ('gpu', 'cpu', 'both'):
            raise ValueError("process must be 'gpu', 'cpu' or 'both'")
        if int(self.n) == 3:
            variants = (eh._epic.epic_hip_reset_free_cells_3d_cpu, eh._epic.epic_hip_reset_free_cells_3d_gpu)
        else:
            variants = (eh._epic.epic_hip_reset_free_cells_2d_cpu, eh._epic.epic_hip_reset_free_cells_2d_gpu)
        for variant, wanted in ((variants[0], ('cpu', 'both')),
                                (variants[1], ('gpu', 'both'))):
            if process in wanted:
                rc = variant(self)
                if rc != 0:
                    raise RuntimeError("epic_amd: %s failed with code %d" % (variant.__name__, rc))

    # -- consumers and sparse edits, 2-D and 3-D ------------------------------------------------------------
    def compute_paths(self, starts, step_size, cd_precision, max_length, process='gpu'):
        """Streamlines from ``starts``, an (N, n) float32 array of points in cell units -- (x, y) for a 2-D grid, (x, y, z) for
        a 3-D one (x along the last axis of m; include/epic_hip.h).  ``process``: 'gpu' walks the device-resident field in one
        batched call (epic_hip_compute_paths_2d_gpu / _3d_gpu), 'cpu' walks the host arrays one start at a time
        (harmonic_compute_path_2d_cpu / epic_hip_compute_path_3d_cpu).  Returns ``(paths, codes)``: a list of N float32 arrays
        of shape (k_i, n) -- empty where the walk failed -- and an int32 array of the N per-path codes."""
        if process not in ('gpu', 'cpu'):
            raise ValueError("process must be 'gpu' or 'cpu'")
        n = int(self.n)
        if n not in (2, 3):
            raise ValueError("streamlines exist for 2-D and 3-D grids, not n = %d" % n)
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float32))
        if starts.ndim != 2 or starts.shape[1] != n:
            raise ValueError("starts must have shape (N, %d)" % n)
        count = starts.shape[0]
        codes = np.zeros(count, dtype=np.int32)
        if count == 0:
            return [], codes
        PF = ct.POINTER(ct.c_float)
        if process == 'gpu':
            batch = eh._epic.epic_hip_compute_paths_2d_gpu if n == 2 else eh._epic.epic_hip_compute_paths_3d_gpu
            points = (2 * int(max_length) & 0xffffffff) // 2      # the walk's own bound: an unsigned product
            k = np.zeros(count, dtype=np.uint32)
            out = np.empty((count, max(n * points, 1)), dtype=np.float32)
            rc = batch(self, count, starts.ctypes.data_as(PF), float(step_size), float(cd_precision), int(max_length),
                       k.ctypes.data_as(ct.POINTER(ct.c_uint)), codes.ctypes.data_as(ct.POINTER(ct.c_int)), out.ctypes.data_as(PF))
            if rc != 0:
                raise RuntimeError("epic_amd: %s failed with code %d" % (batch.__name__, rc))
            return [out[i, :n * int(k[i])].reshape(-1, n).copy() for i in range(count)], codes
        walk = eh._epic.harmonic_compute_path_2d_cpu if n == 2 else eh._epic.epic_hip_compute_path_3d_cpu
        paths = []
        for i in range(count):
            k, raw = ct.c_uint(0), PF()
            codes[i] = walk(self, *[float(c) for c in starts[i]], float(step_size), float(cd_precision), int(max_length),
                            ct.byref(k), ct.byref(raw))
            if codes[i] == 0:
                paths.append(np.ctypeslib.as_array(raw, shape=(n * k.value,)).reshape(-1, n).copy())
                eh._epic.harmonic_free_path_cpu(ct.byref(raw))
            else:
                paths.append(np.empty((0, n), dtype=np.float32))
        return paths, codes

    def set_cells(self, v, types, process='both', numThreads=1024):
        """Sparse edits: ``v`` is a (k, n) array of cells -- (x, y) or (x, y, z), x along the last axis of m -- and ``types`` k
        EPIC_CELL_TYPE_* values.  ``process`` as in ``set_occupancy``: 'cpu' edits the host arrays, 'gpu' the device-resident
        state, 'both' the host arrays and then the device state (harmonic_utilities_set_cells_2d_cpu / _gpu for a 2-D grid,
        epic_hip_set_cells_3d_cpu / _gpu for a 3-D one).  A list for the device must not name a cell twice."""
        if process not in ('gpu', 'cpu', 'both'):
            raise ValueError("process must be 'gpu', 'cpu' or 'both'")
        n = int(self.n)
        if n not in (2, 3):
            raise ValueError("sparse edits exist for 2-D and 3-D grids, not n = %d" % n)
        v = np.ascontiguousarray(np.asarray(v, dtype=np.uint32))
        types = np.ascontiguousarray(np.asarray(types, dtype=np.uint32)).reshape(-1)
        if v.ndim != 2 or v.shape[1] != n or v.shape[0] != types.size:
            raise ValueError("v must have shape (k, %d) and types k entries" % n)
        UP = ct.POINTER(ct.c_uint)
        args = (int(types.size), v.ctypes.data_as(UP), types.ctypes.data_as(UP))
        if n == 2:
            variants = ((eh._epic.harmonic_utilities_set_cells_2d_cpu, (self,) + args, ('cpu', 'both')),
                        (eh._epic.harmonic_utilities_set_cells_2d_gpu, (self, int(numThreads)) + args, ('gpu', 'both')))
        else:
            variants = ((eh._epic.epic_hip_set_cells_3d_cpu, (self,) + args, ('cpu', 'both')),
                        (eh._epic.epic_hip_set_cells_3d_gpu, (self,) + args, ('gpu', 'both')))
        for variant, call_args, wanted in variants:
            if process in wanted:
                rc = variant(*call_args)
                if rc != 0:
                    raise RuntimeError("epic_amd: %s failed with code %d" % (variant.__name__, rc))

    # -- queries of the field, 2-D and 3-D -------------------------------------------------------------------
    def _query_points(self, points):
        n = int(self.n)
        if n not in (2, 3):
            raise ValueError("field queries exist for 2-D and 3-D grids, not n = %d" % n)
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
        if points.ndim != 2 or points.shape[1] != n:
            raise ValueError("points must have shape (N, %d)" % n)
        return n, points

    def _query_region(self, origin, extent):
        """(origin pointer, extent pointer, shape, keep-alive) of a region given in the order of m; both None: the grid"""
        n = int(self.n)
        if n not in (2, 3):
            raise ValueError("field queries exist for 2-D and 3-D grids, not n = %d" % n)
        if origin is None and extent is None:
            return None, None, self.shape, ()
        if origin is None or extent is None:
            raise ValueError("origin and extent go together")
        origin = np.ascontiguousarray(np.asarray(origin, dtype=np.uint32)).reshape(-1)
        extent = np.ascontiguousarray(np.asarray(extent, dtype=np.uint32)).reshape(-1)
        if origin.size != n or extent.size != n:
            raise ValueError("origin and extent need %d entries each" % n)
        if np.any(extent < 1) or np.any(origin.astype(np.int64) + extent > np.array(self.shape, dtype=np.int64)):
            raise ValueError("the region must lie inside the grid")
        UP = ct.POINTER(ct.c_uint)
        return origin.ctypes.data_as(UP), extent.ctypes.data_as(UP), tuple(int(e) for e in extent), (origin, extent)

    @staticmethod
    def _device_out(tensor, shape, itemsize, what):
        """data_ptr() of a torch tensor that can take a device-side result of `shape` elements of `itemsize` bytes"""
        if tensor is None:
            return None
        if not tensor.is_cuda or not tensor.is_contiguous() or tuple(tensor.shape) != tuple(shape) or tensor.element_size() != itemsize:
            raise ValueError("%s must be a contiguous device tensor of shape %s with %d-byte elements" % (what, tuple(shape), itemsize))
        return tensor.data_ptr()

    def potential_at(self, points, process='gpu'):
        """The interpolated potential at ``points``, an (N, n) float32 array of (x, y[, z]) in cell units (x along the last
        axis of m): epic_hip_sample_potential_gpu on the device-resident field, or _cpu on the host arrays.  Returns
        ``(potential, status)``: N float32 and N uint8 (EPIC_HIP_QUERY_*; the potential is 0 where the status is not OK)."""
        if process not in ('gpu', 'cpu'):
            raise ValueError("process must be 'gpu' or 'cpu'")
        n, points = self._query_points(points)
        count = points.shape[0]
        potential = np.zeros(count, dtype=np.float32)
        status = np.zeros(count, dtype=np.uint8)
        call = eh._epic.epic_hip_sample_potential_gpu if process == 'gpu' else eh._epic.epic_hip_sample_potential_cpu
        rc = call(self, count, points.ctypes.data, potential.ctypes.data, status.ctypes.data)
        if rc != 0:
            raise RuntimeError("epic_amd: %s failed with code %d" % (call.__name__, rc))
        return potential, status

    def gradient_at(self, points, cd_precision, process='gpu'):
        """The normalised central-difference gradient at ``points`` (as in ``potential_at``): epic_hip_sample_gradient_*.
        Returns ``(gradient, status)``: (N, n) float32 and N uint8; the gradient is 0 where the status is not OK."""
        if process not in ('gpu', 'cpu'):
            raise ValueError("process must be 'gpu' or 'cpu'")
        n, points = self._query_points(points)
        count = points.shape[0]
        gradient = np.zeros((count, n), dtype=np.float32)
        status = np.zeros(count, dtype=np.uint8)
        call = eh._epic.epic_hip_sample_gradient_gpu if process == 'gpu' else eh._epic.epic_hip_sample_gradient_cpu
        rc = call(self, count, points.ctypes.data, float(cd_precision), gradient.ctypes.data, status.ctypes.data)
        if rc != 0:
            raise RuntimeError("epic_amd: %s failed with code %d" % (call.__name__, rc))
        return gradient, status

    def flow_field(self, cd_precision=0.5, origin=None, extent=None, process='gpu', out=None):
        """The gradient at every cell of a region (``origin`` / ``extent``: n entries in the order of m; both None: the grid):
        epic_hip_flow_field_*.  Returns ``(gradient, status)`` as numpy arrays of shape ``extent + (n,)`` (float32) and
        ``extent`` (uint8).  ``out=(gradient, status)`` -- torch tensors of those shapes on the context's device, float32 and
        uint8; ``status`` may be None -- makes the kernel write straight into them (EPIC_HIP_QUERY_DEVICE_OUT; 'gpu' only) and
        returns them; torch's current stream is synchronised before the call."""
        if process not in ('gpu', 'cpu'):
            raise ValueError("process must be 'gpu' or 'cpu'")
        o, e, shape, keep = self._query_region(origin, extent)
        n = int(self.n)
        if out is not None:
            if process != 'gpu':
                raise ValueError("out= needs process='gpu'")
            import torch

            g_out, s_out = out if isinstance(out, (tuple, list)) else (out, None)
            g_ptr = self._device_out(g_out, shape + (n,), 4, "out[0]")
            s_ptr = self._device_out(s_out, shape, 1, "out[1]")
            torch.cuda.current_stream(g_out.device).synchronize()
            rc = eh._epic.epic_hip_flow_field_gpu(self, o, e, float(cd_precision), eh.EPIC_HIP_QUERY_DEVICE_OUT, g_ptr, s_ptr)
            if rc != 0:
                raise RuntimeError("epic_amd: epic_hip_flow_field_gpu failed with code %d" % rc)
            return g_out, s_out
        gradient = np.zeros(shape + (n,), dtype=np.float32)
        status = np.zeros(shape, dtype=np.uint8)
        call = eh._epic.epic_hip_flow_field_gpu if process == 'gpu' else eh._epic.epic_hip_flow_field_cpu
        rc = call(self, o, e, float(cd_precision), 0, gradient.ctypes.data, status.ctypes.data)
        if rc != 0:
            raise RuntimeError("epic_amd: %s failed with code %d" % (call.__name__, rc))
        return gradient, status

    def get_cells(self, v):
        """Value and lock state of the cells ``v`` -- a (k, n) array of (x, y[, z]) as for ``set_cells`` -- as the device holds
        them (epic_hip_get_cells_gpu).  Returns ``(u, locked)``: k float32 and k uint32."""
        n = int(self.n)
        v = np.ascontiguousarray(np.asarray(v, dtype=np.uint32))
        if n not in (2, 3) or v.ndim != 2 or v.shape[1] != n:
            raise ValueError("v must have shape (k, n) on a 2-D or 3-D grid")
        u = np.zeros(v.shape[0], dtype=np.float32)
        locked = np.zeros(v.shape[0], dtype=np.uint32)
        rc = eh._epic.epic_hip_get_cells_gpu(self, v.shape[0], v.ctypes.data, u.ctypes.data, locked.ctypes.data)
        if rc != 0:
            raise RuntimeError("epic_amd: epic_hip_get_cells_gpu failed with code %d" % rc)
        return u, locked

    def get_region(self, origin=None, extent=None, out=None):
        """Values and lock states of a region of the device-resident field (epic_hip_get_region_gpu).  Returns ``(u, locked)``
        as numpy arrays of shape ``extent`` (float32, uint32).  ``out=(u, locked)`` -- torch device tensors of that shape,
        float32 and int32; either may be None -- makes the kernel write straight into them and returns them."""
        o, e, shape, keep = self._query_region(origin, extent)
        if out is not None:
            import torch

            u_out, l_out = out
            u_ptr = self._device_out(u_out, shape, 4, "out[0]")
            l_ptr = self._device_out(l_out, shape, 4, "out[1]")
            if u_ptr is None and l_ptr is None:
                raise ValueError("out= needs at least one tensor")
            torch.cuda.current_stream((u_out if u_out is not None else l_out).device).synchronize()
            rc = eh._epic.epic_hip_get_region_gpu(self, o, e, eh.EPIC_HIP_QUERY_DEVICE_OUT, u_ptr, l_ptr)
            if rc != 0:
                raise RuntimeError("epic_amd: epic_hip_get_region_gpu failed with code %d" % rc)
            return u_out, l_out
        u = np.zeros(shape, dtype=np.float32)
        locked = np.zeros(shape, dtype=np.uint32)
        rc = eh._epic.epic_hip_get_region_gpu(self, o, e, 0, u.ctypes.data, locked.ctypes.data)
        if rc != 0:
            raise RuntimeError("epic_amd: epic_hip_get_region_gpu failed with code %d" % rc)
        return u, locked

    def __str__(self):
        s = "n: %d\nm: %s\nepsilon: %g\ndelta: %g\nnumIterationsToStaggerCheck: %d\ncurrentIteration: %d\n" % (
            self.n, list(self.shape), self.epsilon, self.delta, self.numIterationsToStaggerCheck,
            self.currentIteration)
        return s
