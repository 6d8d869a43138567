"""altro_amd -- MI355X-native ALTRO iLQR inner loop.

The product is the C-ABI shared library (include/altro_hip/altro_hip.h, built from altro_amd/csrc by
`python -m altro_amd.build`).  This module is only the ctypes binding a Python caller would write:
it holds no arithmetic and no CPU fallback -- if the library or a HIP device is missing, calls fail.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libaltro_hip.so")

F64, F32 = 0, 1
PLAN_AUTO, PLAN_GENERIC, PLAN_MFMA16, PLAN_LANE, PLAN_MFMA32 = 0, 1, 2, 3, 4
STORE_QBLOCKS = 0x1
LANE_FUSED = 0x4   # plan LANE: FMA-fused TVLQR kernels (not bit-identical to the CPU path, ~20 % faster at small batch)
F32_PURE = 0x2   # ALTRO_HIP_F32 on plan MFMA16: backward sweep in pure fp32 (v_mfma_f32_16x16x4_f32)
TILE_USER_BLOCKS = 0x2   # fp64 on plan MFMA16: a source with the constraint pair is accepted and the handle stays on the tile (F32_PURE's bit: that one is fp32's)
GENERIC_MATRIX_CORES = 0x8  # plan GENERIC, fp64: the backward sweep's products on the matrix cores (equal to rounding, not bit for bit)
TVLQR_SUCCESS = -1

# every symbol include/altro_hip/altro_hip.h declares (tests check the .so exports all of them)
C_ABI_SYMBOLS = [
    "altro_hip_version", "altro_hip_last_error", "altro_hip_device_count", "altro_hip_device_info", "altro_hip_device_pci_bus_id",
    "altro_hip_batch_create", "altro_hip_batch_create_dims", "altro_hip_batch_destroy", "altro_hip_batch_plan",
    "altro_hip_batch_device_bytes", "altro_hip_set_dynamics", "altro_hip_set_dynamics_range", "altro_hip_get_dynamics_knot",
    "altro_hip_shift_dynamics", "altro_hip_shift_linear_costs", "altro_hip_set_cost",
    "altro_hip_set_initial_state", "altro_hip_set_host_batch", "altro_hip_backward", "altro_hip_backward_per_problem", "altro_hip_forward_ltv", "altro_hip_sweep",
    "altro_hip_synchronize", "altro_hip_get_K", "altro_hip_get_d", "altro_hip_get_P",
    "altro_hip_get_p", "altro_hip_get_x", "altro_hip_get_u", "altro_hip_get_y",
    "altro_hip_get_delta_V", "altro_hip_get_status", "altro_hip_get_qblocks",
    "altro_hip_stats_reduce", "altro_hip_comm_unique_id", "altro_hip_comm_create", "altro_hip_comm_create_all",
    "altro_hip_comm_destroy", "altro_hip_comm_rank", "altro_hip_comm_world", "altro_hip_comm_device", "altro_hip_stats_allreduce", "altro_hip_stats_allreduce_multi",
    "altro_hip_profile_enable", "altro_hip_profile_reset",
    "altro_hip_profile_get", "altro_hip_profile_get_range", "altro_hip_profile_dropped", "altro_hip_sweep_variant", "altro_hip_algorithmic_bytes",
    "altro_hip_set_model", "altro_hip_set_model_source", "altro_hip_set_model_source_params", "altro_hip_set_model_params", "altro_hip_get_model_params",
    "altro_hip_model_num_params", "altro_hip_set_time_steps", "altro_hip_get_time_steps", "altro_hip_model_row_layout", "altro_hip_set_tracking_cost", "altro_hip_set_quadratic_cost",
    "altro_hip_set_input_guess", "altro_hip_set_state_guess",
    "altro_hip_open_loop_rollout", "altro_hip_accept", "altro_hip_expand", "altro_hip_merit", "altro_hip_merit_affine",
    "altro_hip_stationarity", "altro_hip_get_nominal", "altro_hip_get_expansion",
    "altro_hip_default_solve_options", "altro_hip_set_forms", "altro_hip_get_forms", "altro_hip_ilqr_solve", "altro_hip_last_solve_counts",
    "altro_hip_ilqr_solve_async", "altro_hip_ilqr_poll", "altro_hip_ilqr_wait",
    "altro_hip_linesearch_host",
    "altro_hip_add_linear_constraint", "altro_hip_add_user_constraint", "altro_hip_clear_constraints", "altro_hip_reset_duals",
    "altro_hip_get_duals", "altro_hip_set_duals", "altro_hip_get_penalty", "altro_hip_set_penalty", "altro_hip_shift_duals", "altro_hip_feasibility",
    "altro_hip_add_linear_constraint_rhs", "altro_hip_set_constraint_rhs", "altro_hip_get_constraint_rhs", "altro_hip_shift_constraint_rhs",
    "altro_hip_shift_trajectory", "altro_hip_update_linear_costs", "altro_hip_get_knot",
    "altro_hip_set_pointer_mode",
]
CONE_EQUALITY, CONE_IDENTITY, CONE_INEQUALITY, CONE_SOC = 0, 1, 2, 3   # ConstraintType, typedefs.hpp:29-34

# altro_hip_solve_options::forms / altro_hip_set_forms (ALTRO_HIP_FORM_*): how a solve is executed.  The C library reads no environment
# for these any more (version 300); THIS binding still translates the variables the test-suite and the tools set (forms_from_env), so
# that one process can alternate forms between calls.
RHS_PER_PROBLEM, RHS_PER_KNOT = 1, 2     # altro_hip_add_linear_constraint_rhs: how g is laid out, [nb][nk][p]
DUAL_TAIL_KEEP, DUAL_TAIL_ZERO = 0, 1   # Batch.shift_duals: what the last knot point of a block's range becomes
FORM_NO_SPECULATION, FORM_NO_RUNAHEAD, FORM_NO_MERIT2, FORM_MERIT_LDS, FORM_MERIT_DPP_ALWAYS = 0x1, 0x2, 0x4, 0x8, 0x10
FORM_EXPAND_LDS, FORM_ALROWS_LDS, FORM_ROLLOUT_ROUNDS, FORM_SEQUENCED, FORM_MERIT_ONE_LAUNCH = 0x20, 0x40, 0x80, 0x100, 0x200
FORM_LANE_QUAD_OFF, FORM_LANE_QUAD_ON, FORM_GENERIC_LATE_Q_OFF, FORM_GENERIC_LATE_Q_ON, FORM_FUSED_CLOCK = 0x400, 0x800, 0x1000, 0x2000, 0x4000
FORM_AFFINE_EXACT = 0x8000
FORM_NO_COMPACTION = 0x10000
FORM_GENERIC_MERIT_LDS = 0x20000
FORM_FORWARD_WAVE = 0x40000
FORM_BACKWARD_WAVE = 0x80000
# altro_hip_sweep_variant (ALTRO_HIP_SWEEP_*): which instantiation of plan GENERIC's sweep kernels the last launch was
SWEEP_LATE_Q, SWEEP_GLOBAL_WORKSPACE, SWEEP_MATRIX_CORES, SWEEP_FORWARD_STAGED = 0x1, 0x2, 0x4, 0x8
SWEEP_GROUP = 0x10   # plan MFMA16, slot 0: the backward sweep ran one workgroup per 16 problems


def forms_from_env():
    """The ALTRO_HIP_* comparison switches of the environment as ALTRO_HIP_FORM_* bits (what the library itself read up to version 200)."""
    e = os.environ
    off = lambda name: e.get(name) is not None and e[name].strip() not in ("",) and _atoi(e[name]) == 0
    f = 0
    if "ALTRO_HIP_NO_SPECULATION" in e: f |= FORM_NO_SPECULATION
    if "ALTRO_HIP_NO_RUNAHEAD" in e and not off("ALTRO_HIP_NO_RUNAHEAD"): f |= FORM_NO_RUNAHEAD
    if off("ALTRO_HIP_MERIT2"): f |= FORM_NO_MERIT2
    if off("ALTRO_HIP_MERIT_DPP"): f |= FORM_MERIT_LDS
    elif e.get("ALTRO_HIP_MERIT_DPP") is not None and _atoi(e["ALTRO_HIP_MERIT_DPP"]) == 2: f |= FORM_MERIT_DPP_ALWAYS
    if off("ALTRO_HIP_EXPAND_DPP"): f |= FORM_EXPAND_LDS
    if off("ALTRO_HIP_ALROWS_DPP"): f |= FORM_ALROWS_LDS
    if off("ALTRO_HIP_AFFINE"): f |= FORM_ROLLOUT_ROUNDS
    if off("ALTRO_HIP_FUSED") or "ALTRO_HIP_NO_FUSED" in e: f |= FORM_SEQUENCED
    if off("ALTRO_HIP_MERIT_SPLIT"): f |= FORM_MERIT_ONE_LAUNCH
    if "ALTRO_HIP_LANE_QUAD" in e: f |= FORM_LANE_QUAD_OFF if _atoi(e["ALTRO_HIP_LANE_QUAD"]) == 0 else FORM_LANE_QUAD_ON
    if "ALTRO_HIP_GENERIC_LATE_Q" in e: f |= FORM_GENERIC_LATE_Q_OFF if _atoi(e["ALTRO_HIP_GENERIC_LATE_Q"]) == 0 else FORM_GENERIC_LATE_Q_ON
    if "ALTRO_HIP_FUSED_CLOCK" in e: f |= FORM_FUSED_CLOCK
    if "ALTRO_HIP_AFFINE_EXACT" in e: f |= FORM_AFFINE_EXACT
    if "ALTRO_HIP_NO_COMPACTION" in e: f |= FORM_NO_COMPACTION
    return f


def _atoi(text):
    try:
        return int(text.strip() or 0)
    except ValueError:
        return 0

MODEL_LINEAR, MODEL_DOUBLE_INTEGRATOR, MODEL_PENDULUM, MODEL_BICYCLE, MODEL_USER, MODEL_QUADROTOR, MODEL_QUADROTOR13 = 0, 1, 2, 3, 4, 5, 6
MERIT_FN = C.CFUNCTYPE(None, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


class SolveOptions(C.Structure):
    _fields_ = [("iterations_max", C.c_int), ("tol_stationarity", C.c_double),
                ("tol_primal_feasibility", C.c_double), ("tol_meritfun_gradient", C.c_double),
                ("use_backtracking_linesearch", C.c_int), ("penalty_initial", C.c_double),
                ("penalty_scaling", C.c_double), ("penalty_max", C.c_double), ("reg_initial", C.c_double),
                ("reg_retry_max", C.c_int), ("reg_scale", C.c_double), ("reg_min", C.c_double),
                ("reg_max", C.c_double), ("stop_when_running_at_most", C.c_int),
                ("forms", C.c_uint), ("fused_sweeps", C.c_int), ("decision_margin", C.c_double)]   # version 300


class SolveResult(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("stationarity", C.c_double),
                ("final_alpha", C.c_double), ("final_phi", C.c_double), ("primal_feasibility", C.c_double),
                ("penalty", C.c_double), ("dual_updates", C.c_int), ("reg_retries", C.c_int)]


class PollRecord(C.Structure):
    """altro_hip_poll_record: one problem's results + first input, published by the solve kernel when the problem stops."""
    _fields_ = [("result", SolveResult), ("u0", C.c_double * 4), ("done", C.c_int), ("reserved", C.c_int)]


class AltroHipError(RuntimeError):
    pass


class Stats(C.Structure):
    """altro_hip_stats: what SolverImpl::Solve reports, reduced over a batch (and over GPUs)."""
    _fields_ = [("problems", C.c_int64), ("cholesky_failures", C.c_int64), ("converged", C.c_int64),
                ("iterations", C.c_int64), ("sum_cost", C.c_double),
                ("sum_delta_V0", C.c_double), ("sum_delta_V1", C.c_double),
                ("max_stationarity", C.c_double), ("max_feasibility", C.c_double), ("max_abs_xN", C.c_double),
                ("non_finite", C.c_int64)]
    SUM_FIELDS = ("problems", "cholesky_failures", "converged", "iterations", "sum_cost", "sum_delta_V0", "sum_delta_V1",
                  "non_finite")
    MAX_FIELDS = ("max_stationarity", "max_feasibility", "max_abs_xN")

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


COMM_ID_BYTES = 128


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64 with the same SONAME (libamdhip64.so.7) as /opt/rocm's.  Whichever
    copy a process loads first serves every later request for that SONAME -- but torch asks for it by file name, so a
    process that loaded the system copy through libaltro_hip.so and imports torch afterwards ends up with TWO HIP
    runtimes, and torch may then fail to find the GPU.  When torch is installed (it need not be imported), load its
    copy first so that this library and a later `import torch` share one runtime.  ALTRO_HIP_SYSTEM_RUNTIME=1 opts out."""
    import sys
    if "torch" in sys.modules or os.environ.get("ALTRO_HIP_SYSTEM_RUNTIME"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass


_lib = None


def lib():
    """Loads the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AltroHipError("%s is missing: run `python -m altro_amd.build` (hipcc, gfx950). "
                                "There is no CPU fallback." % LIB_PATH)
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.altro_hip_last_error.restype = C.c_char_p
        L.altro_hip_device_info.argtypes = [i, C.c_char_p, i, C.POINTER(i), C.POINTER(i)]
        L.altro_hip_device_pci_bus_id.argtypes = [i, C.c_char_p, i]
        L.altro_hip_batch_create.argtypes = [C.POINTER(vp), i, i, i, i, i, i, C.c_uint, i, vp]
        L.altro_hip_batch_create_dims.argtypes = [C.POINTER(vp), i, vp, vp, i, i, C.c_uint, i, vp]
        L.altro_hip_batch_destroy.argtypes = [vp]
        L.altro_hip_batch_destroy.restype = None
        L.altro_hip_batch_plan.argtypes = [vp]
        L.altro_hip_batch_device_bytes.argtypes = [vp]
        L.altro_hip_batch_device_bytes.restype = C.c_size_t
        L.altro_hip_set_dynamics.argtypes = [vp, vp, vp, vp, i, i]
        L.altro_hip_set_dynamics_range.argtypes = [vp, vp, vp, vp, i, i, i]
        L.altro_hip_get_dynamics_knot.argtypes = [vp, i, vp, vp, vp]
        L.altro_hip_shift_dynamics.argtypes = [vp]
        L.altro_hip_shift_linear_costs.argtypes = [vp]
        L.altro_hip_set_cost.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i]
        L.altro_hip_set_initial_state.argtypes = [vp, vp, i]
        L.altro_hip_set_host_batch.argtypes = [vp, i]
        L.altro_hip_backward.argtypes = [vp, d]
        L.altro_hip_backward_per_problem.argtypes = [vp, vp]
        L.altro_hip_forward_ltv.argtypes = [vp]
        L.altro_hip_sweep.argtypes = [vp, d]
        L.altro_hip_synchronize.argtypes = [vp]
        for g in ("K", "d", "P", "p", "x", "u", "y", "delta_V", "status", "qblocks"):
            getattr(L, "altro_hip_get_" + g).argtypes = [vp, vp]
        L.altro_hip_stats_reduce.argtypes = [vp, C.POINTER(Stats)]
        L.altro_hip_comm_unique_id.argtypes = [vp]
        L.altro_hip_comm_create.argtypes = [C.POINTER(vp), i, i, i, vp]
        L.altro_hip_comm_create_all.argtypes = [C.POINTER(vp), i, C.POINTER(i)]
        L.altro_hip_comm_destroy.argtypes = [vp]
        L.altro_hip_comm_destroy.restype = None
        for fn in ("rank", "world", "device"):
            getattr(L, "altro_hip_comm_" + fn).argtypes = [vp]
        L.altro_hip_stats_allreduce.argtypes = [vp, vp, C.POINTER(Stats)]
        L.altro_hip_stats_allreduce_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), i, C.POINTER(Stats)]
        L.altro_hip_profile_enable.argtypes = [vp, i]
        L.altro_hip_profile_reset.argtypes = [vp]
        L.altro_hip_profile_get.argtypes = [vp, i, C.POINTER(i), C.POINTER(d), C.POINTER(C.c_char_p)]
        L.altro_hip_profile_get_range.argtypes = [vp, i, C.POINTER(d), C.POINTER(d)]
        L.altro_hip_sweep_variant.argtypes = [vp, i, C.POINTER(i)]
        L.altro_hip_profile_dropped.argtypes = [vp, i]
        L.altro_hip_algorithmic_bytes.argtypes = [vp, i]
        L.altro_hip_algorithmic_bytes.restype = d
        L.altro_hip_set_model.argtypes = [vp, i, C.c_float, i, d, d]
        L.altro_hip_set_model_source.argtypes = [vp, C.c_char_p, C.c_float]
        L.altro_hip_set_model_source_params.argtypes = [vp, C.c_char_p, C.c_float, i]
        L.altro_hip_set_model_params.argtypes = [vp, vp, i]
        L.altro_hip_get_model_params.argtypes = [vp, vp]
        L.altro_hip_model_num_params.argtypes = [vp]
        L.altro_hip_set_time_steps.argtypes = [vp, vp]
        L.altro_hip_get_time_steps.argtypes = [vp, vp]
        L.altro_hip_model_row_layout.argtypes = [vp]
        L.altro_hip_set_tracking_cost.argtypes = [vp, vp, vp, vp, vp, i, i]
        L.altro_hip_set_quadratic_cost.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i]
        L.altro_hip_set_input_guess.argtypes = [vp, vp, i, i]
        L.altro_hip_set_state_guess.argtypes = [vp, vp, i, i]
        for fn in ("open_loop_rollout", "accept", "expand"):
            getattr(L, "altro_hip_" + fn).argtypes = [vp]
        L.altro_hip_merit.argtypes = [vp, vp, i, i, vp, vp]
        L.altro_hip_merit_affine.argtypes = [vp, vp, vp, i, vp, vp]
        L.altro_hip_stationarity.argtypes = [vp, vp]
        L.altro_hip_get_nominal.argtypes = [vp, vp, vp]
        L.altro_hip_get_expansion.argtypes = [vp, vp, vp, vp, vp]
        L.altro_hip_add_linear_constraint.argtypes = [vp, i, i, i, i, vp, vp, i]
        L.altro_hip_add_user_constraint.argtypes = [vp, i, i, i, i, i]
        L.altro_hip_clear_constraints.argtypes = [vp]
        L.altro_hip_reset_duals.argtypes = [vp, d]
        L.altro_hip_get_duals.argtypes = [vp, i, i, vp]
        L.altro_hip_set_duals.argtypes = [vp, i, i, vp]
        L.altro_hip_get_penalty.argtypes = [vp, vp]
        L.altro_hip_set_penalty.argtypes = [vp, vp, i]
        L.altro_hip_shift_duals.argtypes = [vp, i]
        L.altro_hip_add_linear_constraint_rhs.argtypes = [vp, i, i, i, i, vp, vp, i]
        L.altro_hip_set_constraint_rhs.argtypes = [vp, i, i, i, vp]
        L.altro_hip_get_constraint_rhs.argtypes = [vp, i, i, vp]
        L.altro_hip_shift_constraint_rhs.argtypes = [vp]
        L.altro_hip_feasibility.argtypes = [vp, vp]
        L.altro_hip_set_pointer_mode.argtypes = [vp, i]
        L.altro_hip_shift_trajectory.argtypes = [vp]
        L.altro_hip_update_linear_costs.argtypes = [vp, vp, vp, vp, i, i, i, i]
        L.altro_hip_get_knot.argtypes = [vp, i, vp, vp]
        L.altro_hip_default_solve_options.argtypes = [C.POINTER(SolveOptions)]
        L.altro_hip_default_solve_options.restype = None
        L.altro_hip_set_forms.argtypes = [vp, C.c_uint]
        L.altro_hip_get_forms.argtypes = [vp]
        L.altro_hip_get_forms.restype = C.c_uint
        L.altro_hip_ilqr_solve.argtypes = [vp, C.POINTER(SolveOptions), vp]
        L.altro_hip_last_solve_counts.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.altro_hip_ilqr_solve_async.argtypes = [vp, C.POINTER(SolveOptions)]
        L.altro_hip_ilqr_poll.argtypes = [vp, C.POINTER(i), C.POINTER(C.POINTER(PollRecord))]
        L.altro_hip_ilqr_wait.argtypes = [vp, vp]
        L.altro_hip_linesearch_host.argtypes = [MERIT_FN, vp, d, d, d, i, i, d, d, C.POINTER(i), C.POINTER(i),
                                                C.POINTER(d), C.POINTER(d)]
        L.altro_hip_linesearch_host.restype = d
        L.altro_hip_selftest_mfma_f64.argtypes = [i]
        L.altro_hip_selftest_mfma_f64.restype = d
        L.altro_hip_selftest_mfma_f32_4b.argtypes = [i]
        L.altro_hip_selftest_mfma_f32_4b.restype = d
        L.altro_hip_selftest_sincos.argtypes = [i, vp, i, vp, vp]
        L.altro_hip_selftest_sincos.restype = i
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise AltroHipError("altro_hip error %d: %s" % (rc, lib().altro_hip_last_error().decode()))


def device_info(device=0):
    """-> (name, compute units, PCI bus id) of a HIP device."""
    L = lib()
    name, pci = C.create_string_buffer(256), C.create_string_buffer(64)
    cus, ws = C.c_int(), C.c_int()
    _check(L.altro_hip_device_info(int(device), name, 256, C.byref(cus), C.byref(ws)))
    _check(L.altro_hip_device_pci_bus_id(int(device), pci, 64))
    return name.value.decode(), cus.value, pci.value.decode()


def _in(a):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


class Batch:
    """`batch` independent TVLQR / iLQR problems on one MI355X (mirror of the C handle)."""

    def __init__(self, N, n, m, batch, dtype=F64, plan=PLAN_AUTO, flags=0, device=0, stream=None):
        self.L = lib()
        self.N, self.n, self.m, self.batch = N, n, m, batch
        self._rhs_shape = {}   # block id -> (per problem, per knot, k_first, k_last, p): the shapes get_constraint_rhs returns
        self.h = C.c_void_p()
        _check(self.L.altro_hip_batch_create(C.byref(self.h), N, n, m, batch, dtype, plan, flags,
                                             device, stream))

    @property
    def plan(self):
        """The plan the handle runs NOW (a small-shape handle created with PLAN_AUTO moves from the padded tile to LANE when a LANE-only
        device model is set on it)."""
        return self.L.altro_hip_batch_plan(self.h)

    @classmethod
    def with_dims(cls, nx, nu, batch, dtype=F64, flags=0, device=0, stream=None):
        """altro_hip_batch_create_dims: per-knot-point dimensions nx[0..N], nu[0..N-1] (plan GENERIC: the TVLQR sweeps and the iLQR
        loop -- set_dynamics / set_quadratic_cost / set_initial_state / set_input_guess / add_linear_constraint / ilqr_solve ...).
        Bulk arrays are flat per problem, [batch, sum_k block_k]; `get` / `get_nominal` return them like that."""
        self = cls.__new__(cls)
        self.L = lib()
        self.nx = np.ascontiguousarray(nx, dtype=np.int32); self.nu = np.ascontiguousarray(nu, dtype=np.int32)
        self.N, self.n, self.m, self.batch = len(self.nu), int(self.nx.max()), int(self.nu.max()), batch
        self._rhs_shape = {}
        assert len(self.nx) == self.N + 1
        self.h = C.c_void_p()
        _check(self.L.altro_hip_batch_create_dims(C.byref(self.h), self.N, self.nx.ctypes.data_as(C.c_void_p),
                                                  self.nu.ctypes.data_as(C.c_void_p), batch, dtype, flags, device, stream))
        return self

    def _ragged_len(self, name):
        nx, nu, N = self.nx.astype(np.int64), self.nu.astype(np.int64), self.N
        return {"K": int((nu * nx[:N]).sum()), "d": int(nu.sum()), "P": int((nx * nx).sum()), "p": int(nx.sum()),
                "x": int(nx.sum()), "u": int(nu.sum()), "y": int(nx.sum())}[name]

    def set_pointer_mode(self, device_pointers):
        """device_pointers=True: the bulk arrays handed to the raw C entry points are device pointers (see
        altro_hip.h).  The numpy-based helpers of this class always pass host arrays; use `self.L` + `self.h` with
        your own device pointers (e.g. torch tensors' data_ptr()) while the mode is on."""
        _check(self.L.altro_hip_set_pointer_mode(self.h, int(bool(device_pointers))))
        self._device_pointers = bool(device_pointers)

    def _bulk(self, a):
        """One bulk array of a call that takes either kind: a numpy array (host; pointer mode off) or a torch device tensor (float64,
        contiguous; pointer mode on).  -> (the object to keep alive, its address).  The kind must match the handle's pointer mode: the
        library would read a host address on the device otherwise."""
        if a is None:
            return None, None
        dev = getattr(self, "_device_pointers", False)
        if hasattr(a, "data_ptr"):
            if not dev:
                raise ValueError("a device tensor needs set_pointer_mode(True)")
            if str(a.dtype) != "torch.float64" or not a.is_contiguous() or not a.is_cuda:
                raise ValueError("device tensors must be contiguous float64 tensors on the GPU")
            return a, C.c_void_p(a.data_ptr())
        if dev:
            raise ValueError("pointer mode is on: pass device tensors, or set_pointer_mode(False) first")
        return _in(a)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.altro_hip_batch_destroy(self.h)
            self.h = None

    __del__ = close

    def device_bytes(self):
        return self.L.altro_hip_batch_device_bytes(self.h)

    def set_dynamics(self, A, B, f=None, k_stride_zero=False, batch_stride_zero=False):
        (a, pa), (b, pb), (c, pc) = _in(A), _in(B), _in(f)
        _check(self.L.altro_hip_set_dynamics(self.h, pa, pb, pc, int(k_stride_zero), int(batch_stride_zero)))

    def set_dynamics_range(self, A, B, f, k_first, k_last, batch_stride_zero=False):
        """altro_hip_set_dynamics_range: set_dynamics for knot points k_first .. k_last (inclusive) only, everything else keeps its
        bits.  A [nb, nk, n*n], B [nb, nk, n*m], f [nb, nk, n] or None (zeros), column-major blocks, nk = k_last - k_first + 1, nb = 1
        with batch_stride_zero.  numpy arrays, or -- under set_pointer_mode(True) -- float64 torch device tensors read in place."""
        nb, nk = (1 if batch_stride_zero else self.batch), int(k_last) - int(k_first) + 1
        keep = [self._bulk(v) for v in (A, B, f)]
        for (a, _), blk in zip(keep, (self.n * self.n, self.n * self.m, self.n)):   # the C side reads nb * nk * block doubles
            if a is not None and nk > 0 and int(np.prod(a.shape)) != nb * nk * blk:
                raise ValueError("expected %d x %d x %d entries, got shape %s" % (nb, nk, blk, tuple(a.shape)))
        _check(self.L.altro_hip_set_dynamics_range(self.h, keep[0][1], keep[1][1], keep[2][1], int(k_first), int(k_last),
                                                   int(batch_stride_zero)))

    def get_dynamics_knot(self, k):
        """altro_hip_get_dynamics_knot: what the device holds at knot point k, as float64 numpy arrays A [batch, n*n], B [batch, n*m],
        f [batch, n] (column-major blocks, the tile's padding stripped), in either pointer mode."""
        A = np.zeros((self.batch, self.n * self.n)); B = np.zeros((self.batch, self.n * self.m)); f = np.zeros((self.batch, self.n))
        _check(self.L.altro_hip_get_dynamics_knot(self.h, int(k), *[v.ctypes.data_as(C.c_void_p) for v in (A, B, f)]))
        return A, B, f

    def shift_dynamics(self):
        """The dynamics' part of shift_trajectory (dynamics given as data): (A, B, f) of knot points 0 .. N-2 become those of k + 1,
        in place; N-1 keeps its values until set_dynamics_range(A, B, f, N-1, N-1) writes the new ones."""
        _check(self.L.altro_hip_shift_dynamics(self.h))

    def shift_linear_costs(self):
        """The companion of update_linear_costs for a reference that moves with the horizon: (q, r, c) of knot points 0 .. N-2 become
        those of k + 1, in place; N-1 and N keep theirs until update_linear_costs(q, None, c, N-1, N) and
        update_linear_costs(None, r, None, N-1, N-1) write the new ones."""
        _check(self.L.altro_hip_shift_linear_costs(self.h))

    def set_cost(self, Q, R, H, q, r, is_diag=False, k_stride_zero=False, batch_stride_zero=False):
        keep = [_in(v) for v in (Q, R, H, q, r)]
        _check(self.L.altro_hip_set_cost(self.h, *[k[1] for k in keep], int(is_diag),
                                         int(k_stride_zero), int(batch_stride_zero)))

    def set_host_batch(self, host_batch):
        _check(self.L.altro_hip_set_host_batch(self.h, int(host_batch)))

    def set_initial_state(self, x0, batch_stride_zero=False):
        a, pa = _in(x0)
        _check(self.L.altro_hip_set_initial_state(self.h, pa, int(batch_stride_zero)))

    def backward(self, reg=0.0):
        self._sync_forms()
        _check(self.L.altro_hip_backward(self.h, float(reg)))

    def backward_per_problem(self, reg):
        """altro_hip_backward_per_problem: the backward sweep with reg[b] added to problem b's Quu."""
        self._sync_forms()
        reg = np.ascontiguousarray(reg, dtype=np.float64)
        assert reg.shape == (self.batch,)
        _check(self.L.altro_hip_backward_per_problem(self.h, reg.ctypes.data))

    def forward_ltv(self):
        self._sync_forms()
        _check(self.L.altro_hip_forward_ltv(self.h))

    def sweep(self, reg=0.0):
        self._sync_forms()
        _check(self.L.altro_hip_sweep(self.h, float(reg)))

    def synchronize(self):
        _check(self.L.altro_hip_synchronize(self.h))

    def get(self, name):
        N, n, m, B = self.N, self.n, self.m, self.batch
        shape = {"K": (B, N, m * n), "d": (B, N, m), "P": (B, N + 1, n * n), "p": (B, N + 1, n),
                 "x": (B, N + 1, n), "u": (B, N, m), "y": (B, N + 1, n), "delta_V": (B, 2),
                 "qblocks": (B, N, n * n + m * m + m * n + n + m)}
        if name == "status":
            out = np.zeros(B, dtype=np.int32)
        elif getattr(self, "nx", None) is not None and name in ("K", "d", "P", "p", "x", "u", "y"):
            out = np.zeros((B, self._ragged_len(name)), dtype=np.float64)
        else:
            out = np.zeros(shape[name], dtype=np.float64)
        _check(getattr(self.L, "altro_hip_get_" + name)(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stats(self, comm=None):
        """This handle's statistics (device-side reduction); with a Comm, the global ones (two RCCL all-reduces)."""
        s = Stats()
        if comm is None:
            _check(self.L.altro_hip_stats_reduce(self.h, C.byref(s)))
        else:
            _check(self.L.altro_hip_stats_allreduce(self.h, comm.c, C.byref(s)))
        return s

    def profile(self, enable=True):
        """True / 1: hipEvents + a wait per launch; 2: events only (read by profile_get), for use inside a timed region."""
        _check(self.L.altro_hip_profile_enable(self.h, int(enable)))
        _check(self.L.altro_hip_profile_reset(self.h))

    def profile_range(self, slot):
        lo, hi = C.c_double(), C.c_double()
        _check(self.L.altro_hip_profile_get_range(self.h, slot, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def profile_dropped(self, slot):
        return self.L.altro_hip_profile_dropped(self.h, slot)

    def profile_get(self, slot):
        n, ms, name = C.c_int(), C.c_double(), C.c_char_p()
        _check(self.L.altro_hip_profile_get(self.h, slot, C.byref(n), C.byref(ms), C.byref(name)))
        return n.value, ms.value, name.value.decode()

    def sweep_variant(self, slot):
        """altro_hip_sweep_variant: SWEEP_* bits of the instantiation the last backward (slot 0) / forward (slot 1) launch was."""
        bits = C.c_int()
        _check(self.L.altro_hip_sweep_variant(self.h, slot, C.byref(bits)))
        return bits.value

    def algorithmic_bytes(self, slot):
        return self.L.altro_hip_algorithmic_bytes(self.h, slot)

    # ---- the iLQR loop around the sweep (device models; plan LANE shapes) ----
    def set_model(self, model, timestep, frame=0, length=2.7, lr=1.5):
        _check(self.L.altro_hip_set_model(self.h, model, float(timestep), frame, length, lr))

    def set_model_source(self, source, timestep, num_params=0):
        """The caller's own continuous dynamics + Jacobian as HIP source (altro_hip_set_model_source), compiled at run time.
        num_params > 0 (altro_hip_set_model_source_params): the source's functions take `const T* p`, that many per-problem
        parameters, which set_model_params must supply before anything steps the model."""
        if num_params == 0:
            _check(self.L.altro_hip_set_model_source(self.h, source.encode(), float(timestep)))
        else:
            _check(self.L.altro_hip_set_model_source_params(self.h, source.encode(), float(timestep), int(num_params)))

    def set_model_params(self, theta):
        """altro_hip_set_model_params: theta [batch, P] -- or [P], one set for every problem."""
        a = np.ascontiguousarray(theta, dtype=np.float64)
        P = self.model_num_params
        if P and a.shape not in ((self.batch, P), (P,)):   # (P = 0: the library says what is missing)
            raise ValueError("theta must have shape (%d, %d) or (%d,), got %s" % (self.batch, P, P, a.shape))
        _check(self.L.altro_hip_set_model_params(self.h, a.ctypes.data_as(C.c_void_p), int(a.ndim == 1)))

    def get_model_params(self):
        """The stored parameters, widened to float64: [batch, P]."""
        out = np.zeros((self.batch, self.model_num_params), dtype=np.float64)
        _check(self.L.altro_hip_get_model_params(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    @property
    def model_num_params(self):
        """Per-problem parameters the handle's model from source takes (0: none)."""
        return int(self.L.altro_hip_model_num_params(self.h))

    def set_time_steps(self, dt):
        """altro_hip_set_time_steps: dt[k] (N floats) = the step from knot point k to k + 1 of the handle's device model, shared by the
        batch (ALTROSolver::SetTimeStep per range); None: the uniform step of set_model / set_model_source again."""
        if dt is None:
            _check(self.L.altro_hip_set_time_steps(self.h, None))
            return
        a = np.ascontiguousarray(dt, dtype=np.float32)
        if a.shape != (self.N,):
            raise ValueError("dt must hold N = %d time steps, got shape %s" % (self.N, a.shape))
        _check(self.L.altro_hip_set_time_steps(self.h, a.ctypes.data_as(C.c_void_p)))

    def get_time_steps(self):
        """The N time steps in effect (float32; N copies of the uniform step without an array)."""
        out = np.zeros(self.N, dtype=np.float32)
        _check(self.L.altro_hip_get_time_steps(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_tracking_cost(self, Qd, Rd, xref, uref, k_stride_zero=False, batch_stride_zero=False):
        keep = [_in(v) for v in (Qd, Rd, xref, uref)]
        _check(self.L.altro_hip_set_tracking_cost(self.h, *[k[1] for k in keep], int(k_stride_zero),
                                                  int(batch_stride_zero)))

    def set_quadratic_cost(self, Q, R, H, q, r, c=None, k_stride_zero=False, batch_stride_zero=False):
        """ALTROSolver::SetQuadraticCost for the device iLQR loop: Q [.][N+1][n*n], R [.][N][m*m], H [.][N][m*n] column-major
        blocks, q [.][N+1][n], r [.][N][m], c [.][N+1] (None: zero); k_stride_zero: {running, terminal} / one knot point."""
        keep = [_in(v) for v in (Q, R, H, q, r)]
        kc = _in(c) if c is not None else (None, None)
        _check(self.L.altro_hip_set_quadratic_cost(self.h, *[k[1] for k in keep], kc[1], int(k_stride_zero),
                                                   int(batch_stride_zero)))

    def set_input_guess(self, u, k_stride_zero=False, batch_stride_zero=False):
        a, pa = _in(u)
        _check(self.L.altro_hip_set_input_guess(self.h, pa, int(k_stride_zero), int(batch_stride_zero)))

    def set_state_guess(self, x, k_stride_zero=False, batch_stride_zero=False):
        """ALTROSolver::SetState: x [.][N+1][n] into the candidate states."""
        a, pa = _in(x)
        _check(self.L.altro_hip_set_state_guess(self.h, pa, int(k_stride_zero), int(batch_stride_zero)))

    def open_loop_rollout(self):
        self._sync_forms()
        _check(self.L.altro_hip_open_loop_rollout(self.h))

    def accept(self):
        self._sync_forms()
        _check(self.L.altro_hip_accept(self.h))

    def expand(self):
        self._sync_forms()
        _check(self.L.altro_hip_expand(self.h))

    def model_row_layout(self):
        """Whether the handle's device model runs the row-layout model kernels (plans GENERIC / MFMA32; altro_hip_model_row_layout)."""
        self._sync_forms()
        return bool(self.L.altro_hip_model_row_layout(self.h))

    def merit(self, alpha, derivative=True):
        self._sync_forms()
        phi = np.zeros(self.batch); dphi = np.zeros(self.batch)
        if np.isscalar(alpha):
            a = np.array([float(alpha)]); uniform = 1
        else:
            a = np.ascontiguousarray(alpha, dtype=np.float64); uniform = 0
        _check(self.L.altro_hip_merit(self.h, a.ctypes.data_as(C.c_void_p), uniform, int(derivative),
                                      phi.ctypes.data_as(C.c_void_p), dphi.ctypes.data_as(C.c_void_p)))
        return phi, (dphi if derivative else None)

    def merit_affine(self, alpha, active=None, trials=1, out=None):
        """One affine line-search round (altro_hip_merit_affine): phi [trials, batch] ([batch] for trials = 1) and phi' [batch] at the
        steps alpha [batch]; trial 1 is alpha * 0.5.  active [batch]: the problems that take part (None: all).  out = (phi, dphi):
        float64 arrays of those shapes that are filled in place -- the entries of a problem that is masked out keep what they held
        (without `out` they are NaN)."""
        self._sync_forms()
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        if a.shape != (self.batch,):
            raise ValueError("alpha must have shape (batch,)")
        if out is None:
            out = (np.full((trials, self.batch) if trials > 1 else (self.batch,), np.nan), np.full(self.batch, np.nan))
        phi, dphi = out
        for v, n in ((phi, max(trials, 1) * self.batch), (dphi, self.batch)):
            if not (isinstance(v, np.ndarray) and v.dtype == np.float64 and v.flags.c_contiguous and v.size == n):
                raise ValueError("out = (phi, dphi): contiguous float64 arrays of trials * batch and batch entries")
        act = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, dtype=np.int32)
        if act is not None and act.shape != (self.batch,):
            raise ValueError("active must have shape (batch,)")
        _check(self.L.altro_hip_merit_affine(self.h, a.ctypes.data_as(C.c_void_p), None if act is None else act.ctypes.data_as(C.c_void_p),
                                             int(trials), phi.ctypes.data_as(C.c_void_p), dphi.ctypes.data_as(C.c_void_p)))
        return phi, dphi

    def stationarity(self):
        self._sync_forms()
        out = np.zeros(self.batch)
        _check(self.L.altro_hip_stationarity(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def get_nominal(self):
        if getattr(self, "nx", None) is not None:   # per-knot-point dimensions: packed [batch, sum nx], [batch, sum nu]
            x = np.zeros((self.batch, self._ragged_len("x"))); u = np.zeros((self.batch, self._ragged_len("u")))
        else:
            x = np.zeros((self.batch, self.N + 1, self.n)); u = np.zeros((self.batch, self.N, self.m))
        _check(self.L.altro_hip_get_nominal(self.h, x.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p)))
        return x, u

    def get_expansion(self):
        B, N, n, m = self.batch, self.N, self.n, self.m
        A = np.zeros((B, N, n * n)); Bm = np.zeros((B, N, n * m)); lx = np.zeros((B, N + 1, n)); lu = np.zeros((B, N, m))
        _check(self.L.altro_hip_get_expansion(self.h, *[v.ctypes.data_as(C.c_void_p) for v in (A, Bm, lx, lu)]))
        return A, Bm, lx, lu

    def shift_trajectory(self):
        _check(self.L.altro_hip_shift_trajectory(self.h))

    def update_linear_costs(self, q, r, c, k_first, k_last, k_stride_zero=False, batch_stride_zero=False):
        """q [nb, nk, n], r [nb, nk, m] or None, c [nb, nk] or None (nk = 1 / nb = 1 when the stride flags are set)."""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (q, r, c)]
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrs]
        _check(self.L.altro_hip_update_linear_costs(self.h, ptr[0], ptr[1], ptr[2], int(k_first), int(k_last),
                                                    int(k_stride_zero), int(batch_stride_zero)))

    def get_knot(self, k, want_u=True):
        nk = self.n if getattr(self, "nx", None) is None else int(self.nx[k])
        mk = self.m if getattr(self, "nx", None) is None or k >= self.N else int(self.nu[k])
        x = np.zeros((self.batch, nk))
        u = np.zeros((self.batch, mk)) if (want_u and k < self.N) else None
        _check(self.L.altro_hip_get_knot(self.h, int(k), x.ctypes.data_as(C.c_void_p),
                                         u.ctypes.data_as(C.c_void_p) if u is not None else None))
        return x, u

    def add_linear_constraint(self, k_first, k_last, cone, G, g, per_knot=False):
        """c = G [x;u] - g in `cone` at knot points k_first..k_last (inclusive).  G: (p, n+m) numpy (row-major
        here, sent column-major); g: (p,) shared by the batch or (batch, p) per problem.  With per_knot a right-hand side of its own
        at every knot point of the range, K = k_last - k_first + 1 of them: g is (K, p) or (batch, K, p)
        (altro_hip_add_linear_constraint_rhs; set_constraint_rhs / shift_constraint_rhs move them later).  Returns the block id."""
        G = np.asarray(G, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        Gc = np.ascontiguousarray(G.T)
        if per_knot:
            K = int(k_last) - int(k_first) + 1
            per_problem = int(g.ndim == 3)
            assert g.shape == ((self.batch, K, G.shape[0]) if per_problem else (K, G.shape[0])), "g is (K, p) or (batch, K, p)"
            rc = self.L.altro_hip_add_linear_constraint_rhs(self.h, int(k_first), int(k_last), int(cone), int(G.shape[0]),
                                                            Gc.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
                                                            RHS_PER_KNOT | (RHS_PER_PROBLEM if per_problem else 0))
            if rc < 0:
                _check(rc)
            self._rhs_shape[rc] = (per_problem, True, int(k_first), int(k_last), int(G.shape[0]))
            return rc
        per_problem = int(g.ndim == 2)
        if per_problem:
            assert g.shape == (self.batch, G.shape[0])
        rc = self.L.altro_hip_add_linear_constraint(self.h, int(k_first), int(k_last), int(cone), int(G.shape[0]),
                                                    Gc.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
                                                    per_problem)
        if rc < 0:
            _check(rc)
        self._rhs_shape[rc] = (per_problem, False, int(k_first), int(k_last), int(G.shape[0]))
        return rc

    def set_constraint_rhs(self, id, g, k_first=None, k_last=None):
        """New right-hand sides for block `id`, in place: duals, penalty and tables stay.  A per_knot block takes (K', p) or
        (batch, K', p) for knot points k_first..k_last inside its range (default: the whole range); any other linear block (p,) or
        (batch, p).  A host array here; under set_pointer_mode(True) pass the integer address of an fp64 device array of that layout."""
        kf, kl = (-1 if k_first is None else int(k_first)), (-1 if k_last is None else int(k_last))
        if g is None or isinstance(g, int):
            ptr = g
        else:
            g = np.ascontiguousarray(g, dtype=np.float64)
            if int(id) in self._rhs_shape:     # the C side reads nb * nk * p doubles: never past the end of a smaller array
                per_problem, per_knot, k0, k1, p = self._rhs_shape[int(id)]
                nk = (k1 - k0 + 1 if (kf, kl) == (-1, -1) else kl - kf + 1) if per_knot else 1
                want = ((self.batch,) if per_problem else ()) + ((nk,) if per_knot else ()) + (p,)
                assert nk < 1 or g.shape == want, "g is %s for this block and range, not %s" % (want, g.shape)
            ptr = g.ctypes.data_as(C.c_void_p)
        _check(self.L.altro_hip_set_constraint_rhs(self.h, int(id), kf, kl, ptr))

    def get_constraint_rhs(self, id, k):
        """What the device holds as block `id`'s right-hand side at knot point k: (p,), or (batch, p) for a per-problem block."""
        per_problem, _, _, _, p = self._rhs_shape.get(int(id), (0, False, 0, 0, 1))
        out = np.zeros((self.batch, p) if per_problem else (p,))
        _check(self.L.altro_hip_get_constraint_rhs(self.h, int(id), int(k), out.ctypes.data_as(C.c_void_p)))
        return out

    def shift_constraint_rhs(self):
        """The right-hand sides' part of shift_trajectory: every per_knot block's g moves one knot point forward; the last knot point
        of its range keeps its values until set_constraint_rhs(id, g, k_last, k_last) writes the new ones."""
        _check(self.L.altro_hip_shift_constraint_rhs(self.h))

    def add_user_constraint(self, k_first, k_last, cone, p, cid):
        """Block `cid` of the constraints the run-time compiled source defines (altro_hip_add_user_constraint)."""
        rc = self.L.altro_hip_add_user_constraint(self.h, int(k_first), int(k_last), int(cone), int(p), int(cid))
        if rc < 0:
            _check(rc)
        return rc

    def clear_constraints(self):
        _check(self.L.altro_hip_clear_constraints(self.h))
        self._rhs_shape.clear()

    def reset_duals(self, penalty=1.0):
        _check(self.L.altro_hip_reset_duals(self.h, float(penalty)))

    def get_duals(self, k, slot, p):
        out = np.zeros((self.batch, p))
        _check(self.L.altro_hip_get_duals(self.h, int(k), int(slot), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_duals(self, k, slot, z):
        """The inverse of get_duals: z [batch][p] becomes the duals of block `slot` of knot point k, as given (no projection)."""
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            assert z.ndim == 2 and z.shape[0] == self.batch, "z is [batch][p]"
        _check(self.L.altro_hip_set_duals(self.h, int(k), int(slot), None if z is None else z.ctypes.data_as(C.c_void_p)))

    def get_penalty(self):
        out = np.zeros(self.batch)
        _check(self.L.altro_hip_get_penalty(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_penalty(self, rho):
        """The constraints' penalty: a scalar for every problem, or [batch] values.  Duals are untouched."""
        rho = np.asarray(rho, dtype=np.float64)
        scalar = rho.ndim == 0
        assert scalar or rho.shape == (self.batch,), "rho is a scalar or [batch]"
        rho = np.ascontiguousarray(rho.reshape(-1))
        _check(self.L.altro_hip_set_penalty(self.h, rho.ctypes.data_as(C.c_void_p), int(scalar)))

    def shift_duals(self, tail=DUAL_TAIL_KEEP):
        """The duals' side of shift_trajectory: every block definition's duals move one knot point forward; the last knot point of
        a definition's range keeps its duals (DUAL_TAIL_KEEP) or gets zeros (DUAL_TAIL_ZERO)."""
        _check(self.L.altro_hip_shift_duals(self.h, int(tail)))

    def feasibility(self):
        self._sync_forms()
        out = np.zeros(self.batch)
        _check(self.L.altro_hip_feasibility(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def _solve_options(self, iterations_max=200, tol_stationarity=1e-4, tol_meritfun_gradient=1e-8,
                       use_backtracking=False, tol_primal_feasibility=1e-4, penalty_initial=1.0, penalty_scaling=10.0,
                       penalty_max=1e8, reg_initial=0.0, reg_retry_max=0, reg_scale=10.0, reg_min=1e-6, reg_max=1e8,
                       stop_when_running_at_most=0, forms=0, fused_sweeps=None, decision_margin=None):
        self._sync_forms()
        o = SolveOptions()
        self.L.altro_hip_default_solve_options(C.byref(o))
        o.forms = int(forms)
        if fused_sweeps is None and "ALTRO_HIP_FUSED_SWEEPS" in os.environ:
            fused_sweeps = _atoi(os.environ["ALTRO_HIP_FUSED_SWEEPS"]) or 1
        o.fused_sweeps = int(fused_sweeps or 0)
        if decision_margin is not None:
            o.decision_margin = float(decision_margin)
        o.tol_primal_feasibility = tol_primal_feasibility
        o.penalty_initial, o.penalty_scaling, o.penalty_max = penalty_initial, penalty_scaling, penalty_max
        o.reg_initial, o.reg_retry_max, o.reg_scale = reg_initial, reg_retry_max, reg_scale
        o.reg_min, o.reg_max = reg_min, reg_max
        o.stop_when_running_at_most = int(stop_when_running_at_most)
        o.iterations_max, o.tol_stationarity = iterations_max, tol_stationarity
        o.tol_meritfun_gradient, o.use_backtracking_linesearch = tol_meritfun_gradient, int(use_backtracking)
        return o

    def set_forms(self, forms):
        """altro_hip_set_forms: ALTRO_HIP_FORM_* bits every later call on this handle runs with (OR-ed with the environment's, see forms_from_env)."""
        self._forms_user = int(forms)
        self._sync_forms()

    def _sync_forms(self):
        want = getattr(self, "_forms_user", 0) | forms_from_env()
        if want != getattr(self, "_forms_set", 0):
            _check(self.L.altro_hip_set_forms(self.h, want))
            self._forms_set = want

    @staticmethod
    def _results(rec, sweeps, merit_launches):
        return dict(status=rec["status"].copy(), iterations=rec["iterations"].copy(),
                    stationarity=rec["stationarity"].copy(), alpha=rec["final_alpha"].copy(), phi=rec["final_phi"].copy(),
                    feasibility=rec["primal_feasibility"].copy(), penalty=rec["penalty"].copy(),
                    dual_updates=rec["dual_updates"].copy(), reg_retries=rec["reg_retries"].copy(),
                    sweeps=sweeps, merit_launches=merit_launches)

    def ilqr_solve(self, **options):
        o = self._solve_options(**options)
        res = (SolveResult * self.batch)()
        _check(self.L.altro_hip_ilqr_solve(self.h, C.byref(o), res))
        sw, ml = C.c_int(), C.c_int()
        self.L.altro_hip_last_solve_counts(self.h, C.byref(sw), C.byref(ml))
        rec = np.frombuffer(res, dtype=np.dtype(SolveResult))     # one view instead of 9 Python loops over the batch
        return self._results(rec, sw.value, ml.value)

    def ilqr_solve_async(self, **options):
        """Start the solve and return at once (altro_hip_ilqr_solve_async); follow with poll() / wait()."""
        o = self._solve_options(**options)
        _check(self.L.altro_hip_ilqr_solve_async(self.h, C.byref(o)))

    def poll(self):
        """(records published so far, numpy view [batch] of the pinned altro_hip_poll_record array -- fields result.*, u0, done)."""
        n, recs = C.c_int(), C.POINTER(PollRecord)()
        _check(self.L.altro_hip_ilqr_poll(self.h, C.byref(n), C.byref(recs)))
        buf = (PollRecord * self.batch).from_address(C.addressof(recs.contents))
        return n.value, np.frombuffer(buf, dtype=np.dtype(PollRecord))

    def wait(self):
        res = (SolveResult * self.batch)()
        _check(self.L.altro_hip_ilqr_wait(self.h, res))
        sw, ml = C.c_int(), C.c_int()
        self.L.altro_hip_last_solve_counts(self.h, C.byref(sw), C.byref(ml))
        return self._results(np.frombuffer(res, dtype=np.dtype(SolveResult)), sw.value, ml.value)


class Comm:
    """One RCCL communicator rank (altro_hip_comm).  `unique_id()` on rank 0, hand the 128 bytes to every rank by any
    channel (bench.py: a torch.distributed broadcast), then Comm(device, rank, world, id) on every rank."""

    @staticmethod
    def unique_id():
        buf = (C.c_char * COMM_ID_BYTES)()
        _check(lib().altro_hip_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    def __init__(self, device, rank, world, uid):
        self.L = lib()
        self.c = C.c_void_p()
        assert len(uid) == COMM_ID_BYTES
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(uid)
        _check(self.L.altro_hip_comm_create(C.byref(self.c), int(device), int(rank), int(world), C.cast(buf, C.c_void_p)))

    @property
    def rank(self):
        return self.L.altro_hip_comm_rank(self.c)

    @property
    def world(self):
        """Number of ranks (= GPUs) the communicator was built over: what a bench line reports as n_gpus."""
        return self.L.altro_hip_comm_world(self.c)

    def close(self):
        if getattr(self, "c", None) is not None and self.c:
            self.L.altro_hip_comm_destroy(self.c)
            self.c = None

    __del__ = close


def linesearch_host(fn, alpha0, phi0, dphi0, try_cubic_first=False, use_backtracking=False, c1=1e-4, c2=0.9):
    """Drives the batched solver's line-search state machine on the host with a Python merit callback."""
    L = lib()
    evals = []

    def cb(a, phi, dphi, ctx):
        p, dp = fn(a)
        evals.append(a)
        phi[0] = p
        if dphi:
            dphi[0] = dp

    st, it, ph, dph = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    alpha = L.altro_hip_linesearch_host(MERIT_FN(cb), None, alpha0, phi0, dphi0, int(try_cubic_first),
                                        int(use_backtracking), c1, c2, C.byref(st), C.byref(it),
                                        C.byref(ph), C.byref(dph))
    return dict(alpha=alpha, status=st.value, iters=it.value, phi=ph.value, dphi=dph.value, evals=evals)
