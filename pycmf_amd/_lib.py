"""ctypes binding of libcmfhip.so (C ABI in include/cmfhip.h).

There is deliberately no CPU fallback: if the shared library has not been built
or no MI355X is visible, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcmfhip.so")

CMF_U, CMF_V, CMF_Z = 0, 1, 2
CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z = 1, 2, 4   # update_mask bits (include/cmfhip.h)
CMF_NN_U, CMF_NN_V, CMF_NN_Z = 1, 2, 4      # nn_mask bits
LINKS = {"linear": 0, "logit": 1}
RELATION_LOSSES = {"frobenius": 0, "logistic": 1}   # cmf_set_relation_loss (include/cmfhip.h)
UPD_U, UPD_V, UPD_Z = 1, 2, 4
K_GEMM_NN, K_GEMM_TN, K_GEMM_NT, K_ELEMWISE, K_EIGEN = 0, 1, 2, 3, 4
KERNEL_CLASSES = {"gemm_nn": 0, "gemm_tn": 1, "gemm_nt": 2, "elementwise": 3, "eigen": 4, "gemm_small": 5, "spmm": 6, "rowhess": 7, "gemm_pair": 8, "topk": 9, "klmu": 10}
# KERNEL_CLASSES mirrors the first enum of include/cmfhip.h, which is frozen at CMF_K_COUNT = 11 entries; the real bound of
# cmf_kernel_time is CMF_K_END.  Classes added since live in the header's second enum and HERE: the next one is added to this
# dict, not to KERNEL_CLASSES.  A caller that wants every class iterates both (tools/hals_timing.py).
LATER_KERNEL_CLASSES = {"hals": 11}

_ERR = {1: ValueError, 2: RuntimeError, 3: MemoryError, 4: RuntimeError, 5: NotImplementedError}

_i64, _i32, _dbl, _vp = C.c_int64, C.c_int, C.c_double, C.c_void_p
_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pi32 = C.POINTER(C.c_int32)
_pi64 = C.POINTER(C.c_int64)

# name -> (argtypes) ; every function returns int except cmf_last_error
PROTOTYPES = {
    "cmf_device_count": [C.POINTER(C.c_int)],
    "cmf_ctx_create": [C.POINTER(_vp), _i32, _vp],
    "cmf_ctx_destroy": [_vp],
    "cmf_sync": [_vp],
    "cmf_set_option": [_vp, C.c_char_p, _i64],
    "cmf_set_problem": [_vp, _i64, _i64, _i64, _i32],
    "cmf_set_data_f64": [_vp, _i32, _pd, _i64, _i64],
    "cmf_set_data_f32": [_vp, _i32, _pf, _i64, _i64],
    "cmf_set_data_csr": [_vp, _i32, _pi64, _pi32, _pd, _i64],
    "cmf_fill_data_synthetic": [_vp, _i32, C.c_uint64, _i64, _i64],
    "cmf_fill_factor_synthetic": [_vp, _i32, C.c_uint64, _i64, _dbl],
    "cmf_fill_data_synthetic_kind": [_vp, _i32, C.c_uint64, _i64, _i64, _i32, _dbl],
    "cmf_get_data_f32": [_vp, _i32, _pf, _i64, _i64],
    "cmf_data_layout": [_vp, _i32, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cmf_sparse_layout": [_vp, _i32, _pi64],
    "cmf_get_data_block_f32": [_vp, _i32, _i64, _i64, _i64, _i64, _pf],
    "cmf_sample_lists": [_vp, _i32, C.c_uint64, _dbl, _i64, _i64, _pi32],
    "cmf_newton_clamp_stats": [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), _i32],
    "cmf_newton_clamp_routes": [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "cmf_data_matmul_f64": [_vp, _i32, _i32, _pd, _i64, _i32, _pd],
    "cmf_rsvd": [_vp, _i32, _i32, _i32, _i32, _i32, _pd, _pd, _pd, _pd],
    "cmf_data_sum": [_vp, _pd, _pd],
    "cmf_data_block_sums_f64": [_vp, _i32, _i32, _pd],
    "cmf_set_factor_f64": [_vp, _i32, _pd, _i64, _i64],
    "cmf_get_factor_f64": [_vp, _i32, _pd, _i64, _i64],
    "cmf_mu_step": [_vp, _dbl, _dbl, _i32],
    "cmf_mu_step_error": [_vp, _dbl, _dbl, _i32, _pd, _pd],
    "cmf_mu_kl_step": [_vp, _dbl, _dbl, _i32],
    "cmf_kl_divergence": [_vp, _pd, _pd],
    "cmf_mu_kl_layout": [_vp, _pi64],
    "cmf_mu_beta_step": [_vp, _dbl, _dbl, _dbl, _i32],
    "cmf_beta_divergence": [_vp, _dbl, _pd, _pd],
    "cmf_mu_beta_products": [_vp, _dbl, _i32, _pf, _pf],
    "cmf_mu_beta_layout": [_vp, _pi64],
    "cmf_set_weight_f64": [_vp, _i32, _pd, _i64, _i64],
    "cmf_set_weight_f32": [_vp, _i32, _pf, _i64, _i64],
    "cmf_set_weighted_csr": [_vp, _i32, _pi64, _pi32, _pd, _pd],
    "cmf_clear_weight": [_vp, _i32],
    "cmf_mu_weighted_step": [_vp, _dbl, _dbl, _i32],
    "cmf_weighted_residual_sq": [_vp, _pd, _pd],
    "cmf_mu_weighted_layout": [_vp, _pi64],
    "cmf_fill_weight_synthetic": [_vp, _i32, C.c_uint64, _dbl],
    "cmf_get_weight_block_f32": [_vp, _i32, _i64, _i64, _i64, _i64, _pf],
    "cmf_hals_step": [_vp, _dbl, _dbl, _i32],
    "cmf_hals_sweep": [_vp, _i32, _pd, _pd, _dbl, _dbl],
    "cmf_als_step": [_vp, _dbl, _i32, _i32],
    "cmf_als_normal": [_vp, _i32, _i64, _i64, _dbl, _pf, _pf],
    "cmf_als_layout": [_vp, _pi64],
    "cmf_als_nnls_step": [_vp, _dbl, _i32, _i32, _i32],
    "cmf_als_nnls_rows": [_vp, _i64, _pf, _pf, _pf, _i32],
    "cmf_als_cg_step": [_vp, _dbl, _i32, _i32, _i32, _i32],
    "cmf_als_cg_rows": [_vp, _i32, _i64, _i64, _dbl, _i32, _pf],
    "cmf_als_cg_last": [_vp, _pi64],
    "cmf_als_nncg_step": [_vp, _dbl, _i32, _i32, _i32, _i32, _i32],
    "cmf_als_nncg_rows": [_vp, _i32, _i64, _i64, _dbl, _i32, _pf],
    "cmf_als_nncg_last": [_vp, _pi64],
    "cmf_als_nncg_passes": [_vp, _pi64],
    "cmf_als_dual_step": [_vp, _dbl, _i32, _i32, _i32, _i32, _i32],
    "cmf_als_dual_rows": [_vp, _i32, _i64, _i64, _dbl, _i32, _pf],
    "cmf_als_dual_last": [_vp, _pi64],
    "cmf_set_l2_rows": [_vp, _i32, _pd],
    "cmf_get_l2_rows": [_vp, _i32, _pd, C.POINTER(C.c_int)],
    "cmf_set_background_weight": [_vp, _i32, _dbl],
    "cmf_get_background_weight": [_vp, _i32, _pd],
    "cmf_als_residual_sq": [_vp, _pd, _pd],
    "cmf_set_biases": [_vp, _i32, _i32, _dbl, _dbl],
    "cmf_get_biases": [_vp, _i32, _pd, _pd, C.POINTER(C.c_int)],
    "cmf_set_bias_f64": [_vp, _i32, _i32, _pd],
    "cmf_get_bias_f64": [_vp, _i32, _i32, _pd],
    "cmf_als_bias_step": [_vp, _dbl, _i32, _i32, _i32, _i32],
    "cmf_als_bias_rows": [_vp, _i32, _i32, _pf],
    "cmf_als_bias_targets": [_vp, _i32, _i32, _i64, _pf, _pf],
    "cmf_predict_pairs": [_vp, _i32, _i32, _i64, _pi64, _pi64, _pf],
    "cmf_set_relation_loss": [_vp, _i32, _i32],
    "cmf_get_relation_loss": [_vp, _i32, C.POINTER(C.c_int)],
    "cmf_als_logistic_loss": [_vp, _pd, _pd],
    "cmf_set_huber_delta": [_vp, _i32, _dbl],
    "cmf_get_huber_delta": [_vp, _i32, _pd],
    "cmf_als_huber_loss": [_vp, _pd, _pd],
    "cmf_als_huber_weights": [_vp, _i32, _i32, _i64, _pf, _pf],
    "cmf_set_logit_pass": [_vp, _i32, _i32],
    "cmf_get_logit_pass": [_vp, _i32, C.POINTER(C.c_int)],
    "cmf_als_logit_weights": [_vp, _i32, _i32, _i64, _pf, _pf],
    "cmf_v_buf_elems": [_vp, _pi64],
    "cmf_data_pass_launches": [_vp, _pi64],
    "cmf_mu_route_launches": [_vp, _pi64],
    "cmf_mu_v_partials": [_vp, _vp],
    "cmf_mu_v_apply": [_vp, _vp, _dbl, _dbl],
    "cmf_mu_v_partials_rows": [_vp, _vp, _i64, _i64, _i32],
    "cmf_mu_uz_update": [_vp, _dbl, _dbl, _i32],
    "cmf_mu_blocked_layout": [_vp, _i32, _pi64, _pi64],
    "cmf_mu_v_partials_split": [_vp, _vp, _vp],
    "cmf_mu_v_apply_rows": [_vp, _vp, _vp, _i64, _i64, _dbl, _dbl],
    "cmf_mu_gram_v_rows": [_vp, _i64, _i64, _vp],
    "cmf_mu_uz_update_gram": [_vp, _vp, _dbl, _dbl, _i32],
    "cmf_newton_step": [_vp, _dbl, _dbl, _dbl, _i32, _i32, _i32, _i32, _dbl, _dbl,
                        _pi32, _pi32, _pi32, _pi32],
    "cmf_newton_step_device_sampled": [_vp, _dbl, _dbl, _dbl, _i32, _i32, _i32, _i32, _dbl, _dbl, C.c_uint64],
    "cmf_newton_uz_update": [_vp, _dbl, _dbl, _dbl, _i32, _i32, _dbl],
    "cmf_newton_v_partials": [_vp, _dbl, _vp],
    "cmf_newton_v_apply": [_vp, _vp, _dbl, _dbl, _i32, _dbl],
    "cmf_newton_v_gram": [_vp, _dbl, _vp],
    "cmf_newton_v_products": [_vp, _dbl, _dbl, _dbl, _vp, _vp],
    "cmf_newton_v_finish": [_vp, _vp, _dbl, _i32],
    "cmf_residual_sq": [_vp, _i32, _i32, _pd, _pd],
    "cmf_data_sq": [_vp, _pd, _pd],
    "cmf_topk": [_vp, _i32, _i32, _i32, _pi64, _i64, _i32, _pi64, _pi32, _pi32, _pf],
    "cmf_topk_queries": [_vp, _pd, _i64, _i64, _i64, _i32, _i32, _i32, _pi64, _pi32, _pi32, _pf],
    "cmf_topk_layout": [_vp, _i64, _i32, _i32, _i64, _i32, _pi64],
    "cmf_rank": [_vp, _i32, _i32, _pi64, _i64, _pi64, _pi32, _pi64, _pi32, _pi32, _pf, _pi32],
    "cmf_rank_queries": [_vp, _pd, _i64, _i64, _i64, _i32, _pi64, _pi32, _pi64, _pi32, _pi32, _pf, _pi32],
    "cmf_rank_layout": [_vp, _i64, _i32, _i64, _i64, _i32, _pi64],
    "cmf_safe_invert_batch": [_vp, _pd, _pd, _i32, _i32, _dbl],
    "cmf_safe_invert_f64": [_vp, _pd, _pd, _i32, _dbl],
    "cmf_safe_solve_batch": [_vp, _pd, _pd, _pd, _pd, _i32, _i32, _dbl, _i32],
    "cmf_debug_clock": [_vp, _pd, _pd],
    "cmf_kernel_timing": [_vp, _i32],
    "cmf_kernel_time": [_vp, _i32, _pd, _pi64, _pd],
    "cmf_kernel_timing_reset": [_vp],
    "cmf_rowhess_samples": [_vp, _pd, _pd],
    "cmf_marker": [_vp],
    "cmf_marker_times": [_vp, _pd, _i64, _pi64],
    "cmf_get_stream": [_vp, C.POINTER(_vp)],
    "cmf_get_geometry": [_vp, _pi64, _pi64, _pi64, C.POINTER(C.c_int)],
    "cmf_factor_dev_ptr": [_vp, _i32, C.POINTER(_pf)],
    "cmf_scratch_alloc": [_vp, _i64, C.POINTER(_vp)],
    "cmf_scratch_free": [_vp, _vp],
    "cmf_export_factor_rows": [_vp, _i32, _vp],
    "cmf_import_factor_rows": [_vp, _i32, _vp],
    "cmf_comm_unique_id": [C.c_char_p],
    "cmf_comm_init": [_vp, _i32, _i32, C.c_char_p],
    "cmf_comm_destroy": [_vp],
    "cmf_comm_info": [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cmf_comm_allreduce_f32": [_vp, _vp, _i64],
    "cmf_comm_allreduce_f64": [_vp, _vp, _i64],
    "cmf_comm_allreduce_f32_bg": [_vp, _vp, _i64],
    "cmf_comm_join": [_vp],
    "cmf_comm_exposed_ms": [_vp, _pd, _i32],
    "cmf_comm_allgather_f32": [_vp, _vp, _i64],
    "cmf_comm_reduce_scatter_f32": [_vp, _vp, _i64],
    "cmf_comm_group_start": [_vp],
    "cmf_comm_group_end": [_vp],
    "cmf_comm_launch_points": [_vp, _pi64],
    "cmf_scale_f32": [_vp, _vp, _i64, _dbl],
    "cmf_comm_count": [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "cmf_comm_stats_kind": [_vp, _i32, _pi64, _pi64, _pd],
    "cmf_comm_allreduce_host_f64": [_vp, _pd, _i32, _i32],
    "cmf_comm_barrier": [_vp],
    "cmf_comm_timing": [_vp, _i32],
    "cmf_comm_stats": [_vp, _pi64, _pi64, _pd, _i32],
    "cmf_copy_to_host": [_vp, _vp, _vp, _i64],
    "cmf_copy_from_host": [_vp, _vp, _vp, _i64],
}



class RunParams(C.Structure):
    """cmf_run_params of include/cmfhip.h"""
    _fields_ = [("solver", C.c_int), ("l1", C.c_double), ("l2", C.c_double), ("alpha", C.c_double), ("alpha_err", C.c_double),
                ("x_link", C.c_int), ("y_link", C.c_int), ("nn_mask", C.c_int), ("update_mask", C.c_int),
                ("hessian_pertubation", C.c_double), ("sg_ratio", C.c_double), ("seed", C.c_uint64)]


PROTOTYPES["cmf_run"] = [_vp, C.POINTER(RunParams), _i32, _dbl, _i32, C.POINTER(C.c_int), _pd, _pd, _i32, C.POINTER(C.c_int)]

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so and
    ask for it by its unversioned name, so if libcmfhip.so pulled in /opt/rocm's copy first, a
    later ``import torch`` would load a second runtime that finds no GPU.  When torch is
    installed (not necessarily imported) its bundled runtime is loaded first; libcmfhip's
    ``libamdhip64.so.7`` dependency then resolves to that same image."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libcmfhip.so (once) and attach prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "pycmf_amd: %s is missing -- build it with `python -m pycmf_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    lib.cmf_last_error.restype = C.c_char_p
    lib.cmf_last_error.argtypes = []
    # the library must have been compiled from the sources next to it (it is git-ignored and travels with the working tree)
    if os.environ.get("PYCMF_AMD_SKIP_HASH_CHECK") != "1" and os.path.isdir(os.path.join(_HERE, "csrc")):
        from . import build as _build
        try:
            lib.cmf_source_hash.restype = C.c_char_p
            lib.cmf_source_hash.argtypes = []
            have = lib.cmf_source_hash().decode()
        except AttributeError:
            have = "unstamped"
        want = _build.source_hash()
        if have != want:
            raise RuntimeError("pycmf_amd: %s was built from other sources than the ones in pycmf_amd/csrc and include/ "
                               "(library %s..., sources %s...): rebuild it with `python -m pycmf_amd.build`"
                               % (LIB_PATH, have[:12], want[:12]))
    for name, args in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().cmf_last_error().decode("utf-8", "replace")
        raise _ERR.get(rc, RuntimeError)("libcmfhip: " + msg)


def device_count():
    n = C.c_int(0)
    _touch()
    check(load().cmf_device_count(C.byref(n)))
    return n.value


def _strides(a):
    return a.strides[0] // a.itemsize, a.strides[1] // a.itemsize


class _Scratch:
    """Device scratch handed out by Context.scratch (freed with the context or by release())."""

    def __init__(self, ctx, ptr, nbytes):
        self._ctx, self._ptr, self.nbytes = ctx, ptr, nbytes

    def data_ptr(self):
        return self._ptr

    def release(self):
        if self._ptr and self._ctx._h:
            check(self._ctx._lib.cmf_scratch_free(self._ctx._h, _vp(self._ptr)))
        self._ptr = None


_gpu_touched = False     # set by the first call that initialises the HIP runtime in this process


def gpu_touched():
    """Has this process made a HIP call through pycmf_amd yet?  (multi_gpu forks its ranks off the caller's process only while
    the answer is no: a forked child must not inherit an initialised runtime.)"""
    return _gpu_touched


def _touch():
    global _gpu_touched
    _gpu_touched = True


class DeviceArray:
    """rows x cols float32 (or float64) matrix in context scratch, row-major: the staging / partial buffers of the sharded
    drivers when no other device allocator is around.  Duck-types what pycmf_amd/sharded.py uses of a torch tensor:
    ``data_ptr()``, ``shape``, ``numel()``, ``element_size()`` and row slicing (a view)."""

    def __init__(self, ctx, rows, cols=1, itemsize=4, _ptr=None, _owner=None):
        self.shape = (int(rows), int(cols))
        self.itemsize = itemsize
        if _ptr is None:
            self._owner = ctx.scratch(max(self.numel() * itemsize, 16))
            self._ptr = self._owner.data_ptr()
        else:
            self._owner, self._ptr = _owner, _ptr
        self._ctx = ctx

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self.shape[0] * self.shape[1]

    def element_size(self):
        return self.itemsize

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("DeviceArray supports contiguous row slices only")
        lo, hi, _ = sl.indices(self.shape[0])
        hi = max(hi, lo)
        return DeviceArray(self._ctx, hi - lo, self.shape[1], self.itemsize,
                           _ptr=self._ptr + lo * self.shape[1] * self.itemsize, _owner=self._owner)

    def release(self):
        if self._owner is not None and hasattr(self._owner, "release"):
            self._owner.release()


class Context:
    """Owns one cmf_ctx (one GPU).  Thin, typed wrapper over the C ABI."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        _touch()
        self._h = _vp()
        check(self._lib.cmf_ctx_create(C.byref(self._h), int(device), _vp(stream or 0)))
        self.shape = None
        self._keep = []

    def close(self):
        if self._h:
            self._lib.cmf_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- problem / data
    def set_problem(self, m, d, p, k):
        check(self._lib.cmf_set_problem(self._h, m, d, p, k))
        self.shape = (int(m), int(d), int(p), int(k))

    def set_data(self, which, A):
        """Upload X (which=0) or Y (which=1): ndarray (any strides) or scipy CSR/CSC."""
        import scipy.sparse as sp
        if sp.issparse(A):
            A = A.tocsr()  # a copy unless A already is CSR
            if not A.has_canonical_format:
                A = A.copy()           # never canonicalise the caller's matrix in place
                A.sum_duplicates()
            indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(A.indices, dtype=np.int32)
            data = np.ascontiguousarray(A.data, dtype=np.float64)
            check(self._lib.cmf_set_data_csr(self._h, which, indptr.ctypes.data_as(_pi64),
                                             indices.ctypes.data_as(_pi32),
                                             data.ctypes.data_as(_pd), A.nnz))
            return
        A = np.asarray(A)
        if A.dtype == np.float32:
            rs, cs = _strides(A)
            check(self._lib.cmf_set_data_f32(self._h, which, A.ctypes.data_as(_pf), rs, cs))
        else:
            A = A if A.dtype == np.float64 else A.astype(np.float64)
            rs, cs = _strides(A)
            check(self._lib.cmf_set_data_f64(self._h, which, A.ctypes.data_as(_pd), rs, cs))

    def get_data(self, which):
        m, d, p, _ = self.shape
        out = np.empty((m, d) if which == 0 else (d, p), dtype=np.float32)
        check(self._lib.cmf_get_data_f32(self._h, which, out.ctypes.data_as(_pf), out.shape[1], 1))
        return out

    def data_matmul(self, which, trans, B):
        """op(X|Y) @ B on the device for a host float64 matrix B; returns a host float64 array."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        m, d, p, _ = self.shape
        ar, ac = ((m, d), (d, p))[which]
        out = np.empty((ac if trans else ar, B.shape[1]))
        check(self._lib.cmf_data_matmul_f64(self._h, which, 1 if trans else 0, B.ctypes.data_as(_pd), B.shape[0], B.shape[1],
                                            out.ctypes.data_as(_pd)))
        return out

    def rsvd(self, which, transpose, k, size, n_iter, omega):
        """Randomized truncated SVD of X / Y on the device copy; returns (U, S, Vt) float64."""
        m, d, p, _ = self.shape
        rows, cols = ((m, d), (d, p))[which]
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        assert omega.shape == ((rows if transpose else cols), size)
        U, S, Vt = np.empty((rows, k)), np.empty(k), np.empty((k, cols))
        check(self._lib.cmf_rsvd(self._h, which, 1 if transpose else 0, k, size, n_iter, omega.ctypes.data_as(_pd),
                                 U.ctypes.data_as(_pd), S.ctypes.data_as(_pd), Vt.ctypes.data_as(_pd)))
        return U, S, Vt

    def data_sum(self):
        sx, sy = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_data_sum(self._h, C.byref(sx), C.byref(sy)))
        return sx.value, sy.value

    def sparse_layout(self, which):
        """(groups, split rows, pieces, accumulator rows per group) of the blocked SpMM image of A and of A^T."""
        out = (C.c_int64 * 8)()
        check(self._lib.cmf_sparse_layout(self._h, which, out))
        v = [int(x) for x in out]
        return tuple(v[:4]), tuple(v[4:])

    def data_layout(self, which):
        """(dense image exists, native CSR pair resident) of X (0) / Y (1)."""
        a, b = C.c_int(0), C.c_int(0)
        check(self._lib.cmf_data_layout(self._h, which, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def get_data_block(self, which, row0, nrows, col0, ncols):
        """float32 block of the dense device image of X (0) / Y (1)."""
        out = np.empty((nrows, ncols), dtype=np.float32)
        check(self._lib.cmf_get_data_block_f32(self._h, which, row0, nrows, col0, ncols, out.ctypes.data_as(_pf)))
        return out

    def sample_lists(self, sweep, seed, ratio, row0, nrows):
        """Index lists of the device sampler for rows [row0, row0 + nrows) of sweep 0 (U) / 1 (Z) / 2 (V, X side) / 3 (V, Y side)."""
        m, d, p = self.shape[:3]
        n = d if sweep <= 1 else (m if sweep == 2 else p)
        per = int(n * ratio)
        out = np.empty((nrows, per), dtype=np.int32)
        check(self._lib.cmf_sample_lists(self._h, sweep, seed, ratio, row0, nrows, out.ctypes.data_as(_pi32)))
        return out

    def fill_data_synthetic(self, which, seed, row0=0, col0=0, kind=0, param=0.0):
        """kind 0: |N(0,1)|; 1: sigmoid(N(0,1)); 2: Bernoulli(param) in {0, 1}"""
        if kind == 0:
            check(self._lib.cmf_fill_data_synthetic(self._h, which, seed, row0, col0))
        else:
            check(self._lib.cmf_fill_data_synthetic_kind(self._h, which, seed, row0, col0, kind, param))

    def fill_factor_synthetic(self, which, seed, row0=0, scale=1.0):
        check(self._lib.cmf_fill_factor_synthetic(self._h, which, seed, row0, scale))

    def set_factor(self, which, F):
        F = np.asarray(F)
        if F.dtype != np.float64:
            F = F.astype(np.float64)
        rs, cs = _strides(F)
        check(self._lib.cmf_set_factor_f64(self._h, which, F.ctypes.data_as(_pd), rs, cs))

    def get_factor_into(self, which, F):
        """Write the device factor back into the caller's float64 array, in place."""
        assert F.dtype == np.float64
        rs, cs = _strides(F)
        check(self._lib.cmf_get_factor_f64(self._h, which, F.ctypes.data_as(_pd), rs, cs))

    def get_factor(self, which):
        m, d, p, k = self.shape
        out = np.empty(((m, d, p)[which], k))
        self.get_factor_into(which, out)
        return out

    # ---- MU
    def mu_step(self, l1, l2, mask=7):
        check(self._lib.cmf_mu_step(self._h, l1, l2, mask))

    def mu_kl_step(self, l1, l2, mask=7):
        """One multiplicative-update iteration (V, U, Z) for the generalised Kullback-Leibler objective."""
        check(self._lib.cmf_mu_kl_step(self._h, l1, l2, mask))

    def kl_divergence(self, want_x=True, want_y=True):
        """(D(X || U V^T), D(Y || V Z^T)) of the factors on the device; a side that is not asked for comes back as 0.0."""
        dx, dy = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_kl_divergence(self._h, C.byref(dx) if want_x else None, C.byref(dy) if want_y else None))
        return dx.value, dy.value

    def mu_kl_layout(self):
        """(shares of the U sweep, of the V sweep, of the Z sweep, device scratch bytes of a step) of the KL passes."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_mu_kl_layout(self._h, out))
        return tuple(out)

    def mu_beta_step(self, beta, l1, l2, mask=7):
        """One multiplicative-update iteration (V, U, Z) for the beta-divergence objective, 0 <= beta <= 2."""
        check(self._lib.cmf_mu_beta_step(self._h, float(beta), l1, l2, mask))

    def beta_divergence(self, beta, want_x=True, want_y=True):
        """(D_beta(X || U V^T), D_beta(Y || V Z^T)) of the factors on the device; a side that is not asked for comes back as 0.0."""
        dx, dy = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_beta_divergence(self._h, float(beta), C.byref(dx) if want_x else None, C.byref(dy) if want_y else None))
        return dx.value, dy.value

    def mu_beta_products(self, beta, sweep):
        """(num, den) of one sweep (0 = U, 1 = V, 2 = Z) from the factors on the device, float32 arrays of rows x k_pad; no update."""
        m, d, p, _ = self.shape
        rows, kp = (m, d, p)[sweep] if sweep in (0, 1, 2) else 1, self.geometry()[3]
        num, den = np.zeros((rows, kp), dtype=np.float32), np.zeros((rows, kp), dtype=np.float32)
        check(self._lib.cmf_mu_beta_products(self._h, float(beta), int(sweep), num.ctypes.data_as(_pf), den.ctypes.data_as(_pf)))
        return num, den

    def mu_beta_layout(self):
        """(shares of the U sweep, of the V sweep, of the Z sweep, device scratch bytes of a step) of the beta-divergence passes."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_mu_beta_layout(self._h, out))
        return tuple(out)

    # ---- MU with per-entry weights (csrc/cmf_wmu.hip.h)
    def set_weight(self, which, W):
        """Dense non-negative weights of the shape of X (which=0) / Y (which=1); the relation's data must be set and dense."""
        W = np.asarray(W)
        if W.dtype == np.float32:
            rs, cs = _strides(W)
            check(self._lib.cmf_set_weight_f32(self._h, which, W.ctypes.data_as(_pf), rs, cs))
        else:
            W = W if W.dtype == np.float64 else W.astype(np.float64)
            rs, cs = _strides(W)
            check(self._lib.cmf_set_weight_f64(self._h, which, W.ctypes.data_as(_pd), rs, cs))

    def set_weighted_csr(self, which, indptr, indices, t_values, w_values):
        """The observed pattern of a relation (CSR arrays) with the data and the weights on it; the loss runs over it only."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        t = np.ascontiguousarray(t_values, dtype=np.float64)
        w = np.ascontiguousarray(w_values, dtype=np.float64)
        if not (indices.shape == t.shape == w.shape and indptr.ndim == 1 and indptr.size and indptr[-1] == indices.size):
            raise ValueError("set_weighted_csr: indices, t_values and w_values must have indptr[-1] entries each")
        check(self._lib.cmf_set_weighted_csr(self._h, which, indptr.ctypes.data_as(_pi64), indices.ctypes.data_as(_pi32),
                                             t.ctypes.data_as(_pd), w.ctypes.data_as(_pd)))

    def clear_weight(self, which):
        check(self._lib.cmf_clear_weight(self._h, which))

    def mu_weighted_step(self, l1, l2, mask=7):
        """One multiplicative-update iteration (V, U, Z) of the weighted Frobenius objective; an unweighted relation counts with W = 1."""
        check(self._lib.cmf_mu_weighted_step(self._h, l1, l2, mask))

    def weighted_residual_sq(self, want_x=True, want_y=True):
        """(sum Wx (X - U V^T)^2, sum Wy (Y - V Z^T)^2) of the factors on the device; a side that is not asked for comes back as 0.0."""
        ex, ey = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_weighted_residual_sq(self._h, C.byref(ex) if want_x else None, C.byref(ey) if want_y else None))
        return ex.value, ey.value

    def mu_weighted_layout(self):
        """(shares of the U sweep, of the V sweep, of the Z sweep, device scratch bytes of a step) of the weighted passes."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_mu_weighted_layout(self._h, out))
        return tuple(out)

    def fill_weight_synthetic(self, which, seed, density):
        """Dense Bernoulli(density) 0/1 weights from the device generator."""
        check(self._lib.cmf_fill_weight_synthetic(self._h, which, seed, density))

    def get_weight_block(self, which, row0, nrows, col0, ncols):
        """float32 block of the dense weight image of X (0) / Y (1)."""
        out = np.empty((nrows, ncols), dtype=np.float32)
        check(self._lib.cmf_get_weight_block_f32(self._h, which, row0, nrows, col0, ncols, out.ctypes.data_as(_pf)))
        return out

    # ---- HALS (csrc/cmf_hals.hip.h)
    def hals_step(self, l1, l2, mask=7):
        """One HALS iteration (coordinate-descent sweeps of V, U, Z) on the non-negative Frobenius objective."""
        check(self._lib.cmf_hals_step(self._h, l1, l2, mask))

    def hals_sweep(self, which, N, G, l1, l2):
        """One coordinate-descent sweep of factor ``which`` with the caller's numerator N (rows x k) and Gram G (k x k)."""
        m, d, p, k = self.shape
        N = np.ascontiguousarray(N, dtype=np.float64)
        G = np.ascontiguousarray(G, dtype=np.float64)
        if N.shape != ((m, d, p)[which], k) or G.shape != (k, k):
            raise ValueError("hals_sweep: N must be %s and G %s, got %s and %s" % (((m, d, p)[which], k), (k, k), N.shape, G.shape))
        check(self._lib.cmf_hals_sweep(self._h, which, N.ctypes.data_as(_pd), G.ctypes.data_as(_pd), l1, l2))

    # ---- ALS (csrc/cmf_als.hip.h)
    def als_step(self, l2, nn_mask=0, mask=7):
        """One ALS iteration (V, U, Z): every row of a swept factor becomes the exact minimiser of its own normal equations over
        the observed entries (relations with CSR weights) and all cells (relations without weights); ``nn_mask`` projects."""
        check(self._lib.cmf_als_step(self._h, l2, nn_mask, mask))

    def als_normal(self, which, row0, nrows, l2):
        """(H float32[nrows, k_pad, k_pad], g float32[nrows, k_pad]): the finished normal equations of rows [row0, row0 + nrows)
        of factor ``which`` as ``als_step`` would hand them to the solver."""
        kp = self.geometry()[3]
        H = np.empty((nrows, kp, kp), dtype=np.float32)
        g = np.empty((nrows, kp), dtype=np.float32)
        check(self._lib.cmf_als_normal(self._h, which, row0, nrows, l2, H.ctypes.data_as(_pf), g.ctypes.data_as(_pf)))
        return H, g

    def als_layout(self):
        """(piece length, pieces of the U sweep, of the V sweep, of the Z sweep) of the ALS normal-equation kernel."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_als_layout(self._h, out))
        return tuple(out)

    def als_nnls_step(self, l2, nn_mask, mask, sweeps):
        """``als_step`` with the factors in ``nn_mask`` swept by ``sweeps`` passes of cyclic coordinate descent on each row's
        non-negative least-squares problem (from the current rows) instead of solved and projected."""
        check(self._lib.cmf_als_nnls_step(self._h, l2, nn_mask, mask, sweeps))

    def als_nnls_rows(self, H, g, f, sweeps):
        """The swept copy of ``f`` (nrows x k_pad): ``sweeps`` passes of the coordinate-descent kernel on the caller's systems
        H float32[nrows, k_pad, k_pad], g float32[nrows, k_pad] (``als_normal``'s layout, k / k_pad of the bound problem)."""
        kp = self.geometry()[3]
        H = np.ascontiguousarray(H, dtype=np.float32)
        g = np.ascontiguousarray(g, dtype=np.float32)
        f = np.array(f, dtype=np.float32, order="C")
        n = f.shape[0] if f.ndim == 2 else -1
        if f.shape != (n, kp) or H.shape != (n, kp, kp) or g.shape != (n, kp):
            raise ValueError("als_nnls_rows: H must be (n, %d, %d), g and f (n, %d), got %s, %s and %s" % (kp, kp, kp, H.shape, g.shape, f.shape))
        check(self._lib.cmf_als_nnls_rows(self._h, n, H.ctypes.data_as(_pf), g.ctypes.data_as(_pf), f.ctypes.data_as(_pf), sweeps))
        return f

    def als_cg_step(self, l2, nn_mask, mask, cg_steps, nn_sweeps=0):
        """``als_step`` with every signed swept factor that has an observed relation fitted by ``cg_steps`` matrix-free
        conjugate-gradient steps per row (from the current rows) instead of the exact solves; the factors in ``nn_mask`` are
        projected (``nn_sweeps=0``) or swept by coordinate descent as ``als_nnls_step`` does."""
        check(self._lib.cmf_als_cg_step(self._h, l2, nn_mask, mask, cg_steps, nn_sweeps))

    def als_cg_rows(self, which, row0, nrows, l2, cg_steps):
        """float32[nrows, k_pad]: the rows ``als_cg_step`` would write for rows [row0, row0 + nrows) of factor ``which``; the
        factors are left unchanged."""
        kp = self.geometry()[3]
        out = np.zeros((max(nrows, 0), kp), dtype=np.float32)
        check(self._lib.cmf_als_cg_rows(self._h, which, row0, nrows, l2, cg_steps, out.ctypes.data_as(_pf)))
        return out

    def als_cg_last(self):
        """(long rows, pieces) of the last sweep of the CG route (``als_cg_step`` or ``als_cg_rows``): the rows longer than option
        ``"als_cg_piece"`` entries, which were cut into that many pieces.  Read-only; for the tests."""
        out = np.zeros(2, dtype=np.int64)
        check(self._lib.cmf_als_cg_last(self._h, out.ctypes.data_as(_pi64)))
        return int(out[0]), int(out[1])

    # ---- matrix-free non-negative rows (csrc/cmf_als_nncg.hip.h)
    def als_nncg_step(self, l2, nn_mask, mask, cg_steps, nn_cg_steps, nn_sweeps=0):
        """``als_cg_step`` (``cg_steps=0``: the exact rows) with every swept factor in ``nn_mask`` that has an observed relation
        fitted by ``nn_cg_steps`` matrix-free projected conjugate-gradient steps per row, from the rows it has clamped at zero; a
        non-negative factor whose relations are all full keeps the route ``nn_sweeps`` names."""
        check(self._lib.cmf_als_nncg_step(self._h, l2, nn_mask, mask, cg_steps, nn_cg_steps, nn_sweeps))

    def als_nncg_rows(self, which, row0, nrows, l2, nn_cg_steps):
        """float32[nrows, k_pad]: the rows ``als_nncg_step`` would write for rows [row0, row0 + nrows) of factor ``which``; the
        factors are left unchanged."""
        kp = self.geometry()[3]
        out = np.zeros((max(nrows, 0), kp), dtype=np.float32)
        check(self._lib.cmf_als_nncg_rows(self._h, which, row0, nrows, l2, nn_cg_steps, out.ctypes.data_as(_pf)))
        return out

    def als_nncg_last(self):
        """(long rows, pieces) of the last sweep of the non-negative CG route (``als_nncg_step`` or ``als_nncg_rows``), as
        ``als_cg_last``.  Read-only; for the tests."""
        out = np.zeros(2, dtype=np.int64)
        check(self._lib.cmf_als_nncg_last(self._h, out.ctypes.data_as(_pi64)))
        return int(out[0]), int(out[1])

    def als_nncg_passes(self):
        """(passes, entry passes) of that sweep: the passes its rows ran, summed, and the stored entries those passes read."""
        out = np.zeros(2, dtype=np.int64)
        check(self._lib.cmf_als_nncg_passes(self._h, out.ctypes.data_as(_pi64)))
        return int(out[0]), int(out[1])

    # ---- exact rows of few stored entries in dual form (csrc/cmf_als_dual.hip.h)
    def als_dual_step(self, l2, nn_mask, mask, dual_max, nn_sweeps=0, nn_cg_steps=0):
        """``als_step`` with the permission ``dual_max`` (0 .. 128): in a sweep on the exact row route that has no shared term and
        reads no logistic relation, a row of 1 .. dual_max stored entries whose class width (32, 64, 128) is below k_pad is solved
        from its n x n dual system -- the same exact row; every other sweep runs what it runs without the permission.  Non-negative
        factors take ``nn_sweeps`` / ``nn_cg_steps`` as ``als_nncg_step`` gives them."""
        check(self._lib.cmf_als_dual_step(self._h, l2, nn_mask, mask, dual_max, nn_sweeps, nn_cg_steps))

    def als_dual_rows(self, which, row0, nrows, l2, dual_max):
        """float32[nrows, k_pad]: the rows an eligible sweep of factor ``which`` would write for rows [row0, row0 + nrows) under
        ``dual_max`` (unprojected); the factors are left unchanged."""
        kp = self.geometry()[3]
        out = np.zeros((max(nrows, 0), kp), dtype=np.float32)
        check(self._lib.cmf_als_dual_rows(self._h, which, row0, nrows, l2, dual_max, out.ctypes.data_as(_pf)))
        return out

    def als_dual_last(self):
        """(rows in class 32, in class 64, in class 128, rows left to the formed route, rows written as zeros) of the last dual
        sweep (``als_dual_step`` or ``als_dual_rows``).  Read-only; for the tests."""
        out = np.zeros(5, dtype=np.int64)
        check(self._lib.cmf_als_dual_last(self._h, out.ctypes.data_as(_pi64)))
        return tuple(int(v) for v in out)

    # ---- a per-row l2 under the ALS steps (cmf_set_l2_rows, csrc/cmf_als_steps.hip.h)
    def set_l2_rows(self, which, mult):
        """Positive multipliers of ``l2``, one per row of factor ``which`` (0 U | 1 V | 2 Z): row i of an ALS sweep of that factor
        is solved under ``l2 * mult[i]``.  ``None`` clears them.  ``ValueError`` (state unchanged) for a bad ``which``, a wrong
        length or a value that is not finite and positive."""
        if mult is None or which not in (0, 1, 2):   # (a bad selector: the library refuses it before it reads anything)
            check(self._lib.cmf_set_l2_rows(self._h, which, None))
            return
        v = np.ascontiguousarray(mult, dtype=np.float64)
        if v.shape != (self.shape[which],):
            raise ValueError("set_l2_rows: expected %d multipliers, got an array of shape %s" % (self.shape[which], v.shape))
        check(self._lib.cmf_set_l2_rows(self._h, which, v.ctypes.data_as(_pd)))

    def get_l2_rows(self, which):
        """float64[rows of factor ``which``]: the multipliers as they were set, or ``None`` when none are bound."""
        if which not in (0, 1, 2):
            check(self._lib.cmf_get_l2_rows(self._h, which, None, None))
        out = np.ones(self.shape[which], dtype=np.float64)
        on = C.c_int(0)
        check(self._lib.cmf_get_l2_rows(self._h, which, out.ctypes.data_as(_pd), C.byref(on)))
        return out if on.value else None

    # ---- ALS for implicit feedback (csrc/cmf_als_bg.hip.h)
    def set_background_weight(self, which, c0):
        """Background weight ``c0`` >= 0 on the cells outside the CSR pattern of relation ``which`` (0 X | 1 Y), honoured by the
        ALS steps; every stored weight must be >= c0.  0 clears it."""
        check(self._lib.cmf_set_background_weight(self._h, which, float(c0)))

    def get_background_weight(self, which):
        c0 = C.c_double(0)
        check(self._lib.cmf_get_background_weight(self._h, which, C.byref(c0)))
        return c0.value

    def als_residual_sq(self, want_x=True, want_y=True):
        """(E_x, E_y), E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B> - sum_O s^2), of the relations with CSR weights; a side that is
        not asked for comes back as 0.0."""
        ex, ey = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_als_residual_sq(self._h, C.byref(ex) if want_x else None, C.byref(ey) if want_y else None))
        return ex.value, ey.value

    # ---- ALS for explicit ratings: offset, row and column biases (csrc/cmf_als_bias.hip.h)
    def _bias_len(self, which, axis):
        m, d, p, _ = self.shape
        return ((m, d), (d, p))[which][axis]

    def set_biases(self, which, enable=True, mu=0.0, lb=0.0):
        """Bind (or with ``enable=False`` free) the bias terms of relation ``which`` (0 X | 1 Y), which must have CSR weights and
        no background weight: the fixed offset ``mu``, zeroed row and column biases, their regulariser ``lb`` >= 0."""
        check(self._lib.cmf_set_biases(self._h, which, 1 if enable else 0, float(mu), float(lb)))

    def get_biases(self, which):
        """(mu, lb, enabled) of relation ``which``."""
        mu, lb, on = C.c_double(0), C.c_double(0), C.c_int(0)
        check(self._lib.cmf_get_biases(self._h, which, C.byref(mu), C.byref(lb), C.byref(on)))
        return mu.value, lb.value, bool(on.value)

    def set_bias(self, which, axis, v):
        """The row (``axis=0``) or column (``axis=1``) biases of relation ``which`` from a float64 vector."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (self._bias_len(which, axis),):
            raise ValueError("set_bias: expected %d values, got an array of shape %s" % (self._bias_len(which, axis), v.shape))
        check(self._lib.cmf_set_bias_f64(self._h, which, axis, v.ctypes.data_as(_pd)))

    def get_bias(self, which, axis):
        out = np.zeros(self._bias_len(which, axis), dtype=np.float64)
        check(self._lib.cmf_get_bias_f64(self._h, which, axis, out.ctypes.data_as(_pd)))
        return out

    def als_bias_step(self, l2, nn_mask=0, mask=7, cg_steps=0, nn_sweeps=0):
        """One iteration of the biased model: the sweeps of ``als_cg_step`` (``cg_steps=0`` and ``nn_sweeps=0``: of ``als_step``)
        on the adjusted targets t - mu - r_i - c_j, then per biased relation the exact row and column bias sweeps ``mask`` allows
        (r_x with U, c_x and r_y with V, c_y with Z)."""
        check(self._lib.cmf_als_bias_step(self._h, l2, nn_mask, mask, cg_steps, nn_sweeps))

    def als_bias_rows(self, which, axis):
        """float32 vector: the biases one bias sweep of relation ``which`` along ``axis`` would write from the current state;
        nothing is changed."""
        out = np.zeros(self._bias_len(which, axis), dtype=np.float32)
        check(self._lib.cmf_als_bias_rows(self._h, which, axis, out.ctypes.data_as(_pf)))
        return out

    def als_bias_targets(self, which, image, nnz):
        """(bt, bp) float32[nnz]: the adjusted targets t - mu - r_i - c_j and w times them of the pattern (``image=0``) or its
        transpose (1) in stored order, as the factor sweeps read them; ``nnz`` must be the stored entries of the pattern
        (``ValueError`` otherwise: the library writes that many).  For the tests."""
        nnz = int(nnz)
        if nnz < 0:
            raise ValueError("als_bias_targets: nnz must be the number of stored entries, got %d" % nnz)
        bt, bp = np.zeros(nnz, dtype=np.float32), np.zeros(nnz, dtype=np.float32)
        check(self._lib.cmf_als_bias_targets(self._h, which, image, nnz, bt.ctypes.data_as(_pf), bp.ctypes.data_as(_pf)))
        return bt, bp

    # ---- ALS with a logistic loss on an observed relation (csrc/cmf_als_logit.hip.h)
    def set_relation_loss(self, which, kind):
        """The loss of relation ``which`` (0 X | 1 Y) under ``als_step`` / ``als_nnls_step`` / ``als_normal``: 'frobenius' (0, the
        default) or 'logistic' (1: weighted cross-entropy of sigmoid(a . b) over the CSR pattern of its weights).  Cleared by
        ``set_problem``."""
        check(self._lib.cmf_set_relation_loss(self._h, which, RELATION_LOSSES.get(kind, kind)))

    def get_relation_loss(self, which):
        kind = C.c_int(0)
        check(self._lib.cmf_get_relation_loss(self._h, which, C.byref(kind)))
        return kind.value

    def als_logistic_loss(self, want_x=True, want_y=True):
        """(L_x, L_y), L = sum_O w [softplus(s) - t s] of the logistic relations with the factors on the device; 0.0 for a
        Frobenius relation and for a side that is not asked for."""
        lx, ly = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_als_logistic_loss(self._h, C.byref(lx) if want_x else None, C.byref(ly) if want_y else None))
        return lx.value, ly.value

    # ---- ALS with a Huber loss on an observed relation (csrc/cmf_als_huber.hip.h)
    def set_huber_delta(self, which, delta):
        """Put relation ``which`` (0 X | 1 Y) under the Huber loss of threshold ``delta`` > 0 for every ALS step and row entry: a
        reweighting pass runs in front of each sweep that reads it.  0 (or None) takes it back.  Cleared by ``set_problem``."""
        check(self._lib.cmf_set_huber_delta(self._h, which, float(delta or 0.0)))

    def get_huber_delta(self, which):
        d = C.c_double(0)
        check(self._lib.cmf_get_huber_delta(self._h, which, C.byref(d)))
        return d.value

    def als_huber_loss(self, want_x=True, want_y=True):
        """(L_x, L_y), L = sum_O w rho_delta(t - s) of the Huber relations with the factors on the device; 0.0 for a relation
        without a delta and for a side that is not asked for."""
        lx, ly = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_als_huber_loss(self._h, C.byref(lx) if want_x else None, C.byref(ly) if want_y else None))
        return lx.value, ly.value

    def als_huber_weights(self, which, image, nnz):
        """(w_eff, p_eff) float32[nnz]: w omega and w t omega of the pattern (``image=0``) or its transpose (1) in stored order at the
        current factors, as a sweep reads them; ``nnz`` must be the stored entries of the pattern.  For the tests."""
        nnz = int(nnz)
        if nnz < 0:
            raise ValueError("als_huber_weights: nnz must be the number of stored entries, got %d" % nnz)
        hw, hp = np.zeros(nnz, dtype=np.float32), np.zeros(nnz, dtype=np.float32)
        check(self._lib.cmf_als_huber_weights(self._h, which, image, nnz, hw.ctypes.data_as(_pf), hp.ctypes.data_as(_pf)))
        return hw, hp

    # ---- ALS with a logistic loss on every route (csrc/cmf_als_logit_pass.hip.h)
    def set_logit_pass(self, which, enable=True):
        """Reweight the logistic relation ``which`` (0 X | 1 Y) by a pass of its own in front of every sweep, so that every ALS route
        honours its loss (CG, projected CG and dual rows included); False: inside the normal-equation kernel, the default.  It acts
        only while the relation is logistic.  Cleared by ``set_problem``."""
        check(self._lib.cmf_set_logit_pass(self._h, which, 1 if enable else 0))

    def get_logit_pass(self, which):
        on = C.c_int(0)
        check(self._lib.cmf_get_logit_pass(self._h, which, C.byref(on)))
        return bool(on.value)

    def als_logit_weights(self, which, image, nnz):
        """(w_eff, p_eff) float32[nnz]: w kappa and w t - w / 2 of the pattern (``image=0``) or its transpose (1) in stored order at
        the current factors, as a sweep reads them; ``nnz`` must be the stored entries of the pattern.  For the tests."""
        nnz = int(nnz)
        if nnz < 0:
            raise ValueError("als_logit_weights: nnz must be the number of stored entries, got %d" % nnz)
        hw, hp = np.zeros(nnz, dtype=np.float32), np.zeros(nnz, dtype=np.float32)
        check(self._lib.cmf_als_logit_weights(self._h, which, image, nnz, hw.ctypes.data_as(_pf), hp.ctypes.data_as(_pf)))
        return hw, hp

    def predict_pairs(self, which, rows, cols, link="linear"):
        """float32[n]: f(offset + r[row] + c[col] + a_row . b_col) of the pairs, a = U, b = V for relation 0 and V, Z for relation 1;
        the bias terms only when biases are bound on the relation.  Nothing is changed."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
        if rows.shape != cols.shape:
            raise ValueError("predict_pairs: rows and cols must have one length, got %d and %d" % (rows.size, cols.size))
        out = np.zeros(rows.size, dtype=np.float32)
        check(self._lib.cmf_predict_pairs(self._h, which, LINKS[link] if isinstance(link, str) else int(link), rows.size,
                                          rows.ctypes.data_as(_pi64), cols.ctypes.data_as(_pi64), out.ctypes.data_as(_pf)))
        return out

    def mu_step_error(self, l1, l2, mask=7):
        """One MU iteration and the squared residuals (ex2, ey2) of the factors it leaves, from the step's own products."""
        ex2, ey2 = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_mu_step_error(self._h, l1, l2, mask, C.byref(ex2), C.byref(ey2)))
        return ex2.value, ey2.value

    def v_buf_elems(self):
        n = C.c_int64(0)
        check(self._lib.cmf_v_buf_elems(self._h, C.byref(n)))
        return n.value

    def data_pass_launches(self):
        """Data passes with a 256-wide factor launched so far, by kernel form: (gemm_kernel, wg256 TN, wg256 NN, TN with the
        factor ring, NN with the factor ring); see option ``"data_pass_wg"``.  Read-only; for the tests."""
        out = np.zeros(5, dtype=np.int64)
        check(self._lib.cmf_data_pass_launches(self._h, out.ctypes.data_as(_pi64)))
        return tuple(int(v) for v in out)

    MU_ROUTE_FORMS = ("epi_mu", "factor_update", "factor_update2", "pair", "gram32", "sum_slabs", "mu_apply", "narrow_copy")

    def mu_route_launches(self):
        """Launches of the plain MU step's routes so far, by form (``MU_ROUTE_FORMS``: gemm_kernel with the fused MU epilogue,
        factor_update_kernel, factor_update2_kernel, gemm_pair_kernel, small-Gram kernel pairs, sum_slabs_kernel, mu_apply_kernel,
        copies of a column-tile image over its factor).  Read-only; for the tests."""
        out = np.zeros(8, dtype=np.int64)
        check(self._lib.cmf_mu_route_launches(self._h, out.ctypes.data_as(_pi64)))
        return dict(zip(self.MU_ROUTE_FORMS, (int(v) for v in out)))

    def mu_v_partials(self, dev_ptr):
        check(self._lib.cmf_mu_v_partials(self._h, _vp(dev_ptr)))

    def mu_v_partials_rows(self, dev_ptr, row0, nrows, with_gram):
        check(self._lib.cmf_mu_v_partials_rows(self._h, _vp(dev_ptr), row0, nrows, 1 if with_gram else 0))

    def mu_v_apply(self, dev_ptr, l1, l2):
        check(self._lib.cmf_mu_v_apply(self._h, _vp(dev_ptr), l1, l2))

    def mu_uz_update(self, l1, l2, mask=7):
        check(self._lib.cmf_mu_uz_update(self._h, l1, l2, mask))

    # row-blocked V update (reduce-scatter + epilogue on the rank's block + all-gather): include/cmfhip.h
    def mu_blocked_layout(self, world):
        """(rows per block, floats of the partial buffer); grows the allocation behind V so that the all-gather runs in place."""
        b, n = C.c_int64(0), C.c_int64(0)
        check(self._lib.cmf_mu_blocked_layout(self._h, int(world), C.byref(b), C.byref(n)))
        return b.value, n.value

    def mu_v_partials_split(self, dev_p, dev_g):
        check(self._lib.cmf_mu_v_partials_split(self._h, _vp(dev_p), _vp(dev_g)))

    def mu_v_apply_rows(self, dev_p_rows, dev_g, row0, nrows, l1, l2):
        check(self._lib.cmf_mu_v_apply_rows(self._h, _vp(dev_p_rows), _vp(dev_g), row0, nrows, l1, l2))

    def mu_gram_v_rows(self, row0, nrows, dev_g2):
        check(self._lib.cmf_mu_gram_v_rows(self._h, row0, nrows, _vp(dev_g2)))

    def mu_uz_update_gram(self, dev_g2, l1, l2, mask=7):
        check(self._lib.cmf_mu_uz_update_gram(self._h, _vp(dev_g2), l1, l2, mask))

    def factor_dev_ptr(self, which):
        p = _pf()
        check(self._lib.cmf_factor_dev_ptr(self._h, which, C.byref(p)))
        return C.cast(p, _vp).value

    def run(self, solver, max_iter, tol, l1=0.0, l2=0.0, alpha=0.5, alpha_err=0.5, x_link="linear", y_link="linear", nn_mask=0,
            update_mask=7, pert=0.2, ratio=1.0, seed=0, check_every=10):
        """The whole outer loop in C (cmf_run): returns (n_iter, errors, seconds) -- errors[0] is the error at init, one more
        entry per convergence check, seconds the time since the call at those points."""
        prm = RunParams(0 if solver == "mu" else 1, l1, l2, alpha, alpha_err, LINKS[x_link], LINKS[y_link], nn_mask, update_mask,
                        pert, ratio, int(seed))
        cap = max_iter // max(check_every, 1) + 2
        errs, secs = (C.c_double * cap)(), (C.c_double * cap)()
        n_iter, n_trace = C.c_int(0), C.c_int(0)
        check(self._lib.cmf_run(self._h, C.byref(prm), int(max_iter), float(tol), int(check_every), C.byref(n_iter), errs, secs, cap,
                                C.byref(n_trace)))
        n = min(n_trace.value, cap)
        return n_iter.value, [errs[i] for i in range(n)], [secs[i] for i in range(n)]

    # ---- Newton
    def newton_step(self, alpha, l1, l2, x_link, y_link, nn_mask, upd_mask, pert, ratio,
                    u_idx=None, z_idx=None, vx_idx=None, vy_idx=None):
        def ptr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.int32)
            self._keep.append(a)
            return a.ctypes.data_as(_pi32)
        self._keep = []
        check(self._lib.cmf_newton_step(self._h, alpha, l1, l2, LINKS[x_link], LINKS[y_link],
                                        nn_mask, upd_mask, pert, ratio,
                                        ptr(u_idx), ptr(z_idx), ptr(vx_idx), ptr(vy_idx)))
        self._keep = []

    def newton_step_device_sampled(self, alpha, l1, l2, x_link, y_link, nn_mask, upd_mask, pert, ratio, seed):
        check(self._lib.cmf_newton_step_device_sampled(self._h, alpha, l1, l2, LINKS[x_link], LINKS[y_link],
                                                       nn_mask, upd_mask, pert, ratio, seed))

    def newton_uz_update(self, alpha, l1, l2, nn_mask, upd_mask, pert):
        check(self._lib.cmf_newton_uz_update(self._h, alpha, l1, l2, nn_mask, upd_mask, pert))

    def newton_v_partials(self, alpha, dev_ptr):
        check(self._lib.cmf_newton_v_partials(self._h, alpha, _vp(dev_ptr)))

    def newton_v_apply(self, dev_ptr, l1, l2, nn_mask, pert):
        check(self._lib.cmf_newton_v_apply(self._h, _vp(dev_ptr), l1, l2, nn_mask, pert))

    def newton_v_gram(self, alpha, dev_gbuf):
        check(self._lib.cmf_newton_v_gram(self._h, alpha, _vp(dev_gbuf)))

    def newton_v_products(self, alpha, l2, pert, dev_gbuf, dev_pbuf):
        check(self._lib.cmf_newton_v_products(self._h, alpha, l2, pert, _vp(dev_gbuf), _vp(dev_pbuf)))

    def newton_v_finish(self, dev_pbuf, l1, nn_mask):
        check(self._lib.cmf_newton_v_finish(self._h, _vp(dev_pbuf), l1, nn_mask))

    # ---- metrics
    def newton_clamp_stats(self, reset=False, full=False):
        """(rows whose float32 Hessian went through the spectral clamp and stayed float32, largest ||H||_F / pert (or condition
        estimate of a plain solve) among the rows left in float32, rows redone in float64) since the last reset; ``full`` adds the
        largest condition estimate over all plain float32 solves."""
        rows, ratio, refined, plain = C.c_int64(0), C.c_double(0), C.c_int64(0), C.c_double(0)
        check(self._lib.cmf_newton_clamp_stats(self._h, C.byref(rows), C.byref(ratio), C.byref(refined), C.byref(plain), 1 if reset else 0))
        return (rows.value, ratio.value, refined.value, plain.value) if full else (rows.value, ratio.value, refined.value)

    def newton_clamp_routes(self):
        """(rows served by the tridiagonal eigen-solve, rows served by the rank-one shortcut) since the context was created."""
        e, r = C.c_int64(0), C.c_int64(0)
        check(self._lib.cmf_newton_clamp_routes(self._h, C.byref(e), C.byref(r)))
        return e.value, r.value

    def residual_sq(self, x_link="linear", y_link="linear"):
        ex, ey = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_residual_sq(self._h, LINKS[x_link], LINKS[y_link], C.byref(ex), C.byref(ey)))
        return ex.value, ey.value

    # ---- prediction
    def topk(self, query, cand, n, link="linear", rows=None, exclude=None, queries=None):
        """The n best candidates (rows of factor ``cand``) per query, by f(q . b_j): ``(idx int32[nq, n], val float32[nq, n])``,
        best first, ties by smaller index; ``-1 / -inf`` where a query has fewer than n candidates left.  Queries: the rows
        ``rows`` (index array; None = all) of factor ``query``, or the (nq x k) array ``queries`` (then ``query`` is ignored).
        ``exclude``: ``(indptr int64[nq + 1], indices int32)`` -- per query a strictly ascending list of candidates to skip."""
        xp = xi = None
        if exclude is not None:
            xp = np.ascontiguousarray(exclude[0], dtype=np.int64)
            xi = np.ascontiguousarray(exclude[1], dtype=np.int32)
        if queries is not None:
            if rows is not None:
                raise ValueError("rows and queries exclude each other")
            Q = np.asarray(queries, dtype=np.float64)
            if Q.ndim != 2 or Q.shape[1] != self.shape[3]:
                raise ValueError("queries must be (nq, %d), got %r" % (self.shape[3], Q.shape))
            nq = Q.shape[0]
        elif rows is not None:
            r = np.ascontiguousarray(rows, dtype=np.int64).ravel()
            nq = r.size
        else:
            nq = self.shape[query] if query in (0, 1, 2) else 0
        if xp is not None and xp.size != nq + 1:
            raise ValueError("exclude: indptr must have nq + 1 = %d entries, got %d" % (nq + 1, xp.size))
        if xp is not None and nq and (xp[-1] > xi.size):
            raise ValueError("exclude: indptr points beyond indices")
        idx = np.empty((nq, int(n)), dtype=np.int32)
        val = np.empty((nq, int(n)), dtype=np.float32)
        xpp = xp.ctypes.data_as(_pi64) if xp is not None else None
        xip = xi.ctypes.data_as(_pi32) if xi is not None else None
        lk = LINKS.get(link, link)
        if queries is not None:
            rs, cs = _strides(Q) if nq else (Q.shape[1], 1)
            check(self._lib.cmf_topk_queries(self._h, Q.ctypes.data_as(_pd), rs, cs, nq, cand, lk, int(n), xpp, xip,
                                             idx.ctypes.data_as(_pi32), val.ctypes.data_as(_pf)))
        else:
            check(self._lib.cmf_topk(self._h, query, cand, lk, r.ctypes.data_as(_pi64) if rows is not None else None, nq, int(n),
                                     xpp, xip, idx.ctypes.data_as(_pi32), val.ctypes.data_as(_pf)))
        return idx, val

    def topk_layout(self, nq, cand, n, excl_nnz=-1, own_queries=False):
        """(queries per workgroup, candidate shares, queries per launch, device scratch bytes) of such a call."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_topk_layout(self._h, int(nq), cand, int(n), int(excl_nnz), int(bool(own_queries)), out))
        return tuple(out)

    def rank(self, query, cand, held, rows=None, exclude=None, queries=None):
        """Exact ranks of held-out entries under ``topk``'s order: ``(rank int32[nnz], score float32[nnz], eligible int32[nq])``.
        ``held`` = ``(indptr int64[nq + 1], indices int32)``: per query a strictly ascending list of held-out candidates; rank =
        how many candidates outside the query's ``exclude`` list precede the entry (larger raw score first, ties by smaller index;
        0-based, -1 where the entry's own score is NaN), score = its raw float32 score, eligible = candidates - len(exclude list).
        Queries, ``rows``, ``exclude`` and ``queries`` as in ``topk``."""
        hp = np.ascontiguousarray(held[0], dtype=np.int64)
        hi = np.ascontiguousarray(held[1], dtype=np.int32)
        xp = xi = None
        if exclude is not None:
            xp = np.ascontiguousarray(exclude[0], dtype=np.int64)
            xi = np.ascontiguousarray(exclude[1], dtype=np.int32)
        if queries is not None:
            if rows is not None:
                raise ValueError("rows and queries exclude each other")
            Q = np.asarray(queries, dtype=np.float64)
            if Q.ndim != 2 or Q.shape[1] != self.shape[3]:
                raise ValueError("queries must be (nq, %d), got %r" % (self.shape[3], Q.shape))
            nq = Q.shape[0]
        elif rows is not None:
            r = np.ascontiguousarray(rows, dtype=np.int64).ravel()
            nq = r.size
        else:
            nq = self.shape[query] if query in (0, 1, 2) else 0
        for name, p, i in (("held", hp, hi), ("exclude", xp, xi)):
            if p is None:
                continue
            if p.ndim != 1 or p.size != nq + 1:
                raise ValueError("%s: indptr must have nq + 1 = %d entries, got %d" % (name, nq + 1, p.size))
            if p[-1] > i.size:
                raise ValueError("%s: indptr points beyond indices" % name)
        nnz = int(hp[-1]) if hp[-1] > 0 else 0
        rank = np.empty(nnz, dtype=np.int32)
        score = np.empty(nnz, dtype=np.float32)
        eligible = np.empty(nq, dtype=np.int32)
        args = (hp.ctypes.data_as(_pi64), hi.ctypes.data_as(_pi32),
                xp.ctypes.data_as(_pi64) if xp is not None else None, xi.ctypes.data_as(_pi32) if xi is not None else None,
                rank.ctypes.data_as(_pi32), score.ctypes.data_as(_pf), eligible.ctypes.data_as(_pi32))
        if queries is not None:
            rs, cs = _strides(Q) if nq else (Q.shape[1], 1)
            check(self._lib.cmf_rank_queries(self._h, Q.ctypes.data_as(_pd), rs, cs, nq, cand, *args))
        else:
            check(self._lib.cmf_rank(self._h, query, cand, r.ctypes.data_as(_pi64) if rows is not None else None, nq, *args))
        return rank, score, eligible

    def rank_layout(self, nq, cand, held_nnz, excl_nnz=-1, own_queries=False):
        """(held-out entries per virtual query HB, candidate shares, virtual queries per launch, device scratch bytes) of such a call."""
        out = (C.c_int64 * 4)()
        check(self._lib.cmf_rank_layout(self._h, int(nq), cand, int(held_nnz), int(excl_nnz), int(bool(own_queries)), out))
        return tuple(out)

    def data_sq(self):
        x2, y2 = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_data_sq(self._h, C.byref(x2), C.byref(y2)))
        return x2.value, y2.value

    def safe_invert_batch(self, H, pert):
        H = np.ascontiguousarray(H, dtype=np.float64)
        n, k, _ = H.shape
        out = np.empty_like(H)
        check(self._lib.cmf_safe_invert_batch(self._h, H.ctypes.data_as(_pd), out.ctypes.data_as(_pd), n, k, pert))
        return out

    def safe_solve_batch(self, H, g, pert, method=0, eigenvalues=False):
        """g_b * safe_inverse(H_b) for a batch (the step of a per-row sweep), float32 device path; method 1: all through the
        tridiagonal eigen-solve.  eigenvalues=True also returns the eigenvalues the QL iteration found (method 1)."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        n, k, _ = H.shape
        out = np.empty((n, k), dtype=np.float64)
        lam = np.empty((n, k), dtype=np.float64) if eigenvalues else None
        check(self._lib.cmf_safe_solve_batch(self._h, H.ctypes.data_as(_pd), g.ctypes.data_as(_pd), out.ctypes.data_as(_pd),
                                             lam.ctypes.data_as(_pd) if eigenvalues else None, n, k, pert, method))
        return (out, lam) if eigenvalues else out

    def safe_invert_f64(self, H, pert):
        """float64 path of the shared Hessian: H is k x k with k = this context's n_components."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        out = np.empty_like(H)
        check(self._lib.cmf_safe_invert_f64(self._h, H.ctypes.data_as(_pd), out.ctypes.data_as(_pd), H.shape[0], pert))
        return out

    def scratch(self, nbytes):
        """Zero-filled device buffer owned by the context; the returned object has ``data_ptr()`` like a torch tensor."""
        p = _vp()
        check(self._lib.cmf_scratch_alloc(self._h, int(nbytes), C.byref(p)))
        return _Scratch(self, p.value, int(nbytes))

    # ---- collectives (RCCL inside the C ABI: csrc/cmf_comm.hip.h)
    def comm_init(self, rank, world, unique_id):
        check(self._lib.cmf_comm_init(self._h, rank, world, bytes(unique_id)))

    def comm_destroy(self):
        check(self._lib.cmf_comm_destroy(self._h))

    def comm_allreduce(self, buf):
        """In-place sum over the ranks of a DeviceArray / scratch / tensor-like (float32, or float64 by element_size)."""
        n = buf.numel()
        if buf.element_size() == 8:
            check(self._lib.cmf_comm_allreduce_f64(self._h, _vp(buf.data_ptr()), n))
        else:
            check(self._lib.cmf_comm_allreduce_f32(self._h, _vp(buf.data_ptr()), n))

    def comm_allreduce_bg(self, buf):
        check(self._lib.cmf_comm_allreduce_f32_bg(self._h, _vp(buf.data_ptr()), buf.numel()))

    def comm_join(self):
        check(self._lib.cmf_comm_join(self._h))

    def comm_exposed_ms(self, reset=False):
        ms = C.c_double(0)
        check(self._lib.cmf_comm_exposed_ms(self._h, C.byref(ms), 1 if reset else 0))
        return ms.value

    def comm_allgather(self, full, elems_per_rank):
        check(self._lib.cmf_comm_allgather_f32(self._h, _vp(full.data_ptr()), elems_per_rank))

    def comm_reduce_scatter(self, full, elems_per_rank):
        check(self._lib.cmf_comm_reduce_scatter_f32(self._h, _vp(full.data_ptr()), elems_per_rank))

    def data_block_sums(self, which, axis):
        """float64 sums of the dense device image of X (0) / Y (1) over blocks of 256 rows (axis 0 -> [rows_pad / 256, cols_pad]) or
        256 columns (axis 1 -> [rows_pad, cols_pad / 256]); padded extents."""
        mp, dp, pp, _ = self.geometry()
        rp, cp = (mp, dp) if which == 0 else (dp, pp)
        out = np.empty((rp // 256, cp) if axis == 0 else (rp, cp // 256), dtype=np.float64)
        check(self._lib.cmf_data_block_sums_f64(self._h, int(which), int(axis), out.ctypes.data_as(_pd)))
        return out

    def comm_group_start(self):
        check(self._lib.cmf_comm_group_start(self._h))

    def comm_group_end(self):
        check(self._lib.cmf_comm_group_end(self._h))

    def comm_launch_points(self):
        n = C.c_int64(0)
        check(self._lib.cmf_comm_launch_points(self._h, C.byref(n)))
        return n.value

    def scale(self, buf, factor):
        """buf *= factor on the context's stream (device array)."""
        check(self._lib.cmf_scale_f32(self._h, _vp(buf.data_ptr()), buf.numel(), float(factor)))

    def comm_count(self):
        """(ranks, this rank) as RCCL reports them (ncclCommCount / ncclCommUserRank)."""
        n, r = C.c_int(0), C.c_int(0)
        check(self._lib.cmf_comm_count(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_stats_kind(self, kind):
        """(calls, payload bytes, ms) of one kind of collective: 0 all-reduce f32, 1 all-reduce f64, 2 all-gather, 3 reduce-scatter, 4 group
        (calls = groups closed, ms = events around the whole group; the members are counted under their own kinds without ms)."""
        calls, nbytes, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(self._lib.cmf_comm_stats_kind(self._h, int(kind), C.byref(calls), C.byref(nbytes), C.byref(ms)))
        return calls.value, nbytes.value, ms.value

    def comm_allreduce_host(self, values, op="sum"):
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(self._lib.cmf_comm_allreduce_host_f64(self._h, a.ctypes.data_as(_pd), a.size, 0 if op == "sum" else 1))
        return a

    def comm_barrier(self):
        check(self._lib.cmf_comm_barrier(self._h))

    def comm_timing(self, enable=True):
        check(self._lib.cmf_comm_timing(self._h, 1 if enable else 0))

    def comm_stats(self, reset=False):
        """(calls, payload bytes, ms on the stream) since the last reset; waits for the stream."""
        calls, nbytes, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(self._lib.cmf_comm_stats(self._h, C.byref(calls), C.byref(nbytes), C.byref(ms), 1 if reset else 0))
        return calls.value, nbytes.value, ms.value

    def copy_to_host(self, buf, dtype=np.float32):
        """numpy copy of a DeviceArray / scratch buffer (waits for the stream)."""
        out = np.empty(buf.numel(), dtype=np.float64 if buf.element_size() == 8 else dtype)
        check(self._lib.cmf_copy_to_host(self._h, _vp(buf.data_ptr()), out.ctypes.data_as(_vp), out.nbytes))
        return out.reshape(buf.shape) if hasattr(buf, "shape") else out

    def copy_from_host(self, buf, a):
        a = np.ascontiguousarray(a)
        check(self._lib.cmf_copy_from_host(self._h, _vp(buf.data_ptr()), a.ctypes.data_as(_vp), a.nbytes))

    def export_factor_rows(self, which, dev_ptr):
        """Device-to-device copy of all valid rows (k_pad floats each) to `dev_ptr`, on the context's stream."""
        check(self._lib.cmf_export_factor_rows(self._h, which, _vp(dev_ptr)))

    def import_factor_rows(self, which, dev_ptr):
        check(self._lib.cmf_import_factor_rows(self._h, which, _vp(dev_ptr)))

    def set_option(self, name, value):
        check(self._lib.cmf_set_option(self._h, name.encode(), int(value)))

    def sync(self):
        check(self._lib.cmf_sync(self._h))

    def debug_clock(self):
        g, u = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_debug_clock(self._h, C.byref(g), C.byref(u)))
        return g.value, u.value

    def kernel_timing(self, enable):
        """False / 0 off, True / 1 every launch, 2 the data-pass classes only (see cmfhip.h)."""
        check(self._lib.cmf_kernel_timing(self._h, int(enable)))

    def kernel_timing_reset(self):
        check(self._lib.cmf_kernel_timing_reset(self._h))

    def kernel_time(self, cls):
        """(accumulated ms, launches, algorithmic flops) of one kernel class."""
        ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        check(self._lib.cmf_kernel_time(self._h, KERNEL_CLASSES.get(cls, LATER_KERNEL_CLASSES.get(cls, cls)), C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    def rowhess_samples(self):
        """(sample rows credited by the algorithm, sample rows gathered by the outer-product kernel) since the last reset."""
        a, b = C.c_double(0), C.c_double(0)
        check(self._lib.cmf_rowhess_samples(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def marker(self):
        check(self._lib.cmf_marker(self._h))

    def marker_times(self, cap=4096):
        """Elapsed ms of every marker since the first one (waits for the stream; clears the markers)."""
        buf = (C.c_double * cap)()
        n = C.c_int64(0)
        check(self._lib.cmf_marker_times(self._h, buf, cap, C.byref(n)))
        return [buf[i] for i in range(min(n.value, cap))]

    def stream_handle(self):
        p = _vp()
        check(self._lib.cmf_get_stream(self._h, C.byref(p)))
        return p.value or 0

    def geometry(self):
        a, b, c_, k = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(self._lib.cmf_get_geometry(self._h, C.byref(a), C.byref(b), C.byref(c_), C.byref(k)))
        return a.value, b.value, c_.value, k.value
