"""Python interface to the CDNA4 HIP kernels.

Loads the in-tree ``libfedops_gfx950.so`` via ctypes (no torch C++ ABI
coupling; launches go onto torch's current HIP stream, so the ops compose
with streams/graphs and RCCL).  On a GPU box a missing extension is a HARD
error -- there is deliberately no silent eager fallback here (the eager
path is an explicit model-level opt-out, ``use_kernels=False``).
"""
from __future__ import annotations

import ctypes
import threading
from typing import Optional, Tuple

import numpy as _np
import torch

from .build import LIB_PATH

__all__ = [
    "kernels_available",
    "require_kernels",
    "gaussian_linear_logp_grad",
    "gaussian_linear_eval_sync",
    "logistic_glm_logp_grad",
    "glm_family_logp_grad",
    "glm_family_padded_k",
    "glm_family_kernel_supports",
    "split_bf16x3",
    "GLM_FAMILY_BATCHED_K",
    "glm_family_batched_supports",
    "glm_family_logp_grad_batched",
    "GLM_SOFTMAX_MAX_CLASSES",
    "glm_softmax_supports",
    "glm_softmax_class_group",
    "glm_softmax_logp_grad",
    "GLM_FAMILY_FISHER_K",
    "glm_family_fisher_supports",
    "glm_family_fisher_tile_rows",
    "glm_family_fisher",
    "glm_family_fisher_vector",
    "glm_family_fisher_diagonal",
    "ode_poly_logp_grad",
]

_FED_F32, _FED_F64, _FED_BF16 = 0, 1, 2
_DTYPE_CODE = {
    torch.float32: _FED_F32,
    torch.float64: _FED_F64,
    torch.bfloat16: _FED_BF16,
}

_lib: Optional[ctypes.CDLL] = None
_load_error: Optional[str] = None


def _try_load() -> Optional[ctypes.CDLL]:
    global _lib, _load_error
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if not path.exists():
        # Cross-compile on the fly when hipcc is present (seconds on CPU box).
        try:
            from .build import build

            build()
        except Exception as ex:  # no hipcc / compile error
            _load_error = f"extension not built and build failed: {ex}"
            return None
    try:
        lib = ctypes.CDLL(str(path))
    except OSError as ex:
        _load_error = f"failed to dlopen {path}: {ex}"
        return None
    lib.fed_gaussian_linear.restype = ctypes.c_int
    lib.fed_gaussian_linear.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_double, ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p,
    ]
    lib.fed_gaussian_linear_eval.restype = ctypes.c_int
    lib.fed_gaussian_linear_eval.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_double, ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong,
    ]
    lib.fed_host_alloc.restype = ctypes.c_void_p
    lib.fed_host_alloc.argtypes = [ctypes.c_longlong]
    lib.fed_gaussian_linear_theta.restype = ctypes.c_int
    lib.fed_gaussian_linear_theta.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_void_p, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p,
    ]
    lib.fed_publish_result.restype = ctypes.c_int
    lib.fed_publish_result.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fed_logistic_glm.restype = ctypes.c_int
    lib.fed_logistic_glm.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p,
    ]
    lib.fed_glm_family.restype = ctypes.c_int
    lib.fed_glm_family.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p,
    ]
    lib.fed_glm_family_batched.restype = ctypes.c_int
    lib.fed_glm_family_batched.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_void_p,
    ]
    lib.fed_glm_softmax_batched.restype = ctypes.c_int
    lib.fed_glm_softmax_batched.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_void_p,
    ]
    lib.fed_glm_family_fisher.restype = ctypes.c_int
    lib.fed_glm_family_fisher.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_void_p,
    ]
    lib.fed_glm_family_fvp.restype = ctypes.c_int
    lib.fed_glm_family_fvp.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_void_p,
    ]
    lib.fed_glm_family_fisher_tile_rows.restype = ctypes.c_int
    lib.fed_glm_family_fisher_tile_rows.argtypes = [ctypes.c_int]
    lib.fed_ode_lv_eval.restype = ctypes.c_int
    lib.fed_ode_lv_eval.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fed_ode_lv_eval_batched.restype = ctypes.c_int
    lib.fed_ode_lv_eval_batched.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fed_ode_poly_eval.restype = ctypes.c_int
    lib.fed_ode_poly_eval.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
    ]
    lib.fed_logistic_glm_batched.restype = ctypes.c_int
    lib.fed_logistic_glm_batched.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_void_p,
    ]
    lib.fed_gaussian_persistent_start.restype = ctypes.c_void_p
    lib.fed_gaussian_persistent_start.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
        ctypes.c_double, ctypes.c_int,
    ]
    lib.fed_gaussian_persistent_eval.restype = ctypes.c_int
    lib.fed_gaussian_persistent_eval.argtypes = [
        ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.fed_gaussian_persistent_stop.restype = ctypes.c_int
    lib.fed_gaussian_persistent_stop.argtypes = [ctypes.c_void_p]
    lib.fed_gaussian_persistent_relaunch_count.restype = ctypes.c_int
    lib.fed_gaussian_persistent_relaunch_count.argtypes = [ctypes.c_void_p]
    lib.fed_last_hip_error.restype = ctypes.c_char_p
    _lib = lib
    return _lib


def kernels_available() -> bool:
    return _try_load() is not None


def require_kernels() -> ctypes.CDLL:
    lib = _try_load()
    if lib is None:
        raise RuntimeError(
            "pytensor_federated_amd HIP extension is not available on this GPU box "
            f"({_load_error}). Build it with `python -m pytensor_federated_amd.ops.build` "
            "or run __graft_entry__.build(). Refusing to fall back to eager torch "
            "on a GPU (pass use_kernels=False to the model to opt out explicitly)."
        )
    return lib


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = _try_load()
        detail = lib.fed_last_hip_error().decode() if lib is not None else "?"
        raise RuntimeError(f"{what} failed with code {rc} ({detail})")


def gaussian_linear_logp_grad(
    x: torch.Tensor,
    y: torch.Tensor,
    a: float,
    b: float,
    sigma: float,
    out: Optional[torch.Tensor] = None,
    ws: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused logp + dlogp/da + dlogp/db on device; returns fp64 0-d views.

    ``out`` (fp64[3] on the same device) may be supplied to keep the result
    buffer stable across calls -- it is the buffer an RCCL all-reduce sums
    in the federated path.  ``ws`` is the per-model workspace from
    :func:`gaussian_workspace`; pass it when several models evaluate
    concurrently on different streams.  Fully async on the current stream.
    """
    lib = require_kernels()
    if x.dtype not in _DTYPE_CODE:
        raise TypeError(f"unsupported dtype {x.dtype}")
    assert x.is_cuda and y.is_cuda and x.is_contiguous() and y.is_contiguous()
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=x.device)
    if ws is None:
        ws = _workspace(x.device, "gaussian", GAUSSIAN_WS_SIZE, zeroed=True)
    rc = lib.fed_gaussian_linear(
        x.data_ptr(), y.data_ptr(), x.numel(),
        float(a), float(b), float(sigma),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
        _DTYPE_CODE[x.dtype], _stream_ptr(),
    )
    _check(rc, "fed_gaussian_linear")
    return out[0], out[1], out[2]


_ws_cache = {}
_mailbox_lock = threading.Lock()
_mailbox = None  # (np.ndarray view over pinned mapped memory)
_mailbox_seq = 0

#: fp64 words in a gaussian workspace: 9 spaced ticket words + 3 per block
GAUSSIAN_WS_SIZE = 72 + 3 * 2048


def _get_mailbox() -> "_np.ndarray":
    """Process-wide pinned mailbox {logp, ga, gb, seq} the fused kernel's
    last block writes into."""
    global _mailbox
    if _mailbox is None:
        lib = require_kernels()
        ptr = lib.fed_host_alloc(4 * 8)
        if not ptr:
            raise RuntimeError("hipHostMalloc failed for the result mailbox")
        _mailbox = _np.ctypeslib.as_array(
            ctypes.cast(ptr, ctypes.POINTER(ctypes.c_double)), shape=(4,)
        )
        _mailbox[:] = 0.0
    return _mailbox


def alloc_mailbox(n_results: int) -> "_np.ndarray":
    """A fresh mapped-pinned mailbox: n_results fp64 + one u64 seq slot."""
    lib = require_kernels()
    ptr = lib.fed_host_alloc((n_results + 1) * 8)
    if not ptr:
        raise RuntimeError("hipHostMalloc failed")
    arr = _np.ctypeslib.as_array(
        ctypes.cast(ptr, ctypes.POINTER(ctypes.c_double)), shape=(n_results + 1,)
    )
    arr[:] = 0.0
    return arr


def gaussian_linear_launch_theta(
    x: torch.Tensor, y: torch.Tensor, theta_dev: torch.Tensor, sigma: float,
    out: torch.Tensor, ws: torch.Tensor,
) -> None:
    """Async fused launch reading [a,b] from device memory (graph-capturable)."""
    lib = require_kernels()
    rc = lib.fed_gaussian_linear_theta(
        x.data_ptr(), y.data_ptr(), x.numel(),
        theta_dev.data_ptr(), float(sigma),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
        _DTYPE_CODE[x.dtype], _stream_ptr(),
    )
    _check(rc, "fed_gaussian_linear_theta")


def publish_result(buf: torch.Tensor, mailbox: "_np.ndarray", epoch_dev: torch.Tensor) -> None:
    """Launch the mailbox-publish kernel (graph-capturable; epoch on device)."""
    lib = require_kernels()
    rc = lib.fed_publish_result(
        buf.data_ptr(), buf.numel(), mailbox.ctypes.data,
        epoch_dev.data_ptr(), _stream_ptr(),
    )
    _check(rc, "fed_publish_result")


def _require_contiguous(**tensors: torch.Tensor) -> None:
    """The kernels read these through data_ptr() as C-ordered arrays."""
    for name, t in tensors.items():
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (strides {t.stride()})")


# Argument checks the GLM entry points share.  Pure torch: they run on CPU
# tensors too (tests/test_ops_arg_checks_cpu.py).  They sit on the host path
# of every launch, so the passing case does no more than the tests themselves.

def _design_shape(X: torch.Tensor) -> torch.Size:
    """``(N, K)`` of the design matrix; it must be 2-D."""
    shape = X.shape
    if len(shape) != 2:
        raise ValueError("X must be [N, K]")
    return shape


def _check_design(X: torch.Tensor) -> None:
    """The kernels read X through data_ptr() as a C-ordered device array, in
    16-byte vectors."""
    if not X.is_contiguous():
        _require_contiguous(X=X)
    if X.data_ptr() % 16:
        raise ValueError("X must be 16-byte aligned")
    if not X.is_cuda:
        raise ValueError("X must be on a ROCm device")


def _check_rows(name: str, t: torch.Tensor, X: torch.Tensor) -> None:
    """A per-row vector (y, offset): contiguous f32[N] on X's device."""
    if t.dtype != torch.float32 or t.shape != (X.shape[0],) or t.device != X.device:
        raise ValueError(f"{name} must be f32[N] on X's device")
    if not t.is_contiguous():
        _require_contiguous(**{name: t})


def _check_sigma(sigma: float) -> None:
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be positive")


def _out_buffer(
    out: Optional[torch.Tensor], shape: Tuple[int, ...], X: torch.Tensor
) -> torch.Tensor:
    """``out``, or a new fp64 buffer of ``shape`` on X's device when it is None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=X.device)
    if (
        out.dtype != torch.float64 or out.shape != shape or out.device != X.device
        or not out.is_contiguous()
    ):
        dims = ", ".join(str(d) for d in shape)
        raise ValueError(f"out must be a contiguous fp64[{dims}] on X's device")
    return out


def ode_lv_logp_grad(
    u0: torch.Tensor,          # [B, 2] f64
    y_obs: torch.Tensor,       # [n_obs, B, 2] f64
    obs_of_step: torch.Tensor, # [n_steps+1] int32 (obs index or -1)
    n_steps: int,
    h: float,
    sigma: float,
    theta: torch.Tensor,       # [4] f64 (any device)
    states_ws: torch.Tensor,   # [(n_steps+1)*B*2] f64 scratch
    out: Optional[torch.Tensor] = None,  # f64[5]
) -> torch.Tensor:
    """Native Lotka-Volterra forward+adjoint: out = [logp_quad, g_theta[4]].

    (The logp normalization constant is added by the caller.)
    """
    lib = require_kernels()
    _require_contiguous(u0=u0, y_obs=y_obs, obs_of_step=obs_of_step, states_ws=states_ws)
    B = u0.shape[0]
    theta_dev = theta.detach().to(device=u0.device, dtype=torch.float64).contiguous()
    if out is None:
        out = torch.empty(5, dtype=torch.float64, device=u0.device)
    rc = lib.fed_ode_lv_eval(
        u0.data_ptr(), y_obs.data_ptr(), obs_of_step.data_ptr(),
        int(n_steps), int(B), float(h), float(sigma),
        theta_dev.data_ptr(), states_ws.data_ptr(), out.data_ptr(),
        _stream_ptr(),
    )
    _check(rc, "fed_ode_lv_eval")
    return out


PT_MAXD = 4


def ode_poly_logp_grad(
    terms,                     # list of (d, j, coef, exponents[≤4])
    D: int,
    P: int,
    u0: torch.Tensor,          # [B, D] f64
    y_obs: torch.Tensor,       # [n_obs, B, D] f64
    obs_of_step: torch.Tensor, # [n_steps+1] int32
    n_steps: int,
    h: float,
    sigma: float,
    theta: torch.Tensor,       # [C, P] f64 (C chains; C=1 for single eval)
    states_ws: torch.Tensor,   # [C*(n_steps+1)*B*D] f64 scratch
    out: Optional[torch.Tensor] = None,  # f64[C, 1+P]
) -> torch.Tensor:
    """Generic polynomial-RHS forward+adjoint: out[c] = [logp_quad, g_theta[P]].

    The RHS family is du_d/dt = sum_t c_t * theta_{j_t} * prod_i u_i^{e_ti}
    interpreted from a term table (see csrc/ode_poly.hip) -- one compiled
    kernel serves Lotka-Volterra, SIR, oscillators, mass-action kinetics...
    The logp normalization constant is added by the caller.
    """
    lib = require_kernels()
    _require_contiguous(u0=u0, y_obs=y_obs, obs_of_step=obs_of_step, states_ws=states_ws)
    B = u0.shape[0]
    T = len(terms)
    d_arr = (ctypes.c_int * T)(*[int(t[0]) for t in terms])
    j_arr = (ctypes.c_int * T)(*[int(t[1]) for t in terms])
    c_arr = (ctypes.c_double * T)(*[float(t[2]) for t in terms])
    e_flat = []
    for t in terms:
        e = list(t[3]) + [0] * (PT_MAXD - len(t[3]))
        e_flat.extend(int(v) for v in e[:PT_MAXD])
    e_arr = (ctypes.c_ubyte * (T * PT_MAXD))(*e_flat)
    theta_dev = theta.detach().to(device=u0.device, dtype=torch.float64).contiguous()
    C = theta_dev.shape[0] if theta_dev.dim() == 2 else 1
    theta_dev = theta_dev.reshape(C, P)
    if out is None:
        out = torch.empty((C, 1 + P), dtype=torch.float64, device=u0.device)
    rc = lib.fed_ode_poly_eval(
        T, int(D), int(P),
        d_arr, j_arr, c_arr, e_arr,
        u0.data_ptr(), y_obs.data_ptr(), obs_of_step.data_ptr(),
        int(n_steps), int(B), int(C), float(h), float(sigma),
        theta_dev.data_ptr(), states_ws.data_ptr(), out.data_ptr(),
        _stream_ptr(),
    )
    _check(rc, "fed_ode_poly_eval")
    return out


class PersistentLinearEngine:
    """Resident eval-server kernel for one gaussian linear shard.

    The kernel stays launched; each call writes {seq, a, b} into a pinned
    request mailbox and spin-reads the pinned result line -- no kernel
    launch, no stream sync, no ramp (the ~18 us fixed cost of the
    launch-per-eval path).  Every device spin is bounded: the server
    self-exits after 1.5 s idle and is relaunched transparently, at the
    host's sequence, on the next call (``relaunch_count`` counts these).

    The shard is snapshotted at every (re)launch: each lane keeps its first
    rows of ``x`` and ``y`` in registers and re-reads only what does not fit.
    ``x`` and ``y`` must therefore not be mutated in place while the engine
    is open -- close it and open a new one to serve changed data.
    """

    def __init__(self, x: torch.Tensor, y: torch.Tensor, sigma: float) -> None:
        lib = require_kernels()
        self._lib = lib
        assert x.is_cuda and x.is_contiguous() and y.is_contiguous()
        self._x, self._y = x, y  # keep alive
        self._sigma = float(sigma)
        self._dtype_code = _DTYPE_CODE[x.dtype]
        self._out = (ctypes.c_double * 3)()
        self._handle = None
        self._lock = threading.Lock()  # one mailbox -> one eval at a time
        self._start()

    def _start(self) -> None:
        # the server runs on a stream of its own and snapshots the shard as
        # it launches: whatever produced x and y must have finished
        torch.cuda.current_stream(self._x.device).synchronize()
        self._handle = self._lib.fed_gaussian_persistent_start(
            self._x.data_ptr(), self._y.data_ptr(), self._x.numel(),
            self._sigma, self._dtype_code,
        )
        if not self._handle:
            raise RuntimeError("fed_gaussian_persistent_start failed")

    def logp_grad_sync(self, a: float, b: float) -> Tuple[float, float, float]:
        with self._lock:
            rc = self._lib.fed_gaussian_persistent_eval(
                self._handle, float(a), float(b), self._out
            )
            if rc == -6:
                # server unreachable; full restart once
                self._lib.fed_gaussian_persistent_stop(self._handle)
                self._handle = None
                self._start()
                rc = self._lib.fed_gaussian_persistent_eval(
                    self._handle, float(a), float(b), self._out
                )
            if rc != 0:
                raise RuntimeError(f"persistent eval failed ({rc})")
            return self._out[0], self._out[1], self._out[2]

    @property
    def relaunch_count(self) -> int:
        """Times the server was launched again after an idle self-exit."""
        with self._lock:
            if not self._handle:
                return 0
            return int(self._lib.fed_gaussian_persistent_relaunch_count(self._handle))

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.fed_gaussian_persistent_stop(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ode_lv_logp_grad_batched(
    u0: torch.Tensor,
    y_obs: torch.Tensor,
    obs_of_step: torch.Tensor,
    n_steps: int,
    h: float,
    sigma: float,
    theta_c: torch.Tensor,     # [C, 4] f64
    states_ws: torch.Tensor,   # [C*(n_steps+1)*B*2] f64 scratch
    out: Optional[torch.Tensor] = None,  # f64[C*5]
) -> torch.Tensor:
    """Batched native Lotka-Volterra: C thetas in one sweep -> [C][5]."""
    lib = require_kernels()
    _require_contiguous(u0=u0, y_obs=y_obs, obs_of_step=obs_of_step, states_ws=states_ws)
    B = u0.shape[0]
    C = theta_c.shape[0]
    theta_dev = theta_c.detach().to(device=u0.device, dtype=torch.float64).contiguous()
    if out is None:
        out = torch.empty(C * 5, dtype=torch.float64, device=u0.device)
    rc = lib.fed_ode_lv_eval_batched(
        u0.data_ptr(), y_obs.data_ptr(), obs_of_step.data_ptr(),
        int(n_steps), int(B), int(C), float(h), float(sigma),
        theta_dev.data_ptr(), states_ws.data_ptr(), out.data_ptr(), _stream_ptr(),
    )
    _check(rc, "fed_ode_lv_eval_batched")
    return out.reshape(C, 5)


BATCH_CHAINS = 16


def logistic_glm_logp_grad_batched(
    X: torch.Tensor,
    y: torch.Tensor,
    theta: torch.Tensor,
    out: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """MFMA-batched evaluation of 16 chains: theta[K,16] -> logp[16], G[K,16].

    One pass over X computes Z = X.theta, the per-chain BCE logp, and
    G = X^T (y - sigmoid(Z)) on the matrix cores (the kernels of
    csrc/glm_logistic_batched.hip).  Per-chain cost ~B x below the single-chain
    kernel -- the multi-chain MCMC axis (reference pm.sample cores=N) on
    one GPU.
    """
    lib = require_kernels()
    n, K = X.shape
    B = BATCH_CHAINS
    if theta.shape != (K, B):
        raise ValueError(f"theta must be [K, {B}], got {tuple(theta.shape)}")
    if X.dtype != torch.bfloat16:
        raise TypeError("batched kernel supports bf16 X only")
    assert X.is_cuda and X.is_contiguous()
    theta_t = theta.detach().t().contiguous().to(device=X.device, dtype=torch.bfloat16)
    if out is None:
        out = torch.empty(B + K * B, dtype=torch.float64, device=X.device)
    ws = _workspace(X.device, f"logistic_batched{K}", 768 * (B + K * B), dtype=torch.float32)
    rc = lib.fed_logistic_glm_batched(
        X.data_ptr(), y.data_ptr(), n, K,
        theta_t.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
        _stream_ptr(),
    )
    _check(rc, "fed_logistic_glm_batched")
    return out[:B], out[B:].reshape(K, B)


def gaussian_workspace(device) -> torch.Tensor:
    """Per-model workspace: [ticket(u32 in word 0) | fp64 slab].  The ticket
    word MUST start at zero (torch.zeros) -- the kernel's monotonic arrival
    counter assumes start ≡ 0 (mod grid)."""
    return torch.zeros(GAUSSIAN_WS_SIZE, dtype=torch.float64, device=device)


def gaussian_linear_eval_sync(
    x: torch.Tensor,
    y: torch.Tensor,
    a: float,
    b: float,
    sigma: float,
    out: Optional[torch.Tensor] = None,
    ws: Optional[torch.Tensor] = None,
) -> Tuple[float, float, float]:
    """Single-GPU hot path: ONE ctypes call = one fused launch + host spin
    on the GPU-written pinned mailbox; returns (logp, d/da, d/db) floats.

    No separate finish kernel, no D2H copy, no hipStreamSynchronize on the
    happy path.
    """
    global _mailbox_seq
    lib = require_kernels()
    assert x.is_cuda and x.is_contiguous() and y.is_contiguous()
    if ws is None:
        ws = _workspace(x.device, "gaussian", GAUSSIAN_WS_SIZE, zeroed=True)
    if out is None:
        out = _workspace(x.device, "gaussian_out", 3)
    with _mailbox_lock:
        mailbox = _get_mailbox()
        _mailbox_seq += 1
        rc = lib.fed_gaussian_linear_eval(
            x.data_ptr(), y.data_ptr(), x.numel(),
            float(a), float(b), float(sigma),
            out.data_ptr(), mailbox.ctypes.data,
            ws.data_ptr(), ws.numel() * 8,
            _DTYPE_CODE[x.dtype], _stream_ptr(), _mailbox_seq,
        )
        _check(rc, "fed_gaussian_linear_eval")
        return float(mailbox[0]), float(mailbox[1]), float(mailbox[2])


def _workspace(device, kind: str, n_elems: int, dtype=torch.float64, zeroed=False) -> torch.Tensor:
    key = (device.index, kind)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < n_elems:
        ws = (torch.zeros if zeroed else torch.empty)(n_elems, dtype=dtype, device=device)
        _ws_cache[key] = ws
    return ws


#: (dtype, K) combinations the fused logistic kernel is compiled for
LOGISTIC_SUPPORTED = {
    (torch.bfloat16, 512),
    (torch.bfloat16, 1024),
    (torch.bfloat16, 2048),
    (torch.float32, 256),
    (torch.float32, 512),
    (torch.float32, 1024),
}


def logistic_kernel_supports(dtype, K: int) -> bool:
    return (dtype, int(K)) in LOGISTIC_SUPPORTED


def logistic_glm_logp_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    beta: torch.Tensor,
    out: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused logistic-GLM logp+grad; X read once. Returns (logp, grad[K]) fp64 views."""
    lib = require_kernels()
    n, K = X.shape
    if X.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"unsupported dtype {X.dtype}")
    assert X.is_cuda and X.is_contiguous()
    beta_f32 = beta.detach().to(device=X.device, dtype=torch.float32).contiguous()
    if out is None:
        out = torch.empty(1 + K, dtype=torch.float64, device=X.device)
    ws = _workspace(X.device, f"logistic{K}", 1024 * K, dtype=torch.float32)
    rc = lib.fed_logistic_glm(
        X.data_ptr(), y.data_ptr(), n, K,
        beta_f32.data_ptr(), out.data_ptr(), ws.data_ptr(),
        ws.numel() * 4, _DTYPE_CODE[X.dtype], _stream_ptr(),
    )
    _check(rc, "fed_logistic_glm")
    return out[0], out[1:]


#: link codes of fed_glm_family (csrc/glm_family.hip)
GLM_FAMILY_LINKS = {"poisson": 0, "gaussian": 1, "logistic": 2}
_GLM_FAMILY_VEC = {torch.bfloat16: 8, torch.float32: 4}
#: lanes per row the family kernel is compiled for: G = 1..64 lanes of one
#: 16-byte vector each, then 2 and 4 column chunks of a whole wave
_GLM_FAMILY_LANES = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def glm_family_padded_k(dtype, K: int) -> Optional[int]:
    """Smallest feature count >= K the family kernel is compiled for at
    ``dtype`` (bf16: 8, 16, ..., 2048; f32: 4, 8, ..., 1024), or ``None``
    when K is above the maximum or the dtype is not supported."""
    vec = _GLM_FAMILY_VEC.get(dtype)
    K = int(K)
    if vec is None or K < 1:
        return None
    for lanes in _GLM_FAMILY_LANES:
        if lanes * vec >= K:
            return lanes * vec
    return None


def glm_family_kernel_supports(dtype, K: int) -> bool:
    return glm_family_padded_k(dtype, K) == int(K)


def glm_family_logp_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    beta: torch.Tensor,
    *,
    link: str,
    offset: Optional[torch.Tensor] = None,
    sigma: float = 1.0,
    logp_const: float = 0.0,
    out: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused GLM logp+grad on the row-group kernel; X read once.

    ``link`` is ``"poisson"`` (log link: ``y*z - exp(z)``), ``"gaussian"``
    (identity: ``-(y-z)^2 / (2 sigma^2)``) or ``"logistic"``, with
    ``z = X @ beta (+ offset)``.  ``X[N,K]`` is bf16 or f32 with K one of
    the sizes of :func:`glm_family_padded_k`; ``y`` and ``offset`` are
    f32[N].  ``logp_const`` (the beta-independent part of logp) is added on
    the device, so the result is final without a further launch.  Returns
    (logp, grad[K]) as fp64 views of ``out``.
    """
    lib = require_kernels()
    if link not in GLM_FAMILY_LINKS:
        raise ValueError(f"unknown link {link!r}; expected one of {sorted(GLM_FAMILY_LINKS)}")
    n, K = _design_shape(X)
    if X.dtype not in _GLM_FAMILY_VEC:
        raise TypeError(f"unsupported dtype {X.dtype}")
    if not glm_family_kernel_supports(X.dtype, K):
        raise ValueError(f"family kernel not compiled for (dtype={X.dtype}, K={K})")
    _check_sigma(sigma)
    _check_rows("y", y, X)
    if offset is not None:
        _check_rows("offset", offset, X)
    _check_design(X)
    beta_f32 = beta.detach().to(device=X.device, dtype=torch.float32).contiguous()
    if beta_f32.shape != (K,):
        raise ValueError(f"beta must have shape ({K},), got {tuple(beta_f32.shape)}")
    out = _out_buffer(out, (1 + K,), X)
    ws = _workspace(X.device, f"glm_family{K}", 1024 * K, dtype=torch.float32)
    rc = lib.fed_glm_family(
        X.data_ptr(), y.data_ptr(), offset.data_ptr() if offset is not None else None,
        n, K, beta_f32.data_ptr(), GLM_FAMILY_LINKS[link],
        float(sigma), float(logp_const),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
        _DTYPE_CODE[X.dtype], _stream_ptr(),
    )
    _check(rc, "fed_glm_family")
    return out[0], out[1:]


def split_bf16x3(theta: torch.Tensor) -> torch.Tensor:
    """Split ``theta[K, B]`` into three bf16 pieces, transposed: ``[3, B, K]``.

    ``p0 = bf16(theta)``, ``p1 = bf16(theta - p0)``, ``p2 = bf16(theta - p0 -
    p1)``, the differences taken in f32.  Each difference is exact and drops
    at least 8 leading bits, so the three pieces sum to any finite f32 whose
    last bit is above bf16's subnormal range exactly -- what lets the MFMA
    batched family kernel take bf16 operands without rounding theta.  Pure
    torch; runs on any device.
    """
    rem = theta.detach().to(torch.float32).t().contiguous()
    pieces = []
    for i in range(3):
        p = rem.to(torch.bfloat16)
        pieces.append(p)
        if i < 2:
            rem = rem - p.to(torch.float32)
    return torch.stack(pieces)


#: feature counts the batched family kernel is compiled for: every padded K
#: the GLM family models produce up to 1024 (at 2048 a block's f32
#: accumulators alone would be 128 registers per lane)
GLM_FAMILY_BATCHED_K = (8, 16, 32, 64, 128, 256, 512, 1024)
#: links of fed_glm_family_batched (the logistic models keep their own kernels)
_GLM_FAMILY_BATCHED_LINKS = ("poisson", "gaussian")
#: fp32 slab workspace: the largest grid of any K times its slab rows
_GLM_FAMILY_BATCHED_WS = 8 << 20


def glm_family_batched_supports(dtype, K: int) -> bool:
    """True for bf16 shards with K in :data:`GLM_FAMILY_BATCHED_K`."""
    return dtype == torch.bfloat16 and int(K) in GLM_FAMILY_BATCHED_K


def glm_family_logp_grad_batched(
    X: torch.Tensor,
    y: torch.Tensor,
    theta: torch.Tensor,
    *,
    link: str,
    offset: Optional[torch.Tensor] = None,
    sigma: float = 1.0,
    logp_const: float = 0.0,
    out: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """16 chains of a Poisson or Gaussian GLM in one pass over X, on the
    matrix cores (csrc/glm_family_batched.hip): ``theta[K,16]`` ->
    ``(logp[16], G[K,16])`` as fp64 views of ``out`` (fp64[16 + K*16]).

    ``X[N,K]`` is bf16 with K in :data:`GLM_FAMILY_BATCHED_K`; ``y`` and
    ``offset`` are f32[N].  theta is handed to the kernel as the three bf16
    pieces of :func:`split_bf16x3` and the residual is split the same way on
    the device, so no operand is rounded: the result is as accurate as the
    single-chain kernel's.  f32 shards are not covered: gfx950's f32-input
    MFMA runs at 1/16 of the bf16 rate and there is no xf32 format.
    ``logp_const`` is added to every chain on the device.
    """
    lib = require_kernels()
    if link not in _GLM_FAMILY_BATCHED_LINKS:
        raise ValueError(
            f"unknown link {link!r}; expected one of {sorted(_GLM_FAMILY_BATCHED_LINKS)}"
        )
    n, K = _design_shape(X)
    B = BATCH_CHAINS
    if X.dtype != torch.bfloat16:
        raise TypeError(f"unsupported dtype {X.dtype}: the batched family kernel reads bf16 X")
    if not glm_family_batched_supports(X.dtype, K):
        raise ValueError(f"batched family kernel not compiled for (dtype={X.dtype}, K={K})")
    _check_sigma(sigma)
    _check_rows("y", y, X)
    if offset is not None:
        _check_rows("offset", offset, X)
    _check_design(X)
    if tuple(theta.shape) != (K, B):
        raise ValueError(f"theta must be [{K}, {B}], got {tuple(theta.shape)}")
    pieces = split_bf16x3(theta.to(device=X.device))
    out = _out_buffer(out, (B + K * B,), X)
    ws = _workspace(X.device, "glm_family_batched", _GLM_FAMILY_BATCHED_WS, dtype=torch.float32)
    rc = lib.fed_glm_family_batched(
        X.data_ptr(), y.data_ptr(), offset.data_ptr() if offset is not None else None,
        n, K, pieces.data_ptr(), _GLM_FAMILY_BATCHED_LINKS.index(link),
        float(sigma), float(logp_const),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(),
    )
    _check(rc, "fed_glm_family_batched")
    return out[:B], out[B:].reshape(K, B)


#: classes the softmax stage of the batched family kernel covers: its 16
#: MFMA columns hold 16 // CP chains of CP class slots each
GLM_SOFTMAX_MAX_CLASSES = BATCH_CHAINS


def glm_softmax_class_group(n_classes: int) -> int:
    """CP: the class-group width, the next power of two >= ``n_classes``
    (2, 4, 8 or 16).  One launch carries ``16 // CP`` chains."""
    n_classes = int(n_classes)
    if not 2 <= n_classes <= GLM_SOFTMAX_MAX_CLASSES:
        raise ValueError(
            f"n_classes must be in [2, {GLM_SOFTMAX_MAX_CLASSES}], got {n_classes}"
        )
    cp = 2
    while cp < n_classes:
        cp *= 2
    return cp


def glm_softmax_supports(dtype, K: int, n_classes: int) -> bool:
    """True for bf16 shards with K in :data:`GLM_FAMILY_BATCHED_K` and
    2 <= ``n_classes`` <= 16."""
    return (
        glm_family_batched_supports(dtype, K)
        and 2 <= int(n_classes) <= GLM_SOFTMAX_MAX_CLASSES
    )


def glm_softmax_logp_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    theta16: torch.Tensor,
    *,
    n_classes: int,
    out: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``16 // CP`` chains of a softmax (multinomial) GLM in one pass over X,
    on the matrix cores (csrc/glm_family_batched.hip with the row-coupled
    softmax stage): ``(logp[16 // CP], G[K,16])``.

    ``theta16[K,16]`` is the packed image: with ``CP =
    glm_softmax_class_group(n_classes)``, column ``g*CP + c`` is class ``c``
    of chain ``g``.  Columns of padded classes (``c >= n_classes``) are not
    read into any result and their columns of ``G`` are exactly 0.
    ``X[N,K]`` is bf16 with K in :data:`GLM_FAMILY_BATCHED_K`; ``y`` holds
    the labels in ``[0, n_classes)`` as f32[N].  theta travels as the three
    bf16 pieces of :func:`split_bf16x3` and the residual is split the same
    way on the device, so no operand is rounded.  ``G`` is an fp64 view of
    ``out`` (fp64[16 + K*16]); ``logp`` sums the per-column fp64 sums in
    ``out[:16]`` over each class group.
    """
    lib = require_kernels()
    n, K = _design_shape(X)
    B = BATCH_CHAINS
    if X.dtype != torch.bfloat16:
        raise TypeError(f"unsupported dtype {X.dtype}: the softmax kernel reads bf16 X")
    if not glm_family_batched_supports(X.dtype, K):
        raise ValueError(f"softmax kernel not compiled for (dtype={X.dtype}, K={K})")
    cp = glm_softmax_class_group(n_classes)
    _check_rows("y", y, X)
    _check_design(X)
    if tuple(theta16.shape) != (K, B):
        raise ValueError(f"theta16 must be [{K}, {B}], got {tuple(theta16.shape)}")
    pieces = split_bf16x3(theta16.to(device=X.device))
    out = _out_buffer(out, (B + K * B,), X)
    ws = _workspace(X.device, "glm_softmax", _GLM_FAMILY_BATCHED_WS, dtype=torch.float32)
    rc = lib.fed_glm_softmax_batched(
        X.data_ptr(), y.data_ptr(), n, K, pieces.data_ptr(), int(n_classes),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(),
    )
    _check(rc, "fed_glm_softmax_batched")
    return out[:B].reshape(B // cp, cp).sum(dim=1), out[B:].reshape(K, B)


#: feature counts the Fisher kernel is compiled for (the batched kernel's)
GLM_FAMILY_FISHER_K = (8, 16, 32, 64, 128, 256, 512, 1024)
#: fp32 slab of the Fisher kernel: at most 512 resident blocks (256 CUs x 2)
#: of one 128 x 128 f32 panel pair each = 32 MiB (K < 128: 1024 blocks x 4
#: slab rows of K*K floats at most, under 4 MiB).  For K > 128 the workspace
#: also holds one f32 weight per row ahead of the slab.
_GLM_FAMILY_FISHER_SLAB = (512 * 128 * 128 * 4) // 4


def glm_family_fisher_supports(dtype, K: int) -> bool:
    """True for bf16 shards with K in :data:`GLM_FAMILY_FISHER_K`."""
    return dtype == torch.bfloat16 and int(K) in GLM_FAMILY_FISHER_K


def glm_family_fisher_tile_rows(K: int) -> int:
    """Rows per tile of the Fisher kernel at ``K`` (its edge-shape tests
    take their row counts from it)."""
    return int(require_kernels().fed_glm_family_fisher_tile_rows(int(K)))


def glm_family_fisher(
    X: torch.Tensor,
    beta: torch.Tensor,
    *,
    link: str,
    offset: Optional[torch.Tensor] = None,
    sigma: float = 1.0,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fisher information ``H = X^T diag(w) X`` of a Poisson or Gaussian GLM
    on the matrix cores (csrc/glm_family_fisher.hip), as fp64[K,K].

    ``w = exp(z)`` (Poisson) or ``1/sigma^2`` (Gaussian) with ``z = X @ beta
    (+ offset)``; both links are canonical, so ``H`` is the negative Hessian
    of logp.  ``X[N,K]`` is bf16 with K in :data:`GLM_FAMILY_FISHER_K`,
    ``offset`` f32[N], ``beta`` any float [K] (used in f32, never rounded to
    bf16).  ``w*x`` is split into three bf16 pieces on the device, so no
    operand of the MFMA is rounded.  The result is exactly symmetric.
    """
    if link not in _GLM_FAMILY_BATCHED_LINKS:
        raise ValueError(
            f"unknown link {link!r}; expected one of {sorted(_GLM_FAMILY_BATCHED_LINKS)}"
        )
    n, K = _design_shape(X)
    if X.dtype != torch.bfloat16:
        raise TypeError(f"unsupported dtype {X.dtype}: the Fisher kernel reads bf16 X")
    if not glm_family_fisher_supports(X.dtype, K):
        raise ValueError(f"Fisher kernel not compiled for (dtype={X.dtype}, K={K})")
    _check_sigma(sigma)
    if tuple(beta.shape) != (K,):
        raise ValueError(f"beta must have shape ({K},), got {tuple(beta.shape)}")
    if offset is not None:
        _check_rows("offset", offset, X)
    _check_design(X)
    out = _out_buffer(out, (K, K), X)
    lib = require_kernels()
    beta_f32 = beta.detach().to(device=X.device, dtype=torch.float32).contiguous()
    w_elems = 4 * ((n + 3) // 4) if K > 128 else 0
    ws = _workspace(
        X.device, "glm_family_fisher", _GLM_FAMILY_FISHER_SLAB + w_elems, dtype=torch.float32
    )
    rc = lib.fed_glm_family_fisher(
        X.data_ptr(), offset.data_ptr() if offset is not None else None,
        n, K, beta_f32.data_ptr(), _GLM_FAMILY_BATCHED_LINKS.index(link), float(sigma),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(),
    )
    _check(rc, "fed_glm_family_fisher")
    return out


def _glm_family_fvp(
    X: torch.Tensor,
    beta: torch.Tensor,
    v: Optional[torch.Tensor],
    *,
    link: str,
    offset: Optional[torch.Tensor],
    sigma: float,
    out: Optional[torch.Tensor],
) -> torch.Tensor:
    """What the product and the diagonal share: ``v is None`` is the diagonal."""
    if link not in GLM_FAMILY_LINKS:
        raise ValueError(f"unknown link {link!r}; expected one of {sorted(GLM_FAMILY_LINKS)}")
    n, K = _design_shape(X)
    if X.dtype not in _GLM_FAMILY_VEC:
        raise TypeError(f"unsupported dtype {X.dtype}")
    if not glm_family_kernel_supports(X.dtype, K):
        raise ValueError(f"family kernel not compiled for (dtype={X.dtype}, K={K})")
    _check_sigma(sigma)
    if tuple(beta.shape) != (K,):
        raise ValueError(f"beta must have shape ({K},), got {tuple(beta.shape)}")
    if v is not None and tuple(v.shape) != (K,):
        raise ValueError(f"v must have shape ({K},), got {tuple(v.shape)}")
    if offset is not None:
        _check_rows("offset", offset, X)
    _check_design(X)
    out = _out_buffer(out, (K,), X)
    lib = require_kernels()
    beta_f32 = beta.detach().to(device=X.device, dtype=torch.float32).contiguous()
    v_f32 = None if v is None else v.detach().to(device=X.device, dtype=torch.float32).contiguous()
    # a slab of its own: glm_family_logp_grad's may be in use on another stream
    ws = _workspace(X.device, f"glm_family_fvp{K}", 1024 * K, dtype=torch.float32)
    rc = lib.fed_glm_family_fvp(
        X.data_ptr(), offset.data_ptr() if offset is not None else None, n, K,
        beta_f32.data_ptr(), v_f32.data_ptr() if v_f32 is not None else None,
        GLM_FAMILY_LINKS[link], float(sigma),
        out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
        _DTYPE_CODE[X.dtype], _stream_ptr(),
    )
    _check(rc, "fed_glm_family_fvp")
    return out


def glm_family_fisher_vector(
    X: torch.Tensor,
    beta: torch.Tensor,
    v: torch.Tensor,
    *,
    link: str,
    offset: Optional[torch.Tensor] = None,
    sigma: float = 1.0,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fisher-vector product ``H v = X^T (w * (X v))`` of a GLM in one pass
    over X (csrc/glm_family_fvp.hip), as fp64[K]; no ``K x K`` object is formed.

    ``w = exp(z)`` (``"poisson"``), ``1/sigma^2`` (``"gaussian"``) or
    ``mu (1 - mu)``, ``mu = sigmoid(z)`` (``"logistic"``), with ``z = X @ beta
    (+ offset)``.  ``X[N,K]`` is bf16 or f32 with K one of the sizes of
    :func:`glm_family_padded_k`; ``offset`` is f32[N]; ``beta`` and ``v`` are
    any float [K], used in f32.
    """
    if v is None:
        raise ValueError("v must have shape (K,); see glm_family_fisher_diagonal")
    return _glm_family_fvp(X, beta, v, link=link, offset=offset, sigma=sigma, out=out)


def glm_family_fisher_diagonal(
    X: torch.Tensor,
    beta: torch.Tensor,
    *,
    link: str,
    offset: Optional[torch.Tensor] = None,
    sigma: float = 1.0,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``diag(H)[k] = sum_r w_r x_rk^2`` as fp64[K], by the kernel of
    :func:`glm_family_fisher_vector` and under the same conditions: the
    Jacobi preconditioner of a conjugate-gradient solve with ``H``."""
    return _glm_family_fvp(X, beta, None, link=link, offset=offset, sigma=sigma, out=out)
