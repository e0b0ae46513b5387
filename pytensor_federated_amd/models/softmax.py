"""Softmax (multinomial logistic) GLM logp+grad model.

Parameters ``beta[K, C]`` for C >= 2 classes, private shard ``X[N,K]`` and
integer labels ``y[N]`` in ``[0, C)``.  With ``Z = X @ beta``:

    logp = sum_n ( Z[n, y_n] - logsumexp_c Z[n, c] )
    grad = X^T @ ( onehot(y) - softmax(Z) )                  # [K, C]

The parameterisation is the full one: no reference class is pinned, so
``beta`` and ``beta + v[:, None]`` (the same vector added to every class
column) have the same logp and the likelihood alone does not identify
``beta``.  A client that wants identifiability pins a column (passes zeros
for it and ignores its gradient) or puts a prior on ``beta``.  There is no
``offset``: a per-row shift cancels in the softmax.

Compute paths:
* eager torch (CPU, ``use_kernels=False``, f32 and f64 shards, a padded K of
  2048, C > 16): ``log_softmax`` of a matmul and a matmul back; fp64 data ->
  fp64 math, otherwise fp32 with fp64 row sums for logp and fp64
  accumulation of the gradient over row chunks;
* MI355X, bf16 shard, padded K <= 1024, C <= 16: the 16-column MFMA kernel
  of the GLM families with its row-coupled softmax stage
  (``ops.glm_softmax_logp_grad``, csrc/glm_family_batched.hip).  The 16
  columns hold ``16 // CP`` chains of ``CP`` class slots each (``CP`` the
  next power of two >= C), so ``logp_grad_batched`` evaluates four chains of
  a four-class model in one pass over X.  The row maximum is subtracted
  before the exponential: ``|z|`` in the thousands gives a finite logp.
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Tuple

import numpy as np
import torch

from .shard import ShardGLMModel, _as_tensor

__all__ = ["SoftmaxGLMModel", "generate_softmax_dataset"]


def generate_softmax_dataset(
    n_rows: int,
    n_features: int,
    n_classes: int,
    *,
    seed: int = 0,
    beta_scale: float = 1.0,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Synthetic (X, y, beta_true) categorical data.

    ``X[:, 0] = 1`` (intercept), the other columns are standard normal over
    sqrt(K), so ``Z = X @ beta`` stays of order ``beta_scale``; ``beta`` is
    ``[K, C]`` and ``y[n]`` is drawn from ``softmax(Z[n])``.
    """
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n_rows, n_features)) / np.sqrt(n_features)
    X[:, 0] = 1.0
    beta = rng.standard_normal((n_features, n_classes)) * beta_scale
    Z = X @ beta
    P = np.exp(Z - Z.max(axis=1, keepdims=True))
    P /= P.sum(axis=1, keepdims=True)
    u = rng.uniform(size=(n_rows, 1))
    y = np.minimum((np.cumsum(P, axis=1) < u).sum(axis=1), n_classes - 1).astype(np.int64)
    return X, y, beta


class SoftmaxGLMModel(ShardGLMModel):
    """Federated worker model: multinomial logistic regression on a private
    shard of categorical responses (full parameterisation, see the module
    docstring for identifiability)."""

    def __init__(
        self,
        X,
        y,
        n_classes: Optional[int] = None,
        *,
        device=None,
        dtype: torch.dtype = None,
        use_kernels: Optional[bool] = None,
        delay: Optional[float] = None,
    ) -> None:
        """
        Parameters
        ----------
        X, y : array-like
            ``X[N,K]`` covariates and ``y[N]`` integer labels in
            ``[0, n_classes)``.
        n_classes : int, optional
            C >= 2; defaults to ``max(y) + 1``.
        device, dtype, use_kernels, delay
            As for :class:`LogisticGLMModel`; ``dtype`` is the storage type
            of ``X`` only.
        """
        super().__init__(delay=delay)
        X, y = _as_tensor(X), _as_tensor(y)
        self._check_shard(X, y)
        y64 = y.detach().to(device="cpu", dtype=torch.float64)
        if y64.numel():
            if not bool(torch.all(torch.isfinite(y64))) or bool(
                torch.any(y64 != torch.floor(y64))
            ):
                raise ValueError("softmax y must hold integer class labels.")
            if bool(torch.any(y64 < 0)):
                raise ValueError("softmax y must hold non-negative class labels.")
        if n_classes is None:
            if not y64.numel():
                raise ValueError("n_classes is required when y is empty.")
            n_classes = int(y64.max()) + 1
        n_classes = int(n_classes)
        if n_classes < 2:
            raise ValueError(f"n_classes must be at least 2, got {n_classes}.")
        if y64.numel() and int(y64.max()) >= n_classes:
            raise ValueError(
                f"softmax y must be below n_classes={n_classes}, got {int(y64.max())}."
            )
        device, dtype = self._placement(X, device, dtype)
        self._acc_dtype = torch.float64 if dtype == torch.float64 else torch.float32
        X = X.to(device=device, dtype=dtype)
        self._labels = y64.to(device=device, dtype=torch.int64).contiguous()
        # what the kernel reads: labels as f32 (exact far beyond 16 classes)
        self._y = self._labels.to(torch.float32).contiguous()
        self._c = n_classes
        self._set_shard(X, use_kernels)

    # -- shape --------------------------------------------------------------
    @property
    def n_classes(self) -> int:
        return int(self._c)

    @property
    def fused_size(self) -> int:
        """Layout of the fused fp64 output buffer: [logp, grad[K*C]]
        (row-major in (K, C))."""
        return 1 + int(self._k) * int(self._c)

    @property
    def chains_per_launch(self) -> int:
        """Chains one kernel launch carries: ``16 // CP``."""
        from ..ops import glm_softmax_class_group

        return 16 // glm_softmax_class_group(self._c)

    # -- dispatch -----------------------------------------------------------
    def _kernel_path(self) -> bool:
        """bf16 shard on a ROCm device, padded K <= 1024 and C <= 16; K = 2048
        and C > 16 warn, f32 / f64 shards take eager silently."""
        if not self._want_kernels() or self._X.dtype != torch.bfloat16:
            return False
        from ..ops import GLM_SOFTMAX_MAX_CLASSES, glm_family_batched_supports

        if not glm_family_batched_supports(self._X.dtype, self._k_eff):
            warnings.warn(
                f"softmax GLM kernel not compiled for K={self._k_eff}; "
                f"using the eager path. Supported: bf16 up to K=1024.",
                stacklevel=3,
            )
            return False
        if self._c > GLM_SOFTMAX_MAX_CLASSES:
            warnings.warn(
                f"softmax GLM kernel not compiled for n_classes={self._c}; "
                f"using the eager path. Supported: up to {GLM_SOFTMAX_MAX_CLASSES} classes.",
                stacklevel=3,
            )
            return False
        return True

    # -- single chain -------------------------------------------------------
    def logp_grad(
        self, beta, out: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """``beta[K,C]`` -> ``(logp, [G[K,C]])``.  ``out`` (fp64[1 + K*C],
        same device) receives the fused [logp, grad] in place -- the
        zero-copy seam to the RCCL all-reduce buffer."""
        beta = torch.as_tensor(beta)
        if beta.shape != (self._k, self._c):
            raise ValueError(
                f"beta must have shape ({self._k}, {self._c}), got {tuple(beta.shape)}."
            )
        if out is not None and (
            out.dtype != torch.float64 or out.shape != (self.fused_size,)
            or out.device != self._X.device
        ):
            raise ValueError(f"out must be fp64[{self.fused_size}] on the shard's device")
        logp, G = self._eval(beta.reshape(self._k, self._c, 1))
        logp, G = logp[0], G[:, :, 0]
        if out is not None:
            logp, flat = self._into_out(out, logp, G.reshape(-1))
            G = flat.view(self._k, self._c)
        return logp, [G]

    # -- several chains -----------------------------------------------------
    def logp_grad_batched(self, theta) -> Tuple[torch.Tensor, torch.Tensor]:
        """Evaluate B chains at once: ``theta[K,C,B]`` -> ``(logp[B],
        G[K,C,B])``, or the flat ``theta[K*C,B]`` (row-major in (K, C), the
        samplers' shape) -> ``(logp[B], G[K*C,B])``.

        On the kernel path ``16 // CP`` chains share one launch, i.e. one
        pass over X (CP = next power of two >= C): ``ceil(B / (16 // CP))``
        launches, the last one padded with zero chains."""
        theta = torch.as_tensor(theta)
        flat = theta.dim() == 2
        if flat:
            if theta.shape[0] != self._k * self._c:
                raise ValueError(
                    f"theta must be [{self._k * self._c}, B] or "
                    f"[{self._k}, {self._c}, B], got {tuple(theta.shape)}"
                )
            theta = theta.reshape(self._k, self._c, theta.shape[1])
        elif theta.dim() != 3 or tuple(theta.shape[:2]) != (self._k, self._c):
            raise ValueError(
                f"theta must be [{self._k * self._c}, B] or "
                f"[{self._k}, {self._c}, B], got {tuple(theta.shape)}"
            )
        logp, G = self._eval(theta)
        if flat:
            G = G.reshape(self._k * self._c, -1)
        return logp, G

    def _eval(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """theta[K,C,B] -> (logp[B], G[K,C,B]) on whichever path applies."""
        if self._kernel_path():
            return self._eval_kernel(theta)
        return self._eval_eager(theta)

    def _eval_kernel(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        from ..ops import BATCH_CHAINS, glm_softmax_class_group, glm_softmax_logp_grad

        dev = self._X.device
        K, C, B = self._k, self._c, theta.shape[2]
        cp = glm_softmax_class_group(C)
        per = BATCH_CHAINS // cp
        launches = -(-B // per)
        # packed images: column g*cp + c of launch l is class c of chain
        # l*per + g; padded feature rows, classes and chains are zeros
        th = torch.zeros((self._k_eff, launches * per, cp), dtype=torch.float32, device=dev)
        th[:K, :B, :C] = theta.to(device=dev, dtype=torch.float32).permute(0, 2, 1)
        th = th.reshape(self._k_eff, launches, BATCH_CHAINS)
        logp = torch.empty(launches * per, dtype=torch.float64, device=dev)
        G = torch.empty((K, launches * per, cp), dtype=torch.float64, device=dev)
        for l in range(launches):
            lg, G16 = glm_softmax_logp_grad(
                self._X, self._y, th[:, l].contiguous(), n_classes=C
            )
            logp[l * per : (l + 1) * per] = lg
            G[:, l * per : (l + 1) * per] = G16[:K].reshape(K, per, cp)
        return logp[:B], G[:, :B, :C].permute(0, 2, 1)

    def _eval_eager(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        X = self._X[:, : self._k]
        acc = self._acc_dtype
        K, C, B = self._k, self._c, theta.shape[2]
        # [K, B*C]: one matmul each way for all chains
        th = theta.to(device=X.device, dtype=acc).permute(0, 2, 1).reshape(K, B * C)
        logp = torch.zeros(B, dtype=torch.float64, device=X.device)
        G = torch.zeros((K, B * C), dtype=torch.float64, device=X.device)
        # on a GPU the [rows, B, C] temporaries: at most 2^27 elements each
        cap = max(1 << 10, (1 << 27) // (B * C)) if X.is_cuda else None
        for chunk in self._row_chunks(X.dtype != acc, cap):
            Xf = X[chunk].to(acc)
            labels = self._labels[chunk]
            rows = Xf.shape[0]
            logsm = torch.log_softmax((Xf @ th).reshape(rows, B, C), dim=2)
            picked = logsm.gather(2, labels[:, None, None].expand(rows, B, 1))[:, :, 0]
            logp += torch.sum(picked, dim=0, dtype=torch.float64)
            resid = -torch.exp(logsm)
            resid.scatter_add_(
                2, labels[:, None, None].expand(rows, B, 1),
                torch.ones((rows, B, 1), dtype=acc, device=X.device),
            )
            G += (Xf.t() @ resid.reshape(rows, B * C)).to(torch.float64)
        return logp, G.reshape(K, B, C).permute(0, 2, 1)
