"""Poisson and Gaussian GLM logp+grad models on the row-group fused kernel.

Parameters ``beta[K]``, private shard ``X[N,K]``, ``y[N]`` and the linear
predictor ``z = X @ beta (+ offset)``:

Poisson regression (log link, optional exposure ``offset = log(exposure)``)

    logp = sum( y*z - exp(z) ) - sum( lgamma(y+1) )
    grad = X^T @ (y - exp(z))

Gaussian regression on K covariates (identity link, fixed ``sigma``)

    r    = y - z
    logp = -N/2 * log(2*pi*sigma^2) - sum(r^2) / (2*sigma^2)
    grad = X^T @ r / sigma^2

Compute paths:
* eager torch (CPU, ``use_kernels=False``, shapes the kernel does not
  cover): a matmul each way + elementwise; fp64 data -> fp64 math,
  otherwise fp32 with fp64 row sums;
* MI355X: ONE fused CDNA4 HIP kernel (``ops.glm_family_logp_grad``,
  csrc/glm_family.hip) reading X exactly once.  A group of G <= 64 lanes
  owns a row, so a narrow model is read at its own size: the feature dim is
  zero-padded only to the next power-of-two multiple of one 16-byte vector
  (8 bf16 / 4 f32), K = 20 -> 32, not to a whole wave.  ``y`` and
  ``offset`` are kept in f32 whatever the dtype of X (counts above 256 do
  not survive bf16).  The beta-independent part of logp is added on the
  device.
* MI355X, several chains (``logp_grad_batched``): bf16 shards go 16 chains
  at a time through the MFMA kernel ``ops.glm_family_logp_grad_batched``
  (csrc/glm_family_batched.hip), one pass over X for all 16; theta and the
  residual travel as three bf16 pieces each, so nothing is rounded to bf16.

Fisher information (``fisher_information``): ``H = X^T diag(w) X`` with
``w = exp(z)`` (Poisson) or ``1/sigma^2`` (Gaussian).  Both links are
canonical, so ``H`` is the expected and the observed information, the
negative Hessian of ``logp``; it is a sum over rows, so shard matrices add.
bf16 shards on the MI355X go through the MFMA kernel
``ops.glm_family_fisher`` (csrc/glm_family_fisher.hip); everything else is
a chunked eager ``X^T @ (w X)``.

Fisher-vector product and diagonal (``fisher_vector_product``,
``fisher_diagonal``; models/fisher_vector.py): ``H v`` and ``diag(H)`` in one
pass over the shard each, a K-vector as the result.  On the MI355X they run
on ``ops.glm_family_fisher_vector`` (csrc/glm_family_fvp.hip) wherever
``logp_grad`` runs on its kernel, f32 shards and a padded K of 2048 included.

Overflow: the fp32 paths (the kernel, and eager on bf16/f32 data) form
``exp(z)`` in fp32.  For a row with ``z > 88`` that is ``inf``, so the
Poisson ``logp`` is ``-inf`` and the gradient is not finite, in both paths
alike.  Only fp64 data evaluated eagerly goes further (to ``z ~ 709``).
Counts are exact in f32 up to 2^24.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from .fisher_vector import FisherVectorMixin
from .shard import ShardGLMModel, _as_tensor

__all__ = [
    "PoissonGLMModel",
    "GaussianGLMModel",
    "generate_poisson_dataset",
    "generate_gaussian_glm_dataset",
]


def generate_poisson_dataset(
    n_rows: int,
    n_features: int,
    *,
    seed: int = 0,
    beta_scale: float = 0.5,
    exposure: bool = True,
) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], np.ndarray]:
    """Synthetic (X, y, offset, beta_true) count data.

    ``X[:, 0] = 1`` (intercept), the other columns are standard normal over
    sqrt(K), so ``z`` stays of order ``beta_scale``.  With ``exposure`` each
    row gets an exposure in [0.5, 2] and ``offset = log(exposure)``;
    otherwise ``offset`` is ``None``.
    """
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n_rows, n_features)) / np.sqrt(n_features)
    X[:, 0] = 1.0
    beta = rng.standard_normal(n_features) * beta_scale
    offset = np.log(rng.uniform(0.5, 2.0, size=n_rows)) if exposure else None
    z = X @ beta + (offset if exposure else 0.0)
    y = rng.poisson(np.exp(z)).astype(np.float64)
    return X, y, offset, beta


def generate_gaussian_glm_dataset(
    n_rows: int,
    n_features: int,
    *,
    sigma: float = 0.5,
    seed: int = 0,
    beta_scale: float = 0.5,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Synthetic (X, y, beta_true) with ``y ~ N(X @ beta, sigma^2)``."""
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n_rows, n_features)) / np.sqrt(n_features)
    X[:, 0] = 1.0
    beta = rng.standard_normal(n_features) * beta_scale
    y = X @ beta + sigma * rng.standard_normal(n_rows)
    return X, y, beta


class _GLMFamilyModel(FisherVectorMixin, ShardGLMModel):
    """What the families share on top of the shard base: the offset, the
    kernel/eager dispatch and the Fisher information.  A family names
    its ``_link`` and gives ``_terms`` (the eager per-row logp term and
    residual) and ``_logp_const``."""

    _link: str = ""

    def __init__(
        self,
        X,
        y,
        *,
        offset=None,
        device=None,
        dtype: torch.dtype = None,
        use_kernels: Optional[bool] = None,
        delay: Optional[float] = None,
    ) -> None:
        super().__init__(delay=delay)
        X, y = _as_tensor(X), _as_tensor(y)
        self._check_shard(X, y)
        if offset is not None:
            offset = _as_tensor(offset)
            if offset.shape != y.shape:
                raise ValueError("offset must be [N].")
        device, dtype = self._placement(X, device, dtype)
        # y and offset: f32 (what the kernel reads) unless the shard is fp64
        self._acc_dtype = torch.float64 if dtype == torch.float64 else torch.float32
        X = X.to(device=device, dtype=dtype)
        self._y = y.to(device=device, dtype=self._acc_dtype).contiguous()
        self._offset = (
            None if offset is None
            else offset.to(device=device, dtype=self._acc_dtype).contiguous()
        )
        self._set_shard(X, use_kernels)

    # -- what a family provides -------------------------------------------
    def _terms(self, y: torch.Tensor, z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(per-row logp term, residual d term / d z), shaped like ``z``."""
        raise NotImplementedError

    def _weights(self, z: torch.Tensor) -> torch.Tensor:
        """Fisher weight ``-d^2 term / dz^2`` per row, shaped like ``z``."""
        raise NotImplementedError

    _logp_const: float = 0.0
    _sigma: float = 1.0

    # -- shared -------------------------------------------------------------
    def _kernel_path(self) -> bool:
        want = self._want_kernels()
        if want and self._use_kernels is None:
            from ..ops import glm_family_kernel_supports

            if not glm_family_kernel_supports(self._X.dtype, self._k_eff):
                import warnings

                warnings.warn(
                    f"fused GLM family kernel not compiled for (dtype={self._X.dtype}, "
                    f"K={self._k_eff}); using the eager two-matmul path (~2x slower). "
                    f"Supported: bf16 up to K=2048, f32 up to K=1024.",
                    stacklevel=3,
                )
                return False
        return want

    def logp_grad(
        self, beta, out: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """``out`` (fp64[1+K], same device) receives the fused [logp, grad]
        in place -- the zero-copy seam to the RCCL all-reduce buffer."""
        beta = torch.as_tensor(beta)
        if beta.shape != (self._k,):
            raise ValueError(f"beta must have shape ({self._k},), got {tuple(beta.shape)}.")
        if self._kernel_path():
            from ..ops import glm_family_logp_grad

            kw = dict(
                link=self._link, offset=self._offset, sigma=self._sigma,
                logp_const=self._logp_const,
            )
            if self._k_pad:
                # ``out`` (if given) is sized [1 + k]; the kernel writes
                # [1 + k_eff] -- evaluate into the kernel's own buffer and
                # copy the un-padded slice over.
                logp, grad = glm_family_logp_grad(self._X, self._y, self._pad_rows(beta), **kw)
                logp, grad = self._into_out(out, logp, grad[: self._k])
                return logp, [grad]
            logp, grad = glm_family_logp_grad(self._X, self._y, beta, out=out, **kw)
            return logp, [grad]
        logp, grads = self._logp_grad_eager(beta)
        logp, grad = self._into_out(out, logp, grads[0])
        return logp, [grad]

    def _logp_grad_eager(self, beta: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        logp, G = self._logp_grad_batched_eager(beta.reshape(self._k, 1))
        return logp[0], [G[:, 0]]

    def logp_grad_batched(self, theta) -> Tuple[torch.Tensor, torch.Tensor]:
        """Evaluate B chains at once: theta[K,B] -> (logp[B], G[K,B]).

        On the kernel path with a bf16 shard whose padded K is one of
        ``ops.GLM_FAMILY_BATCHED_K`` (up to 1024) the chains go through the
        MFMA batched family kernel in groups of 16, the last group padded
        with zero columns; theta and the residual are carried as three bf16
        pieces each, so the result is as accurate as ``logp_grad``'s.
        Everything else is eager torch: CPU, ``use_kernels=False``, f32 and
        f64 shards (gfx950's f32-input MFMA runs at 1/16 of the bf16 rate
        and there is no xf32), and a padded K of 2048, which warns."""
        theta = torch.as_tensor(theta)
        if theta.dim() != 2 or theta.shape[0] != self._k:
            raise ValueError(f"theta must be [{self._k}, B], got {tuple(theta.shape)}")
        if self._batched_kernel_path():
            return self._logp_grad_batched_kernel(theta)
        return self._logp_grad_batched_eager(theta)

    def _batched_kernel_path(self) -> bool:
        if self._X.dtype != torch.bfloat16 or not self._kernel_path():
            return False
        from ..ops import glm_family_batched_supports

        if not glm_family_batched_supports(self._X.dtype, self._k_eff):
            import warnings

            warnings.warn(
                f"batched GLM family kernel not compiled for K={self._k_eff}; "
                f"using the eager batched path. Supported: bf16 up to K=1024.",
                stacklevel=3,
            )
            return False
        return True

    def _logp_grad_batched_kernel(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        from ..ops import BATCH_CHAINS, glm_family_logp_grad_batched

        dev = self._X.device
        B = theta.shape[1]
        kw = dict(link=self._link, offset=self._offset, sigma=self._sigma,
                  logp_const=self._logp_const)
        if B == BATCH_CHAINS and not self._k_pad:
            # the samplers' shape: nothing to pad, slice or copy
            return glm_family_logp_grad_batched(self._X, self._y, theta, **kw)
        groups = -(-B // BATCH_CHAINS)
        # padded feature rows and padded chains are zero columns / rows of theta
        th = torch.zeros(
            (self._k_eff, groups * BATCH_CHAINS), dtype=torch.float32, device=dev
        )
        th[: self._k, :B] = theta.to(device=dev, dtype=torch.float32)
        logp = torch.empty(groups * BATCH_CHAINS, dtype=torch.float64, device=dev)
        G = torch.empty((self._k, groups * BATCH_CHAINS), dtype=torch.float64, device=dev)
        for g in range(groups):
            cols = slice(g * BATCH_CHAINS, (g + 1) * BATCH_CHAINS)
            lg, Gg = glm_family_logp_grad_batched(self._X, self._y, th[:, cols], **kw)
            logp[cols] = lg
            G[:, cols] = Gg[: self._k]
        return logp[:B], G[:, :B]

    def _logp_grad_batched_eager(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        X = self._X[:, : self._k]
        acc = self._acc_dtype
        theta = theta.to(device=X.device, dtype=acc)
        B = theta.shape[1]
        logp = torch.full((B,), self._logp_const, dtype=torch.float64, device=X.device)
        G = torch.zeros((self._k, B), dtype=torch.float64, device=X.device)
        for rows in self._row_chunks(X.dtype != acc):
            Xf = X[rows].to(acc)
            Z = Xf @ theta
            if self._offset is not None:
                Z = Z + self._offset[rows, None]
            term, resid = self._terms(self._y[rows, None], Z)
            logp += torch.sum(term, dim=0, dtype=torch.float64)
            G += (Xf.t() @ resid).to(torch.float64)
        return logp, G

    # -- Fisher information --------------------------------------------------
    def fisher_information(self, beta, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``H(beta) = X^T diag(w(z)) X`` as fp64[K,K]: the negative Hessian
        of ``logp`` (both links are canonical, so also the expected Fisher
        information).  Zero-padded columns are sliced off.  ``out``
        (fp64[K,K], same device) receives the result in place.

        bf16 shards on the kernel path whose padded K is one of
        ``ops.GLM_FAMILY_FISHER_K`` (up to 1024) go through the MFMA kernel
        ``ops.glm_family_fisher``, where ``w*x`` is carried as three bf16
        pieces so that no operand is rounded.  Everything else is eager
        torch: CPU, ``use_kernels=False``, f32 and f64 shards, and a padded
        K of 2048, which warns."""
        beta = torch.as_tensor(beta)
        if beta.shape != (self._k,):
            raise ValueError(f"beta must have shape ({self._k},), got {tuple(beta.shape)}.")
        if out is not None and (
            out.dtype != torch.float64 or out.shape != (self._k, self._k)
            or out.device != self._X.device
        ):
            raise ValueError(f"out must be fp64[{self._k}, {self._k}] on the shard's device")
        if self._fisher_kernel_path():
            from ..ops import glm_family_fisher

            kw = dict(link=self._link, offset=self._offset, sigma=self._sigma)
            beta = beta.to(device=self._X.device, dtype=torch.float32)
            if self._k_pad:
                H = glm_family_fisher(self._X, self._pad_rows(beta), **kw)[: self._k, : self._k]
            elif out is not None and out.is_contiguous():
                return glm_family_fisher(self._X, beta, out=out, **kw)
            else:
                H = glm_family_fisher(self._X, beta, **kw)
        else:
            H = self._fisher_eager(beta)
        if out is not None:
            out.copy_(H)
            return out
        return H

    def _fisher_kernel_path(self) -> bool:
        if self._X.dtype != torch.bfloat16 or not self._kernel_path():
            return False
        from ..ops import glm_family_fisher_supports

        if not glm_family_fisher_supports(self._X.dtype, self._k_eff):
            import warnings

            warnings.warn(
                f"GLM Fisher kernel not compiled for K={self._k_eff}; "
                f"using the eager path. Supported: bf16 up to K=1024.",
                stacklevel=3,
            )
            return False
        return True

    #: rows of one f32 chain of the eager Fisher matmul on a GPU.  The
    #: device's f32 GEMM adds a long reduction in one chain, and its error
    #: grows with the length: over 5000 rows up to 133 units of 2^-24 *
    #: H_scale, at 128 rows 3.3 (measured on the accuracy sets).  The chains
    #: are added in fp64.
    _FISHER_CHAIN_ROWS = 128

    def _fisher_eager(self, beta: torch.Tensor) -> torch.Tensor:
        X = self._X[:, : self._k]
        acc = self._acc_dtype
        K = self._k
        beta = beta.to(device=X.device, dtype=acc)
        H = torch.zeros((K, K), dtype=torch.float64, device=X.device)
        # short f32 chains on a GPU (one batched matmul per step, at most
        # 256 MB of chain results); fp64 data and the CPU's BLAS need none
        R = self._FISHER_CHAIN_ROWS if (X.is_cuda and acc != torch.float64) else 0
        cap = R * max(1, (1 << 26) // (K * K)) if R else None
        for rows in self._row_chunks(X.dtype != acc, cap):
            Xf = X[rows].to(acc)
            z = Xf @ beta
            if self._offset is not None:
                z = z + self._offset[rows]
            WX = self._weights(z)[:, None] * Xf
            full = (Xf.shape[0] // R) * R if R else 0
            if full:
                H += torch.bmm(
                    Xf[:full].reshape(-1, R, K).transpose(1, 2), WX[:full].reshape(-1, R, K)
                ).sum(dim=0, dtype=torch.float64)
            if full < Xf.shape[0]:
                H += (Xf[full:].t() @ WX[full:]).to(torch.float64)
        # X^T (w X) is symmetric only up to the matmul's rounding
        return 0.5 * (H + H.t())

    def as_fisher_func(self):
        """A ``ComputeFunc``: numpy ``beta`` -> ``[H]`` (fp64[K,K]), which a
        worker serves through ``ArraysToArraysService`` like any other."""

        def fisher_func(beta):
            # copy: wire-decoded arrays are read-only zero-copy views
            b = torch.from_numpy(np.array(beta, dtype=np.float64))
            H = self.fisher_information(b)
            return [np.asarray(H.detach().cpu().double().numpy())]

        return fisher_func

    # -- Fisher-vector product (FisherVectorMixin) ----------------------------
    def _fvp_kernel_path(self) -> bool:
        return self._kernel_path()


class PoissonGLMModel(_GLMFamilyModel):
    """Federated worker model: Poisson regression (log link) on a private
    shard of counts, with an optional exposure offset."""

    _link = "poisson"

    def __init__(
        self,
        X,
        y,
        *,
        offset=None,
        device=None,
        dtype: torch.dtype = None,
        use_kernels: Optional[bool] = None,
        delay: Optional[float] = None,
    ) -> None:
        """
        Parameters
        ----------
        X, y : array-like
            ``X[N,K]`` covariates and ``y[N]`` non-negative integer counts.
        offset : array-like, optional
            ``offset[N]`` added to ``X @ beta`` (``log(exposure)``).
        device, dtype, use_kernels, delay
            As for :class:`LogisticGLMModel`; ``dtype`` is the storage type
            of ``X`` only.
        """
        y64 = _as_tensor(y).detach().to(device="cpu", dtype=torch.float64)
        if y64.dim() == 1 and y64.numel():
            if not bool(torch.all(torch.isfinite(y64))):
                raise ValueError("Poisson y must be finite.")
            if bool(torch.any(y64 < 0)) or bool(torch.any(y64 != torch.floor(y64))):
                raise ValueError("Poisson y must hold non-negative integer counts.")
        super().__init__(
            X, y, offset=offset, device=device, dtype=dtype, use_kernels=use_kernels,
            delay=delay,
        )
        # the beta-independent part of logp, once, in fp64
        self._logp_const = -float(torch.sum(torch.lgamma(y64 + 1.0)))

    def _terms(self, y, z):
        mu = torch.exp(z)
        return y * z - mu, y - mu

    def _weights(self, z):
        return torch.exp(z)


class GaussianGLMModel(_GLMFamilyModel):
    """Federated worker model: Gaussian regression on K covariates
    (identity link, fixed noise scale) on a private shard."""

    _link = "gaussian"

    def __init__(
        self,
        X,
        y,
        sigma: float,
        *,
        offset=None,
        device=None,
        dtype: torch.dtype = None,
        use_kernels: Optional[bool] = None,
        delay: Optional[float] = None,
    ) -> None:
        sigma = float(sigma)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError("sigma must be positive and finite.")
        super().__init__(
            X, y, offset=offset, device=device, dtype=dtype, use_kernels=use_kernels,
            delay=delay,
        )
        self._sigma = sigma
        self._logp_const = -0.5 * self._n * math.log(2.0 * math.pi * sigma * sigma)

    def _terms(self, y, z):
        r = y - z
        sig2 = self._sigma * self._sigma
        return -(r * r) * (0.5 / sig2), r * (1.0 / sig2)

    def _weights(self, z):
        return torch.full_like(z, 1.0 / (self._sigma * self._sigma))
