"""Logistic-GLM logp+grad model (BASELINE.json config 4 family).

The GLM generalization of the reference's ComputeFunc contract
(signatures.py:27-33): parameters ``beta[K]``, private shard ``X[N,K]``,
``y[N] in {0,1}``:

    z    = X @ beta
    logp = sum( y*z - softplus(z) )          (numerically stable BCE)
    grad = X^T @ (y - sigmoid(z))

Compute paths:
* eager torch (CPU fallback / golden reference): two rocBLAS matmuls +
  elementwise;
* MI355X: ONE fused CDNA4 HIP kernel reading X exactly once -- per row-tile
  it computes z, sigmoid, the logp term and the rank-1 grad update while the
  tile is still in registers.  At N=1e8 x K=1024 bf16 the shard is 25.6 GB
  per GPU; the op is HBM-bound, so single-pass is ~2x over the eager
  two-matmul shape.

Second order (``fisher_vector_product``, ``fisher_diagonal``;
models/fisher_vector.py): ``H v = X^T (w * (X v))`` and ``diag(H)`` with
``w = mu (1 - mu)``, one pass over the shard each.  The padded K of the fused
kernel is also a size of the row-group family kernel, so on the MI355X the
stored X goes to ``ops.glm_family_fisher_vector`` with ``link="logistic"`` as
it is; other shapes, the CPU and ``use_kernels=False`` are eager.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .fisher_vector import FisherVectorMixin
from .shard import ShardGLMModel, _as_tensor

__all__ = ["LogisticGLMModel", "generate_logistic_dataset"]


def generate_logistic_dataset(
    n_rows: int,
    n_features: int,
    *,
    seed: int = 0,
    beta_scale: float = 0.5,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Synthetic (X, y, beta_true) with ~balanced classes."""
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n_rows, n_features)) / np.sqrt(n_features)
    beta = rng.standard_normal(n_features) * beta_scale
    p = 1.0 / (1.0 + np.exp(-(X @ beta)))
    y = (rng.uniform(size=n_rows) < p).astype(np.float64)
    return X, y, beta


class LogisticGLMModel(FisherVectorMixin, ShardGLMModel):
    """Federated worker model: logistic regression on a private shard."""

    # what FisherVectorMixin reads: the link of ops.glm_family_fisher_vector,
    # no offset, no noise scale
    _link = "logistic"
    _offset = None
    _sigma = 1.0

    def __init__(
        self,
        X,
        y,
        *,
        device=None,
        dtype: torch.dtype = None,
        use_kernels: Optional[bool] = None,
        delay: Optional[float] = None,
    ) -> None:
        super().__init__(delay=delay)
        X, y = _as_tensor(X), _as_tensor(y)
        device, dtype = self._placement(X, device, dtype)
        X = X.to(device=device, dtype=dtype)
        self._y = y.to(device=device, dtype=dtype).contiguous()
        self._check_shard(X, self._y, min_columns=0)
        self._set_shard(X, use_kernels)

    def _padded_k(self) -> int:
        # the fused kernel's lane-slice granule: 512 bf16 / 256 f32 per
        # wave64 pass
        granule = 512 if self._X.dtype == torch.bfloat16 else 256
        return -(-self._k // granule) * granule

    def _kernel_path(self) -> bool:
        want = self._want_kernels()
        if want and self._use_kernels is None:
            from ..ops import logistic_kernel_supports

            if not logistic_kernel_supports(self._X.dtype, self._k_eff):
                import warnings

                warnings.warn(
                    f"fused logistic kernel not compiled for (dtype={self._X.dtype}, "
                    f"K={self._k_eff}); using the eager two-matmul path (~2x slower). "
                    f"Supported padded K: up to 2048 (bf16) / 1024 (f32).",
                    stacklevel=3,
                )
                return False
        return want

    # -- Fisher-vector product (FisherVectorMixin) ----------------------------
    @property
    def _acc_dtype(self) -> torch.dtype:
        return torch.float64 if self._X.dtype == torch.float64 else torch.float32

    def _weights(self, z: torch.Tensor) -> torch.Tensor:
        mu = torch.sigmoid(z)
        return mu * (1.0 - mu)

    def _fvp_kernel_path(self) -> bool:
        """No warning: a shape without a kernel (a padded K of 1536) is
        eager here as it is for ``logp_grad``, which says so."""
        if not self._want_kernels():
            return False
        from ..ops import glm_family_kernel_supports

        return glm_family_kernel_supports(self._X.dtype, self._k_eff)

    def logp_grad(
        self, beta, out: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        beta = torch.as_tensor(beta)
        if beta.shape != (self._k,):
            raise ValueError(f"beta must have shape ({self._k},), got {tuple(beta.shape)}.")
        if self._kernel_path():
            from ..ops import logistic_glm_logp_grad

            if self._k_pad:
                # ``out`` (if given) is sized [1 + k]; the kernel writes
                # [1 + k_eff] -- evaluate into the kernel's own buffer and
                # copy the un-padded slice over.
                logp, grad = logistic_glm_logp_grad(self._X, self._y, self._pad_rows(beta))
                logp, grad = self._into_out(out, logp, grad[: self._k])
                return logp, [grad]
            logp, grad = logistic_glm_logp_grad(self._X, self._y, beta, out=out)
            return logp, [grad]
        logp, grads = self._logp_grad_eager(beta)
        logp, grad = self._into_out(out, logp, grads[0])
        return logp, [grad]

    def logp_grad_batched(self, theta) -> Tuple[torch.Tensor, torch.Tensor]:
        """Evaluate 16 chains at once: theta[K,16] -> (logp[16], G[K,16]).

        On an MI355X shard this runs the MFMA-batched kernel (one pass over
        X for all 16 proposal vectors); elsewhere an eager batched matmul.
        """
        theta = torch.as_tensor(theta)
        if theta.dim() != 2 or theta.shape[0] != self._k:
            raise ValueError(f"theta must be [{self._k}, B], got {tuple(theta.shape)}")
        if (
            self._kernel_path()
            and self._X.dtype == torch.bfloat16
            and theta.shape[1] == 16
            and self._k_eff in (512, 1024)
        ):
            from ..ops import logistic_glm_logp_grad_batched

            if self._k_pad:
                theta = self._pad_rows(theta)
            logp, G = logistic_glm_logp_grad_batched(self._X, self._y, theta)
            return logp, (G[: self._k] if self._k_pad else G)
        return self._logp_grad_batched_eager(theta)

    def _logp_grad_batched_eager(self, theta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        X, y = self._X[:, : self._k], self._y
        acc_dtype = self._acc_dtype
        theta = theta.to(device=X.device, dtype=acc_dtype)
        B = theta.shape[1]
        logp = torch.zeros(B, dtype=torch.float64, device=X.device)
        G = torch.zeros((self._k, B), dtype=torch.float64, device=X.device)
        # this is the fallback path for K or B outside the MFMA kernel's
        # coverage; only a bf16 shard counts as narrow here
        for rows in self._row_chunks(X.dtype == torch.bfloat16):
            Xf = X[rows].to(acc_dtype)
            yf = y[rows].to(acc_dtype)
            Z = Xf @ theta
            logp += torch.sum(
                yf[:, None] * Z - torch.nn.functional.softplus(Z), dim=0, dtype=torch.float64
            )
            R = yf[:, None] - torch.sigmoid(Z)
            G += (Xf.t() @ R).to(torch.float64)
        return logp, G

    def _logp_grad_eager(self, beta: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        X, y = self._X[:, : self._k], self._y
        acc_dtype = self._acc_dtype
        beta = beta.to(device=X.device, dtype=acc_dtype)
        Xf = X.to(acc_dtype)
        yf = y.to(acc_dtype)
        z = Xf @ beta
        logp = torch.sum(yf * z - torch.nn.functional.softplus(z), dtype=torch.float64)
        resid = yf - torch.sigmoid(z)
        grad = Xf.t() @ resid
        return logp, [grad.to(torch.float64)]
