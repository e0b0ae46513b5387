"""Fisher-vector products of the GLM models: what ``PoissonGLMModel``,
``GaussianGLMModel`` and ``LogisticGLMModel`` share.

``H v = X^T (w(z) * (X v))`` and ``diag(H)[k] = sum_r w_r x_rk^2`` with
``z = X @ beta (+ offset)`` and the model's Fisher weight ``w``: one pass
over the shard each and a K-vector as the result, where ``fisher_information``
forms and ships ``K^2`` numbers.  Both are sums over rows, so shard results
add.  They drive ``inference.find_map_newton_cg``.

Compute paths:
* MI355X: the row-group kernel ``ops.glm_family_fisher_vector`` /
  ``ops.glm_family_fisher_diagonal`` (csrc/glm_family_fvp.hip) at every size
  and dtype of the single-chain family kernel: bf16 to a padded K of 2048,
  f32 to 1024;
* eager torch everywhere else (CPU, ``use_kernels=False``, other shapes):
  ``Xf @ v``, the weights, ``Xf.t() @ (w * u)``, chunked over the rows like
  the eager logp+grad and summed in fp64.

A model provides ``_X`` (zero-padded to ``_k_eff`` columns on the kernel
path), ``_n``, ``_k``, ``_k_pad``, ``_acc_dtype``, ``_link``, ``_offset``,
``_sigma``, ``_weights(z)`` and ``_fvp_kernel_path()``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

__all__ = ["FisherVectorMixin"]


class FisherVectorMixin:
    def _fvp_kernel_path(self) -> bool:
        raise NotImplementedError

    def _fvp_args(self, beta, v, out):
        beta = torch.as_tensor(beta)
        if beta.shape != (self._k,):
            raise ValueError(f"beta must have shape ({self._k},), got {tuple(beta.shape)}.")
        if v is not None:
            v = torch.as_tensor(v)
            if v.shape != (self._k,):
                raise ValueError(f"v must have shape ({self._k},), got {tuple(v.shape)}.")
        if out is not None and (
            out.dtype != torch.float64 or out.shape != (self._k,)
            or out.device != self._X.device
        ):
            raise ValueError(f"out must be fp64[{self._k}] on the shard's device")
        return beta, v

    def _fisher_vector(self, beta, v, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``v is None``: the diagonal."""
        beta, v = self._fvp_args(beta, v, out)
        if self._fvp_kernel_path():
            from ..ops import glm_family_fisher_diagonal, glm_family_fisher_vector

            dev = self._X.device

            def padded(t):
                t = t.to(device=dev, dtype=torch.float32)
                if self._k_pad:
                    t = torch.cat([t, torch.zeros(self._k_pad, dtype=torch.float32, device=dev)])
                return t

            kw = dict(link=self._link, offset=self._offset, sigma=self._sigma)
            if not self._k_pad and out is not None and out.is_contiguous():
                kw["out"] = out
            if v is None:
                r = glm_family_fisher_diagonal(self._X, padded(beta), **kw)
            else:
                r = glm_family_fisher_vector(self._X, padded(beta), padded(v), **kw)
            if "out" in kw:
                return out
            r = r[: self._k]
        else:
            r = self._fisher_vector_eager(beta, v)
        if out is not None:
            out.copy_(r)
            return out
        return r

    def _fisher_vector_eager(self, beta: torch.Tensor, v: Optional[torch.Tensor]) -> torch.Tensor:
        X = self._X[:, : self._k]
        acc = self._acc_dtype
        beta = beta.to(device=X.device, dtype=acc)
        if v is not None:
            v = v.to(device=X.device, dtype=acc)
        r = torch.zeros(self._k, dtype=torch.float64, device=X.device)
        # chunked like the eager logp+grad: the upcast of X stays O(chunk)
        chunked = X.dtype != acc and X.is_cuda and self._n > 1 << 20
        step = 1 << 21 if chunked else max(self._n, 1)
        for s in range(0, self._n, step):
            Xf = X[s : s + step].to(acc)
            z = Xf @ beta
            if self._offset is not None:
                z = z + self._offset[s : s + step]
            w = self._weights(z)
            if v is None:
                # same-sign terms: a long f32 chain drifts, so the rows are
                # added in fp64 (a matmul would add them in f32)
                r += torch.sum((Xf * Xf) * w[:, None], dim=0, dtype=torch.float64)
            else:
                r += (Xf.t() @ (w * (Xf @ v))).to(torch.float64)
        return r

    def fisher_vector_product(self, beta, v, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``H(beta) @ v = X^T (w(z) * (X v))`` as fp64[K], without forming
        ``H``: one pass over the shard.  ``out`` (fp64[K], same device)
        receives the result in place."""
        if v is None:
            raise ValueError(f"v must have shape ({self._k},); see fisher_diagonal")
        return self._fisher_vector(beta, v, out)

    def fisher_diagonal(self, beta, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``diag(H(beta))[k] = sum_r w_r x_rk^2`` as fp64[K]: the Jacobi
        preconditioner of a conjugate-gradient solve with ``H``."""
        return self._fisher_vector(beta, None, out)

    def as_fisher_vector_func(self):
        """A ``ComputeFunc``: numpy ``(beta, v)`` -> ``[H v]`` (fp64[K]),
        which a worker serves through ``ArraysToArraysService``."""

        def fisher_vector_func(beta, v):
            # copy: wire-decoded arrays are read-only zero-copy views
            b = torch.from_numpy(np.array(beta, dtype=np.float64))
            u = torch.from_numpy(np.array(v, dtype=np.float64))
            r = self.fisher_vector_product(b, u)
            return [np.asarray(r.detach().cpu().double().numpy())]

        return fisher_vector_func

    def as_fisher_diagonal_func(self):
        """A ``ComputeFunc``: numpy ``beta`` -> ``[diag(H)]`` (fp64[K])."""

        def fisher_diagonal_func(beta):
            b = torch.from_numpy(np.array(beta, dtype=np.float64))
            r = self.fisher_diagonal(b)
            return [np.asarray(r.detach().cpu().double().numpy())]

        return fisher_diagonal_func
