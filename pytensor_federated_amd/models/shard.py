"""What the GLM models share: a private shard ``X[N,K]`` whose feature dim is
zero-padded to a size the model's kernel is compiled for, a parameter with one
row per feature, and the fused fp64 ``[logp, grad]`` output buffer."""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .base import LogpGradModel

__all__ = ["ShardGLMModel"]


def _as_tensor(a) -> torch.Tensor:
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


class ShardGLMModel(LogpGradModel):
    """Base of ``LogisticGLMModel``, the link families and ``SoftmaxGLMModel``.

    A constructor converts with ``_as_tensor``, validates with
    ``_check_shard``, resolves ``_placement`` and hands the placed X to
    ``_set_shard``; what ``_y`` holds is the model's own business."""

    param_names = ("beta",)

    @staticmethod
    def _check_shard(X: torch.Tensor, y: torch.Tensor, *, min_columns: int = 1) -> None:
        if X.dim() != 2 or y.dim() != 1 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be [N,K] and y [N].")
        if X.shape[1] < min_columns:
            raise ValueError("X must have at least one column.")

    @staticmethod
    def _placement(X: torch.Tensor, device, dtype):
        """The defaults: X's own device, and its dtype if it is a float type."""
        if dtype is None:
            dtype = X.dtype if X.is_floating_point() else torch.float64
        if device is None:
            device = X.device
        return device, dtype

    def _set_shard(self, X: torch.Tensor, use_kernels: Optional[bool]) -> None:
        """Store the placed ``X[N,K]``; on a GPU, unless kernels are off, pad
        its feature dim to ``_padded_k()``.  Zero columns change nothing: z is
        unaffected and their gradient is exactly 0."""
        self._X = X.contiguous()
        self._use_kernels = use_kernels
        self._n, self._k = self._X.shape
        self._k_pad = 0
        if (use_kernels is None or use_kernels) and self._X.is_cuda:
            k_eff = self._padded_k()
            if k_eff is not None and k_eff != self._k:
                self._k_pad = k_eff - self._k
                pad = torch.zeros(
                    (self._n, self._k_pad), device=self._X.device, dtype=self._X.dtype
                )
                self._X = torch.cat([self._X, pad], dim=1).contiguous()

    def _padded_k(self) -> Optional[int]:
        """The kernel size ``_k`` columns of ``_X.dtype`` pad to, or None."""
        from ..ops import glm_family_padded_k

        return glm_family_padded_k(self._X.dtype, self._k)

    @property
    def device(self):
        return self._X.device

    @property
    def n_rows(self) -> int:
        return int(self._n)

    @property
    def n_features(self) -> int:
        return int(self._k)

    @property
    def _k_eff(self) -> int:
        """Feature dim as the kernel sees it (incl. zero padding)."""
        return self._k + self._k_pad

    @property
    def fused_size(self) -> int:
        """Layout of the fused fp64 output buffer: [logp, grad[K]]."""
        return 1 + int(self._k)

    def _want_kernels(self) -> bool:
        """Kernels asked for: ``use_kernels``, or by default a GPU shard."""
        return self._X.is_cuda if self._use_kernels is None else self._use_kernels

    def _pad_rows(self, p: torch.Tensor) -> torch.Tensor:
        """``p[K]`` or ``p[K,B]`` as float32 with zero rows for the padded
        columns of X."""
        p = p.to(torch.float32)
        zeros = torch.zeros((self._k_pad,) + tuple(p.shape[1:]), dtype=torch.float32,
                            device=p.device)
        return torch.cat([p, zeros])

    @staticmethod
    def _into_out(out: Optional[torch.Tensor], logp: torch.Tensor, grad: torch.Tensor):
        """Write ``(logp, flat grad)`` into ``out`` (fp64[1 + len(grad)]) and
        return its views; without ``out``, the pair as it is."""
        if out is None:
            return logp, grad
        out[0] = logp
        out[1:] = grad
        return out[0], out[1:]

    def _row_chunks(self, narrow: bool, max_step: Optional[int] = None) -> Iterator[slice]:
        """Row slices for an eager pass.  A large GPU shard in a ``narrow``
        type (one the pass upcasts) is walked in chunks, so that the upcast of
        X stays O(chunk) instead of a second copy of a multi-GB shard;
        everything else is one slice, unless ``max_step`` caps it."""
        chunked = narrow and self._X.is_cuda and self._n > 1 << 20
        step = 1 << 21 if chunked else max(self._n, 1)
        if max_step is not None:
            step = min(step, max_step)
        for s in range(0, self._n, step):
            yield slice(s, s + step)
