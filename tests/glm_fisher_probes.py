"""Probe inputs and references for the GLM Fisher-information kernel
(glm_family_fisher.hip): ``H = X^T diag(w) X``, ``w = exp(z)`` (Poisson) or
``1/sigma^2`` (Gaussian), ``z = X @ beta (+ offset)``.

Plain helper module (imported by ``test_glm_fisher_cpu.py`` and
``test_gpu_glm_fisher.py``), in the style of ``glm_batched_probes.py``; it
reuses the shards of ``glm_probes.py``.

Exact probes: every ``w*x`` is exact in bf16 (so the second and third piece
are zero) and every partial sum of ``x_i * w * x_j`` is a whole number of its
unit below 2^24 of them, so any summation order in f32 is exact and the
kernel is held to fp64 numpy with ``assert_array_equal``.

(a) ``poisson_zero_beta``  gp.poisson_zero_beta_probe: dense X = j/8,
    beta = 0, offset in {0, -128}: w is exactly 1 or 0; every entry of H is
    filled.  Terms are multiples of 1/64 below 4.
(b) ``gaussian_sigma1`` / ``gaussian_sigma2``  gp.gaussian_sparse_probe:
    w = 1 or 1/4; terms are multiples of 1/16 below 4.
(c) ``poisson_gate``  the probe whose w depends on X . beta: min(3, K)
    non-zeros per row from {1, 2}, beta_k = -128 where k % 4 == 0 and 0
    elsewhere, no offset: z is 0 (w = 1) when the row misses every gated
    column, and at most -128 (w = 0: exp(z) flushes in fp32) otherwise.

Accuracy sets: gp.accuracy_case data (it carries z and sigma) under

    |got - ref| <= M * 2^-24 * H_scale,   H_scale = |X|^T diag(w) |X|

per entry; ``FISHER_EAGER_M`` for the eager path, ``FISHER_KERNEL_M`` for the
kernel.
"""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np

import glm_probes as gp

#: feature counts of the kernel (asserted equal to ops.GLM_FAMILY_FISHER_K)
FISHER_K = (8, 16, 32, 64, 128, 256, 512, 1024)
#: FED_GLM_FISHER_GRID for the three-trip case
DEEP_GRID = 2
#: row counts at which the share condition of probe (c) is checked on the CPU
GATE_SHARE_ROWS = (31, 32, 33, 65, 129, 257, 500)

#: Worst ratio |eager - fp64 reference| / (2^-24 * H_scale) over every entry
#: of every accuracy case (2 families x 2 dtypes x 3 K), measured on the CPU
#: with
#:
#:     python -m pytest tests/test_glm_fisher_cpu.py -k eager_meets -s
#:
#: which prints each case's ratio: FISHER_EAGER_MEASURED with one thread (the
#: longest f32 chain of the 5000-row ``X^T @ (w X)``), less with more
#: threads.  Rounded up to the next power of two, as EAGER_M is.
FISHER_EAGER_MEASURED = 12.2
FISHER_EAGER_M = 16.0
#: the kernel: 4x, for the same reasons as KERNEL_M (__expf's argument
#: scaling and another summation order)
FISHER_KERNEL_M = 4.0 * FISHER_EAGER_M


def tile_rows(K: int) -> int:
    """TR: rows per block tile of the kernel (FsGeom<K>::TR; asserted equal
    to ops.glm_family_fisher_tile_rows on the GPU)."""
    return 64 if K >= 128 else (128 if K == 64 else 256)


def edge_rows(K: int) -> Tuple[int, ...]:
    T = tile_rows(K)
    return (1, T - 1, T, T + 1, 2 * T + 1)


def deep_rows(K: int) -> int:
    """Under FED_GLM_FISHER_GRID=2: seven tiles, three full trips per block
    and a one-row ragged tile."""
    return 6 * tile_rows(K) + 1


def stale_small_rows(K: int) -> int:
    return tile_rows(K) + 1


def stale_big_rows(K: int) -> int:
    return 20 * tile_rows(K) + 3


def _freeze(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------
# probes: dict(X, beta, offset?, w)
# ---------------------------------------------------------------------------

def flushed_weights(X, beta, offset=None) -> np.ndarray:
    """exp(z) as fp32 gives it on the Poisson probes: 1 at z = 0, 0 at
    z <= -128 (every z of these probes is one of them)."""
    z = np.asarray(X, dtype=np.float64) @ np.asarray(beta, dtype=np.float64)
    if offset is not None:
        z = z + np.asarray(offset, dtype=np.float64)
    assert np.all((z <= -gp.SAT) | (z == 0.0))
    return (z == 0.0).astype(np.float64)


@functools.lru_cache(maxsize=8)
def poisson_zero_beta(n: int, K: int) -> Dict[str, np.ndarray]:
    p = gp.poisson_zero_beta_probe(n, K)
    return _freeze(X=p["X"], beta=p["beta"], offset=p["offset"],
                   w=flushed_weights(p["X"], p["beta"], p["offset"]))


@functools.lru_cache(maxsize=8)
def gaussian_sparse(n: int, K: int, sigma: float) -> Dict[str, np.ndarray]:
    p = gp.gaussian_sparse_probe(n, K, sigma)
    return _freeze(X=p["X"], beta=p["beta"], w=np.full(n, 1.0 / (sigma * sigma)))


@functools.lru_cache(maxsize=8)
def poisson_gate_probe(n: int, K: int) -> Dict[str, np.ndarray]:
    rng = np.random.RandomState(np.array([0x54, n, K], dtype=np.uint32))
    nnz = min(3, K)
    X = np.zeros((n, K))
    for r in range(n):
        X[r, rng.choice(K, size=nnz, replace=False)] = rng.randint(1, 3, size=nnz)
    beta = np.where(np.arange(K) % 4 == 0, -gp.SAT, 0.0)
    return _freeze(X=X, beta=beta, w=flushed_weights(X, beta))


#: probe id -> (link, builder(n, K) -> dict, sigma)
EXACT_PROBES = {
    "poisson_zero_beta": ("poisson", poisson_zero_beta, 1.0),
    "gaussian_sigma1": ("gaussian", lambda n, K: gaussian_sparse(n, K, 1.0), 1.0),
    "gaussian_sigma2": ("gaussian", lambda n, K: gaussian_sparse(n, K, 2.0), 2.0),
    "poisson_gate": ("poisson", poisson_gate_probe, 1.0),
}


def fisher_reference(X, w) -> np.ndarray:
    """H_ref = X^T diag(w) X in fp64 numpy."""
    X = np.asarray(X, dtype=np.float64)
    return X.T @ (np.asarray(w, dtype=np.float64)[:, None] * X)


def fisher_scale(X, w) -> np.ndarray:
    """H_scale = |X|^T diag(w) |X|: per entry, the sum of the magnitudes of
    the rows' contributions."""
    A = np.abs(np.asarray(X, dtype=np.float64))
    return A.T @ (np.asarray(w, dtype=np.float64)[:, None] * A)


@functools.lru_cache(maxsize=None)
def exact_reference(probe: str, n: int, K: int) -> np.ndarray:
    """Computed once per (probe, n, K) and shared; read-only."""
    p = EXACT_PROBES[probe][1](n, K)
    H = fisher_reference(p["X"], p["w"])
    H.setflags(write=False)
    return H


# ---------------------------------------------------------------------------
# accuracy sets
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def accuracy_fisher(family: str, dtype_name: str, K: int):
    """(H_ref, H_scale) in fp64 on the stored data of gp.accuracy_case."""
    c = gp.accuracy_case(family, dtype_name, K)
    if family == "poisson":
        w = np.exp(c["z"])
    else:
        w = np.full(c["z"].shape, 1.0 / (c["sigma"] * c["sigma"]))
    H, S = fisher_reference(c["X"], w), fisher_scale(c["X"], w)
    H.setflags(write=False)
    S.setflags(write=False)
    return H, S


def fisher_ratio(family: str, dtype_name: str, K: int, H) -> float:
    """Worst entry of |H - H_ref| / (2^-24 * H_scale)."""
    ref, scale = accuracy_fisher(family, dtype_name, K)
    return float(np.max(np.abs(np.asarray(H, dtype=np.float64) - ref) / (2.0 ** -24 * scale)))
