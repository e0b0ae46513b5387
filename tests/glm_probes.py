"""Probe inputs and references for the GLM family kernel (glm_family.hip).

Plain helper module (imported by ``test_glm_probes_cpu.py`` and
``test_gpu_glm_family.py``), in the style of ``exact_probes.py``, whose
logistic probes and references it reuses unchanged.

Exact probes: every intermediate of the kernel (bf16/f32 operands, fp32
products and partial sums, the per-row term and residual) is exactly
representable, so the kernel is held to an fp64 reference bit-tight and one
lost, doubled or mis-addressed row or column shows as a whole unit.

(p1) ``poisson_saturated_probe``  X in {0,1,2} ("dense") or one-hot on the
     stride-37 walk ("onehot"); beta = -128*w_k, w in 1..4; y in 0..7.
     z <= -128, and exp(z <= -128) < 2^-184 is exactly 0 in fp32 (smallest
     subnormal 2^-149): logp = sum y*z and G = X^T y, both integers.
(p2) ``poisson_zero_beta_probe``  beta = 0, X = j/8, offset in {0, -128}
     per row: exp(z) is exactly 1 or 0, resid = y - [offset == 0].
(g)  ``gaussian_sparse_probe``    at most 4 non-zeros per row from
     {+-1/2, +-1, +-2}; beta multiples of 1/4, |beta| <= 2; y multiples of
     1/8, |y| <= 4; sigma in {1, 2}.  r = y - z is a multiple of 1/8 with
     |r| <= 20, so r*r (units 2^-6, < 2^15 of them) and r*x are exact.

The Poisson references are the closed forms above (exact in fp64); the
fp64 evaluation of the general formula differs from them only by the
exp(-128) ~ 2.6e-56 remainders, which the CPU premise test bounds.

Accuracy sets (where exp matters): seeded Poisson and Gaussian data with
|z| <= 4, compared with fp64 numpy on the stored data under the bound

    |got - ref| <= M * 2^-24 * sum_r |row r's contribution|

per output component.  M for the eager fp32 path is ``EAGER_M``; the
kernel is allowed ``KERNEL_M = 4 * EAGER_M`` (fast exponential's argument
scaling, another summation order).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Tuple

import numpy as np
import torch

import exact_probes as ep

VEC = {"bfloat16": 8, "float32": 4}
GROUPS = (1, 2, 4, 8, 16, 32, 64)
KITERS = (2, 4)
WAVE = 64

#: dyadic stand-in for logp_const in the exact probes: added exactly once
PROBE_CONST = -1024.5
#: FED_GLM_GRID for the two-trip case
DEEP_GRID = 2

SAT = 128.0
#: exp(-128) in fp64: what the general formula keeps and fp32 flushes
EXP_SAT = math.exp(-SAT)


def family_shapes(dtype_name: str) -> Tuple[Tuple[int, int], ...]:
    """(K, R = rows per wave step) of every instantiation of one dtype:
    K = G*VEC for every G, then K = KITER*64*VEC."""
    vec = VEC[dtype_name]
    shapes = [(g * vec, WAVE // g) for g in GROUPS]
    shapes += [(it * WAVE * vec, 1) for it in KITERS]
    return tuple(shapes)


def family_rows(R: int) -> Tuple[int, ...]:
    """One row, one short of / exactly / one past a step, a pair and a
    ragged third step, one short of / one past a block's 8 steps."""
    return tuple(sorted({n for n in (1, R - 1, R, R + 1, 2 * R + 1, 8 * R - 1, 8 * R + 1)
                         if n > 0}))


def deep_rows(R: int) -> int:
    """Under FED_GLM_GRID=2 (8 waves, 16 steps a trip): two full trips, a
    third with one full step and a one-row ragged last step."""
    return 33 * R + 1


def stale_big_rows(R: int) -> int:
    """A larger problem of the same K (21 steps, 3 blocks), evaluated
    between two calls of a small one so that the workspace slab and the LDS
    hold non-zero leftovers."""
    return 20 * R + 3


def all_sizes(dtype_name: str):
    """Every (K, n) the GPU exact tests evaluate."""
    for K, R in family_shapes(dtype_name):
        for n in family_rows(R) + (deep_rows(R), stale_big_rows(R)):
            yield K, n


def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(np.array(key, dtype=np.uint32))


def _freeze(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def poisson_saturated_probe(kind: str, n: int, K: int) -> Dict[str, np.ndarray]:
    rng = _rng(0x51, kind == "dense", n, K)
    if kind == "dense":
        X = rng.randint(0, 3, size=(n, K)).astype(np.float64)
        empty = ~X.any(axis=1)
        X[empty, np.arange(n)[empty] % K] = 1.0
    else:
        cols = (np.arange(n, dtype=np.int64) * ep.ONEHOT_STRIDE) % K
        X = np.zeros((n, K))
        X[np.arange(n), cols] = 1.0
    beta = -SAT * rng.randint(1, 5, size=K).astype(np.float64)
    y = rng.randint(0, 8, size=n).astype(np.float64)
    return _freeze(X=X, y=y, beta=beta)


@functools.lru_cache(maxsize=8)
def poisson_zero_beta_probe(n: int, K: int) -> Dict[str, np.ndarray]:
    rng = _rng(0x52, n, K)
    X = rng.randint(-16, 17, size=(n, K)) / 8.0
    offset = -SAT * rng.randint(0, 2, size=n).astype(np.float64)
    y = rng.randint(0, 8, size=n).astype(np.float64)
    return _freeze(X=X, y=y, beta=np.zeros(K), offset=offset)


@functools.lru_cache(maxsize=8)
def gaussian_sparse_probe(n: int, K: int, sigma: float) -> Dict[str, np.ndarray]:
    rng = _rng(0x53, n, K, int(sigma))
    values = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
    X = np.zeros((n, K))
    nnz = min(4, K)
    for r in range(n):
        X[r, rng.choice(K, size=nnz, replace=False)] = values[rng.randint(0, 6, size=nnz)]
    beta = rng.randint(-8, 9, size=K) / 4.0
    y = rng.randint(-32, 33, size=n) / 8.0
    return _freeze(X=X, y=y, beta=beta)


def poisson_reference(X, y, beta, offset=None, const: float = 0.0):
    """Plain fp64 numpy: (logp, G) of the general Poisson formula."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    z = X @ np.asarray(beta, dtype=np.float64)
    if offset is not None:
        z = z + np.asarray(offset, dtype=np.float64)
    mu = np.exp(z)
    return float(np.sum(y * z - mu) + const), X.T @ (y - mu)


def poisson_flushed_reference(X, y, beta, offset=None, const: float = 0.0):
    """The exactly representable answer of probes (p1)/(p2): exp(z) is 0
    for z <= -128 and 1 for z = 0 (every z of these probes is one of them)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    z = X @ np.asarray(beta, dtype=np.float64)
    if offset is not None:
        z = z + np.asarray(offset, dtype=np.float64)
    assert np.all((z <= -SAT) | (z == 0.0))
    mu = (z == 0.0).astype(np.float64)
    return float(np.sum(y * z - mu) + const), X.T @ (y - mu)


def gaussian_reference(X, y, beta, sigma: float, offset=None, const: float = 0.0):
    """Plain fp64 numpy: (logp, G) of the Gaussian GLM."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    z = X @ np.asarray(beta, dtype=np.float64)
    if offset is not None:
        z = z + np.asarray(offset, dtype=np.float64)
    r = y - z
    return float(-np.sum(r * r) / (2.0 * sigma * sigma) + const), X.T @ r / (sigma * sigma)


def _p1(kind):
    return lambda n, K: poisson_saturated_probe(kind, n, K)


def _pois_ref(p):
    return poisson_flushed_reference(p["X"], p["y"], p["beta"], p.get("offset"), PROBE_CONST)


def _gauss(sigma):
    return (
        "gaussian",
        lambda n, K: gaussian_sparse_probe(n, K, sigma),
        lambda p: gaussian_reference(p["X"], p["y"], p["beta"], sigma, None, PROBE_CONST),
        sigma,
    )


#: exact probe id -> (link, builder(n, K) -> dict, reference(dict) -> (logp, G), sigma);
#: the references include PROBE_CONST
EXACT_PROBES = {
    "poisson_dense": ("poisson", _p1("dense"), _pois_ref, 1.0),
    "poisson_onehot": ("poisson", _p1("onehot"), _pois_ref, 1.0),
    "poisson_zero_beta": ("poisson", poisson_zero_beta_probe, _pois_ref, 1.0),
    "gaussian_sigma1": _gauss(1.0),
    "gaussian_sigma2": _gauss(2.0),
}


@functools.lru_cache(maxsize=None)
def exact_reference(probe: str, n: int, K: int):
    """Computed once per (probe, n, K) and shared; read-only."""
    _, build, ref, _ = EXACT_PROBES[probe]
    logp, G = ref(build(n, K))
    G = np.array(G)
    G.setflags(write=False)
    return logp, G


# ---------------------------------------------------------------------------
# accuracy sets
# ---------------------------------------------------------------------------

ACC_N = 5000
ACC_K = (8, 100, 512)
ACC_ZMAX = 4.0

#: Worst ratio |eager fp32 - fp64 reference| / (2^-24 * sum_r |row r's
#: contribution|) over every output component of every accuracy case below
#: (2 families x 2 dtypes x 3 K), measured on the CPU with
#:
#:     python -m pytest tests/test_glm_probes_cpu.py -k eager_meets -s
#:
#: which prints each case's ratio.  The ratio is the gradient's and depends
#: on how the BLAS splits the 5000-row sum of ``X^T @ resid``: worst over
#: the cases 3.15 with one thread (the longest fp32 chain; Poisson,
#: bfloat16, K = 512), 1.32 with 2, 0.79 with 4, 0.49 with 8, 0.42 with 16
#: threads; logp (fp64 row sum) stays below 0.1.  The one-thread figure is
#: the path's own worst, rounded up to the next power of two so that a BLAS
#: with another vector width does not move the eager path across its own
#: yardstick.  The test evaluates with one thread and with the default.
EAGER_M = 4.0
#: the kernel: 4x, for __expf's argument scaling (one more rounding of
#: z*log2(e), relative 2^-24 * |z| <= 4 * 2^-24 in the exponent) and its
#: own summation order
KERNEL_M = 4.0 * EAGER_M


def _round_bf16(a: np.ndarray) -> np.ndarray:
    return torch.tensor(a).to(torch.bfloat16).to(torch.float64).numpy()


def _round_f32(a: np.ndarray) -> np.ndarray:
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def accuracy_case(family: str, dtype_name: str, K: int):
    """Stored data (already rounded to the formats the model keeps: X in
    ``dtype_name``, y / offset / beta in f32), the fp64 reference on it and
    the per-component bound denominators sum_r |contribution|."""
    from pytensor_federated_amd.models import (
        generate_gaussian_glm_dataset,
        generate_poisson_dataset,
    )

    seed = 100 + K
    sigma = 0.5
    if family == "poisson":
        X, y, offset, beta = generate_poisson_dataset(ACC_N, K, seed=seed)
        offset = _round_f32(offset)
    else:
        X, y, beta = generate_gaussian_glm_dataset(ACC_N, K, sigma=sigma, seed=seed)
        offset = None
    X = _round_bf16(X) if dtype_name == "bfloat16" else _round_f32(X)
    y, beta = _round_f32(y), _round_f32(beta)
    z = X @ beta + (offset if offset is not None else 0.0)
    if family == "poisson":
        mu = np.exp(z)
        term, resid = y * z - mu, y - mu
        const = -float(sum(math.lgamma(v + 1.0) for v in y))
    else:
        r = y - z
        term, resid = -r * r / (2 * sigma * sigma), r / (sigma * sigma)
        const = -0.5 * ACC_N * math.log(2 * math.pi * sigma * sigma)
    out = dict(
        X=X, y=y, beta=beta, z=z,
        logp=float(np.sum(term) + const), G=X.T @ resid,
        logp_scale=float(np.sum(np.abs(term))),
        G_scale=np.abs(X).T @ np.abs(resid),
    )
    if offset is not None:
        out["offset"] = offset
    _freeze(**out)
    out["sigma"] = sigma
    return out


def accuracy_model(family: str, dtype_name: str, K: int, **kw):
    from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel

    c = accuracy_case(family, dtype_name, K)
    X, y = torch.tensor(c["X"]), torch.tensor(c["y"])
    dtype = getattr(torch, dtype_name)
    if family == "poisson":
        return PoissonGLMModel(X, y, offset=torch.tensor(c["offset"]), dtype=dtype, **kw)
    return GaussianGLMModel(X, y, c["sigma"], dtype=dtype, **kw)


def accuracy_ratios(case, logp: float, G: np.ndarray) -> Tuple[float, float]:
    """(logp ratio, worst grad ratio): error over 2^-24 * sum |contribution|."""
    unit = 2.0 ** -24
    r_logp = abs(logp - case["logp"]) / (unit * case["logp_scale"])
    r_grad = float(np.max(np.abs(np.asarray(G) - case["G"]) / (unit * case["G_scale"])))
    return r_logp, r_grad
