"""Probe inputs and references for the GLM Fisher-vector kernel
(glm_family_fvp.hip): ``H v = X^T (w * (X v))`` and ``diag(H) = (X*X)^T w``,
``w`` the Fisher weight of ``z = X @ beta (+ offset)``.

Plain helper module (imported by ``test_glm_fvp_cpu.py`` and
``test_gpu_glm_fvp.py``).  It reuses ``glm_fisher_probes.EXACT_PROBES``, which
give ``X``, ``beta``, ``offset`` and the exact ``w`` (1 or 0 for the Poisson
probes, ``1/sigma^2`` for the Gaussian ones).

Exact probes.  ``v`` holds multiples of 1/4 with ``|v| <= 1``, X multiples of
1/8, w is 1, 1/4 or 0: every product ``x v`` is a multiple of 1/32, every
``w u x`` and ``w x x`` a multiple of 1/1024, and the CPU test checks that the
sums of their magnitudes stay below 2^24 of those units (the worst over every
probe and size are 39,496, 3,744,128 and 3,834,112), so any summation
order in f32 is exact and the kernel is held to fp64 numpy with
``assert_array_equal``.

Logistic probes: the two Poisson probes under ``link="logistic"``.  At
``z = 0`` mu = 1/(1 + 1) = 1/2 exactly and w = 1/4; at ``z <= -128``
``exp(128)`` overflows f32 (or, by another route, mu flushes), mu = 0 and
w = 0: the exact weight is the Poisson probe's over 4.

Sizes: ``glm_probes.all_sizes(dtype)`` for both dtypes: every G, KITER 2 and
4, at the rows of ``family_rows``, ``deep_rows`` and ``stale_big_rows``.

Accuracy sets: ``glm_probes.accuracy_case`` data and a logistic case, under

    |got - ref| <= M * 2^-24 * S
    S_k = sum_r |x_rk| w_r (|x_r| . |v|)      (product)
    S_k = sum_r w_r x_rk^2                    (diagonal)

per component.
"""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np
import torch

import glm_fisher_probes as fp
import glm_probes as gp

#: probe id -> (link, builder(n, K) -> dict(X, beta, offset?, w), sigma)
EXACT_PROBES: Dict[str, Tuple] = dict(fp.EXACT_PROBES)


def _as_logistic(build):
    def logistic(n: int, K: int):
        p = build(n, K)
        w = p["w"] / 4.0
        w.setflags(write=False)
        return {**p, "w": w}

    return logistic


for _name in ("poisson_zero_beta", "poisson_gate"):
    EXACT_PROBES["logistic_" + _name[len("poisson_"):]] = (
        "logistic", _as_logistic(fp.EXACT_PROBES[_name][1]), 1.0
    )

PROBES = sorted(EXACT_PROBES)
DTYPES = ("bfloat16", "float32")


@functools.lru_cache(maxsize=None)
def probe_vector(K: int) -> np.ndarray:
    """Multiples of 1/4 with |v| <= 1, seeded by K."""
    rng = np.random.RandomState(np.array([0x55, K], dtype=np.uint32))
    v = rng.randint(-4, 5, size=K) / 4.0
    v.setflags(write=False)
    return v


def fvp_reference(X, w, v) -> np.ndarray:
    """``X^T (w * (X v))`` in fp64 numpy."""
    X = np.asarray(X, dtype=np.float64)
    return X.T @ (np.asarray(w, dtype=np.float64) * (X @ np.asarray(v, dtype=np.float64)))


def diag_reference(X, w) -> np.ndarray:
    """``(X*X)^T w`` in fp64 numpy."""
    X = np.asarray(X, dtype=np.float64)
    return (X * X).T @ np.asarray(w, dtype=np.float64)


def fvp_scale(X, w, v) -> np.ndarray:
    """``S_k = sum_r |x_rk| w_r (|x_r| . |v|)``."""
    A = np.abs(np.asarray(X, dtype=np.float64))
    return A.T @ (np.asarray(w, dtype=np.float64) * (A @ np.abs(np.asarray(v, dtype=np.float64))))


@functools.lru_cache(maxsize=None)
def exact_reference(probe: str, n: int, K: int) -> Tuple[np.ndarray, np.ndarray]:
    """(H v, diag H) of an exact probe; computed once per (probe, n, K) and
    shared; read-only."""
    p = EXACT_PROBES[probe][1](n, K)
    Hv = fvp_reference(p["X"], p["w"], probe_vector(K))
    d = diag_reference(p["X"], p["w"])
    Hv.setflags(write=False)
    d.setflags(write=False)
    return Hv, d


# ---------------------------------------------------------------------------
# accuracy sets
# ---------------------------------------------------------------------------

#: Worst ratio |eager - fp64 reference| / (2^-24 * S) over every component of
#: the product and the diagonal of every accuracy case (Poisson and Gaussian x
#: 2 dtypes x K in gp.ACC_K, and the logistic case in both dtypes), measured
#: on the CPU with
#:
#:     python -m pytest tests/test_glm_fvp_cpu.py -k eager_meets -s
#:
#: which prints each case's ratio: FVP_EAGER_MEASURED with one thread (the
#: longest f32 chain of the 5000-row ``X^T @ (w u)``; the product of the
#: Gaussian float32 K = 8 case), 1.31 with 8 threads.  The diagonal adds its
#: rows in fp64 and stays below 0.21.  Rounded up to the next power of two, as
#: EAGER_M is.
FVP_EAGER_MEASURED = 7.52
FVP_EAGER_M = 8.0
#: the kernel: 4x, for the same reasons as KERNEL_M (__expf's argument scaling
#: and another summation order)
FVP_KERNEL_M = 4.0 * FVP_EAGER_M

LOGISTIC_K = 100


@functools.lru_cache(maxsize=None)
def accuracy_vector(K: int) -> np.ndarray:
    """A seeded standard-normal direction, stored in f32."""
    v = gp._round_f32(np.random.RandomState(900 + K).standard_normal(K))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def logistic_case(dtype_name: str):
    """Stored logistic data at K = LOGISTIC_K (X in ``dtype_name``, beta in
    f32) and its z, as gp.accuracy_case gives them."""
    from pytensor_federated_amd.models import generate_logistic_dataset

    X, y, beta = generate_logistic_dataset(gp.ACC_N, LOGISTIC_K, seed=100 + LOGISTIC_K)
    X = gp._round_bf16(X) if dtype_name == "bfloat16" else gp._round_f32(X)
    beta = gp._round_f32(beta)
    return gp._freeze(X=X, y=y, beta=beta, z=X @ beta)


def accuracy_data(family: str, dtype_name: str, K: int):
    """(case dict with X, beta, z [, offset, sigma], exact fp64 weights)."""
    if family == "logistic":
        assert K == LOGISTIC_K
        c = logistic_case(dtype_name)
        mu = 1.0 / (1.0 + np.exp(-c["z"]))
        return c, mu * (1.0 - mu)
    c = gp.accuracy_case(family, dtype_name, K)
    if family == "poisson":
        return c, np.exp(c["z"])
    return c, np.full(c["z"].shape, 1.0 / (c["sigma"] * c["sigma"]))


#: every accuracy case: (family, dtype, K)
ACCURACY_CASES = tuple(
    (family, dtype_name, K)
    for family in ("poisson", "gaussian")
    for dtype_name in DTYPES
    for K in gp.ACC_K
) + tuple(("logistic", dtype_name, LOGISTIC_K) for dtype_name in DTYPES)


@functools.lru_cache(maxsize=None)
def accuracy_fvp(family: str, dtype_name: str, K: int):
    """(Hv_ref, Hv_scale, diag_ref) in fp64 on the stored data; the scale of
    the diagonal is the diagonal itself (every term is non-negative)."""
    c, w = accuracy_data(family, dtype_name, K)
    v = accuracy_vector(K)
    out = (fvp_reference(c["X"], w, v), fvp_scale(c["X"], w, v), diag_reference(c["X"], w))
    for a in out:
        a.setflags(write=False)
    return out


def accuracy_model(family: str, dtype_name: str, K: int, **kw):
    if family != "logistic":
        return gp.accuracy_model(family, dtype_name, K, **kw)
    from pytensor_federated_amd.models import LogisticGLMModel

    c = logistic_case(dtype_name)
    return LogisticGLMModel(torch.tensor(c["X"]), torch.tensor(c["y"]),
                            dtype=getattr(torch, dtype_name), **kw)


def fvp_ratios(family: str, dtype_name: str, K: int, Hv, d) -> Tuple[float, float]:
    """(worst product ratio, worst diagonal ratio): error over 2^-24 * S."""
    ref, scale, dref = accuracy_fvp(family, dtype_name, K)
    unit = 2.0 ** -24
    r_v = float(np.max(np.abs(np.asarray(Hv, dtype=np.float64) - ref) / (unit * scale)))
    r_d = float(np.max(np.abs(np.asarray(d, dtype=np.float64) - dref) / (unit * dref)))
    return r_v, r_d


# ---------------------------------------------------------------------------
# fp64 numpy callables for the Newton-CG driver
# ---------------------------------------------------------------------------

def numpy_poisson_funcs(X, y, offset, counter=None):
    """(logp_grad, fisher, product, diagonal) in fp64 numpy on stored data."""
    def weights(b):
        return np.exp(X @ b + offset)

    def logp_grad(b):
        z = X @ b + offset
        mu = np.exp(z)
        return float(np.sum(y * z - mu)), [X.T @ (y - mu)]

    def fisher(b):
        return [fp.fisher_reference(X, weights(b))]

    def product(b, v):
        if counter is not None:
            counter.append(1)
        return [fvp_reference(X, weights(b), v)]

    def diagonal(b):
        return [diag_reference(X, weights(b))]

    return logp_grad, fisher, product, diagonal
