"""Probe inputs whose logp/grad answers are exactly representable.

Plain helper module (imported by ``test_exact_probes_cpu.py`` and
``test_gpu_exact_probes.py``).  Every probe chooses its inputs so that each
intermediate of the HIP kernels -- bf16 operands, fp32 MFMA/FMA products and
partial sums, the bf16-rounded residual -- is an exactly representable
number.  Accumulation order and fp32-vs-fp64 then cannot change the result,
so a kernel can be held to its fp64 numpy reference bit-tight: one dropped,
duplicated or mis-addressed row, column or chain moves an entry by a whole
unit instead of hiding inside a 2e-2 tolerance.

Probes
------
(a) ``onehot_probe``      X one-hot, theta = +-32: z = theta[c(r), b] exactly,
                          resid in {0, +-1}, G entries are small integers
                          each naming (row, chain) pairs.
(b) ``dense_int_probe``   X in {0,1,2}, theta = sigma_b*32*w_k: z is an exact
                          multiple of 32 with |z| >= 32; logp and G depend
                          linearly on every X element.
(c) ``zero_theta_probe``  theta = 0, X = j/8: z = 0, resid = y - 1/2,
                          G = X^T (y - 1/2) exact, logp = -N ln 2.
(d) ``gaussian_probe``    x, y multiples of 1/8, dyadic (a, b), sigma = 1.

The only inexact terms are the saturation remainders of (a)/(b):
``sigmoid(-32)`` and ``log1p(exp(-32))`` are e^-32 < 2^-46 instead of 0, so
an N-row sum carries at most N*2^-46 of them (times max|X| <= 2 for G).
The GPU tests compare with ``atol = N * 2^-40``.  No remainder may land in a
G entry whose exact part is non-zero: the MFMA accumulate is not rounded to
nearest (see ``onehot_probe``), so "integer + remainder" is not guaranteed
to give the integer.
"""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np

BCH = 16                 # chains per batched call
SAT = 32.0               # saturating |z| unit
TINY = 2.0 ** -46        # bound on sigmoid(-32), log1p(exp(-32))
ONEHOT_STRIDE = 37       # odd: c(r) = r*37 mod K walks every column of a 2^m K

# ---------------------------------------------------------------------------
# shapes shared by the CPU premise checks and the GPU tests
# ---------------------------------------------------------------------------

#: single-chain logistic kernel: (torch dtype name, K)
SINGLE_COMBOS = (("bfloat16", 512), ("bfloat16", 2048), ("float32", 256), ("float32", 1024))
#: odd tail alone, one pair, pair+tail, fewer rows than a block's waves,
#: an odd N spanning several blocks
SINGLE_N = (1, 2, 3, 7, 8, 9, 4097)

#: batched kernels, default grid: every N mod 32 / mod 64 class that takes
#: another staging path, below / at / above one and two tiles
BATCHED_N = (1, 3, 4, 5, 20, 31, 32, 33, 52, 63, 64, 65, 97)
#: batched kernels at FED_BATCHED_GRID=16: 4 full 32-row tiles per block;
#: 65 tiles at 5 per block (full block, block ending on the 20-row tail,
#: empty blocks); 33 tiles at 3 per block with a 12-row tail
BATCHED_DEEP_N = (2048, 2068, 16 * 32 * 2 + 12)
BATCHED_K = (512, 1024)
#: a larger problem evaluated between two calls of a small one, so that the
#: workspace slab and the LDS hold non-zero leftovers
STALE_BIG_N = 4131
STALE_N = (52, 2068)

#: gaussian kernel: elements per 16-byte vector load
GAUSS_VEC = {"float32": 4, "float64": 2, "bfloat16": 8}
GAUSS_SMALL_N = (1, 3, 7, 9)
GAUSS_GROUPS = (1, 2, 3, 4, 16)
GAUSS_THETAS = ((0.5, -0.25), (-0.25, 0.5))


def gaussian_sizes(dtype_name: str) -> Tuple[int, ...]:
    """n < VEC / tail-only sizes, then VEC*256*g + 3 (grids 1, 2, 2, 4, 16
    for the 4- and 8-wide types).  The 2-wide f64 type turns the +3 tail
    into one more vector, i.e. one more block (grids 2, 2, 4, 4, 16), so it
    also gets VEC*256*g + 1 for g = 1 and 3 (grids 1 and 3 -> 2)."""
    vec = GAUSS_VEC[dtype_name]
    sizes = list(GAUSS_SMALL_N) + [vec * 256 * g + 3 for g in GAUSS_GROUPS]
    if vec == 2:
        sizes += [vec * 256 * g + 1 for g in (1, 3)]
    return tuple(sizes)


# ---------------------------------------------------------------------------
# number-format helpers
# ---------------------------------------------------------------------------

def is_bf16_exact(a) -> bool:
    """True when every element survives a round trip through bfloat16."""
    f = np.ascontiguousarray(a, dtype=np.float32)
    if not np.array_equal(f.astype(np.float64), np.asarray(a, dtype=np.float64)):
        return False
    return not np.any(f.view(np.uint32) & 0xFFFF)


def round_to_bf16(a) -> np.ndarray:
    """fp32 -> bf16 round-to-nearest-even (the kernels' residual rounding),
    returned as fp32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    rnd = np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (((u + rnd) >> np.uint32(16)) << np.uint32(16)).view(np.float32)


# ---------------------------------------------------------------------------
# logistic probes
# ---------------------------------------------------------------------------

def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(np.array(key, dtype=np.uint32))


@functools.lru_cache(maxsize=16)
def onehot_probe(n: int, K: int, chains: int = BCH) -> Dict[str, np.ndarray]:
    """(a) X[r, (r*s) mod K] = 1; theta[k, b] = +-32 seeded; y in {0, 1}.

    y is seeded over r mod K: rows K apart share a column AND a label.  With
    independent labels a (y=0, theta=-32) row's -e^-32 remainder and a
    (y=1, theta=-32) row's unit residual of the same column could meet in
    one fp32 MFMA accumulator, and that sum is not rounded to nearest on
    gfx950: a one-instruction probe measured (-e^-32) + 1*1 = 1 - 2^-24
    (while 1 + 1*(-e^-32) = 1).  That is a property of the matrix cores,
    not a mapping error, so the probe keeps remainders and units apart.
    Independent labels per row are covered by (b) and (c).
    """
    rng = _rng(0xA, n, K, chains)
    cols = (np.arange(n, dtype=np.int64) * ONEHOT_STRIDE) % K
    X = np.zeros((n, K))
    X[np.arange(n), cols] = 1.0
    theta = SAT * (2.0 * rng.randint(0, 2, size=(K, chains)) - 1.0)
    y = rng.randint(0, 2, size=K).astype(np.float64)[np.arange(n) % K]
    return _freeze(X=X, y=y, theta=theta, cols=cols)


@functools.lru_cache(maxsize=16)
def dense_int_probe(n: int, K: int, chains: int = BCH) -> Dict[str, np.ndarray]:
    """(b) X in {0,1,2} (>= 1 non-zero per row); theta = sigma_b*32*w_k."""
    rng = _rng(0xB, n, K, chains)
    X = rng.randint(0, 3, size=(n, K)).astype(np.float64)
    empty = ~X.any(axis=1)
    X[empty, np.arange(n)[empty] % K] = 1.0
    w = rng.randint(1, 5, size=K).astype(np.float64)
    sigma = 2.0 * rng.randint(0, 2, size=chains) - 1.0
    sigma[: 2] = (1.0, -1.0)  # both signs always present
    theta = SAT * w[:, None] * sigma[None, :chains]
    y = rng.randint(0, 2, size=n).astype(np.float64)
    return _freeze(X=X, y=y, theta=theta)


@functools.lru_cache(maxsize=16)
def zero_theta_probe(n: int, K: int, chains: int = BCH) -> Dict[str, np.ndarray]:
    """(c) theta = 0; X = j/8 with |j| <= 16; y in {0, 1}."""
    rng = _rng(0xC, n, K, chains)
    X = rng.randint(-16, 17, size=(n, K)) / 8.0
    theta = np.zeros((K, chains))
    y = rng.randint(0, 2, size=n).astype(np.float64)
    return _freeze(X=X, y=y, theta=theta)


LOGISTIC_PROBES = {
    "onehot": onehot_probe,
    "dense_int": dense_int_probe,
    "zero_theta": zero_theta_probe,
}


def _freeze(**arrays) -> Dict[str, np.ndarray]:
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


def logistic_reference(X, y, theta) -> Tuple[np.ndarray, np.ndarray]:
    """Plain fp64 numpy reference: theta[K, B] -> (logp[B], G[K, B])."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    Z = X @ theta
    logp = np.sum(y[:, None] * Z - np.logaddexp(0.0, Z), axis=0)
    e = np.exp(-np.abs(Z))  # stable sigmoid; exactly 1/2 at z = 0
    R = y[:, None] - np.where(Z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return logp, X.T @ R


def logistic_saturated(X, y, theta) -> Tuple[np.ndarray, np.ndarray]:
    """The exactly representable part of the answer for probes (a)/(b):
    softplus(z) -> max(z, 0), sigmoid(z) -> [z > 0]  (|z| >= 32 required)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Z = X @ np.asarray(theta, dtype=np.float64)
    assert np.all(np.abs(Z) >= SAT)
    logp = np.sum(y[:, None] * Z - np.maximum(Z, 0.0), axis=0)
    R = y[:, None] - (Z > 0)
    return logp, X.T @ R


@functools.lru_cache(maxsize=None)
def batched_reference(probe: str, n: int, K: int):
    p = LOGISTIC_PROBES[probe](n, K)
    logp, G = logistic_reference(p["X"], p["y"], p["theta"])
    return _freeze(logp=logp, G=G)


@functools.lru_cache(maxsize=None)
def single_reference(probe: str, n: int, K: int):
    """Single-chain reference: chain 0 of the batched probe is beta."""
    p = LOGISTIC_PROBES[probe](n, K)
    logp, G = logistic_reference(p["X"], p["y"], p["theta"][:, :1])
    return _freeze(logp=logp[0:1].copy(), G=G[:, 0].copy())


def saturation_atol(n: int) -> float:
    """Room for the <= 2^-46 saturation remainders of an n-row sum."""
    return n * 2.0 ** -40


# ---------------------------------------------------------------------------
# gaussian probe
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=16)
def gaussian_probe(n: int) -> Dict[str, np.ndarray]:
    """(d) x, y multiples of 1/8 with |.| <= 4 (bf16-exact)."""
    rng = _rng(0xD, n)
    x = rng.randint(-32, 33, size=n) / 8.0
    y = rng.randint(-32, 33, size=n) / 8.0
    return _freeze(x=x, y=y)


def gaussian_reference(x, y, a: float, b: float, sigma: float = 1.0):
    """fp64 numpy reference -> (logp, dlogp/da, dlogp/db)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    r = y - (a + b * x)
    sig2 = sigma * sigma
    logp = -0.5 * x.size * np.log(2.0 * np.pi * sig2) - 0.5 * np.sum(r * r) / sig2
    return float(logp), float(np.sum(r) / sig2), float(np.sum(r * x) / sig2)
