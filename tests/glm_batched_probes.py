"""16-chain probe inputs and references for the batched GLM family kernel
(glm_family_batched.hip).

Plain helper module (imported by ``test_glm_batched_probes_cpu.py`` and
``test_gpu_glm_family_batched.py``), in the style of ``glm_probes.py``,
whose shards (X, y, offset) it reuses: only theta grows a chain axis.  The
chains are pairwise different, so a swapped or duplicated chain shows; only
the zero-beta probe is chain-blind.

Exact probes: every operand is bf16-exact or exact as three bf16 pieces,
and every z, term, residual and gradient partial sum is a whole number of
its unit below 2^24 of them, so the kernel is held to fp64 numpy bit-tight.

``poisson_dense`` / ``poisson_onehot``  theta[k, b] = -128 * w[k, b], w in
     1..4: z <= -128, exp(z) flushes to 0 in fp32; logp = sum y*z, G = X^T y.
``poisson_zero_beta``  theta = 0, offset in {0, -128}: exp(z) is 1 or 0.
``gaussian_sigma1`` / ``gaussian_sigma2``  the sparse probe with per-chain
     beta in multiples of 1/4, |beta| <= 2: r = y - z is a multiple of 1/8
     with |r| <= 20.
``gaussian_wide_onehot``  the probe that exposes a dropped third piece.
     One-hot rows on the stride-37 walk; y and theta are multiples of 2^-17
     with |.| < 2, so theta needs up to 18 bits and r = y - theta up to 19:
     neither survives one or two bf16 pieces.  sigma = 1, so the residual
     is r itself and G (sums of r over at most 32 rows: < 2^24 units of
     2^-17) is bit-exact.  r*r is not exact in fp32, so logp is compared to
     rtol 1e-6.  Only used where every column sums at most 32 rows.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Tuple

import numpy as np

import exact_probes as ep
import glm_probes as gp

BCH = 16
#: feature counts of the kernel (asserted equal to ops.GLM_FAMILY_BATCHED_K)
BATCHED_K = (8, 16, 32, 64, 128, 256, 512, 1024)
#: FED_GLM_BATCHED_GRID for the two-trip case
DEEP_GRID = 2
PROBE_CONST = gp.PROBE_CONST
#: rows of one column the wide probe may sum: 32 * |r| < 2^7 = 2^24 * 2^-17
WIDE_MAX_ROWS_PER_COLUMN = 32
WIDE_UNIT = 2.0 ** -17

#: accuracy yardstick of the batched kernel: the single-chain kernel's.
#: With three theta pieces and three residual pieces the operands are exact;
#: what is left are the single-chain kernel's own error sources, fp32
#: partial sums and __expf.
BATCHED_M = gp.KERNEL_M
#: per-chain scales of beta in the accuracy cases: 16 distinct values in
#: [-1, 1], which keep |z| <= ACC_ZMAX
ACC_SCALES = tuple(np.linspace(-1.0, 1.0, BCH))


def tile_rows(K: int) -> int:
    """T: rows per block tile (K >= 128: four waves split K over 32 rows;
    below, four waves take 32 rows each)."""
    return 32 if K >= 128 else 128


def edge_rows(K: int) -> Tuple[int, ...]:
    T = tile_rows(K)
    return tuple(sorted({1, 15, 16, 17, 31, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1}))


def deep_rows(K: int) -> int:
    """Under FED_GLM_BATCHED_GRID=2: six tiles, three per block, the last
    ragged by five rows."""
    return 5 * tile_rows(K) + 5


def stale_small_rows(K: int) -> int:
    return tile_rows(K) + 1


def stale_big_rows(K: int) -> int:
    return 20 * tile_rows(K) + 3


def all_rows(K: int) -> Tuple[int, ...]:
    """Every row count the GPU exact tests evaluate at this K."""
    return tuple(sorted(set(edge_rows(K)) | {deep_rows(K), stale_small_rows(K),
                                             stale_big_rows(K)}))


def wide_ok(n: int, K: int) -> bool:
    """The wide probe's condition: the stride-37 walk visits the columns
    evenly, so a column sums at most ceil(n / K) rows."""
    return -(-n // K) <= WIDE_MAX_ROWS_PER_COLUMN


def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(np.array(key, dtype=np.uint32))


def _freeze(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------
# probes: dict(X, y, theta[K,16], offset?)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def poisson_saturated(kind: str, n: int, K: int) -> Dict[str, np.ndarray]:
    p = gp.poisson_saturated_probe(kind, n, K)
    w = _rng(0x61, kind == "dense", n, K).randint(1, 5, size=(K, BCH)).astype(np.float64)
    w[0] = 1 + np.arange(BCH) % 4           # chains pairwise different even at K = 8:
    w[1] = 1 + (np.arange(BCH) // 4) % 4    # (w[0], w[1]) is the chain index in base 4
    return _freeze(X=p["X"], y=p["y"], theta=-gp.SAT * w)


@functools.lru_cache(maxsize=8)
def poisson_zero_beta(n: int, K: int) -> Dict[str, np.ndarray]:
    p = gp.poisson_zero_beta_probe(n, K)
    return _freeze(X=p["X"], y=p["y"], offset=p["offset"], theta=np.zeros((K, BCH)))


@functools.lru_cache(maxsize=8)
def gaussian_sparse(n: int, K: int, sigma: float) -> Dict[str, np.ndarray]:
    p = gp.gaussian_sparse_probe(n, K, sigma)
    theta = _rng(0x63, n, K, int(sigma)).randint(-8, 9, size=(K, BCH)) / 4.0
    theta[0] = (np.arange(BCH) % 4 - 2) / 4.0
    theta[1] = (np.arange(BCH) // 4 - 2) / 4.0
    return _freeze(X=p["X"], y=p["y"], theta=theta)


@functools.lru_cache(maxsize=8)
def gaussian_wide_onehot(n: int, K: int) -> Dict[str, np.ndarray]:
    assert wide_ok(n, K)
    rng = _rng(0x64, n, K)
    cols = (np.arange(n, dtype=np.int64) * ep.ONEHOT_STRIDE) % K
    X = np.zeros((n, K))
    X[np.arange(n), cols] = 1.0
    lim = 1 << 18  # |.| < 2 in units of 2^-17
    y = rng.randint(-lim + 1, lim, size=n) * WIDE_UNIT
    theta = rng.randint(-lim + 1, lim, size=(K, BCH)) * WIDE_UNIT
    # every chain needs all three pieces somewhere: top*2^10 + an odd
    # remainder in [257, 511] leaves nine significant bits after the first piece
    theta[0] = (rng.randint(128, 256, size=BCH) * 1024 + 257 + 2 * np.arange(BCH)) * WIDE_UNIT
    return _freeze(X=X, y=y, theta=theta, cols=cols)


# ---------------------------------------------------------------------------
# fp64 references: theta[K,B] -> (logp[B], G[K,B])
# ---------------------------------------------------------------------------

def _z(X, theta, offset):
    Z = np.asarray(X, dtype=np.float64) @ np.asarray(theta, dtype=np.float64)
    if offset is not None:
        Z = Z + np.asarray(offset, dtype=np.float64)[:, None]
    return Z


def poisson_reference(X, y, theta, offset=None, const: float = 0.0):
    """The general Poisson formula."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    Z = _z(X, theta, offset)
    mu = np.exp(Z)
    return np.sum(y[:, None] * Z - mu, axis=0) + const, X.T @ (y[:, None] - mu)


def poisson_flushed_reference(X, y, theta, offset=None, const: float = 0.0):
    """The exactly representable answer: exp(z) is 0 for z <= -128 and 1
    for z = 0 (every z of the Poisson probes is one of them)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    Z = _z(X, theta, offset)
    assert np.all((Z <= -gp.SAT) | (Z == 0.0))
    mu = (Z == 0.0).astype(np.float64)
    return np.sum(y[:, None] * Z - mu, axis=0) + const, X.T @ (y[:, None] - mu)


def gaussian_reference(X, y, theta, sigma: float, offset=None, const: float = 0.0):
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    R = y[:, None] - _z(X, theta, offset)
    s2 = sigma * sigma
    return -np.sum(R * R, axis=0) / (2.0 * s2) + const, X.T @ R / s2


def _pois_ref(p):
    return poisson_flushed_reference(p["X"], p["y"], p["theta"], p.get("offset"), PROBE_CONST)


def _gauss_ref(sigma):
    return lambda p: gaussian_reference(p["X"], p["y"], p["theta"], sigma, None, PROBE_CONST)


#: probe id -> (link, builder(n, K) -> dict, reference(dict) -> (logp[16], G[K,16]),
#:              sigma, logp exact?); the references include PROBE_CONST
EXACT_PROBES = {
    "poisson_dense": ("poisson", lambda n, K: poisson_saturated("dense", n, K), _pois_ref,
                      1.0, True),
    "poisson_onehot": ("poisson", lambda n, K: poisson_saturated("onehot", n, K), _pois_ref,
                       1.0, True),
    "poisson_zero_beta": ("poisson", poisson_zero_beta, _pois_ref, 1.0, True),
    "gaussian_sigma1": ("gaussian", lambda n, K: gaussian_sparse(n, K, 1.0), _gauss_ref(1.0),
                        1.0, True),
    "gaussian_sigma2": ("gaussian", lambda n, K: gaussian_sparse(n, K, 2.0), _gauss_ref(2.0),
                        2.0, True),
    "gaussian_wide_onehot": ("gaussian", gaussian_wide_onehot, _gauss_ref(1.0), 1.0, False),
}
WIDE_LOGP_RTOL = 1e-6


def probe_applies(probe: str, n: int, K: int) -> bool:
    return probe != "gaussian_wide_onehot" or wide_ok(n, K)


@functools.lru_cache(maxsize=None)
def exact_reference(probe: str, n: int, K: int):
    """Computed once per (probe, n, K) and shared; read-only."""
    _, build, ref, _, _ = EXACT_PROBES[probe]
    logp, G = ref(build(n, K))
    logp, G = np.array(logp), np.array(G)
    logp.setflags(write=False)
    G.setflags(write=False)
    return logp, G


# ---------------------------------------------------------------------------
# accuracy cases: glm_probes.accuracy_case data, 16 scaled copies of beta
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def accuracy_chains(family: str, K: int):
    """theta[K,16] (f32-exact) and one accuracy_case-shaped dict per chain:
    fp64 reference and bound denominators on the stored bf16 data."""
    c = gp.accuracy_case(family, "bfloat16", K)
    theta = np.stack([gp._round_f32(c["beta"] * s) for s in ACC_SCALES], axis=1)
    X, y, offset = c["X"], c["y"], c.get("offset")
    Z = _z(X, theta, offset)
    assert np.max(np.abs(Z)) <= gp.ACC_ZMAX
    if family == "poisson":
        const = -float(sum(math.lgamma(v + 1.0) for v in y))
    else:
        const = -0.5 * gp.ACC_N * math.log(2 * math.pi * c["sigma"] ** 2)
    cases = []
    for b in range(BCH):
        z = Z[:, b]
        if family == "poisson":
            mu = np.exp(z)
            term, resid = y * z - mu, y - mu
        else:
            s2 = c["sigma"] ** 2
            r = y - z
            term, resid = -r * r / (2 * s2), r / s2
        cases.append(_freeze(
            logp=np.float64(np.sum(term) + const), G=X.T @ resid,
            logp_scale=np.float64(np.sum(np.abs(term))), G_scale=np.abs(X).T @ np.abs(resid),
        ))
    theta.setflags(write=False)
    return theta, tuple(cases)
