"""Probe inputs and references for the softmax (multinomial) stage of the
batched GLM family kernel (glm_family_batched.hip, SoftmaxStage).

Plain helper module (imported by ``test_glm_softmax_cpu.py`` and
``test_gpu_glm_softmax.py``), in the style of ``glm_batched_probes.py``.
A probe is ``dict(X[n,K], y[n] labels, theta[K,16], C)``; ``theta`` is the
packed image the kernel takes: with ``CP = class_group(C)`` column
``g*CP + c`` is class ``c`` of chain ``g`` and the columns of padded classes
(``c >= C``) are zero.  The ``16 // CP`` chains of every probe are pairwise
different, so a swapped group shows.  The general reference is fp64 numpy
with ``logsumexp`` formed by max subtraction.

The exact probes rest on ``__expf(0) = 1`` and ``__expf(z <= -127) = 0`` in
fp32 (the Poisson probes rely on the same at -128) and on ``__logf(1) = 0``.

``saturated_onehot``  one-hot rows on the stride-37 walk; ``theta[k, c] =
     -128 * perm_k[c] + m * 2^-10`` with ``perm_k`` a permutation of 1..C and
     ``|m| <= 8``.  Every real z is negative, so a padded class that leaks
     in with z = 0 wins the max and shows.  The classes of a row are at
     least 127 apart, so the softmax is the one-hot of the argmax and s = 1:
     resid = onehot(y) - onehot(argmax), term = z_y - max z.  theta needs 21
     significant bits, so a dropped third piece shows in logp.  Bit-exact.
``saturated_dense``  rows with several entries from {1, 2} in the columns of
     one parity; ``theta[k, c] = -128 * a_k * perm_{k%2}[c]``, a in 1..3, so
     ``z_c = -128 * perm[c] * S`` with an integer S >= 1: the largest z of a
     row exceeds the second by >= 128.  Bit-exact.
``uniform``  all real classes of a chain share one theta column: z - m = 0,
     e = 1, s = C.  For C in {2, 4, 8, 16} p = 1/C is exact, the residuals
     are multiples of 1/16 and G is bit-exact; logp = -N log C is compared
     at ``WIDE_LOGP_RTOL``.  For other C both fall under the accuracy bound.
     The probe that catches padded classes counted into s.

Accuracy sets: seeded categorical data compared with fp64 numpy on the
stored data under ``|got - ref| <= M * 2^-24 * sum_r |row r's contribution|``
per output component (the form of ``glm_probes.accuracy_ratios``).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Tuple

import numpy as np

import exact_probes as ep
import glm_batched_probes as bp
import glm_probes as gp

BCH = bp.BCH
BATCHED_K = bp.BATCHED_K
DEEP_GRID = bp.DEEP_GRID
WIDE_LOGP_RTOL = bp.WIDE_LOGP_RTOL
SAT = gp.SAT
UNIT = 2.0 ** -10
#: class counts of the exact GPU tests: the full row sweep, and three rows
EDGE_CLASSES = (3, 16)
FEW_CLASSES = (2, 4, 5, 8, 9)
POW2_CLASSES = (2, 4, 8, 16)

tile_rows, edge_rows, deep_rows = bp.tile_rows, bp.edge_rows, bp.deep_rows
stale_small_rows, stale_big_rows = bp.stale_small_rows, bp.stale_big_rows


def few_rows(K: int) -> Tuple[int, ...]:
    return (1, 17, tile_rows(K) + 1)


def class_group(C: int) -> int:
    """CP: the next power of two >= C."""
    assert 2 <= C <= BCH
    cp = 2
    while cp < C:
        cp *= 2
    return cp


def n_groups(C: int) -> int:
    return BCH // class_group(C)


def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(np.array(key, dtype=np.uint32))


_freeze = bp._freeze


def _pack(per_group: np.ndarray, C: int) -> np.ndarray:
    """per_group[K, G, C] -> the packed image theta[K,16], padded classes 0."""
    K, G, _ = per_group.shape
    cp = class_group(C)
    th = np.zeros((K, G, cp))
    th[:, :, :C] = per_group
    return th.reshape(K, BCH)


def unpack(theta16: np.ndarray, C: int) -> np.ndarray:
    """theta[K,16] -> [K, G, C] (the real classes of every chain)."""
    K = theta16.shape[0]
    return np.asarray(theta16).reshape(K, n_groups(C), class_group(C))[:, :, :C]


# ---------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def saturated_onehot(n: int, K: int, C: int) -> Dict[str, np.ndarray]:
    rng = _rng(0x71, n, K, C)
    G = n_groups(C)
    cols = (np.arange(n, dtype=np.int64) * ep.ONEHOT_STRIDE) % K
    X = np.zeros((n, K))
    X[np.arange(n), cols] = 1.0
    perm = np.argsort(rng.random_sample((K, G, C)), axis=2) + 1.0   # a permutation of 1..C
    m = rng.randint(-8, 9, size=(K, G, C)).astype(np.float64)
    m[0] = (np.arange(G) + 1.0)[:, None]    # row 0 reads column 0: chains pairwise different
    th = -SAT * perm + m * UNIT
    y = rng.randint(0, C, size=n)
    # every other row is labelled with chain 0's argmax: term = 0, resid = 0 there
    y[1::2] = np.argmax(th[cols[1::2], 0, :], axis=1)
    return _freeze(X=X, y=y, theta=_pack(th, C), cols=cols) | {"C": C}


@functools.lru_cache(maxsize=8)
def saturated_dense(n: int, K: int, C: int) -> Dict[str, np.ndarray]:
    rng = _rng(0x72, n, K, C)
    G = n_groups(C)
    parity = rng.randint(0, 2, size=n)
    nnz = min(6, K // 2)
    X = np.zeros((n, K))
    for r in range(n):
        ks = 2 * rng.choice(K // 2, size=nnz, replace=False) + parity[r]
        X[r, ks] = rng.randint(1, 3, size=nnz)
    a = rng.randint(1, 4, size=(K, G)).astype(np.float64)
    a[0] = 1 + np.arange(G) % 3          # (a[0], a[1]) is the chain index in base 3,
    a[1] = 1 + np.arange(G) // 3         # read by the rows of parity 0 and 1
    perm = np.argsort(rng.random_sample((2, G, C)), axis=2) + 1.0
    th = -SAT * a[:, :, None] * perm[np.arange(K) % 2]
    y = rng.randint(0, C, size=n)
    return _freeze(X=X, y=y, theta=_pack(th, C), parity=parity) | {"C": C}


@functools.lru_cache(maxsize=8)
def uniform(n: int, K: int, C: int) -> Dict[str, np.ndarray]:
    rng = _rng(0x73, n, K, C)
    G = n_groups(C)
    X = gp.gaussian_sparse_probe(n, K, 1.0)["X"]
    t = rng.randint(-8, 9, size=(K, G)) / 4.0
    t[0] = (np.arange(G) % 4 - 2) / 4.0
    t[1] = (np.arange(G) // 4 - 2) / 4.0
    th = np.repeat(t[:, :, None], C, axis=2)
    y = rng.randint(0, C, size=n)
    return _freeze(X=X, y=y, theta=_pack(th, C)) | {"C": C}


# ---------------------------------------------------------------------------
# references: (logp[G], G16[K,16]) with the columns of padded classes zero
# ---------------------------------------------------------------------------

def _onehot(y, C):
    return (np.asarray(y)[:, None] == np.arange(C)[None, :]).astype(np.float64)


def chain_terms(X, y, beta):
    """fp64, logsumexp by max subtraction: per-row (term[n], resid[n,C])."""
    X = np.asarray(X, dtype=np.float64)
    Z = X @ np.asarray(beta, dtype=np.float64)
    m = Z.max(axis=1, keepdims=True)
    E = np.exp(Z - m)
    s = E.sum(axis=1, keepdims=True)
    term = (Z - m)[np.arange(len(y)), np.asarray(y)] - np.log(s[:, 0])
    return term, _onehot(y, Z.shape[1]) - E / s


def chain_reference(X, y, beta):
    """The general formula for one chain: beta[K,C] -> (logp, G[K,C])."""
    term, resid = chain_terms(X, y, beta)
    return float(np.sum(term)), np.asarray(X, dtype=np.float64).T @ resid


def _per_group(p, one_chain):
    C, cp = p["C"], class_group(p["C"])
    th = unpack(p["theta"], C)
    K, G = th.shape[0], th.shape[1]
    logp, G16 = np.zeros(G), np.zeros((K, G, cp))
    for g in range(G):
        logp[g], G16[:, g, :C] = one_chain(p["X"], p["y"], th[:, g, :])
    return logp, G16.reshape(K, BCH)


def reference(p):
    return _per_group(p, chain_reference)


def _saturated_chain(X, y, beta):
    """The exactly representable answer of the saturated probes: exp of a
    difference <= -127 is 0 in fp32, so softmax = onehot(argmax), s = 1."""
    X = np.asarray(X, dtype=np.float64)
    Z = X @ beta
    top = np.sort(Z, axis=1)
    assert np.all(top[:, -1] - top[:, -2] >= SAT - 1.0) and np.all(Z < 0)
    m = Z.max(axis=1)
    resid = _onehot(y, Z.shape[1]) - _onehot(np.argmax(Z, axis=1), Z.shape[1])
    return float(np.sum(Z[np.arange(len(y)), y] - m)), X.T @ resid


def saturated_reference(p):
    return _per_group(p, _saturated_chain)


def _uniform_chain(X, y, beta):
    X = np.asarray(X, dtype=np.float64)
    C = beta.shape[1]
    assert np.all(beta == beta[:, :1])
    return -len(y) * math.log(C), X.T @ (_onehot(y, C) - 1.0 / C)


def uniform_reference(p):
    return _per_group(p, _uniform_chain)


#: probe id -> (builder(n, K, C) -> dict, reference(dict) -> (logp[G], G16[K,16]))
EXACT_PROBES = {
    "saturated_onehot": (saturated_onehot, saturated_reference),
    "saturated_dense": (saturated_dense, saturated_reference),
    "uniform": (uniform, uniform_reference),
}


def probe_check(probe: str, C: int) -> str:
    """How a probe is held at C: 'exact' (logp and G bit-exact), 'exact_G'
    (G bit-exact, logp at WIDE_LOGP_RTOL) or 'bound' (the accuracy bound)."""
    if probe != "uniform":
        return "exact"
    return "exact_G" if C in POW2_CLASSES else "bound"


@functools.lru_cache(maxsize=None)
def exact_reference(probe: str, n: int, K: int, C: int):
    """Computed once per (probe, n, K, C) and shared; read-only."""
    build, ref = EXACT_PROBES[probe]
    logp, G16 = ref(build(n, K, C))
    logp.setflags(write=False)
    G16.setflags(write=False)
    return logp, G16


def uniform_scales(p):
    """Bound denominators of the uniform probe: (sum |term| [G], |X|^T |resid| [K,16])."""
    C, cp = p["C"], class_group(p["C"])
    K = p["X"].shape[1]
    G = n_groups(C)
    n = len(p["y"])
    Gs = np.zeros((K, G, cp))
    Gs[:, :, :C] = (np.abs(p["X"]).T @ np.abs(_onehot(p["y"], C) - 1.0 / C))[:, None, :]
    return np.full(G, n * math.log(C)), Gs.reshape(K, BCH)


# ---------------------------------------------------------------------------
# accuracy sets
# ---------------------------------------------------------------------------

ACC_N = gp.ACC_N
ACC_K = (20, 100, 512)
ACC_C = (3, 16)
ACC_DTYPES = ("bfloat16", "float32")

#: Worst ratio |eager fp32 - fp64 reference| / (2^-24 * sum_r |row r's
#: contribution|) over every output component of every accuracy case (2
#: dtypes x K in {20, 100, 512} x C in {3, 16} at ACC_N rows), measured on
#: the CPU with one thread by
#:
#:     python -m pytest tests/test_glm_softmax_cpu.py -k eager_meets -s
#:
#: which prints each case's ratio: worst 2.09 (the gradient, bfloat16,
#: K = 512, C = 16; the 5000-row fp32 chain of ``X^T @ resid``), 1.88 for
#: float32 at the same shape, at most 0.81 at C = 3; logp (fp64 row sum) at
#: most 0.13.  Rounded up to the next power of two, as EAGER_M, FVP_EAGER_M and
#: FISHER_EAGER_M were fixed.
SOFTMAX_EAGER_M = 4.0
#: the kernel: the project's rule KERNEL_M = 4 * EAGER_M (fast exponential,
#: another summation order)
SOFTMAX_KERNEL_M = 4.0 * SOFTMAX_EAGER_M


def _case(X, y, beta):
    term, resid = chain_terms(X, y, beta)
    return _freeze(
        logp=np.float64(np.sum(term)), G=X.T @ resid,
        logp_scale=np.float64(np.sum(np.abs(term))), G_scale=np.abs(X).T @ np.abs(resid),
    )


@functools.lru_cache(maxsize=None)
def accuracy_case(dtype_name: str, K: int, C: int, scale: float = 1.0):
    """Stored data (X rounded to ``dtype_name``, beta to f32), the fp64
    reference on it and the bound denominators.  ``scale`` multiplies the
    generating beta (the overflow case evaluates far from it)."""
    from pytensor_federated_amd.models import generate_softmax_dataset

    X, y, beta = generate_softmax_dataset(ACC_N, K, C, seed=300 + K + C)
    X = gp._round_bf16(X) if dtype_name == "bfloat16" else gp._round_f32(X)
    beta = gp._round_f32(beta * scale)
    out = dict(X=X, y=y, beta=beta, **_case(X, y, beta))
    _freeze(**out)
    return out


def accuracy_model(dtype_name: str, K: int, C: int, **kw):
    import torch

    from pytensor_federated_amd.models import SoftmaxGLMModel

    c = accuracy_case(dtype_name, K, C)
    return SoftmaxGLMModel(torch.tensor(c["X"]), torch.tensor(c["y"]), C,
                           dtype=getattr(torch, dtype_name), **kw)


#: per-chain scales of beta when several chains share a launch
ACC_SCALES = (1.0, -1.0, 0.5, -0.5, 0.75, -0.75, 0.25, -0.25)


@functools.lru_cache(maxsize=None)
def accuracy_chains(K: int, C: int):
    """theta[K,C,G] (f32-exact) for the G chains of one launch and one case
    dict per chain, on the bf16 data."""
    c = accuracy_case("bfloat16", K, C)
    G = n_groups(C)
    theta = np.stack([gp._round_f32(c["beta"] * s) for s in ACC_SCALES[:G]], axis=2)
    cases = tuple(_case(c["X"], c["y"], theta[:, :, g]) for g in range(G))
    theta.setflags(write=False)
    return theta, cases


def accuracy_ratios(case, logp: float, G: np.ndarray) -> Tuple[float, float]:
    """(logp ratio, worst grad ratio), as glm_probes.accuracy_ratios; a
    component no row contributes to must be exactly the reference's."""
    unit = 2.0 ** -24
    r_logp = abs(logp - case["logp"]) / (unit * case["logp_scale"])
    err, scale = np.abs(np.asarray(G) - case["G"]), case["G_scale"]
    assert np.all(err[scale == 0] == 0)
    r_grad = float(np.max(err[scale > 0] / (unit * scale[scale > 0])))
    return float(r_logp), r_grad


#: the overflow case: beta scaled so that the largest |z| is about 1e3
OVERFLOW_K, OVERFLOW_C = 20, 5


@functools.lru_cache(maxsize=None)
def overflow_case():
    base = accuracy_case("bfloat16", OVERFLOW_K, OVERFLOW_C)
    zmax = float(np.max(np.abs(base["X"] @ base["beta"])))
    c = accuracy_case("bfloat16", OVERFLOW_K, OVERFLOW_C, scale=round(1e3 / zmax))
    assert 5e2 <= np.max(np.abs(c["X"] @ c["beta"])) <= 2e3
    return c
