"""Premise checks for tests/glm_batched_probes.py and the CPU side of the
batched GLM family path (no GPU needed).

test_gpu_glm_family_batched.py holds the MFMA kernel to fp64 references
bit-tight.  That is fair only if, at every (probe, K, n) it uses, every
operand reaches the matrix cores unrounded (bf16-exact, or exact as three
bf16 pieces) and every intermediate -- z, term, residual, each gradient
partial sum -- is a whole number of its unit below 2^24 units, so that no
fp32 accumulation order can change it.
"""
import numpy as np
import pytest
import torch

import exact_probes as ep
import glm_batched_probes as bp
import glm_probes as gp

from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel
from pytensor_federated_amd.ops import (
    GLM_FAMILY_BATCHED_K,
    glm_family_batched_supports,
    split_bf16x3,
)

TWO24 = 2.0 ** 24


def _pieces_sum64(v: np.ndarray) -> np.ndarray:
    """The three pieces of ``v`` (any shape, taken as [K, B]) summed in fp64,
    back in v's layout."""
    v2 = np.atleast_2d(np.asarray(v, dtype=np.float64))
    p = split_bf16x3(torch.tensor(v2, dtype=torch.float32))
    assert p.shape == (3, v2.shape[1], v2.shape[0])
    return p.to(torch.float64).sum(dim=0).t().numpy().reshape(np.shape(v))


def _whole_units(a, unit, what):
    q = np.asarray(a, dtype=np.float64) / unit
    assert np.array_equal(q, np.round(q)), f"{what}: not a multiple of {unit}"
    assert np.max(np.abs(q), initial=0.0) <= TWO24, f"{what}: above 2^24 units of {unit}"


# ---------------------------------------------------------------------------
# split_bf16x3
# ---------------------------------------------------------------------------

def test_split_bf16x3_is_exact_over_many_exponents():
    rng = np.random.RandomState(20240)
    n = 1 << 16
    mant = rng.uniform(1.0, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    v = (mant * 2.0 ** rng.randint(-60, 61, size=n)).astype(np.float32)
    v[:4] = (0.0, 1.0, -1.0, np.float32(1.0) + np.float32(2.0 ** -23))
    theta = torch.tensor(v).reshape(-1, 16)
    p = split_bf16x3(theta)
    assert p.dtype == torch.bfloat16 and p.shape == (3, 16, n // 16)
    for piece in p:
        assert piece.dtype == torch.bfloat16
    got = p.to(torch.float64).sum(dim=0).t().numpy()
    np.testing.assert_array_equal(got, v.reshape(-1, 16).astype(np.float64))
    # the pieces are what the issue defines, differences taken in f32
    t32 = theta.t().contiguous()
    p0 = t32.to(torch.bfloat16)
    p1 = (t32 - p0.float()).to(torch.bfloat16)
    p2 = (t32 - p0.float() - p1.float()).to(torch.bfloat16)
    assert torch.equal(p[0], p0) and torch.equal(p[1], p1) and torch.equal(p[2], p2)


def test_two_pieces_are_not_enough_for_the_wide_probe():
    """What makes gaussian_wide_onehot a test of the third piece."""
    p = bp.gaussian_wide_onehot(64, 16)
    pieces = split_bf16x3(torch.tensor(p["theta"], dtype=torch.float32)).to(torch.float64)
    two = pieces[:2].sum(dim=0).t().numpy()
    assert np.all(np.any(two != p["theta"], axis=0)), "every chain needs its third piece"
    r = p["y"][:, None] - p["X"] @ p["theta"]
    rp = split_bf16x3(torch.tensor(r, dtype=torch.float32)).to(torch.float64)
    assert np.any(rp[:2].sum(dim=0).t().numpy() != r)
    np.testing.assert_array_equal(rp.sum(dim=0).t().numpy(), r)


# ---------------------------------------------------------------------------
# shapes and support
# ---------------------------------------------------------------------------

def test_supported_shapes():
    assert tuple(GLM_FAMILY_BATCHED_K) == bp.BATCHED_K
    for K in (1, 4, 8, 12, 16, 24, 32, 64, 100, 128, 256, 512, 1024, 1536, 2048, 4096):
        assert glm_family_batched_supports(torch.bfloat16, K) == (K in GLM_FAMILY_BATCHED_K)
        assert not glm_family_batched_supports(torch.float32, K)
        assert not glm_family_batched_supports(torch.float64, K)
    assert not glm_family_batched_supports(torch.bfloat16, 2048)


@pytest.mark.parametrize("K", bp.BATCHED_K)
def test_row_lists(K):
    T = bp.tile_rows(K)
    rows = bp.edge_rows(K)
    assert {1, 15, 16, 17, 31, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1} == set(rows)
    assert bp.deep_rows(K) == 5 * T + 5
    # six tiles on two blocks: three each, the last ragged by five rows
    assert -(-bp.deep_rows(K) // T) == 3 * bp.DEEP_GRID and bp.deep_rows(K) % T == 5
    assert bp.stale_big_rows(K) == 20 * T + 3 and bp.stale_small_rows(K) == T + 1


def test_wide_probe_row_condition():
    """At most 32 rows per column wherever the wide probe is used, and it is
    used at every (K, n) but the few narrow-K ones that break the condition."""
    skipped = []
    for K in bp.BATCHED_K:
        for n in bp.all_rows(K):
            if not bp.probe_applies("gaussian_wide_onehot", n, K):
                skipped.append((K, n))
                continue
            p = bp.gaussian_wide_onehot(n, K)
            per_col = np.bincount(p["cols"], minlength=K)
            assert per_col.max() <= bp.WIDE_MAX_ROWS_PER_COLUMN, (K, n)
    assert all(K <= 64 for K, _ in skipped)
    # every K keeps its single-row, ragged and multi-tile cases
    for K in bp.BATCHED_K:
        kept = [n for n in bp.edge_rows(K) if bp.wide_ok(n, K)]
        assert {1, 17, 65} <= set(kept) and max(kept) > bp.tile_rows(K)


# ---------------------------------------------------------------------------
# premises of the exact probes at every (K, n) of the GPU tests
# ---------------------------------------------------------------------------

def _units(probe, sigma):
    """(z unit, term unit or None when logp is not claimed exact, resid unit,
    unit of resid * x)."""
    if probe.startswith("poisson"):
        return gp.SAT, 1.0, 1.0, 1.0 / 8
    if probe == "gaussian_wide_onehot":
        return bp.WIDE_UNIT, None, bp.WIDE_UNIT, bp.WIDE_UNIT
    s2 = sigma * sigma
    return 1.0 / 8, 1.0 / (128 * s2), 1.0 / (8 * s2), 1.0 / (16 * s2)


@pytest.mark.parametrize("probe", sorted(bp.EXACT_PROBES))
@pytest.mark.parametrize("K", bp.BATCHED_K)
def test_exact_probe_premises(K, probe):
    link, build, ref, sigma, logp_exact = bp.EXACT_PROBES[probe]
    z_unit, term_unit, resid_unit, gx_unit = _units(probe, sigma)
    for n in bp.all_rows(K):
        if not bp.probe_applies(probe, n, K):
            continue
        p = build(n, K)
        X, y, theta, offset = p["X"], p["y"], p["theta"], p.get("offset")
        what = f"{probe} K={K} n={n}"
        assert theta.shape == (K, bp.BCH)
        # operands: X bf16-exact; y, offset f32-exact; theta exact as three pieces
        assert ep.is_bf16_exact(X), what
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y), what
        if offset is not None:
            assert np.array_equal(offset.astype(np.float32).astype(np.float64), offset), what
        np.testing.assert_array_equal(_pieces_sum64(theta), theta, err_msg=what)
        if probe != "poisson_zero_beta":
            cols = {tuple(theta[:, b]) for b in range(bp.BCH)}
            assert len(cols) == bp.BCH, f"{what}: chains must be pairwise different"
        # z: every product and every partial sum a whole number of units
        _whole_units(np.abs(X) @ np.abs(theta) + (np.abs(offset)[:, None] if offset is not None
                                                  else 0.0), z_unit, what + " z")
        Z = bp._z(X, theta, offset)
        if link == "poisson":
            assert np.all((Z <= -gp.SAT) | (Z == 0.0)), what
            mu = (Z == 0.0).astype(np.float64)
            term, resid = y[:, None] * Z - mu, y[:, None] - mu
        else:
            r = y[:, None] - Z
            _whole_units(r, z_unit, what + " r")
            term, resid = -(r * r) / (2 * sigma * sigma), r / (sigma * sigma)
        if term_unit is not None:
            _whole_units(term, term_unit, what + " term")
            if link == "gaussian":
                _whole_units(r * r, 1.0 / 64, what + " r*r")
        _whole_units(resid, resid_unit, what + " resid")
        # the residual reaches phase B unrounded as three pieces
        np.testing.assert_array_equal(_pieces_sum64(resid), resid, err_msg=what)
        # gradient: sum |x * resid| bounds every partial sum in any order
        _whole_units(np.abs(X).T @ np.abs(resid), gx_unit, what + " G partial sums")
        # and the reference is what the fp64 formula gives on these numbers
        logp_ref, G_ref = bp.exact_reference(probe, n, K)
        assert logp_ref.shape == (bp.BCH,) and G_ref.shape == (K, bp.BCH)
        np.testing.assert_array_equal(G_ref, X.T @ resid, err_msg=what)
        if logp_exact:
            np.testing.assert_array_equal(
                logp_ref, np.sum(term, axis=0) + bp.PROBE_CONST, err_msg=what)
            # fp64 holds the integer sums exactly although they pass 2^24
            assert np.max(np.abs(np.sum(np.abs(term), axis=0))) < 2.0 ** 52 * term_unit


@pytest.mark.parametrize("probe", ["poisson_dense", "poisson_onehot", "poisson_zero_beta"])
@pytest.mark.parametrize("K", bp.BATCHED_K)
def test_closed_forms_agree_with_the_general_formula(K, probe):
    _, build, _, _, _ = bp.EXACT_PROBES[probe]
    for n in (1, bp.tile_rows(K) + 1, bp.stale_big_rows(K)):
        p = build(n, K)
        logp_ref, G_ref = bp.exact_reference(probe, n, K)
        logp, G = bp.poisson_reference(p["X"], p["y"], p["theta"], p.get("offset"),
                                       bp.PROBE_CONST)
        # each z <= -128 row keeps exp(-128) in the general formula; z = 0 rows agree
        slack = n * gp.EXP_SAT
        np.testing.assert_allclose(logp, logp_ref, rtol=1e-15, atol=slack)
        np.testing.assert_allclose(
            G, G_ref, rtol=0, atol=float(np.max(np.abs(p["X"]))) * slack + 1e-300)


def test_poisson_probe_logp_passes_two_to_the_24():
    """Why a per-thread fp32 logp accumulator would not do."""
    K = 64
    logp, _ = bp.exact_reference("poisson_dense", bp.stale_big_rows(K), K)
    assert np.max(np.abs(logp)) > TWO24


# ---------------------------------------------------------------------------
# models on the CPU: logp_grad_batched is the eager path
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 16, 17])
@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_cpu_models_batched_is_eager(family, B):
    n, K = 77, 20
    if family == "poisson":
        p = gp.poisson_zero_beta_probe(n, K)
        m = PoissonGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]),
                            offset=torch.tensor(p["offset"]), dtype=torch.bfloat16)
    else:
        p = gp.gaussian_sparse_probe(n, K, 2.0)
        m = GaussianGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), 2.0,
                             dtype=torch.bfloat16)
    assert not m._batched_kernel_path()
    theta = torch.tensor(np.random.RandomState(B).randint(-4, 5, size=(K, B)) / 8.0)
    logp, G = m.logp_grad_batched(theta)
    logp_e, G_e = m._logp_grad_batched_eager(theta)
    assert logp.shape == (B,) and G.shape == (K, B)
    assert torch.equal(logp, logp_e) and torch.equal(G, G_e)
    with pytest.raises(ValueError, match="theta must be"):
        m.logp_grad_batched(torch.zeros(K + 1, B))
