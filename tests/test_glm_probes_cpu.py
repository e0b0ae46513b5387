"""Premise checks for tests/glm_probes.py (no GPU needed).

test_gpu_glm_family.py holds the family kernel to fp64 references
bit-tight.  That is only fair if, for every probe and every shape it uses,
the answer does not depend on accumulation order or on fp32-vs-fp64.  Here
the kernel's arithmetic is replayed in numpy fp32 -- sequential
accumulation over columns and over rows, forward and permuted -- and must
equal the fp64 reference bit for bit.  The logistic link reuses the checks
of test_exact_probes_cpu.py at the family kernel's shapes.

The accuracy bound's premise is checked too: the eager fp32 path meets
``EAGER_M`` on every accuracy case (``-s`` prints the ratios EAGER_M was
read from).
"""
import numpy as np
import pytest
import torch

import exact_probes as ep
import glm_probes as gp
import test_exact_probes_cpu as logistic_premises

F32 = np.float32
DTYPES = sorted(gp.VEC)


def _shape_params():
    for dtype in DTYPES:
        for K, R in gp.family_shapes(dtype):
            yield pytest.param(dtype, K, R, id=f"{dtype}-K{K}")


def _all_rows(R):
    return gp.family_rows(R) + (gp.deep_rows(R), gp.stale_big_rows(R))


def _f32_z(X, beta, offset, col_order):
    X32, b32 = X.astype(F32), beta.astype(F32)
    z = np.zeros(X.shape[0], dtype=F32)
    for k in col_order:
        z += X32[:, k] * b32[k]
    if offset is not None:
        z = offset.astype(F32) + z
    assert z.dtype == F32
    return z


def _f32_terms(link, y, z, sigma):
    y32 = y.astype(F32)
    if link == "poisson":
        with np.errstate(under="ignore"):
            mu = np.exp(z)
        term, resid = y32 * z - mu, y32 - mu
    else:
        r = y32 - z
        term = -(r * r) * F32(0.5 / (sigma * sigma))
        resid = r * F32(1.0 / (sigma * sigma))
    assert term.dtype == resid.dtype == F32
    return term, resid


def _f32_sum(v, order):
    acc = F32(0)
    for r in order:
        acc = F32(acc + v[r])
    return acc


def _f32_xt_r(X, resid, order):
    X32 = X.astype(F32)
    acc = np.zeros(X.shape[1], dtype=F32)
    for r in order:
        acc += X32[r] * resid[r]
    return acc


@pytest.mark.parametrize("probe", sorted(gp.EXACT_PROBES))
@pytest.mark.parametrize("dtype,K,R", list(_shape_params()))
def test_family_probe_is_order_independent(probe, dtype, K, R):
    link, build, _, sigma = gp.EXACT_PROBES[probe]
    for n in _all_rows(R):
        p = build(n, K)
        X, y, beta, offset = p["X"], p["y"], p["beta"], p.get("offset")
        # operands are exact in the storage formats: X in bf16 (hence f32),
        # y / offset / beta in f32
        assert ep.is_bf16_exact(X)
        for a in (y, beta) + (() if offset is None else (offset,)):
            assert np.array_equal(a.astype(F32).astype(np.float64), a)
        logp_ref, G_ref = gp.exact_reference(probe, n, K)

        cols_f, cols_p = np.arange(K), np.random.RandomState(1).permutation(K)
        rows_f, rows_p = np.arange(n), np.random.RandomState(2).permutation(n)
        z_f = _f32_z(X, beta, offset, cols_f)
        z_p = _f32_z(X, beta, offset, cols_p)
        assert np.array_equal(z_f, z_p)
        z64 = X @ beta + (0.0 if offset is None else offset)
        assert np.array_equal(z_f.astype(np.float64), z64)

        term, resid = _f32_terms(link, y, z_f, sigma)
        lp = [float(_f32_sum(term, o)) for o in (rows_f, rows_p)]
        assert lp[0] == lp[1] == logp_ref - gp.PROBE_CONST
        # ... and the constant is added without rounding
        assert (lp[0] + gp.PROBE_CONST) - gp.PROBE_CONST == lp[0]
        G = [_f32_xt_r(X, resid, o) for o in (rows_f, rows_p)]
        assert np.array_equal(G[0], G[1])
        assert np.array_equal(G[0].astype(np.float64), G_ref)

        # the general formula in fp64 differs from the closed form only by
        # the exp(-128) remainders
        if link == "poisson":
            logp_gen, G_gen = gp.poisson_reference(X, y, beta, offset, gp.PROBE_CONST)
            assert abs(logp_gen - logp_ref) <= n * gp.EXP_SAT
            assert np.max(np.abs(G_gen - G_ref)) <= 2 * n * gp.EXP_SAT
            assert np.float32(gp.EXP_SAT) == 0 and gp.EXP_SAT < 2.0 ** -149


@pytest.mark.parametrize("probe", sorted(ep.LOGISTIC_PROBES))
@pytest.mark.parametrize("dtype,K,R", list(_shape_params()))
def test_logistic_link_probe_is_order_independent(probe, dtype, K, R):
    """exact_probes.py's probes, chain 0, at the family kernel's shapes."""
    for n in _all_rows(R):
        logistic_premises._check_logistic_probe(probe, n, K, 1, bf16=(dtype == "bfloat16"))
        assert np.array_equal(
            ep.LOGISTIC_PROBES[probe](n, K)["y"].astype(F32).astype(np.float64),
            ep.LOGISTIC_PROBES[probe](n, K)["y"],
        )


def test_shapes_cover_every_instantiation():
    bf16_K = [K for K, _ in gp.family_shapes("bfloat16")]
    assert bf16_K == [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    assert [K for K, _ in gp.family_shapes("float32")] == [4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert gp.family_rows(64) == (1, 63, 64, 65, 129, 511, 513)
    assert gp.family_rows(1) == (1, 2, 3, 7, 9)
    # the largest case is 2113 x 8
    assert max(n for dt in DTYPES for _, n in gp.all_sizes(dt)) == 2113
    assert gp.deep_rows(64) == 2113 and gp.family_shapes("bfloat16")[0] == (8, 64)
    # 33R+1 rows at FED_GLM_GRID=2: 34 steps over 8 waves x 2 steps a trip
    for R in (1, 2, 64):
        steps = -(-gp.deep_rows(R) // R)
        assert steps == 34 and steps > 2 * gp.DEEP_GRID * 4 * 2


# ---------------------------------------------------------------------------
# accuracy sets
# ---------------------------------------------------------------------------

ACC_CASES = [
    pytest.param(family, dtype, K, id=f"{family}-{dtype}-K{K}")
    for family in ("poisson", "gaussian") for dtype in DTYPES for K in gp.ACC_K
]


@pytest.mark.parametrize("family,dtype,K", ACC_CASES)
def test_accuracy_case_premises(family, dtype, K):
    c = gp.accuracy_case(family, dtype, K)
    assert c["X"].shape == (gp.ACC_N, K)
    assert np.max(np.abs(c["z"])) <= gp.ACC_ZMAX
    for name in ("y", "beta") + (("offset",) if family == "poisson" else ()):
        assert np.array_equal(c[name].astype(F32).astype(np.float64), c[name])
    if dtype == "bfloat16":
        assert ep.is_bf16_exact(c["X"])
    else:
        assert np.array_equal(c["X"].astype(F32).astype(np.float64), c["X"])
    assert c["logp_scale"] > 0 and np.all(c["G_scale"] > 0)


@pytest.mark.parametrize("family,dtype,K", ACC_CASES)
def test_eager_meets_unscaled_bound(family, dtype, K):
    c = gp.accuracy_case(family, dtype, K)
    m = gp.accuracy_model(family, dtype, K, use_kernels=False)
    assert m._acc_dtype == torch.float32
    default_threads = torch.get_num_threads()
    try:
        for threads in (1, default_threads):
            torch.set_num_threads(threads)
            logp, (g,) = m.logp_grad(torch.tensor(c["beta"]))
            r_logp, r_grad = gp.accuracy_ratios(c, float(logp), g.numpy())
            print(f"\n{family} {dtype} K={K} threads={threads}: "
                  f"logp ratio {r_logp:.4f}, worst grad ratio {r_grad:.4f}")
            assert r_logp <= gp.EAGER_M
            assert r_grad <= gp.EAGER_M
    finally:
        torch.set_num_threads(default_threads)
    assert gp.KERNEL_M == 4 * gp.EAGER_M
