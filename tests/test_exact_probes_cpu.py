"""Premise checks for tests/exact_probes.py (no GPU needed).

The GPU tests hold the HIP kernels to an fp64 numpy reference bit-tight.
That is only fair if, for every probe and every shape those tests use, the
answer does not depend on accumulation order or on fp32-vs-fp64.  Here the
kernels' arithmetic is replayed in numpy fp32 -- sequential accumulation in
forward and in a permuted order, with the bf16 rounding of the residual
where the batched kernels do it -- and must agree with the fp64 reference
bit for bit.  The only inexact terms, the saturation remainders
sigmoid(-32) and log1p(exp(-32)), are split off and bounded by N * 2^-46.

A probe/shape pair that fails here gets changed, not given a tolerance.
"""
import numpy as np
import pytest

import exact_probes as ep

F32 = np.float32


def _f32_forward(X, y, theta, col_order, bf16_resid):
    """z, per-row logp term and residual the way the kernels form them:
    fp32 products, fp32 sequential accumulation over columns."""
    X32, y32, th32 = X.astype(F32), y.astype(F32), theta.astype(F32)
    z = np.zeros((X.shape[0], theta.shape[1]), dtype=F32)
    for k in col_order:
        z += X32[:, k, None] * th32[k][None, :]
    with np.errstate(over="ignore"):
        sp = np.maximum(z, F32(0)) + np.log1p(np.exp(-np.abs(z)))
        resid = y32[:, None] - F32(1) / (F32(1) + np.exp(-z))
    term = y32[:, None] * z - sp
    assert z.dtype == term.dtype == resid.dtype == F32
    if bf16_resid:
        resid = ep.round_to_bf16(resid)
    return z, term, resid


def _f32_rowsum(term, row_order):
    acc = np.zeros(term.shape[1], dtype=F32)
    for r in row_order:
        acc += term[r]
    return acc


def _f32_xt_r(X, R, row_order):
    X32 = X.astype(F32)
    acc = np.zeros((X.shape[1], R.shape[1]), dtype=F32)
    for r in row_order:
        acc += X32[r][:, None] * R[r][None, :]
    return acc


def _orders(n, seed):
    fwd = np.arange(n)
    return fwd, np.random.RandomState(seed).permutation(n)


def _check_logistic_probe(probe, n, K, chains, bf16):
    p = ep.LOGISTIC_PROBES[probe](n, K)
    X, y, theta = p["X"], p["y"], p["theta"][:, :chains]
    # operands are exact in the storage formats (theta always goes through
    # bf16 in the batched kernel, through fp32 in the single-chain one)
    for a in (X, y) + ((theta,) if bf16 else ()):
        assert ep.is_bf16_exact(a)
    assert np.array_equal(theta.astype(F32).astype(np.float64), theta)

    logp_ref, G_ref = ep.logistic_reference(X, y, theta)
    cols_f, cols_p = _orders(K, 1)
    rows_f, rows_p = _orders(n, 2)
    z_f, term_f, res_f = _f32_forward(X, y, theta, cols_f, bf16)
    z_p, term_p, res_p = _f32_forward(X, y, theta, cols_p, bf16)
    # z itself: order-independent and equal to the fp64 product
    assert np.array_equal(z_f, z_p)
    assert np.array_equal(z_f.astype(np.float64), X @ theta)

    if probe == "zero_theta":
        assert not z_f.any()
        # resid = y - 1/2 exactly; G exact in fp32 in any order
        assert np.array_equal(res_f.astype(np.float64), (y - 0.5)[:, None] + 0 * z_f)
        G_f = _f32_xt_r(X, res_f, rows_f)
        G_p = _f32_xt_r(X, res_p, rows_p)
        assert np.array_equal(G_f, G_p)
        assert np.array_equal(G_f.astype(np.float64), G_ref)
        # logp = -N ln 2: every term is the fp32 rounding of ln 2; the
        # kernels sum at most a few dozen of them in fp32 before going to
        # fp64, replayed here as 32-term fp32 spans
        assert np.all(term_f == term_f[0, 0])
        spans = [
            _f32_rowsum(term_f[s : s + 32], range(min(32, n - s))).astype(np.float64)
            for s in range(0, n, 32)
        ]
        np.testing.assert_allclose(np.sum(spans, axis=0), logp_ref, rtol=1e-6)
        # (the reference's own fp64 summation error is ~1e-13 at these N)
        np.testing.assert_allclose(logp_ref, -n * np.log(2.0), rtol=1e-12)
        return

    # saturated probes: split the exact part from the <= 2^-46 remainders
    logp_sat, G_sat = ep.logistic_saturated(X, y, theta)
    for term, res in ((term_f, res_f), (term_p, res_p)):
        term_main = np.rint(term)
        res_main = np.rint(res)
        assert np.max(np.abs(term - term_main)) <= ep.TINY
        assert np.max(np.abs(res - res_main)) <= ep.TINY
        assert set(np.unique(res_main)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(np.rint(term_f), np.rint(term_p))
    assert np.array_equal(np.rint(res_f), np.rint(res_p))
    term_main = np.rint(term_f).astype(F32)
    res_main = np.rint(res_f).astype(F32)
    # every partial sum stays an exact fp32 integer in ANY order: the sum
    # of magnitudes, over its common power-of-two factor, is below 2^24
    assert np.all(np.abs(term_main).sum(axis=0, dtype=np.float64) / ep.SAT < 2 ** 24)
    assert np.all(np.abs(z_f) / ep.SAT < 2 ** 24)
    assert (np.abs(X).T @ np.abs(res_main.astype(np.float64))).max() < 2 ** 24
    # the remainders must not depend on the accumulate's rounding mode (the
    # matrix cores do not round to nearest): none may land in a G entry
    # whose exact part is non-zero
    res_rem = np.abs(res_f.astype(np.float64) - res_main)
    hit_rem = (np.abs(X).T @ res_rem) > 0
    hit_main = (np.abs(X).T @ np.abs(res_main.astype(np.float64))) > 0
    assert not np.any(hit_rem & hit_main)
    if probe == "dense_int":
        assert not res_rem.any()
    lp_f = _f32_rowsum(term_main, rows_f)
    lp_p = _f32_rowsum(term_main, rows_p)
    assert np.array_equal(lp_f, lp_p)
    assert np.array_equal(lp_f.astype(np.float64), logp_sat)
    G_f = _f32_xt_r(X, res_main, rows_f)
    G_p = _f32_xt_r(X, res_main, rows_p)
    assert np.array_equal(G_f, G_p)
    assert np.array_equal(G_f.astype(np.float64), G_sat)
    # the fp64 reference is the exact part plus at most N remainders of
    # 2^-46 each, plus its own rounding once remainders make the sum
    # inexact (pairwise summation: ~log2 N roundings of the running sum);
    # together they stay well inside the GPU tests' atol = N * 2^-40
    for ref, sat in ((logp_ref, logp_sat), (G_ref, G_sat)):
        diff = np.max(np.abs(ref - sat))
        rounding = (np.log2(n) + 2) * np.spacing(max(np.max(np.abs(sat)), 1.0))
        assert diff <= n * ep.TINY + rounding
        assert 2 * diff < ep.saturation_atol(n)
    assert 2 * n * ep.TINY < ep.saturation_atol(n) < 0.25


@pytest.mark.parametrize("n", ep.BATCHED_N + ep.BATCHED_DEEP_N + (ep.STALE_BIG_N,))
@pytest.mark.parametrize("K", ep.BATCHED_K)
@pytest.mark.parametrize("probe", sorted(ep.LOGISTIC_PROBES))
def test_batched_probe_is_order_independent(probe, K, n):
    _check_logistic_probe(probe, n, K, ep.BCH, bf16=True)


@pytest.mark.parametrize("n", ep.SINGLE_N)
@pytest.mark.parametrize("dtype,K", ep.SINGLE_COMBOS)
@pytest.mark.parametrize("probe", ["onehot", "zero_theta"])
def test_single_chain_probe_is_order_independent(probe, dtype, K, n):
    # the single-chain kernel keeps the residual in fp32 (no bf16 rounding)
    _check_logistic_probe(probe, n, K, 1, bf16=(dtype == "bfloat16"))
    ref = ep.single_reference(probe, n, K)
    p = ep.LOGISTIC_PROBES[probe](n, K)
    logp, G = ep.logistic_reference(p["X"], p["y"], p["theta"][:, :1])
    assert np.array_equal(ref["logp"], logp) and np.array_equal(ref["G"], G[:, 0])


def test_onehot_probe_names_rows():
    """Below K rows every row owns its own column, and a row's 16 residuals
    spell out y and the theta sign pattern of that column."""
    n, K = 97, 512
    p = ep.onehot_probe(n, K)
    assert len(set(p["cols"])) == n
    _, G = ep.logistic_saturated(p["X"], p["y"], p["theta"])
    for r in range(n):
        expect = p["y"][r] - (p["theta"][p["cols"][r]] > 0)
        assert np.array_equal(G[p["cols"][r]], expect)
    untouched = np.setdiff1d(np.arange(K), p["cols"])
    assert not G[untouched].any()


@pytest.mark.parametrize("dtype", sorted(ep.GAUSS_VEC))
def test_gaussian_probe_is_exact(dtype):
    for n in ep.gaussian_sizes(dtype):
        p = ep.gaussian_probe(n)
        x, y = p["x"], p["y"]
        assert ep.is_bf16_exact(x) and ep.is_bf16_exact(y)
        assert np.max(np.abs(x)) <= 4 and np.max(np.abs(y)) <= 4
        perm = np.random.RandomState(n).permutation(n)
        for a, b in ep.GAUSS_THETAS:
            r = y - (a + b * x)
            # r, r*x, r^2 are multiples of 2^-5, 2^-8, 2^-10 and need <= 24
            # bits, so the fp32 products the kernel forms are exact
            for v, unit in ((r, 2.0 ** -5), (r * x, 2.0 ** -8), (r * r, 2.0 ** -10)):
                assert np.array_equal(np.rint(v / unit) * unit, v)
                assert np.max(np.abs(v)) / unit < 2 ** 24
                assert np.array_equal(v.astype(F32).astype(np.float64), v)
            r32 = r.astype(F32)
            assert np.array_equal((r32 * x.astype(F32)).astype(np.float64), r * x)
            assert np.array_equal((r32 * r32).astype(np.float64), r * r)
            # kernel scheme: short fp32 spans per lane (at most 2 vector
            # loads + 1 tail element at these sizes; 64 is generous), fp64
            # across lanes -- replayed forward and permuted
            for v in (r * x, r * r):
                totals = []
                for order in (np.arange(n), perm):
                    v32 = v.astype(F32)[order]
                    spans = [
                        np.cumsum(v32[s : s + 64], dtype=F32)[-1] for s in range(0, n, 64)
                    ]
                    totals.append(float(np.sum(np.asarray(spans, dtype=np.float64))))
                assert totals[0] == totals[1] == float(np.sum(v))
            # fp64 sums are exact in any order
            for v, unit in ((r, 2.0 ** -5), (r * x, 2.0 ** -8), (r * r, 2.0 ** -10)):
                assert np.sum(np.abs(v)) / unit < 2 ** 53
                assert float(np.sum(v)) == float(np.sum(v[perm])) == float(np.cumsum(v)[-1])
            logp, ga, gb = ep.gaussian_reference(x, y, a, b)
            assert ga == float(np.sum(r)) and gb == float(np.sum(r * x))


def test_bf16_rounding_helper():
    v = np.array([1.0, -0.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -1.2660e-14], dtype=F32)
    out = ep.round_to_bf16(v)
    assert out[0] == 1.0 and out[1] == -0.5
    assert out[2] == 1.0                      # tie -> even
    assert out[3] == F32(1.0 + 2.0 ** -7)     # above the tie -> up
    assert abs(out[4] - v[4]) <= abs(v[4]) * 2.0 ** -8
    assert ep.is_bf16_exact(out) and not ep.is_bf16_exact(v[2:3])
