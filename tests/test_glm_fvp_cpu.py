"""CPU tests of the GLM Fisher-vector product: the premises of the exact
probes (tests/glm_fvp_probes.py), the eager ``fisher_vector_product`` and
``fisher_diagonal`` of the three GLM models, Newton-CG MAP
(``find_map_newton_cg``) and the served product function.  No GPU; the kernel
itself is tested in test_gpu_glm_fvp.py.
"""
import numpy as np
import pytest
import torch

import glm_fisher_probes as fp
import glm_fvp_probes as vp
import glm_probes as gp

from pytensor_federated_amd.inference import (
    NewtonCGResult,
    find_map_newton,
    find_map_newton_cg,
)
from pytensor_federated_amd.models import (
    GaussianGLMModel,
    LogisticGLMModel,
    PoissonGLMModel,
    generate_gaussian_glm_dataset,
    generate_logistic_dataset,
    generate_poisson_dataset,
)
from pytensor_federated_amd.ops import (
    glm_family_fisher_diagonal,
    glm_family_fisher_vector,
)


# ---------------------------------------------------------------------------
# probe premises
# ---------------------------------------------------------------------------

def test_probe_set():
    assert set(vp.EXACT_PROBES) == set(fp.EXACT_PROBES) | {"logistic_zero_beta", "logistic_gate"}
    for K in (4, 8, 2048):
        v = vp.probe_vector(K)
        assert v.shape == (K,) and np.max(np.abs(v)) <= 1.0
        assert np.array_equal(np.round(v * 4), v * 4)
    assert not np.array_equal(vp.probe_vector(8), vp.probe_vector(16)[:8])


def test_logistic_weight_is_exact_at_the_probe_points():
    """mu as the link forms it, 1 / (1 + exp(-z)) in f32: 1/2 at z = 0; at
    z <= -128 exp(128) overflows to inf and mu is exactly 0."""
    z = torch.tensor([0.0, -gp.SAT, -6 * gp.SAT], dtype=torch.float32)
    mu = 1.0 / (1.0 + torch.exp(-z))
    assert mu.tolist() == [0.5, 0.0, 0.0]
    assert (mu * (1.0 - mu)).tolist() == [0.25, 0.0, 0.0]
    mu = torch.sigmoid(z)
    assert (mu * (1.0 - mu)).tolist() == [0.25, 0.0, 0.0]


_WORST = {"xv": 0.0, "wux": 0.0, "wxx": 0.0}


@pytest.mark.parametrize("probe", vp.PROBES)
@pytest.mark.parametrize("dtype_name", vp.DTYPES)
def test_probe_sums_are_exact_in_f32(dtype_name, probe):
    """Every operand survives the storage type, every term is a whole number
    of its unit and the sums of the magnitudes stay below 2^24 units: any f32
    summation order is exact.  The weight is the link's on the probe's z."""
    link = vp.EXACT_PROBES[probe][0]
    for K, n in gp.all_sizes(dtype_name):
        p = vp.EXACT_PROBES[probe][1](n, K)
        X, w, v = p["X"], p["w"], vp.probe_vector(K)
        assert X.shape == (n, K) and w.shape == (n,)
        assert np.array_equal(gp._round_bf16(X), X)
        z = X @ p["beta"] + (p["offset"] if p.get("offset") is not None else 0.0)
        if link == "poisson":
            assert np.array_equal(w, (z == 0.0).astype(float))
        elif link == "logistic":
            assert np.all((z == 0.0) | (z <= -gp.SAT))
            assert np.array_equal(w, (z == 0.0) / 4.0)
        A = np.abs(X)
        xv = np.max(A @ np.abs(v)) * 32
        u = X @ v
        assert np.array_equal(np.round(u * 32), u * 32)
        wux = np.max(A.T @ (w * np.abs(u))) * 1024
        wxx = np.max((A * A).T @ w) * 1024
        for t in (w[:, None] * u[:, None] * X, w[:, None] * X * X):
            assert np.array_equal(np.round(t * 1024), t * 1024)
        assert max(xv, wux, wxx) < 2.0 ** 24, (probe, K, n, xv, wux, wxx)
        Hv, d = vp.exact_reference(probe, n, K)
        assert np.array_equal(gp._round_f32(Hv), Hv) and np.array_equal(gp._round_f32(d), d)
        for key, val in (("xv", xv), ("wux", wux), ("wxx", wxx)):
            _WORST[key] = max(_WORST[key], val)
    print(f"\n{probe} {dtype_name}: worst so far {_WORST}")


# ---------------------------------------------------------------------------
# eager accuracy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [1, None])
def test_eager_meets_the_fvp_bound(threads):
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        worst = 0.0
        for family, dtype_name, K in vp.ACCURACY_CASES:
            c, _ = vp.accuracy_data(family, dtype_name, K)
            m = vp.accuracy_model(family, dtype_name, K)
            beta = torch.tensor(c["beta"])
            Hv = m.fisher_vector_product(beta, torch.tensor(vp.accuracy_vector(K)))
            d = m.fisher_diagonal(beta)
            for r in (Hv, d):
                assert r.dtype == torch.float64 and r.shape == (K,)
            r_v, r_d = vp.fvp_ratios(family, dtype_name, K, Hv.numpy(), d.numpy())
            print(f"\n{family} {dtype_name} K={K} threads={torch.get_num_threads()}: "
                  f"eager worst ratio product {r_v:.3f} diagonal {r_d:.3f}")
            worst = max(worst, r_v, r_d)
            assert r_v <= vp.FVP_EAGER_M and r_d <= vp.FVP_EAGER_M
        print(f"\nworst eager ratio {worst:.3f} (recorded {vp.FVP_EAGER_MEASURED}, "
              f"allowed {vp.FVP_EAGER_M})")
    finally:
        torch.set_num_threads(before)


def test_bound_constants():
    assert vp.FVP_EAGER_MEASURED <= vp.FVP_EAGER_M < 2 * vp.FVP_EAGER_MEASURED
    assert np.log2(vp.FVP_EAGER_M) == round(np.log2(vp.FVP_EAGER_M))
    assert vp.FVP_KERNEL_M == 4 * vp.FVP_EAGER_M


# ---------------------------------------------------------------------------
# fp64 models: consistency with fisher_information, padding, out=, shards
# ---------------------------------------------------------------------------

def _fp64_models(n=300, K=7):
    Xp, yp, offset, bp = generate_poisson_dataset(n, K, seed=4)
    Xg, yg, bg = generate_gaussian_glm_dataset(n, K, sigma=0.7, seed=4)
    return [
        (PoissonGLMModel(Xp, yp, offset=offset), bp),
        (GaussianGLMModel(Xg, yg, 0.7), bg),
    ]


@pytest.mark.parametrize("which", [0, 1])
def test_product_and_diagonal_agree_with_fisher_information(which):
    m, beta = _fp64_models()[which]
    K = beta.shape[0]
    v = np.random.RandomState(1).standard_normal(K)
    H = m.fisher_information(torch.tensor(beta)).numpy()
    Hv = m.fisher_vector_product(torch.tensor(beta), torch.tensor(v)).numpy()
    d = m.fisher_diagonal(torch.tensor(beta)).numpy()
    np.testing.assert_allclose(Hv, H @ v, rtol=0, atol=1e-12 * np.max(np.abs(H @ v)))
    np.testing.assert_allclose(d, np.diag(H), rtol=1e-12)


def test_logistic_product_is_the_negative_hessian_times_v():
    n, K = 300, 7
    X, y, beta = generate_logistic_dataset(n, K, seed=4)
    m = LogisticGLMModel(X, y)
    v = np.random.RandomState(1).standard_normal(K)
    mu = 1.0 / (1.0 + np.exp(-(X @ beta)))
    w = mu * (1.0 - mu)
    Hv = m.fisher_vector_product(torch.tensor(beta), torch.tensor(v)).numpy()
    d = m.fisher_diagonal(torch.tensor(beta)).numpy()
    np.testing.assert_allclose(Hv, vp.fvp_reference(X, w, v), rtol=0,
                               atol=1e-12 * np.max(np.abs(Hv)))
    np.testing.assert_allclose(d, vp.diag_reference(X, w), rtol=1e-12)
    # ... and of logp: central differences of the gradient along v
    h = 1e-5
    _, (g1,) = m(beta + h * v)
    _, (g0,) = m(beta - h * v)
    np.testing.assert_allclose(Hv, -(g1 - g0) / (2 * h), rtol=0, atol=1e-6 * np.max(np.abs(Hv)))


def test_padding_shapes_out_and_errors():
    """K = 20 (padded to 32 on the kernel path, plain here), an exact probe
    on a bf16 shard."""
    n, K = 150, 20
    p = gp.gaussian_sparse_probe(n, K, 2.0)
    m = GaussianGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), 2.0, dtype=torch.bfloat16)
    beta = torch.tensor(p["beta"])
    v = vp.probe_vector(K)
    w = np.full(n, 0.25)
    Hv = m.fisher_vector_product(beta, torch.tensor(v))
    d = m.fisher_diagonal(beta)
    assert Hv.shape == (K,) and Hv.dtype == torch.float64
    assert d.shape == (K,) and d.dtype == torch.float64
    np.testing.assert_array_equal(Hv.numpy(), vp.fvp_reference(p["X"], w, v))
    np.testing.assert_array_equal(d.numpy(), vp.diag_reference(p["X"], w))
    out = torch.full((K,), -3.0, dtype=torch.float64)
    got = m.fisher_vector_product(beta, torch.tensor(v), out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.numpy(), Hv.numpy())
    got = m.fisher_diagonal(beta, out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.numpy(), d.numpy())
    with pytest.raises(ValueError, match="beta must have shape"):
        m.fisher_vector_product(torch.zeros(K + 1), torch.tensor(v))
    with pytest.raises(ValueError, match="v must have shape"):
        m.fisher_vector_product(beta, torch.zeros(K + 1))
    with pytest.raises(ValueError, match="v must have shape"):
        m.fisher_vector_product(beta, None)
    with pytest.raises(ValueError, match="beta must have shape"):
        m.fisher_diagonal(torch.zeros(K - 1))
    for bad in (torch.zeros(K, dtype=torch.float32), torch.zeros(K + 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be"):
            m.fisher_vector_product(beta, torch.tensor(v), out=bad)
        with pytest.raises(ValueError, match="out must be"):
            m.fisher_diagonal(beta, out=bad)


def test_shard_results_add_to_the_whole():
    X, y, offset, beta = generate_poisson_dataset(900, 6, seed=9)
    v = torch.tensor(np.random.RandomState(2).standard_normal(6))
    b = torch.tensor(beta)
    whole = PoissonGLMModel(X, y, offset=offset)
    parts = [PoissonGLMModel(X[s], y[s], offset=offset[s])
             for s in (slice(0, 250), slice(250, 900))]
    Hv = sum(p.fisher_vector_product(b, v) for p in parts).numpy()
    d = sum(p.fisher_diagonal(b) for p in parts).numpy()
    np.testing.assert_allclose(Hv, whole.fisher_vector_product(b, v).numpy(), rtol=1e-12,
                               atol=1e-12 * np.max(np.abs(Hv)))
    np.testing.assert_allclose(d, whole.fisher_diagonal(b).numpy(), rtol=1e-12)


def test_ops_validation_needs_no_gpu():
    X = torch.zeros((4, 16), dtype=torch.bfloat16)
    beta = v = torch.zeros(16)
    for call in (
        lambda X, beta, **kw: glm_family_fisher_vector(X, beta, torch.zeros(beta.shape), **kw),
        glm_family_fisher_diagonal,
    ):
        with pytest.raises(ValueError, match="unknown link"):
            call(X, beta, link="probit")
        with pytest.raises(TypeError, match="unsupported dtype"):
            call(X.double(), beta, link="poisson")
        with pytest.raises(ValueError, match="not compiled"):
            call(torch.zeros((4, 24), dtype=torch.bfloat16), torch.zeros(24), link="poisson")
        with pytest.raises(ValueError, match="not compiled"):
            call(torch.zeros((4, 2048), dtype=torch.float32), torch.zeros(2048), link="poisson")
        with pytest.raises(ValueError, match="sigma must be positive"):
            call(X, beta, link="gaussian", sigma=0.0)
        with pytest.raises(ValueError, match="beta must have shape"):
            glm_family_fisher_diagonal(X, torch.zeros(8), link="poisson")
        with pytest.raises(ValueError, match="offset must be f32"):
            call(X, beta, link="poisson", offset=torch.zeros(4, dtype=torch.float64))
        with pytest.raises(ValueError, match="offset must be f32"):
            call(X, beta, link="poisson", offset=torch.zeros(5))
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros((16, 4), dtype=torch.bfloat16).t(), torch.zeros(16), link="logistic")
        with pytest.raises(ValueError, match="ROCm device"):
            call(X, beta, link="logistic")
    with pytest.raises(ValueError, match="v must have shape"):
        glm_family_fisher_vector(X, beta, torch.zeros(8), link="poisson")
    with pytest.raises(ValueError, match="v must have shape"):
        glm_family_fisher_vector(X, beta, None, link="poisson")
    del v


# ---------------------------------------------------------------------------
# Newton-CG on fp64 numpy callables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("diagonals", [False, True])
@pytest.mark.parametrize("K", [8, 100])
def test_newton_cg_reaches_the_newton_mode(K, diagonals):
    c = gp.accuracy_case("poisson", "bfloat16", K)
    calls = []
    lg, H, hv, dg = vp.numpy_poisson_funcs(c["X"], c["y"], c["offset"], calls)
    ref = find_map_newton(lg, H, np.zeros(K))
    res = find_map_newton_cg(lg, hv, np.zeros(K), fisher_diagonal_funcs=dg if diagonals else None)
    assert isinstance(res, NewtonCGResult) and not hasattr(res, "cov")
    assert ref.converged and res.converged
    print(f"\nK={K} diagonals={diagonals}: {res.n_steps} outer steps, {res.n_products} products "
          f"(Newton: {ref.n_steps} steps)")
    assert np.max(np.abs(res.theta - ref.theta)) <= 1e-8
    assert res.n_products == len(calls)
    assert res.n_steps <= 12 and res.n_products <= 40
    _, (g,) = lg(res.theta)
    assert np.max(np.abs(g)) <= 1e-9 * max(1.0, abs(res.logp))
    np.testing.assert_allclose(res.logp, ref.logp, rtol=1e-12)


def test_newton_cg_gaussian_one_outer_step():
    """Orthogonal columns of equal norm: H is a multiple of the identity, CG
    is exact after one product and gtol is met after one outer step."""
    n, K, sigma = 64, 6, 0.5
    rng = np.random.RandomState(3)
    Q, _ = np.linalg.qr(rng.standard_normal((n, K)))
    X = 3.0 * Q
    y = X @ rng.standard_normal(K) + sigma * rng.standard_normal(n)
    m = GaussianGLMModel(X, y, sigma)
    for dfuncs in (None, m.as_fisher_diagonal_func()):
        res = find_map_newton_cg(m.as_logp_grad_func(), m.as_fisher_vector_func(), np.zeros(K),
                                 fisher_diagonal_funcs=dfuncs)
        assert res.converged and res.n_steps == 1 and res.n_products == 1
        np.testing.assert_allclose(res.theta, np.linalg.lstsq(X, y, rcond=None)[0], rtol=1e-10)


def test_newton_cg_gaussian_general_design():
    X, y, _ = generate_gaussian_glm_dataset(400, 6, sigma=0.5, seed=8)
    m = GaussianGLMModel(X, y, 0.5)
    res = find_map_newton_cg(m.as_logp_grad_func(), m.as_fisher_vector_func(), np.zeros(6),
                             fisher_diagonal_funcs=m.as_fisher_diagonal_func())
    assert res.converged
    np.testing.assert_allclose(res.theta, np.linalg.lstsq(X, y, rcond=None)[0], rtol=1e-8)


@pytest.mark.parametrize("matrix", [False, True])
def test_newton_cg_prior_precision_closed_form(matrix):
    sigma, tau, K = 0.5, 3.0, 6
    X, y, _ = generate_gaussian_glm_dataset(400, K, sigma=sigma, seed=8)
    m = GaussianGLMModel(X, y, sigma)
    P = tau * np.eye(K)
    if matrix:
        A = np.random.RandomState(2).standard_normal((K, K))
        P = A @ A.T + np.eye(K)
    funcs = (m.as_logp_grad_func(), m.as_fisher_vector_func())
    A_post = X.T @ X / sigma ** 2 + P
    ref = np.linalg.solve(A_post, X.T @ y / sigma ** 2)
    for dfuncs in (None, m.as_fisher_diagonal_func()):
        res = find_map_newton_cg(*funcs, np.zeros(K), prior_precision=P if matrix else tau,
                                 fisher_diagonal_funcs=dfuncs)
        assert res.converged
        np.testing.assert_allclose(res.theta, ref, rtol=1e-8)
        logp0, _ = m(ref)
        np.testing.assert_allclose(res.logp, float(logp0) - 0.5 * ref @ P @ ref, rtol=1e-12)
    with pytest.raises(ValueError, match="prior_precision"):
        find_map_newton_cg(*funcs, np.zeros(K), prior_precision=np.eye(K + 1))


def test_newton_cg_two_shards_equal_the_union():
    X, y, offset, _ = generate_poisson_dataset(2000, 8)
    whole = PoissonGLMModel(X, y, offset=offset)
    a = PoissonGLMModel(X[:700], y[:700], offset=offset[:700])
    b = PoissonGLMModel(X[700:], y[700:], offset=offset[700:])

    def run(models):
        return find_map_newton_cg(
            [m.as_logp_grad_func() for m in models],
            [m.as_fisher_vector_func() for m in models],
            np.zeros(8),
            fisher_diagonal_funcs=[m.as_fisher_diagonal_func() for m in models],
        )

    one, two = run([whole]), run([a, b])
    assert two.converged and (two.n_steps, two.n_products) == (one.n_steps, one.n_products)
    np.testing.assert_allclose(two.theta, one.theta, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(two.logp, one.logp, rtol=1e-12)
    with pytest.raises(ValueError, match="per shard"):
        find_map_newton_cg([a.as_logp_grad_func()], [], np.zeros(8))
    with pytest.raises(ValueError, match="per shard"):
        find_map_newton_cg(a.as_logp_grad_func(), a.as_fisher_vector_func(), np.zeros(8),
                           fisher_diagonal_funcs=[])
    with pytest.raises(ValueError, match="vector"):
        find_map_newton_cg(a.as_logp_grad_func(), a.as_fisher_vector_func(), np.zeros((8, 1)))


def test_newton_cg_step_halving_rescues_a_poor_start():
    """From an intercept of -12 the weights are ~e^-12, the full step
    overflows the Poisson link and has to be halved."""
    X, y, offset, _ = generate_poisson_dataset(2000, 8)
    m = PoissonGLMModel(X, y, offset=offset)
    good = find_map_newton(m.as_logp_grad_func(), m.as_fisher_func(), np.zeros(8))
    lg_calls, hv_calls = [], []

    def counted(b):
        lg_calls.append(1)
        return m(b)

    def counted_product(b, v):
        hv_calls.append(1)
        return m.as_fisher_vector_func()(b, v)

    poor = find_map_newton_cg(counted, counted_product, -12.0 * np.eye(8)[0], max_steps=80)
    assert poor.converged
    np.testing.assert_allclose(poor.theta, good.theta, rtol=1e-8, atol=1e-8)
    # more logp evaluations than steps: at least one step was halved
    assert len(lg_calls) > poor.n_steps + 1
    assert poor.n_products == len(hv_calls)


def test_newton_cg_max_cg_bounds_the_products_of_a_step():
    c = gp.accuracy_case("poisson", "bfloat16", 8)
    lg, _, hv, _ = vp.numpy_poisson_funcs(c["X"], c["y"], c["offset"])
    res = find_map_newton_cg(lg, hv, np.zeros(8), max_cg=1, max_steps=3)
    assert res.n_steps == 3 and res.n_products == 3 and not res.converged
    with pytest.raises(ValueError, match="max_cg"):
        find_map_newton_cg(lg, hv, np.zeros(8), max_cg=0)


# ---------------------------------------------------------------------------
# service
# ---------------------------------------------------------------------------

def test_fisher_vector_func_through_the_service_unit():
    """In process: the service runs the product function on a wire message
    of two arrays (read-only views) and returns the local result."""
    from pytensor_federated_amd.npproto.utils import ndarray_from_numpy, ndarray_to_numpy
    from pytensor_federated_amd.rpc import InputArrays
    from pytensor_federated_amd.service import ArraysToArraysService, _run_compute_func

    X, y, offset, beta = generate_poisson_dataset(200, 8, seed=6)
    model = PoissonGLMModel(X, y, offset=offset)
    v = np.random.RandomState(7).standard_normal(8)
    ArraysToArraysService(model.as_fisher_vector_func())
    out = _run_compute_func(
        InputArrays(items=[ndarray_from_numpy(beta), ndarray_from_numpy(v)], uuid="hv"),
        model.as_fisher_vector_func(),
    )
    assert out.uuid == "hv" and len(out.items) == 1
    Hv = ndarray_to_numpy(out.items[0])
    assert Hv.shape == (8,) and Hv.dtype == np.float64
    np.testing.assert_array_equal(
        Hv, model.fisher_vector_product(torch.tensor(beta), torch.tensor(v)).numpy()
    )
    out = _run_compute_func(InputArrays(items=[ndarray_from_numpy(beta)], uuid="d"),
                            model.as_fisher_diagonal_func())
    np.testing.assert_array_equal(ndarray_to_numpy(out.items[0]),
                                  model.fisher_diagonal(torch.tensor(beta)).numpy())
