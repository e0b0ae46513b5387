"""CPU tests of the GLM Fisher information: the premises of the exact probes
(tests/glm_fisher_probes.py), the eager ``fisher_information`` of the
Poisson / Gaussian GLM models, Newton MAP (``find_map_newton``) and the
served Fisher function.  No GPU; the kernel itself is tested in
test_gpu_glm_fisher.py.
"""
import multiprocessing
import socket
import time

import numpy as np
import pytest
import torch

import glm_fisher_probes as fp
import glm_probes as gp

from pytensor_federated_amd.inference import NUTS, find_map_newton, laplace_mass
from pytensor_federated_amd.models import (
    GaussianGLMModel,
    PoissonGLMModel,
    generate_gaussian_glm_dataset,
    generate_poisson_dataset,
)
from pytensor_federated_amd.ops import (
    GLM_FAMILY_FISHER_K,
    glm_family_fisher,
    glm_family_fisher_supports,
)

FISHER_PORT = 9691
PREMISE_ROWS = (1, 31, 257, 500)


# ---------------------------------------------------------------------------
# probe premises
# ---------------------------------------------------------------------------

def test_sizes_match_the_ops_module():
    assert tuple(GLM_FAMILY_FISHER_K) == fp.FISHER_K
    assert glm_family_fisher_supports(torch.bfloat16, 128)
    assert not glm_family_fisher_supports(torch.float32, 128)
    assert not glm_family_fisher_supports(torch.bfloat16, 2048)
    assert not glm_family_fisher_supports(torch.bfloat16, 24)


def test_exp_of_minus_128_flushes_in_fp32():
    assert float(torch.exp(torch.tensor(-gp.SAT, dtype=torch.float32))) == 0.0
    assert float(torch.exp(torch.tensor(0.0, dtype=torch.float32))) == 1.0


@pytest.mark.parametrize("probe", sorted(fp.EXACT_PROBES))
@pytest.mark.parametrize("K", fp.FISHER_K)
def test_probe_operands_and_reference_are_exact(probe, K):
    """X and w*x survive bf16 (so the second and third piece are zero), and
    H_ref survives f32; the largest row count of the GPU tests bounds the
    partial sums (every term has one sign pattern at most |x_i| w |x_j|, so
    H_scale bounds every partial sum of every order)."""
    for n in PREMISE_ROWS + (fp.stale_big_rows(K),):
        p = fp.EXACT_PROBES[probe][1](n, K)
        X, w = p["X"], p["w"]
        assert np.array_equal(gp._round_bf16(X), X)
        wx = w[:, None] * X
        assert np.array_equal(gp._round_bf16(wx), wx)
        H = fp.exact_reference(probe, n, K)
        assert np.array_equal(gp._round_f32(H), H)
        # every term is a multiple of 2^-6; f32 adds them exactly below 2^24 units
        terms_unit = 2.0 ** -6
        assert np.array_equal(np.round(wx / 2.0 ** -3), wx / 2.0 ** -3)
        assert np.max(fp.fisher_scale(X, w)) / terms_unit < 2.0 ** 24


@pytest.mark.parametrize("K", fp.FISHER_K)
def test_gate_probe_share(K):
    """Between 1/8 and 7/8 of the rows have w = 1, so the gate matters."""
    for n in fp.GATE_SHARE_ROWS:
        p = fp.poisson_gate_probe(n, K)
        z = p["X"] @ p["beta"]
        assert np.all((z == 0.0) | (z <= -gp.SAT))
        share = float(np.mean(p["w"]))
        assert 1 / 8 <= share <= 7 / 8, (n, K, share)


# ---------------------------------------------------------------------------
# eager accuracy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [1, None])
def test_eager_meets_the_fisher_bound(threads):
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        worst = 0.0
        for family in ("poisson", "gaussian"):
            for dtype_name in ("bfloat16", "float32"):
                for K in gp.ACC_K:
                    c = gp.accuracy_case(family, dtype_name, K)
                    m = gp.accuracy_model(family, dtype_name, K)
                    H = m.fisher_information(torch.tensor(c["beta"]))
                    assert H.dtype == torch.float64 and H.shape == (K, K)
                    ratio = fp.fisher_ratio(family, dtype_name, K, H.numpy())
                    print(f"\n{family} {dtype_name} K={K} threads={torch.get_num_threads()}: "
                          f"eager worst ratio {ratio:.3f}")
                    worst = max(worst, ratio)
                    assert ratio <= fp.FISHER_EAGER_M
        print(f"\nworst eager ratio {worst:.3f} (recorded {fp.FISHER_EAGER_MEASURED}, "
              f"allowed {fp.FISHER_EAGER_M})")
    finally:
        torch.set_num_threads(before)


def test_bound_constants():
    assert fp.FISHER_EAGER_MEASURED <= fp.FISHER_EAGER_M < 2 * fp.FISHER_EAGER_MEASURED
    assert fp.FISHER_KERNEL_M == 4 * fp.FISHER_EAGER_M


# ---------------------------------------------------------------------------
# fp64 eager model against central differences of logp_grad
# ---------------------------------------------------------------------------

def _central_differences(model, beta, h=1e-4):
    K = beta.shape[0]
    H = np.zeros((K, K))
    for k in range(K):
        e = np.zeros(K)
        e[k] = h
        _, (gp_,) = model(beta + e)
        _, (gm_,) = model(beta - e)
        H[:, k] = -(gp_ - gm_) / (2 * h)
    return H


@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_fisher_is_the_negative_hessian(family):
    n, K = 300, 5
    if family == "poisson":
        X, y, offset, beta = generate_poisson_dataset(n, K, seed=4)
        m = PoissonGLMModel(X, y, offset=offset)
    else:
        X, y, beta = generate_gaussian_glm_dataset(n, K, sigma=0.7, seed=4)
        m = GaussianGLMModel(X, y, 0.7)
    H = m.fisher_information(torch.tensor(beta)).numpy()
    fd = _central_differences(m, beta)
    assert np.max(np.abs(H - fd)) <= 1e-6 * np.max(np.abs(H))
    assert np.array_equal(H, H.T)


# ---------------------------------------------------------------------------
# padding, shapes, out= and errors
# ---------------------------------------------------------------------------

def test_shapes_out_and_errors():
    n, K = 150, 20
    p = gp.gaussian_sparse_probe(n, K, 2.0)
    m = GaussianGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), 2.0, dtype=torch.bfloat16)
    beta = torch.tensor(p["beta"])
    H = m.fisher_information(beta)
    assert H.shape == (K, K) and H.dtype == torch.float64
    np.testing.assert_array_equal(H.numpy(), p["X"].T @ p["X"] / 4.0)
    out = torch.full((K, K), -3.0, dtype=torch.float64)
    got = m.fisher_information(beta, out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.numpy(), H.numpy())
    with pytest.raises(ValueError, match="beta must have shape"):
        m.fisher_information(torch.zeros(K + 1))
    with pytest.raises(ValueError, match="out must be"):
        m.fisher_information(beta, out=torch.zeros((K, K), dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        m.fisher_information(beta, out=torch.zeros((K, K + 1), dtype=torch.float64))


def test_ops_validation_needs_no_gpu():
    X = torch.zeros((4, 16), dtype=torch.bfloat16)
    beta = torch.zeros(16)
    with pytest.raises(ValueError, match="unknown link"):
        glm_family_fisher(X, beta, link="logistic")
    with pytest.raises(TypeError, match="unsupported dtype"):
        glm_family_fisher(X.float(), beta, link="poisson")
    with pytest.raises(ValueError, match="not compiled"):
        glm_family_fisher(torch.zeros((4, 24), dtype=torch.bfloat16), torch.zeros(24),
                          link="poisson")
    with pytest.raises(ValueError, match="sigma must be positive"):
        glm_family_fisher(X, beta, link="gaussian", sigma=0.0)
    with pytest.raises(ValueError, match="beta must have shape"):
        glm_family_fisher(X, torch.zeros(8), link="poisson")
    with pytest.raises(ValueError, match="offset must be f32"):
        glm_family_fisher(X, beta, link="poisson", offset=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="offset must be f32"):
        glm_family_fisher(X, beta, link="poisson", offset=torch.zeros(5))
    with pytest.raises(ValueError, match="contiguous"):
        glm_family_fisher(torch.zeros((16, 4), dtype=torch.bfloat16).t(), beta, link="poisson")
    with pytest.raises(ValueError, match="ROCm device"):
        glm_family_fisher(X, beta, link="poisson")


# ---------------------------------------------------------------------------
# Newton
# ---------------------------------------------------------------------------

def _funcs(m):
    return m.as_logp_grad_func(), m.as_fisher_func()


def test_newton_gaussian_converges_in_one_step():
    X, y, _ = generate_gaussian_glm_dataset(400, 6, sigma=0.5, seed=8)
    m = GaussianGLMModel(X, y, 0.5)
    res = find_map_newton(*_funcs(m), np.zeros(6))
    assert res.converged and res.n_steps == 1
    ref = np.linalg.lstsq(X, y, rcond=None)[0]
    np.testing.assert_allclose(res.theta, ref, rtol=1e-10)
    np.testing.assert_allclose(res.cov, np.linalg.inv(X.T @ X / 0.25), rtol=1e-9)
    np.testing.assert_allclose(np.sqrt(np.diag(laplace_mass(res))),
                               0.5 * np.sqrt(np.diag(np.linalg.inv(X.T @ X))), rtol=1e-9)


def test_newton_poisson_converges_and_gives_the_laplace_covariance():
    X, y, offset, _ = generate_poisson_dataset(2000, 8)
    m = PoissonGLMModel(X, y, offset=offset)
    res = find_map_newton(*_funcs(m), np.zeros(8))
    assert res.converged and res.n_steps <= 10
    _, (g,) = m(res.theta)
    assert np.max(np.abs(g)) <= 1e-9 * max(1.0, abs(res.logp))
    H_ref = fp.fisher_reference(X, np.exp(X @ res.theta + offset))
    np.testing.assert_allclose(res.cov, np.linalg.inv(H_ref), rtol=1e-8, atol=0)
    # the metric NUTS takes
    sampler = NUTS(m.as_logp_grad_func(), [res.theta], seed=1)
    sampler.set_dense_mass(laplace_mass(res))
    np.testing.assert_array_equal(sampler.mass_sigma, sampler.mass_sigma.T)


def test_newton_two_shards_equal_the_union():
    X, y, offset, _ = generate_poisson_dataset(2000, 8)
    whole = PoissonGLMModel(X, y, offset=offset)
    a = PoissonGLMModel(X[:700], y[:700], offset=offset[:700])
    b = PoissonGLMModel(X[700:], y[700:], offset=offset[700:])
    one = find_map_newton(*_funcs(whole), np.zeros(8))
    two = find_map_newton([a.as_logp_grad_func(), b.as_logp_grad_func()],
                          [a.as_fisher_func(), b.as_fisher_func()], np.zeros(8))
    assert two.converged and two.n_steps == one.n_steps
    np.testing.assert_allclose(two.theta, one.theta, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(two.cov, one.cov, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(two.logp, one.logp, rtol=1e-12)
    with pytest.raises(ValueError, match="per shard"):
        find_map_newton([a.as_logp_grad_func()], [], np.zeros(8))


@pytest.mark.parametrize("matrix", [False, True])
def test_newton_prior_precision_closed_form(matrix):
    sigma, tau, K = 0.5, 3.0, 6
    X, y, _ = generate_gaussian_glm_dataset(400, K, sigma=sigma, seed=8)
    m = GaussianGLMModel(X, y, sigma)
    P = tau * np.eye(K)
    if matrix:
        A = np.random.RandomState(2).standard_normal((K, K))
        P = A @ A.T + np.eye(K)
    res = find_map_newton(*_funcs(m), np.zeros(K), prior_precision=P if matrix else tau)
    A_post = X.T @ X / sigma ** 2 + P
    ref = np.linalg.solve(A_post, X.T @ y / sigma ** 2)
    assert res.converged and res.n_steps == 1
    np.testing.assert_allclose(res.theta, ref, rtol=1e-10)
    np.testing.assert_allclose(res.cov, np.linalg.inv(A_post), rtol=1e-9)
    logp0, _ = m(ref)
    np.testing.assert_allclose(res.logp, float(logp0) - 0.5 * ref @ P @ ref, rtol=1e-12)
    with pytest.raises(ValueError, match="prior_precision"):
        find_map_newton(*_funcs(m), np.zeros(K), prior_precision=np.eye(K + 1))


@pytest.mark.parametrize("start", [3.0, -12.0])
def test_newton_step_halving_rescues_a_poor_start(start):
    """From 3 * ones the full steps already ascend (the slow, safe descent
    from an overestimated mean); from an intercept of -12 the weights are
    ~e^-12, the full step overflows the link and has to be halved."""
    X, y, offset, _ = generate_poisson_dataset(2000, 8)
    m = PoissonGLMModel(X, y, offset=offset)
    good = find_map_newton(*_funcs(m), np.zeros(8))
    calls = []

    def counted(b):
        calls.append(1)
        return m(b)

    init = start * np.ones(8) if start > 0 else start * np.eye(8)[0]
    poor = find_map_newton(counted, m.as_fisher_func(), init, max_steps=60)
    assert poor.converged
    np.testing.assert_allclose(poor.theta, good.theta, rtol=1e-8, atol=1e-10)
    if start < 0:
        # more logp evaluations than steps: at least one step was halved
        assert len(calls) > poor.n_steps + 1


# ---------------------------------------------------------------------------
# service round trip
# ---------------------------------------------------------------------------

def _fisher_model():
    X, y, offset, beta = generate_poisson_dataset(200, 8, seed=6)
    return PoissonGLMModel(X, y, offset=offset), beta


def _serve_fisher(port: int):
    from pytensor_federated_amd.service import serve_compute_func

    model, _ = _fisher_model()
    serve_compute_func(model.as_fisher_func(), "127.0.0.1", port)


def _wait_tcp(port, timeout=30.0):
    deadline = time.time() + timeout
    while time.time() < deadline:
        try:
            with socket.create_connection(("127.0.0.1", port), timeout=1):
                return
        except OSError:
            time.sleep(0.1)
    raise TimeoutError(f"port {port} never opened")


def test_fisher_func_through_the_service_unit():
    """In process: the service runs the Fisher function on wire messages."""
    from pytensor_federated_amd.npproto.utils import ndarray_from_numpy, ndarray_to_numpy
    from pytensor_federated_amd.rpc import InputArrays
    from pytensor_federated_amd.service import ArraysToArraysService, _run_compute_func

    model, beta = _fisher_model()
    ArraysToArraysService(model.as_fisher_func())
    out = _run_compute_func(InputArrays(items=[ndarray_from_numpy(beta)], uuid="h"),
                            model.as_fisher_func())
    assert out.uuid == "h" and len(out.items) == 1
    H = ndarray_to_numpy(out.items[0])
    assert H.shape == (8, 8)
    np.testing.assert_array_equal(H, model.fisher_information(torch.tensor(beta)).numpy())


@pytest.mark.timeout(180)
def test_fisher_func_served_to_a_client():
    from pytensor_federated_amd.service import ArraysToArraysServiceClient

    ctx = multiprocessing.get_context("spawn")
    proc = ctx.Process(target=_serve_fisher, args=(FISHER_PORT,), daemon=True)
    proc.start()
    try:
        _wait_tcp(FISHER_PORT)
        model, beta = _fisher_model()
        client = ArraysToArraysServiceClient("127.0.0.1", FISHER_PORT)
        (H,) = client.evaluate(beta)
        assert H.shape == (8, 8) and H.dtype == np.float64
        np.testing.assert_array_equal(H, model.fisher_information(torch.tensor(beta)).numpy())
        del client
    finally:
        proc.terminate()
        proc.join(timeout=10)
