"""GPU (MI355X) tests of the GLM Fisher-information kernel
(csrc/glm_family_fisher.hip), of the Poisson / Gaussian GLM models'
``fisher_information`` on it, and of Newton MAP driven by the kernel model.

Exact probes (tests/glm_fisher_probes.py): every ``w*x`` is exact in bf16
and every partial sum exact in f32, so H is compared with fp64 numpy by
``assert_array_equal`` at every K of the kernel, at the row counts where a
tile or the block's tile loop ends.  The premises are checked without a GPU
in test_glm_fisher_cpu.py.

Accuracy sets: glm_probes.accuracy_case data within
``FISHER_KERNEL_M * 2^-24 * H_scale`` of fp64 numpy per entry.
"""
import warnings

import numpy as np
import pytest
import torch

import glm_fisher_probes as fp
import glm_probes as gp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.inference import find_map_newton
from pytensor_federated_amd.models import GaussianGLMModel
from pytensor_federated_amd.ops import (
    GLM_FAMILY_FISHER_K,
    glm_family_fisher,
    glm_family_fisher_tile_rows,
)

PROBES = sorted(fp.EXACT_PROBES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_grid(monkeypatch):
    monkeypatch.delenv("FED_GLM_FISHER_GRID", raising=False)


def _np(t):
    return t.detach().cpu().numpy()


def _eval(dev, probe, n, K):
    link, build, sigma = fp.EXACT_PROBES[probe]
    p = build(n, K)
    X = torch.tensor(p["X"], dtype=torch.bfloat16, device=dev)
    offset = p.get("offset")
    if offset is not None:
        offset = torch.tensor(offset, dtype=torch.float32, device=dev)
    beta = torch.tensor(p["beta"], dtype=torch.float32)
    return lambda: glm_family_fisher(X, beta, link=link, offset=offset, sigma=sigma)


def _check(call, probe, n, K, what):
    H = call()
    assert H.shape == (K, K) and H.dtype == torch.float64
    np.testing.assert_array_equal(_np(H), fp.exact_reference(probe, n, K),
                                  err_msg=f"{probe} N={n} K={K} {what}")


def test_kernel_sizes_match_the_probe_module():
    assert tuple(GLM_FAMILY_FISHER_K) == fp.FISHER_K
    for K in fp.FISHER_K:
        assert glm_family_fisher_tile_rows(K) == fp.tile_rows(K)


# ---------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", fp.FISHER_K)
def test_fisher_exact_edge_rows(dev, K, probe):
    """One row, one short of / exactly / one past a tile, and two tiles plus
    a row; each evaluated twice on the same workspace."""
    for n in fp.edge_rows(K):
        call = _eval(dev, probe, n, K)
        _check(call, probe, n, K, "first call")
        _check(call, probe, n, K, "second call")


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", fp.FISHER_K)
def test_fisher_three_trips(dev, monkeypatch, K, probe):
    """6*TR + 1 rows on two row-chunk blocks per panel pair: three full
    tiles each and a one-row ragged tile."""
    n = fp.deep_rows(K)
    monkeypatch.setenv("FED_GLM_FISHER_GRID", str(fp.DEEP_GRID))
    call = _eval(dev, probe, n, K)
    _check(call, probe, n, K, f"grid={fp.DEEP_GRID}")
    _check(call, probe, n, K, f"grid={fp.DEEP_GRID} again")


@pytest.mark.parametrize("probe", ["poisson_zero_beta", "poisson_gate", "gaussian_sigma2"])
@pytest.mark.parametrize("K", fp.FISHER_K)
def test_fisher_after_larger_problem(dev, K, probe):
    """The same small problem evaluated again after a larger one of the
    same K has left non-zero leftovers in the workspace and in LDS."""
    n, big = fp.stale_small_rows(K), fp.stale_big_rows(K)
    small_call = _eval(dev, probe, n, K)
    big_call = _eval(dev, probe, big, K)
    _check(small_call, probe, n, K, "before")
    _check(big_call, probe, big, K, "big")
    _check(small_call, probe, n, K, "after big")


# ---------------------------------------------------------------------------
# symmetry and accuracy where exp matters
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("K", fp.FISHER_K)
def test_fisher_is_exactly_symmetric(dev, K):
    """Bit for bit, on data whose products are not exact (the Poisson
    accuracy generator at 1000 rows)."""
    from pytensor_federated_amd.models import generate_poisson_dataset

    X, _, offset, beta = generate_poisson_dataset(1000, K, seed=3)
    H = glm_family_fisher(
        torch.tensor(X, dtype=torch.bfloat16, device=dev), torch.tensor(beta),
        link="poisson", offset=torch.tensor(offset, dtype=torch.float32, device=dev),
    )
    assert torch.equal(H, H.t())
    assert bool(torch.all(torch.diagonal(H) > 0))


@pytest.mark.parametrize("K", gp.ACC_K)
@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_fisher_kernel_accuracy(dev, family, K):
    c = gp.accuracy_case(family, "bfloat16", K)
    m = gp.accuracy_model(family, "bfloat16", K, device=dev, use_kernels=True)
    assert m._fisher_kernel_path() and m._k_eff == {8: 8, 100: 128, 512: 512}[K]
    H = m.fisher_information(torch.tensor(c["beta"]))
    assert H.shape == (K, K) and H.dtype == torch.float64
    assert torch.equal(H, H.t())
    ratio = fp.fisher_ratio(family, "bfloat16", K, _np(H))
    print(f"\n{family} bf16 K={K}: Fisher kernel worst ratio {ratio:.4f} "
          f"(allowed {fp.FISHER_KERNEL_M})")
    assert ratio <= fp.FISHER_KERNEL_M


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["poisson", "gaussian"])
@pytest.mark.parametrize("dtype_name,kw", [("float32", {}), ("bfloat16", {"use_kernels": False})])
def test_fisher_eager_on_the_gpu(dev, family, dtype_name, kw):
    """f32 shards and use_kernels=False take the eager path on the GPU."""
    K = 100
    c = gp.accuracy_case(family, dtype_name, K)
    m = gp.accuracy_model(family, dtype_name, K, device=dev, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not m._fisher_kernel_path()
        H = m.fisher_information(torch.tensor(c["beta"]))
    assert H.shape == (K, K) and H.is_cuda
    ratio = fp.fisher_ratio(family, dtype_name, K, _np(H))
    print(f"\n{family} {dtype_name} K={K} {kw}: eager on the GPU, worst ratio {ratio:.4f}")
    assert ratio <= fp.FISHER_EAGER_M


def test_fisher_k2048_warns_and_goes_eager(dev):
    n, K = 64, 2048
    rng = np.random.RandomState(5)
    X = rng.randint(-2, 3, size=(n, K)).astype(np.float64)
    y = rng.randint(-8, 9, size=n) / 8.0
    m = GaussianGLMModel(torch.tensor(X), torch.tensor(y), 2.0, device=dev,
                         dtype=torch.bfloat16)
    with pytest.warns(UserWarning, match="Fisher kernel not compiled for K=2048"):
        H = m.fisher_information(torch.zeros(K))
    np.testing.assert_array_equal(_np(H), X.T @ X / 4.0)


def test_fisher_out_seam(dev):
    K, n = 32, 300
    p = fp.poisson_gate_probe(n, K)
    X = torch.tensor(p["X"], dtype=torch.bfloat16, device=dev)
    out = torch.full((K, K), -7.0, dtype=torch.float64, device=dev)
    H = glm_family_fisher(X, torch.tensor(p["beta"]), link="poisson", out=out)
    assert H.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(out), fp.exact_reference("poisson_gate", n, K))


# ---------------------------------------------------------------------------
# Newton on the kernel model
# ---------------------------------------------------------------------------

def test_newton_on_the_kernel_model(dev):
    """The mode found with the kernel's logp, grad and H is within
    2 * |H_ref^-1| @ (KERNEL_M * 2^-24 * G_scale) of the fp64 numpy Newton
    solution on the stored data: the root of a gradient that is off by e is
    off by H^-1 e, and the 2 covers the second-order effect of the error in
    H."""
    K = 8
    c = gp.accuracy_case("poisson", "bfloat16", K)
    X, y, offset = c["X"], c["y"], c["offset"]

    def ref_logp_grad(b):
        z = X @ b + offset
        mu = np.exp(z)
        return float(np.sum(y * z - mu)), [X.T @ (y - mu)]

    def ref_fisher(b):
        return [fp.fisher_reference(X, np.exp(X @ b + offset))]

    ref = find_map_newton(ref_logp_grad, ref_fisher, np.zeros(K))
    assert ref.converged
    mu = np.exp(X @ ref.theta + offset)
    G_scale = np.abs(X).T @ np.abs(y - mu)
    H_inv = np.linalg.inv(ref_fisher(ref.theta)[0])
    bound = 2.0 * np.abs(H_inv) @ (gp.KERNEL_M * 2.0 ** -24 * G_scale)

    m = gp.accuracy_model("poisson", "bfloat16", K, device=dev, use_kernels=True)
    assert m._fisher_kernel_path()
    got = find_map_newton(m.as_logp_grad_func(), m.as_fisher_func(), np.zeros(K))
    err = np.abs(got.theta - ref.theta)
    print(f"\nNewton on the kernel model: {got.n_steps} steps, worst error/bound "
          f"{float(np.max(err / bound)):.4f}")
    assert got.n_steps <= 25
    assert np.all(err <= bound)
    np.testing.assert_allclose(got.cov, ref.cov, rtol=0, atol=1e-4 * np.max(np.abs(ref.cov)))


# ---------------------------------------------------------------------------
# return codes of the C entry point (all before anything is launched)
# ---------------------------------------------------------------------------

def test_fisher_return_codes(dev):
    from pytensor_federated_amd.ops import require_kernels

    lib = require_kernels()
    n = 64
    stream = torch.cuda.current_stream().cuda_stream

    def call(K, link, ws_bytes):
        X = torch.zeros((n, K), dtype=torch.bfloat16, device=dev)
        beta = torch.zeros(K, dtype=torch.float32, device=dev)
        out = torch.full((K, K), -7.0, dtype=torch.float64, device=dev)
        ws = torch.zeros(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
        rc = lib.fed_glm_family_fisher(X.data_ptr(), None, n, K, beta.data_ptr(), link, 1.0,
                                       out.data_ptr(), ws.data_ptr(), ws_bytes, stream)
        torch.cuda.synchronize()
        return rc, out

    for K, link, ws_bytes, want in [
        (16, 2, 1 << 20, -5),            # logistic has no Fisher weight here
        (16, -1, 1 << 20, -5),
        (24, 0, 1 << 20, -4),
        (2048, 0, 1 << 20, -4),
        (16, 0, 4 * 16 * 16 * 4 - 4, -3),           # one block's four slab rows, less a float
        (256, 1, n * 4 - 16, -3),                   # not even the weights
        (256, 1, n * 4 + 3 * 128 * 128 * 4 - 4, -3),  # the weights, not one row chunk of slabs
    ]:
        rc, out = call(K, link, ws_bytes)
        assert rc == want, (K, link, ws_bytes, rc)
        assert bool(torch.all(out == -7.0)), "nothing may be written"
    # the smallest workspaces that do run
    rc, out = call(16, 0, 4 * 16 * 16 * 4)
    assert rc == 0 and bool(torch.all(out == 0.0))
    rc, out = call(256, 1, n * 4 + 3 * 128 * 128 * 4)
    assert rc == 0 and bool(torch.all(out == 0.0))
