"""GPU (MI355X) tests of the GLM Fisher-vector kernel
(csrc/glm_family_fvp.hip), of the three GLM models' ``fisher_vector_product``
and ``fisher_diagonal`` on it, and of Newton-CG MAP driven by the kernel
model.

Exact probes (tests/glm_fvp_probes.py): every operand, product and partial
sum is exact in f32, so the product and the diagonal are compared with fp64
numpy by ``assert_array_equal`` at every instantiation of both dtypes, at the
row counts where a step, a pair or a block's share ends.  The premises are
checked without a GPU in test_glm_fvp_cpu.py.

Accuracy sets: within ``FVP_KERNEL_M * 2^-24 * S`` of fp64 numpy per
component.
"""
import warnings

import numpy as np
import pytest
import torch

import glm_fisher_probes as fp
import glm_fvp_probes as vp
import glm_probes as gp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.inference import find_map_newton, find_map_newton_cg
from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel
from pytensor_federated_amd.ops import (
    glm_family_fisher_diagonal,
    glm_family_fisher_vector,
)

SHAPES = [(d, K, R) for d in vp.DTYPES for K, R in gp.family_shapes(d)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_grid(monkeypatch):
    monkeypatch.delenv("FED_GLM_GRID", raising=False)


def _np(t):
    return t.detach().cpu().numpy()


def _eval(dev, dtype, probe, n, K):
    """(product call, diagonal call) on device copies of a probe."""
    link, build, sigma = vp.EXACT_PROBES[probe]
    p = build(n, K)
    X = torch.tensor(p["X"], dtype=getattr(torch, dtype), device=dev)
    offset = p.get("offset")
    if offset is not None:
        offset = torch.tensor(offset, dtype=torch.float32, device=dev)
    beta = torch.tensor(p["beta"], dtype=torch.float32)
    v = torch.tensor(vp.probe_vector(K), dtype=torch.float32)
    kw = dict(link=link, offset=offset, sigma=sigma)
    return (lambda: glm_family_fisher_vector(X, beta, v, **kw),
            lambda: glm_family_fisher_diagonal(X, beta, **kw))


def _check(calls, probe, n, K, what):
    for call, ref, name in zip(calls, vp.exact_reference(probe, n, K), ("product", "diagonal")):
        r = call()
        assert r.shape == (K,) and r.dtype == torch.float64
        np.testing.assert_array_equal(_np(r), ref, err_msg=f"{probe} N={n} K={K} {what} {name}")


# ---------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("probe", vp.PROBES)
@pytest.mark.parametrize("dtype,K,R", SHAPES)
def test_fvp_exact_edge_rows(dev, monkeypatch, dtype, K, R, probe):
    """One row, a step short of / at / past full, a ragged third step, a
    block's 8 steps short of / past full; the product and the diagonal each
    evaluated twice on the same workspace.  Then 33R+1 rows on two blocks:
    two trips of the grid-stride loop and a third that ends on a one-row
    step."""
    for n in gp.family_rows(R):
        calls = _eval(dev, dtype, probe, n, K)
        _check(calls, probe, n, K, f"{dtype} first call")
        _check(calls, probe, n, K, f"{dtype} second call")
    monkeypatch.setenv("FED_GLM_GRID", str(gp.DEEP_GRID))
    n = gp.deep_rows(R)
    calls = _eval(dev, dtype, probe, n, K)
    _check(calls, probe, n, K, f"{dtype} grid={gp.DEEP_GRID}")
    _check(calls, probe, n, K, f"{dtype} grid={gp.DEEP_GRID} again")


@pytest.mark.parametrize("probe", ["poisson_zero_beta", "logistic_gate", "gaussian_sigma2"])
@pytest.mark.parametrize("dtype,K,R", SHAPES)
def test_fvp_after_larger_problem(dev, dtype, K, R, probe):
    """The same small problem evaluated again after a larger one of the
    same K has left non-zero leftovers in the workspace slab and in LDS."""
    n, big = R + 1, gp.stale_big_rows(R)
    small = _eval(dev, dtype, probe, n, K)
    _check(small, probe, n, K, f"{dtype} before")
    _check(_eval(dev, dtype, probe, big, K), probe, big, K, f"{dtype} big")
    _check(small, probe, n, K, f"{dtype} after big")


def test_fvp_out_seam(dev):
    K, n = 32, 300
    p = vp.EXACT_PROBES["logistic_gate"][1](n, K)
    X = torch.tensor(p["X"], dtype=torch.bfloat16, device=dev)
    beta, v = torch.tensor(p["beta"]), torch.tensor(vp.probe_vector(K))
    Hv_ref, d_ref = vp.exact_reference("logistic_gate", n, K)
    out = torch.full((K,), -7.0, dtype=torch.float64, device=dev)
    r = glm_family_fisher_vector(X, beta, v, link="logistic", out=out)
    assert r.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(out), Hv_ref)
    r = glm_family_fisher_diagonal(X, beta, link="logistic", out=out)
    assert r.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(out), d_ref)
    with pytest.raises(ValueError, match="out must be"):
        glm_family_fisher_vector(X, beta, v, link="logistic",
                                 out=torch.zeros(K, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        glm_family_fisher_diagonal(X, beta, link="logistic",
                                   out=torch.zeros(2 * K, dtype=torch.float64, device=dev)[::2])
    # through a model: K = 20 is padded to 32, out keeps the model's size
    q = gp.gaussian_sparse_probe(150, 20, 2.0)
    m = GaussianGLMModel(torch.tensor(q["X"]), torch.tensor(q["y"]), 2.0, device=dev,
                         dtype=torch.bfloat16)
    assert m._k_eff == 32 and m._fvp_kernel_path()
    v20 = vp.probe_vector(20)
    out = torch.full((20,), -7.0, dtype=torch.float64, device=dev)
    r = m.fisher_vector_product(torch.tensor(q["beta"]), torch.tensor(v20), out=out)
    assert r.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(out), vp.fvp_reference(q["X"], np.full(150, 0.25), v20))
    np.testing.assert_array_equal(_np(m.fisher_diagonal(torch.tensor(q["beta"]))),
                                  vp.diag_reference(q["X"], np.full(150, 0.25)))


# ---------------------------------------------------------------------------
# accuracy where exp matters, through the models
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family,dtype,K", vp.ACCURACY_CASES)
def test_fvp_kernel_accuracy(dev, family, dtype, K):
    """Every accuracy case takes the kernel without a warning: f32 shards,
    where ``fisher_information`` goes eager, and the logistic model at a
    padded K of 512 (bf16) / 256 (f32) included."""
    c, _ = vp.accuracy_data(family, dtype, K)
    m = vp.accuracy_model(family, dtype, K, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert m._fvp_kernel_path()
        if family == "logistic":
            assert m._k_eff == {"bfloat16": 512, "float32": 256}[dtype]
        elif dtype == "float32":
            assert not m._fisher_kernel_path()
        beta = torch.tensor(c["beta"])
        Hv = m.fisher_vector_product(beta, torch.tensor(vp.accuracy_vector(K)))
        d = m.fisher_diagonal(beta)
    for r in (Hv, d):
        assert r.shape == (K,) and r.dtype == torch.float64 and r.is_cuda
    r_v, r_d = vp.fvp_ratios(family, dtype, K, _np(Hv), _np(d))
    print(f"\n{family} {dtype} K={K}: kernel worst ratio product {r_v:.4f} "
          f"diagonal {r_d:.4f} (allowed {vp.FVP_KERNEL_M})")
    assert r_v <= vp.FVP_KERNEL_M and r_d <= vp.FVP_KERNEL_M


def test_fvp_k2048_takes_the_kernel(dev):
    """A bf16 shard at K = 2048 (64 rows): the product and the diagonal run
    on the kernel without a warning; ``fisher_information`` warns and goes
    eager."""
    n, K = 64, 2048
    X, y, offset, beta = (gp._round_f32(a) for a in _poisson_data(n, K))
    X = gp._round_bf16(X)
    v = vp.accuracy_vector(K)
    m = PoissonGLMModel(torch.tensor(X), torch.tensor(y), offset=torch.tensor(offset),
                        device=dev, dtype=torch.bfloat16)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert m._fvp_kernel_path() and m._k_eff == K
        Hv = m.fisher_vector_product(torch.tensor(beta), torch.tensor(v))
        d = m.fisher_diagonal(torch.tensor(beta))
    with pytest.warns(UserWarning, match="Fisher kernel not compiled for K=2048"):
        assert not m._fisher_kernel_path()
    w = np.exp(X @ beta + offset)
    unit = 2.0 ** -24
    r_v = np.max(np.abs(_np(Hv) - vp.fvp_reference(X, w, v)) / (unit * vp.fvp_scale(X, w, v)))
    d_ref = vp.diag_reference(X, w)
    r_d = np.max(np.abs(_np(d) - d_ref) / (unit * d_ref))
    print(f"\npoisson bfloat16 K={K} N={n}: kernel worst ratio product {r_v:.4f} "
          f"diagonal {r_d:.4f} (allowed {vp.FVP_KERNEL_M})")
    assert r_v <= vp.FVP_KERNEL_M and r_d <= vp.FVP_KERNEL_M


def _poisson_data(n, K):
    from pytensor_federated_amd.models import generate_poisson_dataset

    return generate_poisson_dataset(n, K, seed=11)


@pytest.mark.parametrize("K", gp.ACC_K)
@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_fvp_agrees_with_the_mfma_fisher_kernel(dev, family, K):
    """``H v`` by the row-group kernel against the MFMA kernel's H times v,
    within the sum of both bounds."""
    c = gp.accuracy_case(family, "bfloat16", K)
    m = gp.accuracy_model(family, "bfloat16", K, device=dev, use_kernels=True)
    assert m._fisher_kernel_path() and m._fvp_kernel_path()
    v = vp.accuracy_vector(K)
    beta = torch.tensor(c["beta"])
    Hv = _np(m.fisher_vector_product(beta, torch.tensor(v)))
    H = _np(m.fisher_information(beta))
    _, S, _ = vp.accuracy_fvp(family, "bfloat16", K)
    _, H_scale = fp.accuracy_fisher(family, "bfloat16", K)
    bound = 2.0 ** -24 * (vp.FVP_KERNEL_M * S + fp.FISHER_KERNEL_M * (H_scale @ np.abs(v)))
    err = np.abs(Hv - H @ v)
    print(f"\n{family} K={K}: product against MFMA H @ v, worst error/bound "
          f"{float(np.max(err / bound)):.4f}")
    assert np.all(err <= bound)
    d_err = np.abs(_np(m.fisher_diagonal(beta)) - np.diag(H))
    assert np.all(d_err <= 2.0 ** -24 * (vp.FVP_KERNEL_M + fp.FISHER_KERNEL_M) * np.diag(H_scale))


# ---------------------------------------------------------------------------
# Newton-CG on the kernel model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("diagonals", [False, True])
@pytest.mark.parametrize("K", [8, 100])
def test_newton_cg_on_the_kernel_model(dev, K, diagonals):
    """The mode found with the kernel's logp, grad, H v (and diag H) is
    within the bound of test_newton_on_the_kernel_model, 2 * |H_ref^-1| @
    (KERNEL_M * 2^-24 * G_scale), of the fp64 Newton solution on the stored
    data, and takes at most 1.5x the products the same driver takes on fp64
    numpy callables."""
    c = gp.accuracy_case("poisson", "bfloat16", K)
    X, y, offset = c["X"], c["y"], c["offset"]
    lg, H, hv, dg = vp.numpy_poisson_funcs(X, y, offset)
    ref = find_map_newton(lg, H, np.zeros(K))
    ref_cg = find_map_newton_cg(lg, hv, np.zeros(K),
                                fisher_diagonal_funcs=dg if diagonals else None)
    assert ref.converged and ref_cg.converged
    G_scale = np.abs(X).T @ np.abs(y - np.exp(X @ ref.theta + offset))
    bound = 2.0 * np.abs(np.linalg.inv(H(ref.theta)[0])) @ (gp.KERNEL_M * 2.0 ** -24 * G_scale)

    m = gp.accuracy_model("poisson", "bfloat16", K, device=dev, use_kernels=True)
    assert m._fvp_kernel_path()
    got = find_map_newton_cg(
        m.as_logp_grad_func(), m.as_fisher_vector_func(), np.zeros(K),
        fisher_diagonal_funcs=m.as_fisher_diagonal_func() if diagonals else None,
    )
    err = np.abs(got.theta - ref.theta)
    print(f"\nNewton-CG on the kernel model K={K} diagonals={diagonals}: {got.n_steps} steps, "
          f"{got.n_products} products (fp64 numpy: {ref_cg.n_steps} steps, "
          f"{ref_cg.n_products} products), converged={got.converged}, worst error/bound "
          f"{float(np.max(err / bound)):.4f}")
    assert np.all(err <= bound)
    assert got.n_products <= 1.5 * ref_cg.n_products


# ---------------------------------------------------------------------------
# return codes of the C entry point (all before anything is launched)
# ---------------------------------------------------------------------------

def test_fvp_return_codes(dev):
    from pytensor_federated_amd.ops import require_kernels

    lib = require_kernels()
    n = 64
    stream = torch.cuda.current_stream().cuda_stream
    BF16, F32, F64 = 2, 0, 1

    def call(dtype, K, link, ws_bytes, with_v=True):
        X = torch.zeros((n, K), dtype=torch.float32 if dtype != BF16 else torch.bfloat16,
                        device=dev)
        beta = torch.zeros(K, dtype=torch.float32, device=dev)
        v = torch.ones(K, dtype=torch.float32, device=dev)
        out = torch.full((K,), -7.0, dtype=torch.float64, device=dev)
        ws = torch.zeros(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
        rc = lib.fed_glm_family_fvp(X.data_ptr(), None, n, K, beta.data_ptr(),
                                    v.data_ptr() if with_v else None, link, 1.0,
                                    out.data_ptr(), ws.data_ptr(), ws_bytes, dtype, stream)
        torch.cuda.synchronize()
        return rc, out

    for dtype, K, link, ws_bytes, want in [
        (F64, 16, 0, 1 << 20, -2),
        (7, 16, 0, 1 << 20, -2),
        (F64, 24, 3, 0, -2),             # the dtype is checked first
        (BF16, 16, 3, 1 << 20, -5),
        (BF16, 16, -1, 1 << 20, -5),
        (BF16, 24, 2, 0, -4),            # ... and K before the workspace
        (BF16, 4, 0, 1 << 20, -4),
        (BF16, 4096, 0, 1 << 20, -4),
        (F32, 2048, 1, 1 << 20, -4),
        (F32, 12, 1, 1 << 20, -4),
        (BF16, 16, 0, 16 * 4 - 4, -3),   # one slab row, less a float
        (F32, 1024, 2, 1024 * 4 - 4, -3),
    ]:
        for with_v in (True, False):
            rc, out = call(dtype, K, link, ws_bytes, with_v)
            assert rc == want, (dtype, K, link, ws_bytes, with_v, rc)
            assert bool(torch.all(out == -7.0)), "nothing may be written"
    # the smallest workspace that does run: one block's slab row (X = 0: the
    # result is 0 whatever the weight)
    for dtype, K, link in [(BF16, 16, 0), (F32, 1024, 2), (BF16, 2048, 1)]:
        for with_v in (True, False):
            rc, out = call(dtype, K, link, K * 4, with_v)
            assert rc == 0 and bool(torch.all(out == 0.0)), (dtype, K, link, with_v, rc)
