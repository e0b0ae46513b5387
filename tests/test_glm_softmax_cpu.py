"""CPU tests of the softmax (multinomial) GLM: the premises of the exact
probes (tests/glm_softmax_probes.py), the eager path of ``SoftmaxGLMModel``
against fp64 numpy and ``torch.autograd``, its accuracy yardstick
``SOFTMAX_EAGER_M``, validation, both batched shapes, the served function and
MAP.  No GPU; the kernel is tested in test_gpu_glm_softmax.py.
"""
import numpy as np
import pytest
import torch

import glm_softmax_probes as sp

from pytensor_federated_amd.inference import find_map
from pytensor_federated_amd.models import SoftmaxGLMModel, generate_softmax_dataset
from pytensor_federated_amd.ops import (
    GLM_FAMILY_BATCHED_K,
    glm_softmax_class_group,
    glm_softmax_supports,
    split_bf16x3,
)

ALL_C = tuple(sorted(set(sp.EDGE_CLASSES + sp.FEW_CLASSES)))
PREMISE_K = (8, 32, 128, 1024)


def _premise_rows(K):
    return (1, 17, sp.tile_rows(K) + 1, sp.deep_rows(K))


# ---------------------------------------------------------------------------
# probe premises
# ---------------------------------------------------------------------------

def test_sizes_match_the_ops_module():
    assert tuple(GLM_FAMILY_BATCHED_K) == sp.BATCHED_K
    for C in range(2, 17):
        assert glm_softmax_class_group(C) == sp.class_group(C)
        assert glm_softmax_supports(torch.bfloat16, 128, C)
    for bad in (0, 1, 17):
        assert not glm_softmax_supports(torch.bfloat16, 128, bad)
        with pytest.raises(ValueError, match="n_classes"):
            glm_softmax_class_group(bad)
    assert not glm_softmax_supports(torch.float32, 128, 4)
    assert not glm_softmax_supports(torch.bfloat16, 2048, 4)
    assert not glm_softmax_supports(torch.bfloat16, 24, 4)


def test_fp32_exp_and_log_premises():
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    assert float(torch.exp(f(-(sp.SAT - 1.0)))) == 0.0
    assert float(torch.exp(f(0.0))) == 1.0
    assert float(torch.log(f(1.0))) == 0.0


def _is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def _is_bf16(a):
    t = torch.tensor(np.asarray(a, dtype=np.float64))
    return torch.equal(t.to(torch.bfloat16).to(torch.float64), t)


@pytest.mark.parametrize("probe", sorted(sp.EXACT_PROBES))
@pytest.mark.parametrize("K", PREMISE_K)
def test_probe_operands_and_intermediates_are_exact(probe, K):
    """X is bf16-exact, theta is exact as three bf16 pieces, the padded
    columns are zero, the chains differ pairwise, and every z, difference,
    residual and gradient partial sum is a whole number of a unit with fewer
    than 2^24 of them (sums of absolute values bound every partial sum)."""
    build, _ = sp.EXACT_PROBES[probe]
    for C in ALL_C:
        cp, G = sp.class_group(C), sp.n_groups(C)
        for n in _premise_rows(K):
            p = build(n, K, C)
            X, y, th16 = p["X"], p["y"], p["theta"]
            assert X.shape == (n, K) and th16.shape == (K, 16) and p["C"] == C
            assert y.min() >= 0 and y.max() < C and _is_bf16(X)
            pieces = split_bf16x3(torch.tensor(th16, dtype=torch.float32))
            assert pieces.shape == (3, 16, K)
            np.testing.assert_array_equal(
                pieces.to(torch.float64).sum(dim=0).t().numpy(), th16)
            img = th16.reshape(K, G, cp)
            assert np.all(img[:, :, C:] == 0.0)
            th = sp.unpack(th16, C)
            for g in range(G):
                for h in range(g):
                    assert not np.array_equal(th[:, g], th[:, h]), (g, h)
            Z = np.einsum("nk,kgc->ngc", X, th)
            unit = sp.UNIT if probe == "saturated_onehot" else 2.0 ** -3
            absZ = np.einsum("nk,kgc->ngc", np.abs(X), np.abs(th))
            assert np.all(Z / unit == np.round(Z / unit)) and absZ.max() / unit < 2 ** 24
            assert _is_f32(Z)
            D = Z - Z.max(axis=2, keepdims=True)
            assert _is_f32(D)
            if probe == "uniform":
                assert np.all(D == 0.0)
                resid_unit, resid_abs = 1.0 / 16, 1.0
            else:
                assert np.all(Z < 0)
                top = np.sort(Z, axis=2)
                gap = sp.SAT if probe == "saturated_dense" else sp.SAT - 1.0
                assert np.all(top[:, :, -1] - top[:, :, -2] >= gap)
                resid_unit, resid_abs = 1.0, 1.0
            # gradient partial sums: units of (X's unit 1/2) * resid_unit
            g_unit = 0.5 * resid_unit
            assert np.all(X / 0.5 == np.round(X / 0.5))
            assert np.abs(X).sum(axis=0).max() * resid_abs / g_unit < 2 ** 24
            # logp: every term is a multiple of the z unit, summed in fp64
            assert np.abs(D).sum() / unit < 2 ** 52


def test_saturated_probes_vary_labels_and_argmax():
    for probe in ("saturated_onehot", "saturated_dense"):
        p = sp.EXACT_PROBES[probe][0](257, 32, 5)
        Z = p["X"] @ sp.unpack(p["theta"], 5)[:, 0]
        top = np.argmax(Z, axis=1)
        assert len(set(top)) > 1 and len(set(p["y"])) == 5
        assert np.any(top == p["y"]) and np.any(top != p["y"])


@pytest.mark.parametrize("probe", sorted(sp.EXACT_PROBES))
def test_closed_form_references_agree_with_the_general_formula(probe):
    """The closed forms differ from the fp64 evaluation of the general
    formula only by the exp(-127) ~ 7e-56 remainders and by fp64 rounding."""
    for C in (3, 4, 16):
        for K in (8, 128):
            n = sp.tile_rows(K) + 1
            p = sp.EXACT_PROBES[probe][0](n, K, C)
            logp, G16 = sp.exact_reference(probe, n, K, C)
            logp_g, G16_g = sp.reference(p)
            np.testing.assert_allclose(logp, logp_g, rtol=1e-13, atol=0)
            np.testing.assert_allclose(G16, G16_g, rtol=0, atol=1e-12)
            assert _is_f32(G16) or sp.probe_check(probe, C) == "bound"
            cp = sp.class_group(C)
            assert np.all(G16.reshape(K, -1, cp)[:, :, C:] == 0.0)


# ---------------------------------------------------------------------------
# the eager path
# ---------------------------------------------------------------------------

def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("C", sp.ACC_C)
@pytest.mark.parametrize("K", sp.ACC_K)
@pytest.mark.parametrize("dtype_name", sp.ACC_DTYPES)
def test_eager_meets_its_yardstick(one_thread, dtype_name, K, C):
    """The measurement that fixes SOFTMAX_EAGER_M (single-threaded; -s
    prints the ratios), and its assertion."""
    c = sp.accuracy_case(dtype_name, K, C)
    m = sp.accuracy_model(dtype_name, K, C)
    assert not m._kernel_path() and m._k_eff == K
    logp, (G,) = m.logp_grad(torch.tensor(c["beta"]))
    assert logp.dtype == torch.float64 and G.dtype == torch.float64 and G.shape == (K, C)
    r_logp, r_grad = sp.accuracy_ratios(c, float(logp), _np(G))
    print(f"\nsoftmax {dtype_name} K={K} C={C}: eager logp ratio {r_logp:.4f}, "
          f"worst grad ratio {r_grad:.4f} (allowed {sp.SOFTMAX_EAGER_M})")
    assert r_logp <= sp.SOFTMAX_EAGER_M
    assert r_grad <= sp.SOFTMAX_EAGER_M


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float32", "float64"])
def test_eager_against_reference_and_autograd(dtype_name):
    n, K, C = 300, 20, 5
    X, y, beta = generate_softmax_dataset(n, K, C, seed=4)
    dtype = getattr(torch, dtype_name)
    m = SoftmaxGLMModel(X, y, dtype=dtype)
    assert m.n_classes == C and m.n_features == K and m.n_rows == n
    Xs = m._X.to(torch.float64)
    logp, (G,) = m.logp_grad(torch.tensor(beta))
    logp_ref, G_ref = sp.chain_reference(_np(Xs), y, beta)
    tol = 1e-12 if dtype_name == "float64" else 2e-6
    np.testing.assert_allclose(float(logp), logp_ref, rtol=tol)
    np.testing.assert_allclose(_np(G), G_ref, rtol=0, atol=tol * np.abs(_np(Xs)).sum(axis=0).max())
    b = torch.tensor(beta, requires_grad=True)
    lp = torch.log_softmax(Xs @ b, dim=1)[torch.arange(n), torch.tensor(y)].sum()
    lp.backward()
    np.testing.assert_allclose(float(logp), float(lp.detach()), rtol=tol)
    np.testing.assert_allclose(_np(G), _np(b.grad), rtol=0,
                               atol=tol * np.abs(_np(Xs)).sum(axis=0).max())


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_huge_predictors_stay_finite(dtype_name):
    """|z| up to 1e4: the maximum is subtracted before the exponential."""
    n, K, C = 200, 8, 4
    X, y, beta = generate_softmax_dataset(n, K, C, seed=5)
    X = X.astype(np.float32).astype(np.float64)
    beta = (beta * (1e4 / np.abs(X @ beta).max())).astype(np.float32).astype(np.float64)
    assert 9e3 <= np.abs(X @ beta).max() <= 1.1e4
    m = SoftmaxGLMModel(X, y, C, dtype=getattr(torch, dtype_name))
    logp, (G,) = m.logp_grad(torch.tensor(beta))
    logp_ref, G_ref = sp.chain_reference(X, y, beta)
    assert np.isfinite(float(logp)) and np.all(np.isfinite(_np(G)))
    assert logp_ref < -1e4
    np.testing.assert_allclose(float(logp), logp_ref, rtol=1e-12 if dtype_name == "float64" else 1e-5)
    np.testing.assert_allclose(_np(G), G_ref, rtol=0, atol=1e-9 if dtype_name == "float64" else 1e-2)


# ---------------------------------------------------------------------------
# construction and shapes
# ---------------------------------------------------------------------------

def test_validation_errors():
    X = np.zeros((6, 3))
    y = np.array([0, 1, 2, 0, 1, 2])
    with pytest.raises(ValueError, match=r"X must be \[N,K\]"):
        SoftmaxGLMModel(X[0], y)
    with pytest.raises(ValueError, match=r"X must be \[N,K\]"):
        SoftmaxGLMModel(X, y[:5])
    with pytest.raises(ValueError, match="at least one column"):
        SoftmaxGLMModel(X[:, :0], y)
    with pytest.raises(ValueError, match="integer class labels"):
        SoftmaxGLMModel(X, y + 0.5)
    with pytest.raises(ValueError, match="integer class labels"):
        SoftmaxGLMModel(X, np.where(y == 0, np.nan, y))
    with pytest.raises(ValueError, match="non-negative"):
        SoftmaxGLMModel(X, y - 1)
    with pytest.raises(ValueError, match="below n_classes"):
        SoftmaxGLMModel(X, y, 2)
    with pytest.raises(ValueError, match="at least 2"):
        SoftmaxGLMModel(X, np.zeros(6))
    with pytest.raises(ValueError, match="at least 2"):
        SoftmaxGLMModel(X, np.zeros(6), 1)
    m = SoftmaxGLMModel(X, y)
    with pytest.raises(ValueError, match="beta must have shape"):
        m.logp_grad(torch.zeros(3))
    with pytest.raises(ValueError, match="beta must have shape"):
        m.logp_grad(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="theta must be"):
        m.logp_grad_batched(torch.zeros(3, 4, 2))
    with pytest.raises(ValueError, match="theta must be"):
        m.logp_grad_batched(torch.zeros(8, 2))
    with pytest.raises(ValueError, match="out must be"):
        m.logp_grad(torch.zeros(3, 3), out=torch.zeros(9, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        m.logp_grad(torch.zeros(3, 3), out=torch.zeros(10, dtype=torch.float32))


def test_n_classes_inferred_and_given():
    X, y, beta = generate_softmax_dataset(50, 4, 3, seed=1)
    assert y.dtype == np.int64 and set(y) == {0, 1, 2} and beta.shape == (4, 3)
    assert SoftmaxGLMModel(X, y).n_classes == 3
    assert SoftmaxGLMModel(X, y.astype(np.float64)).n_classes == 3
    wide = SoftmaxGLMModel(X, y, 5)
    assert wide.n_classes == 5 and wide.fused_size == 1 + 4 * 5
    # a class nobody was labelled with only takes probability mass
    logp3, (G3,) = SoftmaxGLMModel(X, y).logp_grad(torch.tensor(beta))
    b5 = np.concatenate([beta, np.zeros((4, 2))], axis=1)
    b5[0, 3:] = -1e3  # X[:, 0] = 1: z = -1000 for the two extra classes
    logp5, (G5,) = wide.logp_grad(torch.tensor(b5))
    np.testing.assert_allclose(float(logp5), float(logp3), rtol=1e-12)
    np.testing.assert_allclose(_np(G5)[:, :3], _np(G3), atol=1e-12)
    assert np.all(_np(G5)[:, 3:] == 0.0)


def test_cpu_model_does_not_pad_or_use_kernels():
    X, y, beta = generate_softmax_dataset(40, 20, 3, seed=2)
    m = SoftmaxGLMModel(X, y, dtype=torch.bfloat16)
    assert m._k_pad == 0 and m._k_eff == 20 and not m._kernel_path()
    assert m.fused_size == 1 + 20 * 3
    logp, (G,) = m.logp_grad(torch.tensor(beta))
    assert G.shape == (20, 3)
    logp_ref, G_ref = sp.chain_reference(_np(m._X.to(torch.float64)), y,
                                         beta.astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(float(logp), logp_ref, rtol=1e-5)
    np.testing.assert_allclose(_np(G), G_ref, atol=1e-4)


def test_out_seam():
    X, y, beta = generate_softmax_dataset(60, 5, 4, seed=3)
    m = SoftmaxGLMModel(X, y)
    logp, (G,) = m.logp_grad(torch.tensor(beta))
    out = torch.full((m.fused_size,), 7.0, dtype=torch.float64)
    logp_o, (G_o,) = m.logp_grad(torch.tensor(beta), out=out)
    assert out.data_ptr() == logp_o.data_ptr() and G_o.shape == (5, 4)
    assert float(out[0]) == float(logp)
    np.testing.assert_array_equal(_np(out[1:]).reshape(5, 4), _np(G))
    np.testing.assert_array_equal(_np(G_o), _np(G))


@pytest.mark.parametrize("B", [1, 4, 5])
def test_batched_in_both_shapes_equals_per_chain(B):
    n, K, C = 80, 6, 4
    X, y, _ = generate_softmax_dataset(n, K, C, seed=8)
    m = SoftmaxGLMModel(X, y)
    theta = torch.tensor(np.random.RandomState(B).standard_normal((K, C, B)))
    logp, G = m.logp_grad_batched(theta)
    assert logp.shape == (B,) and G.shape == (K, C, B)
    logp_f, G_f = m.logp_grad_batched(theta.reshape(K * C, B))
    assert logp_f.shape == (B,) and G_f.shape == (K * C, B)
    np.testing.assert_array_equal(_np(logp_f), _np(logp))
    np.testing.assert_array_equal(_np(G_f), _np(G).reshape(K * C, B))
    for b in range(B):
        lb, (gb,) = m.logp_grad(theta[:, :, b])
        np.testing.assert_allclose(float(lb), float(logp[b]), rtol=1e-13)
        np.testing.assert_allclose(_np(gb), _np(G[:, :, b]), rtol=0, atol=1e-12)
        # flat rows are row-major in (K, C)
        np.testing.assert_array_equal(_np(G_f[:, b]), _np(G[:, :, b]).reshape(-1))


# ---------------------------------------------------------------------------
# service and MAP
# ---------------------------------------------------------------------------

def test_served_with_a_2d_parameter():
    """beta[K,C] through wrap_logp_grad_func and the npproto codec, in
    process: the service runs the model on a wire message."""
    from pytensor_federated_amd.common import wrap_logp_grad_func
    from pytensor_federated_amd.npproto.utils import ndarray_from_numpy, ndarray_to_numpy
    from pytensor_federated_amd.rpc import InputArrays
    from pytensor_federated_amd.service import ArraysToArraysService, _run_compute_func

    X, y, beta = generate_softmax_dataset(100, 5, 3, seed=9)
    model = SoftmaxGLMModel(X, y)
    func = wrap_logp_grad_func(model.as_logp_grad_func())
    ArraysToArraysService(func)
    out = _run_compute_func(InputArrays(items=[ndarray_from_numpy(beta)], uuid="s"), func)
    assert out.uuid == "s" and len(out.items) == 2
    logp, G = ndarray_to_numpy(out.items[0]), ndarray_to_numpy(out.items[1])
    logp_m, (G_m,) = model.logp_grad(torch.tensor(beta))
    assert logp.shape == () and G.shape == (5, 3) and G.dtype == np.float64
    assert float(logp) == float(logp_m)
    np.testing.assert_array_equal(G, _np(G_m))


def test_find_map_reaches_the_generating_logp():
    """Adam ascent from zero raises logp to the generating beta's within its
    sampling error: logp(beta_hat) >= logp(beta_true), and by Wilks the gap
    2 * (logp_hat - logp_true) is chi^2 with K*(C-1) = 8 degrees of freedom
    (mean 8, sd 4): below 8 + 6 * 4 = 32."""
    n, K, C = 2000, 4, 3
    X, y, beta = generate_softmax_dataset(n, K, C, seed=11)
    model = SoftmaxGLMModel(X, y)
    logp_true = float(model.logp_grad(torch.tensor(beta))[0])
    logp_zero = float(model.logp_grad(torch.zeros(K, C))[0])
    np.testing.assert_allclose(logp_zero, -n * np.log(C), rtol=1e-12)
    (est,), logp_hat = find_map(model, [np.zeros((K, C))], steps=2000, lr=0.05, tol=1e-13)
    assert est.shape == (K, C)
    assert logp_hat > logp_zero
    assert logp_true - 1e-6 <= logp_hat <= logp_true + 16.0
    # the gradient columns sum to zero over the classes: the unpinned direction
    _, (G,) = model.logp_grad(torch.tensor(est))
    np.testing.assert_allclose(_np(G).sum(axis=1), 0.0, atol=1e-9)
