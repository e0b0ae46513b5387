"""GPU (MI355X) tests of the softmax stage of the batched GLM family kernel
(csrc/glm_family_batched.hip, ``fed_glm_softmax_batched``) and of
``SoftmaxGLMModel`` on it.

Exact probes (tests/glm_softmax_probes.py): operands exact as three bf16
pieces and every intermediate exactly representable, so every chain of a
launch is compared with fp64 numpy bit-tight at every K of the kernel, at
the row counts where a 16-row fragment, a wave's 32 rows, a tile or the
block's tile loop ends, and at class counts on both sides of every class
group width.  The premises are checked without a GPU in
test_glm_softmax_cpu.py.

Accuracy sets: seeded categorical data within ``SOFTMAX_KERNEL_M * 2^-24 *
sum |row contribution|`` of fp64 numpy.
"""
import warnings

import numpy as np
import pytest
import torch

import glm_softmax_probes as sp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd import ops
from pytensor_federated_amd.models import SoftmaxGLMModel
from pytensor_federated_amd.ops import (
    GLM_FAMILY_BATCHED_K,
    glm_softmax_logp_grad,
    require_kernels,
    split_bf16x3,
)

BCH = sp.BCH
PROBES = sorted(sp.EXACT_PROBES)
UNIT24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_grid(monkeypatch):
    monkeypatch.delenv("FED_GLM_BATCHED_GRID", raising=False)


def _np(t):
    return t.detach().cpu().numpy()


def _eval(dev, probe, n, K, C):
    p = sp.EXACT_PROBES[probe][0](n, K, C)
    X = torch.tensor(p["X"], dtype=torch.bfloat16, device=dev)
    y = torch.tensor(p["y"], dtype=torch.float32, device=dev)
    theta = torch.tensor(p["theta"], dtype=torch.float32)
    return lambda: glm_softmax_logp_grad(X, y, theta, n_classes=C)


def _check(call, probe, n, K, C, what):
    logp_ref, G_ref = sp.exact_reference(probe, n, K, C)
    logp, G = call()
    logp, G = _np(logp), _np(G)
    msg = f"{probe} N={n} K={K} C={C} {what}"
    assert logp.shape == (sp.n_groups(C),) and G.shape == (K, BCH), msg
    assert logp.dtype == np.float64 and G.dtype == np.float64
    how = sp.probe_check(probe, C)
    if how == "bound":
        p = sp.EXACT_PROBES[probe][0](n, K, C)
        logp_scale, G_scale = sp.uniform_scales(p)
        bound = sp.SOFTMAX_KERNEL_M * UNIT24
        assert np.all(np.abs(logp - logp_ref) <= bound * logp_scale), msg
        assert np.all(np.abs(G - G_ref) <= bound * G_scale), msg
        return
    np.testing.assert_array_equal(G, G_ref, err_msg=msg)
    if how == "exact":
        np.testing.assert_array_equal(logp, logp_ref, err_msg=msg)
    else:
        np.testing.assert_allclose(logp, logp_ref, rtol=sp.WIDE_LOGP_RTOL, atol=0, err_msg=msg)


def test_kernel_sizes_match_the_probe_module():
    assert tuple(GLM_FAMILY_BATCHED_K) == sp.BATCHED_K


# ---------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", sp.BATCHED_K)
def test_softmax_exact_edge_rows(dev, K, probe):
    """C = 3 and 16 at one row, around a 16-row fragment, a wave's 32 rows,
    64 rows and the tile T, and two tiles plus a row; C = 2, 4, 5, 8, 9 at
    1, 17 and T+1 rows; each evaluated twice on the same workspace."""
    sizes = [(C, n) for C in sp.EDGE_CLASSES for n in sp.edge_rows(K)]
    sizes += [(C, n) for C in sp.FEW_CLASSES for n in sp.few_rows(K)]
    for C, n in sizes:
        call = _eval(dev, probe, n, K, C)
        _check(call, probe, n, K, C, "first call")
        _check(call, probe, n, K, C, "second call")


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", sp.BATCHED_K)
def test_softmax_two_trips(dev, monkeypatch, K, probe):
    """5T+5 rows on two blocks: three tiles each, the last ragged by five
    rows."""
    n = sp.deep_rows(K)
    monkeypatch.setenv("FED_GLM_BATCHED_GRID", str(sp.DEEP_GRID))
    for C in (3, 4, 16):
        call = _eval(dev, probe, n, K, C)
        _check(call, probe, n, K, C, f"grid={sp.DEEP_GRID}")
        _check(call, probe, n, K, C, f"grid={sp.DEEP_GRID} again")


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", sp.BATCHED_K)
def test_softmax_after_larger_problem(dev, K, probe):
    """A small problem evaluated again after a larger one of the same K and
    another class count has left non-zero leftovers in the workspace slab
    and in LDS (the larger one fills all 16 columns)."""
    n, big = sp.stale_small_rows(K), sp.stale_big_rows(K)
    for C_small, C_big in ((3, 16), (2, 5)):
        small_call = _eval(dev, probe, n, K, C_small)
        big_call = _eval(dev, probe, big, K, C_big)
        _check(small_call, probe, n, K, C_small, "before")
        _check(big_call, probe, big, K, C_big, "big")
        _check(small_call, probe, n, K, C_small, "after big")


# ---------------------------------------------------------------------------
# packing: 16 // CP chains per launch
# ---------------------------------------------------------------------------

class _Spy:
    def __init__(self, monkeypatch):
        self.calls = 0
        real = ops.glm_softmax_logp_grad

        def spy(*a, **kw):
            self.calls += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, "glm_softmax_logp_grad", spy)


@pytest.mark.parametrize("K", [8, 128, 1024])
def test_four_chains_of_four_classes_share_a_launch(dev, monkeypatch, K):
    """C = 4: B = 4 chains in one launch equal four single ``logp_grad``
    calls bit for bit (the probe's sums are exact in any order), and B = 5
    takes two launches."""
    C, n = 4, sp.deep_rows(K)
    p = sp.saturated_onehot(n, K, C)
    m = SoftmaxGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), C, device=dev,
                        dtype=torch.bfloat16, use_kernels=True)
    assert m._k_eff == K and m._kernel_path() and m.chains_per_launch == 4
    theta = torch.tensor(sp.unpack(p["theta"], C)).permute(0, 2, 1).contiguous()  # [K, C, 4]
    logp_ref, G_ref = sp.exact_reference("saturated_onehot", n, K, C)
    spy = _Spy(monkeypatch)
    logp, G = m.logp_grad_batched(theta)
    assert spy.calls == 1
    assert logp.shape == (4,) and G.shape == (K, C, 4)
    np.testing.assert_array_equal(_np(logp), logp_ref)
    np.testing.assert_array_equal(_np(G).transpose(0, 2, 1).reshape(K, BCH), G_ref)
    for b in range(4):
        lb, (gb,) = m.logp_grad(theta[:, :, b])
        assert gb.shape == (K, C)
        assert torch.equal(lb, logp[b]) and torch.equal(gb, G[:, :, b]), b
    assert spy.calls == 5

    theta5 = torch.cat([theta, theta[:, :, :1]], dim=2)
    spy.calls = 0
    logp5, G5 = m.logp_grad_batched(theta5.reshape(K * C, 5))
    assert spy.calls == 2
    assert logp5.shape == (5,) and G5.shape == (K * C, 5)
    assert torch.equal(logp5[:4], logp) and torch.equal(logp5[4], logp[0])
    assert torch.equal(G5[:, :4], G.reshape(K * C, 4)) and torch.equal(G5[:, 4], G5[:, 0])


# ---------------------------------------------------------------------------
# accuracy where exp matters (model level; K = 20 is zero-padded to 32 and
# K = 100 to 128)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("C", sp.ACC_C)
@pytest.mark.parametrize("K", sp.ACC_K)
def test_softmax_kernel_accuracy(dev, K, C):
    theta, cases = sp.accuracy_chains(K, C)
    m = sp.accuracy_model("bfloat16", K, C, device=dev, use_kernels=True)
    assert m._kernel_path() and m._k_eff == {20: 32, 100: 128, 512: 512}[K]
    logp, G = m.logp_grad_batched(torch.tensor(theta))
    n_chains = sp.n_groups(C)
    assert logp.shape == (n_chains,) and G.shape == (K, C, n_chains)
    logp, G = _np(logp), _np(G)
    ratios = [sp.accuracy_ratios(cases[g], float(logp[g]), G[:, :, g]) for g in range(n_chains)]
    r_logp, r_grad = max(r[0] for r in ratios), max(r[1] for r in ratios)
    print(f"\nsoftmax bf16 K={K} C={C}: kernel worst logp ratio {r_logp:.4f}, worst grad "
          f"ratio {r_grad:.4f} over {n_chains} chains (allowed {sp.SOFTMAX_KERNEL_M})")
    assert r_logp <= sp.SOFTMAX_KERNEL_M
    assert r_grad <= sp.SOFTMAX_KERNEL_M


def test_softmax_kernel_survives_huge_predictors(dev):
    """|z| ~ 1e3: without the max subtraction exp overflows at 88."""
    c = sp.overflow_case()
    K, C = sp.OVERFLOW_K, sp.OVERFLOW_C
    m = SoftmaxGLMModel(torch.tensor(c["X"]), torch.tensor(c["y"]), C, device=dev,
                        dtype=torch.bfloat16, use_kernels=True)
    assert m._kernel_path()
    logp, (G,) = m.logp_grad(torch.tensor(c["beta"]))
    logp, G = float(logp), _np(G)
    assert np.isfinite(logp) and np.all(np.isfinite(G)) and G.shape == (K, C)
    r_logp, r_grad = sp.accuracy_ratios(c, logp, G)
    print(f"\nsoftmax bf16 K={K} C={C} |z| <= {np.abs(c['X'] @ c['beta']).max():.0f}: kernel "
          f"logp ratio {r_logp:.4f}, worst grad ratio {r_grad:.4f} "
          f"(allowed {sp.SOFTMAX_KERNEL_M})")
    assert r_logp <= sp.SOFTMAX_KERNEL_M
    assert r_grad <= sp.SOFTMAX_KERNEL_M


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------

def _small_model(dev, K=16, C=4, n=50, **kw):
    rng = np.random.RandomState(K + C)
    X, y = rng.standard_normal((n, K)) / 4, rng.randint(0, C, size=n)
    y[:C] = np.arange(C)
    return SoftmaxGLMModel(X, y, C, device=dev, **kw), rng


def test_bf16_on_the_device_takes_the_kernel(dev, monkeypatch):
    m, rng = _small_model(dev, dtype=torch.bfloat16)
    spy = _Spy(monkeypatch)
    beta = torch.tensor(rng.standard_normal((16, 4)))
    logp, (G,) = m.logp_grad(beta)
    assert spy.calls == 1 and G.shape == (16, 4) and G.is_cuda
    logp_e, G_e = m._eval_eager(beta.reshape(16, 4, 1))
    np.testing.assert_allclose(float(logp), float(logp_e[0]), rtol=1e-5)
    np.testing.assert_allclose(_np(G), _np(G_e[:, :, 0]), atol=1e-4)
    out = torch.zeros(m.fused_size, dtype=torch.float64, device=dev)
    logp_o, (G_o,) = m.logp_grad(beta, out=out)
    assert torch.equal(out[0], logp) and torch.equal(out[1:].view(16, 4), G)
    # the explicit opt-out
    m_off, _ = _small_model(dev, dtype=torch.bfloat16, use_kernels=False)
    spy.calls = 0
    m_off.logp_grad(beta)
    assert spy.calls == 0


def test_f32_shard_and_17_classes_take_the_eager_path(dev, monkeypatch):
    spy = _Spy(monkeypatch)
    m, rng = _small_model(dev, dtype=torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not m._kernel_path()
        logp, (G,) = m.logp_grad(torch.tensor(rng.standard_normal((16, 4))))
    assert np.isfinite(float(logp)) and G.shape == (16, 4)
    m17, rng = _small_model(dev, C=17, dtype=torch.bfloat16)
    beta = torch.tensor(rng.standard_normal((16, 17)))
    with pytest.warns(UserWarning, match="softmax GLM kernel not compiled for n_classes=17"):
        logp, (G,) = m17.logp_grad(beta)
    logp_e, G_e = m17._eval_eager(beta.reshape(16, 17, 1))
    assert torch.equal(logp, logp_e[0]) and torch.equal(G, G_e[:, :, 0])
    assert spy.calls == 0


def test_model_falls_back_with_a_warning_at_2048(dev, monkeypatch):
    spy = _Spy(monkeypatch)
    m, rng = _small_model(dev, K=1100, C=3, n=5, dtype=torch.bfloat16)
    assert m._k_eff == 2048
    theta = torch.tensor(rng.standard_normal((1100, 3, 2)) / 8)
    with pytest.warns(UserWarning, match="softmax GLM kernel not compiled for K=2048"):
        logp, G = m.logp_grad_batched(theta)
    logp_e, G_e = m._eval_eager(theta)
    assert G.shape == (1100, 3, 2) and spy.calls == 0
    assert torch.equal(logp, logp_e) and torch.equal(G, G_e)


# ---------------------------------------------------------------------------
# entry-point errors (all returned before anything is launched)
# ---------------------------------------------------------------------------

def test_softmax_entry_point_return_codes(dev):
    lib = require_kernels()
    n, K = 4, 8
    X = torch.zeros((n, K), dtype=torch.bfloat16, device=dev)
    y = torch.zeros(n, dtype=torch.float32, device=dev)
    theta = torch.zeros((K, BCH), dtype=torch.float32, device=dev)
    pieces = split_bf16x3(theta)
    out = torch.zeros(BCH + K * BCH, dtype=torch.float64, device=dev)
    ws = torch.zeros(4 * K * BCH, dtype=torch.float32, device=dev)  # one block's 4 slab rows
    stream = torch.cuda.current_stream().cuda_stream

    def call(K=K, C=4, ws_bytes=ws.numel() * 4):
        return lib.fed_glm_softmax_batched(
            X.data_ptr(), y.data_ptr(), n, K, pieces.data_ptr(), C,
            out.data_ptr(), ws.data_ptr(), ws_bytes, stream,
        )

    assert call() == 0
    torch.cuda.synchronize()
    # theta = 0: four rows of label 0 at C = 4, logp = -4 log 4 on column 0 of every chain
    np.testing.assert_allclose(_np(out[:BCH]).reshape(4, 4)[:, 0], -4 * np.log(4.0), rtol=1e-6)
    assert np.all(_np(out[:BCH]).reshape(4, 4)[:, 1:] == 0.0)
    assert call(ws_bytes=ws.numel() * 4 - 1) == -3
    for bad_k in (0, 4, 12, 24, 2048, 4096):
        assert call(K=bad_k) == -4, bad_k
    for bad_c in (-1, 0, 1, 17, 32):
        assert call(C=bad_c) == -6, bad_c
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="n_classes"):
        glm_softmax_logp_grad(X, y, theta, n_classes=17)
    with pytest.raises(ValueError, match="not compiled"):
        glm_softmax_logp_grad(X[:, :4], y, theta[:4], n_classes=4)
    with pytest.raises(TypeError, match="bf16"):
        glm_softmax_logp_grad(X.float(), y, theta, n_classes=4)
    with pytest.raises(ValueError, match="y must be f32"):
        glm_softmax_logp_grad(X, y.to(torch.bfloat16), theta, n_classes=4)
    with pytest.raises(ValueError, match="theta16 must be"):
        glm_softmax_logp_grad(X, y, theta[:, :8], n_classes=4)
