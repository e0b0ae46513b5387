"""GPU (MI355X) tests of the GLM family kernel (csrc/glm_family.hip) and of
the Poisson / Gaussian GLM models on it.

Exact probes (tests/glm_probes.py, exact_probes.py): every intermediate is
exactly representable, so the kernel is compared with fp64 numpy bit-tight
in every instantiation -- each link, both dtypes, every lane-group size G
(K = G*VEC) and KITER = 2, 4 -- at the row counts where a step, a pair of
steps, a block or the grid-stride loop ends.  The premises are checked
without a GPU in test_glm_probes_cpu.py.

Accuracy sets: seeded data with |z| <= 4, where exp() is not trivial,
within ``KERNEL_M * 2^-24 * sum |row contribution|`` of fp64 numpy.
"""
import numpy as np
import pytest
import torch

import exact_probes as ep
import glm_probes as gp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel
from pytensor_federated_amd.ops import (
    glm_family_logp_grad,
    logistic_glm_logp_grad,
    logistic_kernel_supports,
    require_kernels,
)

DTYPES = sorted(gp.VEC)
SHAPES = [
    pytest.param(dtype, K, R, id=f"{dtype}-K{K}")
    for dtype in DTYPES for K, R in gp.family_shapes(dtype)
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_grid(monkeypatch):
    monkeypatch.delenv("FED_GLM_GRID", raising=False)


def _np(t):
    return t.detach().cpu().numpy()


def _device_probe(dev, dtype, p, beta):
    """Probe arrays -> what the kernel reads (torch.tensor copies: the cached
    probe arrays are read-only)."""
    X = torch.tensor(p["X"], dtype=getattr(torch, dtype), device=dev)
    y = torch.tensor(p["y"], dtype=torch.float32, device=dev)
    offset = p.get("offset")
    if offset is not None:
        offset = torch.tensor(offset, dtype=torch.float32, device=dev)
    return X, y, offset, torch.tensor(beta, dtype=torch.float32)


def _eval_family(dev, dtype, probe, n, K):
    link, build, _, sigma = gp.EXACT_PROBES[probe]
    p = build(n, K)
    X, y, offset, beta = _device_probe(dev, dtype, p, p["beta"])
    return lambda: glm_family_logp_grad(
        X, y, beta, link=link, offset=offset, sigma=sigma, logp_const=gp.PROBE_CONST
    )


def _check_family(call, probe, n, K, what):
    logp_ref, G_ref = gp.exact_reference(probe, n, K)
    logp, g = call()
    logp, g = float(logp), _np(g)
    msg = f"{probe} N={n} K={K} {what}"
    assert g.shape == (K,)
    np.testing.assert_array_equal(g, G_ref, err_msg=msg)
    assert logp == logp_ref, f"{msg}: logp {logp!r} != {logp_ref!r}"


# ---------------------------------------------------------------------------
# exact probes: Poisson and Gaussian links
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("probe", sorted(gp.EXACT_PROBES))
@pytest.mark.parametrize("dtype,K,R", SHAPES)
def test_family_exact_edge_rows(dev, monkeypatch, dtype, K, R, probe):
    """One row, a step short of / at / past full, a ragged third step, a
    block's 8 steps short of / past full; each evaluated twice on the same
    workspace.  Then 33R+1 rows on two blocks: two trips of the grid-stride
    loop and a third that ends on a one-row step."""
    for n in gp.family_rows(R):
        call = _eval_family(dev, dtype, probe, n, K)
        _check_family(call, probe, n, K, f"{dtype} first call")
        _check_family(call, probe, n, K, f"{dtype} second call")
    monkeypatch.setenv("FED_GLM_GRID", str(gp.DEEP_GRID))
    n = gp.deep_rows(R)
    call = _eval_family(dev, dtype, probe, n, K)
    _check_family(call, probe, n, K, f"{dtype} grid={gp.DEEP_GRID}")
    _check_family(call, probe, n, K, f"{dtype} grid={gp.DEEP_GRID} again")


@pytest.mark.parametrize("probe", ["poisson_dense", "poisson_zero_beta", "gaussian_sigma2"])
@pytest.mark.parametrize("dtype,K,R", SHAPES)
def test_family_after_larger_problem(dev, dtype, K, R, probe):
    """The same small problem evaluated again after a larger one of the
    same K has left non-zero leftovers in the workspace slab and in LDS."""
    n, big = R + 1, gp.stale_big_rows(R)
    small_call = _eval_family(dev, dtype, probe, n, K)
    big_call = _eval_family(dev, dtype, probe, big, K)
    _check_family(small_call, probe, n, K, f"{dtype} before")
    _check_family(big_call, probe, big, K, f"{dtype} big")
    _check_family(small_call, probe, n, K, f"{dtype} after big")


# ---------------------------------------------------------------------------
# exact probes: logistic link
# ---------------------------------------------------------------------------

def _check_logistic(logp, g, probe, n, K, msg):
    ref = ep.single_reference(probe, n, K)
    assert g.shape == (K,)
    if probe == "zero_theta":
        np.testing.assert_array_equal(g, ref["G"], err_msg=msg)
        np.testing.assert_allclose(logp, ref["logp"][0], rtol=1e-6, atol=0, err_msg=msg)
    else:
        atol = ep.saturation_atol(n)
        np.testing.assert_allclose(g, ref["G"], rtol=0, atol=atol, err_msg=msg)
        np.testing.assert_allclose(logp, ref["logp"][0], rtol=0, atol=atol, err_msg=msg)


@pytest.mark.parametrize("probe", sorted(ep.LOGISTIC_PROBES))
@pytest.mark.parametrize("dtype,K,R", SHAPES)
def test_logistic_link_exact_edge_rows(dev, monkeypatch, dtype, K, R, probe):
    rows = [(n, None) for n in gp.family_rows(R)] + [(gp.deep_rows(R), gp.DEEP_GRID)]
    for n, grid in rows:
        if grid is not None:
            monkeypatch.setenv("FED_GLM_GRID", str(grid))
        p = ep.LOGISTIC_PROBES[probe](n, K)
        X, y, _, beta = _device_probe(dev, dtype, p, p["theta"][:, 0])
        for rnd in range(2):
            logp, g = glm_family_logp_grad(X, y, beta, link="logistic")
            _check_logistic(float(logp), _np(g), probe, n, K,
                            f"{probe} {dtype} N={n} K={K} grid={grid} call {rnd}")
        if grid is None and logistic_kernel_supports(getattr(torch, dtype), K):
            # wave-per-row layout: the existing kernel on the same probe
            logp_w, g_w = logistic_glm_logp_grad(X, y.to(X.dtype), beta)
            msg = f"{probe} {dtype} N={n} K={K} vs k_logistic_glm_reg"
            if probe == "zero_theta":
                np.testing.assert_array_equal(_np(g), _np(g_w), err_msg=msg)
                np.testing.assert_allclose(float(logp), float(logp_w), rtol=1e-12, err_msg=msg)
            else:
                atol = ep.saturation_atol(n)
                np.testing.assert_allclose(_np(g), _np(g_w), rtol=0, atol=atol, err_msg=msg)
                np.testing.assert_allclose(float(logp), float(logp_w), rtol=0, atol=atol,
                                           err_msg=msg)


def test_wave_per_row_shapes_meet_existing_kernel():
    """The comparison above runs at G = 64: every size of the existing
    kernel is a family size of the same dtype."""
    from pytensor_federated_amd.ops import LOGISTIC_SUPPORTED

    family = {(getattr(torch, dt), K) for dt in DTYPES for K, R in gp.family_shapes(dt) if R == 1}
    assert LOGISTIC_SUPPORTED <= family


# ---------------------------------------------------------------------------
# accuracy where exp matters (model level; K = 100 is zero-padded to 128)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("K", gp.ACC_K)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_kernel_accuracy(dev, family, dtype, K):
    c = gp.accuracy_case(family, dtype, K)
    m = gp.accuracy_model(family, dtype, K, device=dev, use_kernels=True)
    assert m._kernel_path() and m._k_eff == {8: 8, 100: 128, 512: 512}[K]
    logp, (g,) = m.logp_grad(torch.tensor(c["beta"]))
    assert g.shape == (K,)
    r_logp, r_grad = gp.accuracy_ratios(c, float(logp), _np(g))
    print(f"\n{family} {dtype} K={K}: kernel logp ratio {r_logp:.4f}, "
          f"worst grad ratio {r_grad:.4f} (allowed {gp.KERNEL_M})")
    assert r_logp <= gp.KERNEL_M
    assert r_grad <= gp.KERNEL_M


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

def _poisson_probe_model(dev, dtype, n, K, rows=slice(None), **kw):
    p = gp.poisson_zero_beta_probe(n, K)
    m = PoissonGLMModel(
        torch.tensor(p["X"][rows]), torch.tensor(p["y"][rows]),
        offset=torch.tensor(p["offset"][rows]), device=dev, dtype=dtype, use_kernels=True, **kw
    )
    return p, m


def _lgamma_const(y):
    return -float(torch.sum(torch.lgamma(torch.tensor(np.asarray(y)) + 1.0)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_model_out_slice_and_padding(dev, dtype):
    """``out=`` into a slice of a larger fp64 buffer, with and without
    zero-column padding; a padded model returns a grad of length K."""
    for n, K in ((131, 16), (131, 20), (77, 100)):
        p, m = _poisson_probe_model(dev, dtype, n, K)
        assert m._k_eff == gp_padded(dtype, K) and m._kernel_path()
        assert m.fused_size == 1 + K
        logp_ref, G_ref = gp.poisson_flushed_reference(p["X"], p["y"], p["beta"], p["offset"])
        logp_ref += _lgamma_const(p["y"])
        buf = torch.full((K + 9,), 7.0, dtype=torch.float64, device=dev)
        logp, (g,) = m.logp_grad(torch.zeros(K), out=buf[3 : 4 + K])
        assert g.shape == (K,)
        assert logp.data_ptr() == buf[3:].data_ptr() and g.data_ptr() == buf[4:].data_ptr()
        got = _np(buf)
        assert np.all(got[:3] == 7.0) and np.all(got[4 + K :] == 7.0)
        np.testing.assert_array_equal(got[4 : 4 + K], G_ref)
        np.testing.assert_allclose(got[3], logp_ref, rtol=1e-14)
        logp2, (g2,) = m.logp_grad(torch.zeros(K))
        np.testing.assert_array_equal(_np(g2), G_ref)
        np.testing.assert_allclose(float(logp2), got[3], rtol=1e-14)


def gp_padded(dtype, K):
    from pytensor_federated_amd.ops import glm_family_padded_k

    return glm_family_padded_k(dtype, K)


def test_model_offset_given_and_omitted(dev):
    n, K = 201, 24
    p = gp.poisson_zero_beta_probe(n, K)
    X, y = torch.tensor(p["X"]), torch.tensor(p["y"])
    kw = dict(device=dev, dtype=torch.float32, use_kernels=True)
    with_off = PoissonGLMModel(X, y, offset=torch.tensor(p["offset"]), **kw)
    without = PoissonGLMModel(X, y, **kw)
    const = _lgamma_const(p["y"])
    for m, offset in ((with_off, p["offset"]), (without, None)):
        logp_ref, G_ref = gp.poisson_flushed_reference(p["X"], p["y"], p["beta"], offset)
        logp, (g,) = m.logp_grad(torch.zeros(K))
        np.testing.assert_array_equal(_np(g), G_ref)
        np.testing.assert_allclose(float(logp), logp_ref + const, rtol=1e-14)
    # the offset matters: rows at -128 drop their exp(z) = 1
    beta0 = torch.zeros(K)
    assert float(with_off.logp_grad(beta0)[0]) != float(without.logp_grad(beta0)[0])


def test_model_non_contiguous_inputs(dev):
    n, K, sigma = 150, 16, 2.0
    p = gp.gaussian_sparse_probe(n, K, sigma)
    Xt = torch.tensor(p["X"].T.copy(), device=dev).t()          # column-major view
    y2 = torch.tensor(np.stack([p["y"], -p["y"]], axis=1), device=dev)[:, 0]  # strided
    assert not Xt.is_contiguous() and not y2.is_contiguous()
    m = GaussianGLMModel(Xt, y2, sigma, dtype=torch.bfloat16, use_kernels=True)
    beta = torch.tensor(np.stack([p["beta"], p["beta"]], axis=1))[:, 0]     # strided too
    logp_ref, G_ref = gp.gaussian_reference(
        p["X"], p["y"], p["beta"], sigma, const=-0.5 * n * np.log(2 * np.pi * sigma * sigma)
    )
    logp, (g,) = m.logp_grad(beta)
    np.testing.assert_array_equal(_np(g), G_ref)
    np.testing.assert_allclose(float(logp), logp_ref, rtol=1e-14)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_half_shards_add_up_through_the_kernel(dev, dtype):
    n, K = 333, 40  # padded to 64; halves of 166 and 167 rows
    p, whole = _poisson_probe_model(dev, dtype, n, K)
    _, a = _poisson_probe_model(dev, dtype, n, K, rows=slice(0, 166))
    _, b = _poisson_probe_model(dev, dtype, n, K, rows=slice(166, None))
    beta = torch.zeros(K)
    lw, (gw,) = whole.logp_grad(beta)
    la, (ga,) = a.logp_grad(beta)
    lb, (gb,) = b.logp_grad(beta)
    np.testing.assert_array_equal(_np(ga) + _np(gb), _np(gw))
    np.testing.assert_allclose(float(la) + float(lb), float(lw), rtol=1e-14)

    sigma = 2.0
    q = gp.gaussian_sparse_probe(n, K, sigma)
    kw = dict(device=dev, dtype=dtype, use_kernels=True)
    parts = [
        GaussianGLMModel(torch.tensor(q["X"][r]), torch.tensor(q["y"][r]), sigma, **kw)
        for r in (slice(None), slice(0, 166), slice(166, None))
    ]
    (lw, (gw,)), (la, (ga,)), (lb, (gb,)) = [m.logp_grad(torch.tensor(q["beta"])) for m in parts]
    np.testing.assert_array_equal(_np(ga) + _np(gb), _np(gw))
    np.testing.assert_allclose(float(la) + float(lb), float(lw), rtol=1e-14)


def test_model_falls_back_with_a_warning_above_the_kernel_sizes(dev):
    n, K = 5, 1100  # above f32's 1024
    rng = np.random.RandomState(0)
    X, y = rng.standard_normal((n, K)) / 40, rng.standard_normal(n)
    m = GaussianGLMModel(X, y, 1.0, device=dev, dtype=torch.float32)
    assert m._k_pad == 0
    with pytest.warns(UserWarning, match="family kernel not compiled"):
        logp, (g,) = m.logp_grad(torch.zeros(K))
    logp_ref, G_ref = gp.gaussian_reference(_np(m._X), _np(m._y), np.zeros(K), 1.0,
                                            const=-0.5 * n * np.log(2 * np.pi))
    np.testing.assert_allclose(float(logp), logp_ref, rtol=1e-6)
    np.testing.assert_allclose(_np(g), G_ref, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# entry-point errors (all returned before anything is launched)
# ---------------------------------------------------------------------------

def test_entry_point_return_codes(dev):
    lib = require_kernels()
    X = torch.zeros((4, 8), dtype=torch.bfloat16, device=dev)
    y = torch.zeros(4, dtype=torch.float32, device=dev)
    beta = torch.zeros(8, dtype=torch.float32, device=dev)
    out = torch.zeros(9, dtype=torch.float64, device=dev)
    ws = torch.zeros(1024 * 8, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(K=8, link=0, ws_bytes=ws.numel() * 4, dtype=2):
        return lib.fed_glm_family(
            X.data_ptr(), y.data_ptr(), None, 4, K, beta.data_ptr(), link, 1.0, 0.0,
            out.data_ptr(), ws.data_ptr(), ws_bytes, dtype, stream,
        )

    assert call() == 0
    assert call(dtype=1) == -2          # f64 is not compiled
    assert call(ws_bytes=8 * 4 - 1) == -3
    for K in (0, 4, 12, 24, 4096):
        assert call(K=K) == -4, K
    assert call(link=3) == -5 and call(link=-1) == -5
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="unknown link"):
        glm_family_logp_grad(X, y, beta, link="probit")
    with pytest.raises(ValueError, match="not compiled"):
        glm_family_logp_grad(X[:, :4], y, beta[:4], link="poisson")
    with pytest.raises(ValueError, match="y must be f32"):
        glm_family_logp_grad(X, y.to(torch.bfloat16), beta, link="poisson")
