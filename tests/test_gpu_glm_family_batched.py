"""GPU (MI355X) tests of the batched GLM family kernel
(csrc/glm_family_batched.hip) and of the Poisson / Gaussian GLM models'
``logp_grad_batched`` on it.

Exact probes (tests/glm_batched_probes.py): operands exact as three bf16
pieces and every intermediate exactly representable, so all 16 chains are
compared with fp64 numpy bit-tight at every K of the kernel, at the row
counts where a 16-row fragment, a wave's 32 rows, a tile or the block's
tile loop ends.  The premises are checked without a GPU in
test_glm_batched_probes_cpu.py.

Accuracy sets: glm_probes.accuracy_case data with 16 scaled copies of beta,
within ``BATCHED_M * 2^-24 * sum |row contribution|`` of fp64 numpy.
"""
import warnings

import numpy as np
import pytest
import torch

import glm_batched_probes as bp
import glm_probes as gp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel
from pytensor_federated_amd.ops import (
    GLM_FAMILY_BATCHED_K,
    glm_family_logp_grad_batched,
    require_kernels,
    split_bf16x3,
)

BCH = bp.BCH
PROBES = sorted(bp.EXACT_PROBES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_grid(monkeypatch):
    monkeypatch.delenv("FED_GLM_BATCHED_GRID", raising=False)
    monkeypatch.delenv("FED_GLM_GRID", raising=False)


def _np(t):
    return t.detach().cpu().numpy()


def _eval(dev, probe, n, K):
    link, build, _, sigma, _ = bp.EXACT_PROBES[probe]
    p = build(n, K)
    X = torch.tensor(p["X"], dtype=torch.bfloat16, device=dev)
    y = torch.tensor(p["y"], dtype=torch.float32, device=dev)
    offset = p.get("offset")
    if offset is not None:
        offset = torch.tensor(offset, dtype=torch.float32, device=dev)
    theta = torch.tensor(p["theta"], dtype=torch.float32)
    return lambda: glm_family_logp_grad_batched(
        X, y, theta, link=link, offset=offset, sigma=sigma, logp_const=bp.PROBE_CONST
    )


def _check(call, probe, n, K, what):
    logp_ref, G_ref = bp.exact_reference(probe, n, K)
    logp, G = call()
    logp, G = _np(logp), _np(G)
    msg = f"{probe} N={n} K={K} {what}"
    assert logp.shape == (BCH,) and G.shape == (K, BCH)
    np.testing.assert_array_equal(G, G_ref, err_msg=msg)
    if bp.EXACT_PROBES[probe][4]:
        np.testing.assert_array_equal(logp, logp_ref, err_msg=msg)
    else:
        np.testing.assert_allclose(logp, logp_ref, rtol=bp.WIDE_LOGP_RTOL, atol=0, err_msg=msg)


def test_kernel_sizes_match_the_probe_module():
    assert tuple(GLM_FAMILY_BATCHED_K) == bp.BATCHED_K


# ---------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("K", bp.BATCHED_K)
def test_batched_exact_edge_rows(dev, K, probe):
    """One row, around a 16-row fragment, a wave's 32 rows, 64 rows and the
    tile T (one short, exactly, one past), and two tiles plus a row; each
    evaluated twice on the same workspace."""
    for n in bp.edge_rows(K):
        if not bp.probe_applies(probe, n, K):
            continue
        call = _eval(dev, probe, n, K)
        _check(call, probe, n, K, "first call")
        _check(call, probe, n, K, "second call")


@pytest.mark.parametrize(
    "K,probe",
    [(K, probe) for K in bp.BATCHED_K for probe in PROBES
     if bp.probe_applies(probe, bp.deep_rows(K), K)],
)
def test_batched_two_trips(dev, monkeypatch, K, probe):
    """5T+5 rows on two blocks: three tiles each, the last ragged by five
    rows.  (The default grid never exceeds the tile count, so there are no
    empty blocks to test; the wide probe is left out at K = 8 and 16, where
    these rows would sum more than 32 per column.)"""
    n = bp.deep_rows(K)
    monkeypatch.setenv("FED_GLM_BATCHED_GRID", str(bp.DEEP_GRID))
    call = _eval(dev, probe, n, K)
    _check(call, probe, n, K, f"grid={bp.DEEP_GRID}")
    _check(call, probe, n, K, f"grid={bp.DEEP_GRID} again")


@pytest.mark.parametrize("probe", ["poisson_dense", "poisson_zero_beta", "gaussian_sigma2"])
@pytest.mark.parametrize("K", bp.BATCHED_K)
def test_batched_after_larger_problem(dev, K, probe):
    """The same small problem evaluated again after a larger one of the
    same K has left non-zero leftovers in the workspace slab and in LDS."""
    n, big = bp.stale_small_rows(K), bp.stale_big_rows(K)
    small_call = _eval(dev, probe, n, K)
    big_call = _eval(dev, probe, big, K)
    _check(small_call, probe, n, K, "before")
    _check(big_call, probe, big, K, "big")
    _check(small_call, probe, n, K, "after big")


# ---------------------------------------------------------------------------
# accuracy where exp matters (model level; K = 100 is zero-padded to 128)
# ---------------------------------------------------------------------------

def _worst_ratios(cases, logp, G):
    ratios = [gp.accuracy_ratios(cases[b], float(logp[b]), G[:, b]) for b in range(BCH)]
    return max(r[0] for r in ratios), max(r[1] for r in ratios)


@pytest.mark.parametrize("K", gp.ACC_K)
@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_batched_kernel_accuracy(dev, family, K):
    theta, cases = bp.accuracy_chains(family, K)
    m = gp.accuracy_model(family, "bfloat16", K, device=dev, use_kernels=True)
    assert m._batched_kernel_path() and m._k_eff == {8: 8, 100: 128, 512: 512}[K]
    logp, G = m.logp_grad_batched(torch.tensor(theta))
    assert logp.shape == (BCH,) and G.shape == (K, BCH)
    r_logp, r_grad = _worst_ratios(cases, _np(logp), _np(G))
    print(f"\n{family} bf16 K={K}: batched kernel worst logp ratio {r_logp:.4f}, "
          f"worst grad ratio {r_grad:.4f} over 16 chains (allowed {bp.BATCHED_M})")
    assert r_logp <= bp.BATCHED_M
    assert r_grad <= bp.BATCHED_M


@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_batched_against_single_chain_kernel(dev, family):
    K = 100
    theta, cases = bp.accuracy_chains(family, K)
    m = gp.accuracy_model(family, "bfloat16", K, device=dev, use_kernels=True)
    logp, G = m.logp_grad_batched(torch.tensor(theta))
    logp, G = _np(logp), _np(G)
    bound = (gp.KERNEL_M + bp.BATCHED_M) * 2.0 ** -24
    for b in range(BCH):
        lb, (gb,) = m.logp_grad(torch.tensor(theta[:, b]))
        assert abs(float(lb) - logp[b]) <= bound * cases[b]["logp_scale"], b
        assert np.all(np.abs(_np(gb) - G[:, b]) <= bound * cases[b]["G_scale"]), b


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

def _gaussian_probe_model(dev, n, K, sigma, rows=slice(None)):
    p = gp.gaussian_sparse_probe(n, K, sigma)
    m = GaussianGLMModel(torch.tensor(p["X"][rows]), torch.tensor(p["y"][rows]), sigma,
                         device=dev, dtype=torch.bfloat16, use_kernels=True)
    return p, m


def _gaussian_const(n, sigma):
    return -0.5 * n * np.log(2 * np.pi * sigma * sigma)


@pytest.mark.parametrize("B", [1, 5, 16, 17, 33])
def test_model_any_number_of_chains(dev, B):
    """Chains go through the kernel in groups of 16, the last group padded:
    the shapes are [B] and [K, B], equal theta columns give equal result
    columns in whichever group they land, and every column is the exact
    answer."""
    n, K, sigma = 150, 20, 2.0  # padded to 32
    p, m = _gaussian_probe_model(dev, n, K, sigma)
    assert m._k_eff == 32 and m._batched_kernel_path()
    base = np.random.RandomState(7).randint(-8, 9, size=(K, 3)) / 4.0
    theta = base[:, np.arange(B) % 3]
    logp, G = m.logp_grad_batched(torch.tensor(theta))
    assert logp.shape == (B,) and G.shape == (K, B)
    assert logp.dtype == torch.float64 and G.dtype == torch.float64
    logp, G = _np(logp), _np(G)
    logp_ref, G_ref = bp.gaussian_reference(p["X"], p["y"], theta, sigma)
    np.testing.assert_array_equal(G, G_ref)
    np.testing.assert_allclose(logp, logp_ref + _gaussian_const(n, sigma), rtol=1e-14)
    for b in range(B):
        np.testing.assert_array_equal(G[:, b], G[:, b % 3])
        # logp: the blocks' fp64 sums meet in atomics, in any order
        np.testing.assert_allclose(logp[b], logp[b % 3], rtol=1e-14)


def _lgamma_const(y):
    return -float(torch.sum(torch.lgamma(torch.tensor(np.asarray(y)) + 1.0)))


@pytest.mark.parametrize("K", [20, 100])
def test_model_padding_and_offset(dev, K):
    """K = 20 is padded to 32 and K = 100 to 128; G comes back as [K, B].
    The same shard with and without its offset."""
    n, B = 201, 16
    p = gp.poisson_zero_beta_probe(n, K)
    X, y = torch.tensor(p["X"]), torch.tensor(p["y"])
    kw = dict(device=dev, dtype=torch.bfloat16, use_kernels=True)
    with_off = PoissonGLMModel(X, y, offset=torch.tensor(p["offset"]), **kw)
    without = PoissonGLMModel(X, y, **kw)
    const = _lgamma_const(p["y"])
    theta = np.zeros((K, B))
    for m, offset in ((with_off, p["offset"]), (without, None)):
        assert m._k_eff == {20: 32, 100: 128}[K] and m._batched_kernel_path()
        logp_ref, G_ref = bp.poisson_flushed_reference(p["X"], p["y"], theta, offset)
        logp, G = m.logp_grad_batched(torch.tensor(theta))
        assert G.shape == (K, B)
        np.testing.assert_array_equal(_np(G), G_ref)
        np.testing.assert_allclose(_np(logp), logp_ref + const, rtol=1e-14)
    l_with = _np(with_off.logp_grad_batched(torch.tensor(theta))[0])
    l_without = _np(without.logp_grad_batched(torch.tensor(theta))[0])
    assert np.all(l_with != l_without)  # rows at -128 drop their exp(z) = 1


def test_half_shards_add_up_through_the_batched_kernel(dev):
    n, K, sigma = 333, 40, 2.0  # padded to 64; halves of 166 and 167 rows
    theta = torch.tensor(np.random.RandomState(3).randint(-8, 9, size=(K, BCH)) / 4.0)
    parts = [_gaussian_probe_model(dev, n, K, sigma, rows=r)[1]
             for r in (slice(None), slice(0, 166), slice(166, None))]
    (lw, Gw), (la, Ga), (lb, Gb) = [m.logp_grad_batched(theta) for m in parts]
    np.testing.assert_array_equal(_np(Ga) + _np(Gb), _np(Gw))
    np.testing.assert_allclose(_np(la) + _np(lb), _np(lw), rtol=1e-14)


def test_overflowing_chain_is_alone(dev):
    """A Poisson chain with z > 88 has exp(z) = inf in fp32: its logp is
    -inf.  The other 15 chains are untouched."""
    n, K, bad = 77, 16, 5
    p = bp.poisson_saturated("dense", n, K)
    m = PoissonGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), device=dev,
                        dtype=torch.bfloat16, use_kernels=True)
    theta = np.array(p["theta"])
    logp0, G0 = m.logp_grad_batched(torch.tensor(theta))
    theta[:, bad] = 128.0  # every row has a non-zero: z >= 128
    logp1, G1 = m.logp_grad_batched(torch.tensor(theta))
    logp0, G0, logp1, G1 = _np(logp0), _np(G0), _np(logp1), _np(G1)
    assert logp1[bad] == -np.inf and not np.all(np.isfinite(G1[:, bad]))
    keep = np.arange(BCH) != bad
    assert np.all(np.isfinite(logp1[keep])) and np.all(np.isfinite(G1[:, keep]))
    np.testing.assert_array_equal(logp1[keep], logp0[keep])
    np.testing.assert_array_equal(G1[:, keep], G0[:, keep])


def test_model_falls_back_with_a_warning_at_2048(dev):
    n, K = 5, 1100  # bf16: padded to 2048, which the batched kernel does not cover
    rng = np.random.RandomState(0)
    X, y = rng.standard_normal((n, K)) / 40, rng.standard_normal(n)
    m = GaussianGLMModel(X, y, 1.0, device=dev, dtype=torch.bfloat16)
    assert m._k_eff == 2048
    theta = torch.tensor(rng.standard_normal((K, 3)) / 8)
    with pytest.warns(UserWarning, match="batched GLM family kernel not compiled"):
        logp, G = m.logp_grad_batched(theta)
    logp_e, G_e = m._logp_grad_batched_eager(theta)
    assert G.shape == (K, 3)
    assert torch.equal(logp, logp_e) and torch.equal(G, G_e)


def test_f32_shard_takes_the_eager_path_silently(dev):
    n, K = 50, 16
    p = gp.gaussian_sparse_probe(n, K, 1.0)
    m = GaussianGLMModel(torch.tensor(p["X"]), torch.tensor(p["y"]), 1.0, device=dev,
                         dtype=torch.float32)
    theta = torch.tensor(np.random.RandomState(1).randint(-8, 9, size=(K, BCH)) / 4.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not m._batched_kernel_path()
        logp, G = m.logp_grad_batched(theta)
    logp_e, G_e = m._logp_grad_batched_eager(theta)
    assert torch.equal(logp, logp_e) and torch.equal(G, G_e)


# ---------------------------------------------------------------------------
# entry-point errors (all returned before anything is launched)
# ---------------------------------------------------------------------------

def test_batched_entry_point_return_codes(dev):
    lib = require_kernels()
    n, K = 4, 8
    X = torch.zeros((n, K), dtype=torch.bfloat16, device=dev)
    y = torch.zeros(n, dtype=torch.float32, device=dev)
    theta = torch.zeros((K, BCH), dtype=torch.float32, device=dev)
    pieces = split_bf16x3(theta)
    out = torch.zeros(BCH + K * BCH, dtype=torch.float64, device=dev)
    ws = torch.zeros(4 * K * BCH, dtype=torch.float32, device=dev)  # one block's 4 slab rows
    stream = torch.cuda.current_stream().cuda_stream

    def call(K=K, link=0, ws_bytes=ws.numel() * 4):
        return lib.fed_glm_family_batched(
            X.data_ptr(), y.data_ptr(), None, n, K, pieces.data_ptr(), link, 1.0, 0.0,
            out.data_ptr(), ws.data_ptr(), ws_bytes, stream,
        )

    assert call() == 0
    assert call(ws_bytes=ws.numel() * 4 - 1) == -3
    for bad_k in (0, 4, 12, 24, 2048, 4096):
        assert call(K=bad_k) == -4, bad_k
    assert call(link=2) == -5 and call(link=3) == -5 and call(link=-1) == -5
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="unknown link"):
        glm_family_logp_grad_batched(X, y, theta, link="logistic")
    with pytest.raises(ValueError, match="not compiled"):
        glm_family_logp_grad_batched(X[:, :4], y, theta[:4], link="poisson")
    with pytest.raises(TypeError, match="bf16"):
        glm_family_logp_grad_batched(X.float(), y, theta, link="poisson")
    with pytest.raises(ValueError, match="y must be f32"):
        glm_family_logp_grad_batched(X, y.to(torch.bfloat16), theta, link="poisson")
    with pytest.raises(ValueError, match="theta must be"):
        glm_family_logp_grad_batched(X, y, theta[:, :8], link="poisson")
