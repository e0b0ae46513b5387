"""GPU (MI355X) tests: HIP kernels vs fp64 numpy on exactly representable
probes, at the smallest shapes where the kernels take another path.

The inputs come from tests/exact_probes.py: every intermediate is exact, so
the comparison is bit-tight (``assert_array_equal``, or ``atol = N * 2^-40``
where the 2^-46 saturation remainders enter) and one lost, doubled or
mis-addressed row / column / chain shows as a whole unit.  The premises are
checked without a GPU in test_exact_probes_cpu.py.
"""
import numpy as np
import pytest
import torch

import exact_probes as ep

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.models import GaussianLinearModel, LogisticGLMModel

BATCHED_ENV = (
    "FED_BATCHED_V3",
    "FED_BATCHED_GRID", "FED_V3_NT",
)

#: id -> (K, kernel-selection switches); read by getenv on every call
BATCHED_VARIANTS = {
    "v3tr_k1024": (1024, {}),                         # default: v3, tr image
    "v2_k1024": (1024, {"FED_BATCHED_V3": "0"}),
    "v2_k512": (512, {}),                             # default at K=512
    "v3s_k512": (512, {"FED_BATCHED_V3": "1"}),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _select(monkeypatch, switches, grid=None):
    for name in BATCHED_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    if grid is not None:
        monkeypatch.setenv("FED_BATCHED_GRID", str(grid))


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------
# batched logistic (MFMA kernels)
# ---------------------------------------------------------------------------

def _batched_model(dev, probe, n, K):
    p = ep.LOGISTIC_PROBES[probe](n, K)
    # torch.tensor copies: the cached probe arrays are read-only
    m = LogisticGLMModel(
        torch.tensor(p["X"]), torch.tensor(p["y"]), device=dev, dtype=torch.bfloat16,
        use_kernels=True,
    )
    assert m._k_pad == 0 and m._kernel_path()
    theta = torch.tensor(p["theta"], dtype=torch.float32)
    return m, theta


def _check_batched(m, theta, probe, n, K, what=""):
    ref = ep.batched_reference(probe, n, K)
    logp, G = m.logp_grad_batched(theta)
    logp, G = _np(logp), _np(G)
    msg = f"{probe} N={n} K={K} {what}"
    assert logp.shape == (ep.BCH,) and G.shape == (K, ep.BCH)
    if probe == "zero_theta":
        np.testing.assert_array_equal(G, ref["G"], err_msg=msg)
        np.testing.assert_allclose(logp, ref["logp"], rtol=1e-6, atol=0, err_msg=msg)
    else:
        atol = ep.saturation_atol(n)
        np.testing.assert_allclose(G, ref["G"], rtol=0, atol=atol, err_msg=msg)
        np.testing.assert_allclose(logp, ref["logp"], rtol=0, atol=atol, err_msg=msg)


@pytest.mark.parametrize("n", ep.BATCHED_N)
@pytest.mark.parametrize("variant", sorted(BATCHED_VARIANTS))
def test_batched_edge_rows(dev, monkeypatch, variant, n):
    """N below, at and above one and two row tiles, every tail length that
    changes how a tile is staged -- default grid (one or two blocks)."""
    K, switches = BATCHED_VARIANTS[variant]
    _select(monkeypatch, switches)
    for probe in sorted(ep.LOGISTIC_PROBES):
        m, theta = _batched_model(dev, probe, n, K)
        _check_batched(m, theta, probe, n, K, variant)


@pytest.mark.parametrize("n", ep.BATCHED_DEEP_N)
@pytest.mark.parametrize("variant", sorted(BATCHED_VARIANTS))
def test_batched_deep_pipeline(dev, monkeypatch, variant, n):
    """16 blocks with several tiles each: full pipelines, a block that ends
    on the tail tile, the tail tile as a prefetch, and empty blocks."""
    K, switches = BATCHED_VARIANTS[variant]
    _select(monkeypatch, switches, grid=16)
    for probe in sorted(ep.LOGISTIC_PROBES):
        m, theta = _batched_model(dev, probe, n, K)
        _check_batched(m, theta, probe, n, K, variant)


@pytest.mark.parametrize("n", ep.STALE_N)
@pytest.mark.parametrize("variant", sorted(BATCHED_VARIANTS))
def test_batched_after_larger_problem(dev, monkeypatch, variant, n):
    """The same small model evaluated again after a larger problem has left
    non-zero leftovers in the shared workspace slab and in LDS."""
    K, switches = BATCHED_VARIANTS[variant]
    grid = 16 if n in ep.BATCHED_DEEP_N else None
    for probe in sorted(ep.LOGISTIC_PROBES):
        _select(monkeypatch, switches, grid=grid)
        m, theta = _batched_model(dev, probe, n, K)
        _check_batched(m, theta, probe, n, K, variant + " first call")
        _select(monkeypatch, switches)  # larger problem on the default grid
        big, big_theta = _batched_model(dev, "dense_int", ep.STALE_BIG_N, K)
        _check_batched(big, big_theta, "dense_int", ep.STALE_BIG_N, K, variant + " big")
        _select(monkeypatch, switches, grid=grid)
        _check_batched(m, theta, probe, n, K, variant + " after big")


# ---------------------------------------------------------------------------
# single-chain logistic
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", ep.SINGLE_N)
@pytest.mark.parametrize("dtype,K", ep.SINGLE_COMBOS)
def test_single_chain_edge_rows(dev, dtype, K, n):
    """Odd tail row alone, one pair, pair + tail, fewer rows than one
    block's waves, an odd N over many blocks -- in every instantiation the
    existing suite leaves out."""
    tdtype = getattr(torch, dtype)
    for probe in ("onehot", "zero_theta"):
        p = ep.LOGISTIC_PROBES[probe](n, K)
        ref = ep.single_reference(probe, n, K)
        m = LogisticGLMModel(
            torch.tensor(p["X"]), torch.tensor(p["y"]), device=dev, dtype=tdtype, use_kernels=True
        )
        assert m._k_pad == 0 and m._kernel_path()
        beta = torch.tensor(p["theta"][:, 0], dtype=torch.float32)
        logp, (g,) = m.logp_grad(beta)
        logp, g = float(logp), _np(g)
        msg = f"{probe} {dtype} N={n} K={K}"
        assert g.shape == (K,)
        if probe == "zero_theta":
            np.testing.assert_array_equal(g, ref["G"], err_msg=msg)
            np.testing.assert_allclose(logp, ref["logp"][0], rtol=1e-6, atol=0, err_msg=msg)
        else:
            atol = ep.saturation_atol(n)
            np.testing.assert_allclose(g, ref["G"], rtol=0, atol=atol, err_msg=msg)
            np.testing.assert_allclose(logp, ref["logp"][0], rtol=0, atol=atol, err_msg=msg)


# ---------------------------------------------------------------------------
# gaussian linear (fused single-launch kernel)
# ---------------------------------------------------------------------------

def _gauss_cases():
    for dtype in sorted(ep.GAUSS_VEC):
        for n in ep.gaussian_sizes(dtype):
            yield pytest.param(dtype, n, id=f"{dtype}-{n}")


@pytest.mark.parametrize("dtype,n", list(_gauss_cases()))
def test_gaussian_dyadic_exact(dev, dtype, n):
    """n < VEC (scalar tail only), grids 1, 2, 2 (rounded down from 3), 4
    and 16; 5 rounds x 2 thetas x 2 entry points on ONE instance walk the
    monotonic arrival tickets through several wraps of the group size."""
    p = ep.gaussian_probe(n)
    m = GaussianLinearModel(
        torch.tensor(p["x"]), torch.tensor(p["y"]), sigma=1.0, device=dev,
        dtype=getattr(torch, dtype), use_kernels=True,
    )
    refs = [ep.gaussian_reference(p["x"], p["y"], a, b) for a, b in ep.GAUSS_THETAS]
    for rnd in range(5):
        for (a, b), (logp_r, ga_r, gb_r) in zip(ep.GAUSS_THETAS, refs):
            logp, (ga, gb) = m(a, b)
            got = [(float(logp), float(ga), float(gb)), tuple(m.logp_grad_sync(a, b))]
            for path, (logp_k, ga_k, gb_k) in zip(("call", "sync"), got):
                msg = f"{dtype} n={n} round {rnd} {path} a={a} b={b}"
                assert ga_k == ga_r, f"{msg}: d/da {ga_k!r} != {ga_r!r}"
                assert gb_k == gb_r, f"{msg}: d/db {gb_k!r} != {gb_r!r}"
                assert abs(logp_k - logp_r) <= 2 * np.spacing(abs(logp_r)), (
                    f"{msg}: logp {logp_k!r} vs {logp_r!r}"
                )
