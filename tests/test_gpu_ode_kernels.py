"""GPU (MI355X) tests: the native ODE kernels (ops/csrc/ode_lv.hip,
ode_poly.hip) through ODEModel, against the independent long-double
forward-sensitivity reference of tests/ode_reference.py.

Every comparison is ``|kernel - ref| <= (8 W + B) u scale`` per output
component (derivation and the measured ``W`` in ode_reference.py; premises
checked without a GPU in test_ode_reference_cpu.py).  One lost, doubled or
mis-addressed lane moves a sum by about ``scale / B``, orders above that.

Shapes are the smallest that reach each path: B around the wave (64) and
block (256) sizes, blocks holding lanes of several chains, a second trip
through each grid-stride loop, every observation layout, and polynomial
tables that exercise each branch of the table interpreter.
"""
import functools

import numpy as np
import pytest
import torch

import ode_reference as R

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.models import ODEModel
from pytensor_federated_amd.models.ode import PolynomialRHS, lotka_volterra_rhs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Per-chain long-double references of a case; computed once, read-only."""
    return tuple(R.case_reference(_case(name)))


def _np(t):
    return t.detach().cpu().numpy()


def _model(case, dev, u0=None, y_obs=None):
    f = (
        lotka_volterra_rhs
        if case["path"] == "lv"
        else PolynomialRHS(case["terms"], case["D"], case["P"])
    )
    m = ODEModel(
        f, case["u0"] if u0 is None else u0, 0.0, case["t1"], case["n_steps"], case["obs"],
        case["y_obs"] if y_obs is None else y_obs, case["sigma"], device=dev, use_kernels=True,
    )
    assert m._native_kind() == _expect_kind(case)
    return m


def _expect_kind(case):
    """"lv" / "poly" kernels; tables over the native limits take the torch path."""
    if case["table"] in R.OVER_LIMIT_NAMES:
        return None
    return case["path"]


def _single(m, case, c=0):
    """(logp_quad, grad[P]) of chain c through the single-theta entry point."""
    logp, (g,) = m.logp_grad(torch.as_tensor(case["thetas"][c]))
    const = R.logp_const(case["y_obs"].size, case["sigma"])
    g = _np(g)
    assert g.shape == (case["P"],)
    return float(logp) - const, g


def _batched(m, case, thetas=None):
    """[(logp_quad, grad[P])] per chain through the batched entry point."""
    thetas = case["thetas"] if thetas is None else thetas
    logps, G = m.logp_grad_batched(torch.as_tensor(np.ascontiguousarray(thetas.T)))
    const = R.logp_const(case["y_obs"].size, case["sigma"])
    logps, G = _np(logps), _np(G)
    assert logps.shape == (len(thetas),) and G.shape == (case["P"], len(thetas))
    return [(float(logps[c]) - const, G[:, c]) for c in range(len(thetas))]


def _assert_close(got, ref, what):
    logp, g = got
    tol_q, tol_g = R.kernel_tol(ref)
    err_q = float(abs(np.longdouble(logp) - ref["logp_quad"]))
    err_g = np.abs(g.astype(np.longdouble) - ref["grad"]).astype(np.float64)
    print(f"{what}: logp err {err_q:.3e} tol {tol_q:.3e}; grad err {err_g} tol {tol_g}")
    assert np.isfinite(logp) and np.all(np.isfinite(g)), what
    assert err_q <= tol_q, what
    assert np.all(err_g <= tol_g), what


def _assert_same(got, other, ref, what):
    """Two kernel results for one chain, held to the same bound."""
    tol_q, tol_g = R.kernel_tol(ref)
    assert abs(got[0] - other[0]) <= tol_q, what
    assert np.all(np.abs(got[1] - other[1]) <= tol_g), what


def _check_case(name, dev, per_chain_single=True):
    case = _case(name)
    m = _model(case, dev)
    assert m._native_kind() == _expect_kind(case)
    refs = _ref(name)
    if case["C"] is None:
        _assert_close(_single(m, case), refs[0], name)
        return m
    got = _batched(m, case)
    for c, ref in enumerate(refs):
        _assert_close(got[c], ref, f"{name}[chain {c}]")
    if per_chain_single:
        for c, ref in enumerate(refs):
            one = _single(m, case, c)
            _assert_close(one, ref, f"{name}[chain {c}, single]")
            _assert_same(got[c], one, ref, f"{name}[chain {c}] batched vs single")
    return m


def _slab(m, case, batched):
    """The forward kernels' states workspace as [C, n_steps+1, B, D]."""
    B, D, n = case["B"], case["D"], case["n_steps"] + 1
    C = (case["C"] or 1) if batched else 1
    if case["path"] == "poly":
        ws = m._poly_ws
    elif batched:
        ws = m._batched_ws
    else:
        ws = m._native_state[1]
    return _np(ws[: C * n * B * D]).reshape(C, n, B, D)


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", R.SINGLE_B)
@pytest.mark.parametrize("path", ["lv", "poly"])
def test_single_theta_shapes(dev, path, B):
    _check_case(f"{path}-B{B}", dev)


@pytest.mark.parametrize("B", R.SINGLE_B)
def test_lv_batched_entry_with_one_chain_shapes(dev, B):
    """The third forward/adjoint pair (k_lv_*_batched) at the single-theta
    shapes: the same inputs through logp_grad_batched with C=1."""
    name = f"lv-B{B}"
    case = _case(name)
    m = _model(case, dev)
    assert m._native_kind() == "lv"
    (got,) = _batched(m, case)
    _assert_close(got, _ref(name)[0], name + " via batched C=1")


@pytest.mark.parametrize("B,C", R.BATCHED_BC)
@pytest.mark.parametrize("path", ["lv", "poly"])
def test_batched_shapes(dev, path, B, C):
    _check_case(f"{path}-B{B}xC{C}", dev)


@pytest.mark.parametrize("name", ["lv-stride", "lv-stride-batched", "poly-stride"])
def test_second_trip_through_grid_stride_loop(dev, name):
    """More lanes than (grid cap) x 256, so some lanes are a thread's second
    iteration: 1024 blocks for the LV single kernels, 2048 for the others."""
    case = _case(name)
    cap = 1024 if name == "lv-stride" else 2048
    assert case["B"] * (case["C"] or 1) > cap * 256
    _check_case(name, dev, per_chain_single=False)


# ---------------------------------------------------------------------------
# observation layouts
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(R.OBS_LAYOUTS))
@pytest.mark.parametrize("path", ["lv", "poly"])
def test_observation_layouts(dev, path, layout):
    """Step 0 observed, last step unobserved, every step, none: the branches
    generate_ode_dataset's linspace(1, n_steps) never reaches.  Single theta
    and C=3 cover k_lv_*, k_lv_*_batched and k_poly_*."""
    for name in (f"{path}-obs_{layout}", f"{path}-obs_{layout}-C3"):
        _check_case(name, dev)
        if layout == "none":
            case = _case(name)
            assert case["y_obs"].shape == (0, 65, 2)
            m = _model(case, dev)
            got = [_single(m, case)] if case["C"] is None else _batched(m, case)
            for logp, g in got:
                assert logp == 0.0
                np.testing.assert_array_equal(g, np.zeros(4))


# ---------------------------------------------------------------------------
# polynomial tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("table", R.POLY_TABLE_NAMES)
def test_poly_tables(dev, table):
    for name in (f"table-{table}", f"table-{table}-C3"):
        m = _check_case(name, dev)
        assert m._native_kind() == "poly"


def test_poly_unreferenced_theta_has_exactly_zero_gradient(dev):
    for name, unused in (("table-unused_theta", 1), ("table-full16", 7)):
        case = _case(name)
        assert all(j != unused for _d, j, _c, _e in case["terms"])
        m = _model(case, dev)
        _logp, g = _single(m, case)
        assert g[unused] == 0.0
        case3 = _case(name + "-C3")
        for _logp, g in _batched(_model(case3, dev), case3):
            assert g[unused] == 0.0


@pytest.mark.parametrize("table", R.OVER_LIMIT_NAMES)
def test_poly_over_the_native_limits_uses_torch_path(dev, table):
    for name in (f"table-{table}", f"table-{table}-C3"):
        m = _check_case(name, dev)
        assert m._native_kind() is None


# ---------------------------------------------------------------------------
# states slab
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lv-obs_mid", "poly-obs_mid", "table-full16"])
def test_states_slab_single(dev, name):
    case = _case(name)
    m = _model(case, dev)
    _single(m, case)
    ref = _ref(name)[0]
    slab = _slab(m, case, batched=False)[0]
    err = np.abs(slab.astype(np.longdouble) - ref["states"]).astype(np.float64)
    print(f"{name}: worst state err/tol {(err / R.state_tol(ref)).max():.3f}")
    assert np.all(err <= R.state_tol(ref))


@pytest.mark.parametrize("name", ["lv-B257xC3", "poly-B257xC3", "table-full16-C3"])
def test_states_slab_batched(dev, name):
    case = _case(name)
    m = _model(case, dev)
    _batched(m, case)
    slab = _slab(m, case, batched=True)
    for c, ref in enumerate(_ref(name)):
        err = np.abs(slab[c].astype(np.longdouble) - ref["states"]).astype(np.float64)
        assert np.all(err <= R.state_tol(ref)), (name, c)


# ---------------------------------------------------------------------------
# reuse of one model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lv-reuse", "poly-reuse"])
def test_chain_count_changes_on_one_model(dev, name):
    """C=16, then 1, then 3, then a single theta on the same model: a stale
    workspace or an ``out`` that is not re-zeroed would show."""
    case = _case(name)
    refs = _ref(name)
    m = _model(case, dev)
    assert m._native_kind() == case["path"]
    for chains in (list(range(16)), [5], [9, 2, 14]):
        got = _batched(m, case, case["thetas"][chains])
        for k, c in enumerate(chains):
            _assert_close(got[k], refs[c], f"{name} C={len(chains)} chain {c}")
    _assert_close(_single(m, case, 11), refs[11], f"{name} single")


# Where the summation order is fixed, a repeated call is bit-identical: the LV
# single kernels add one block sum per block (two blocks at B=257 commute),
# the per-lane-atomic kernels are run with a single wave per chain.
@pytest.mark.parametrize(
    "name,batched", [("lv-B257", False), ("lv-B64", True), ("poly-B64", False), ("poly-B64", True)]
)
def test_same_theta_twice(dev, name, batched):
    case = _case(name)
    m = _model(case, dev)
    run = (lambda: _batched(m, case)[0]) if batched else (lambda: _single(m, case))
    a, b = run(), run()
    assert a[0] == b[0]
    _assert_same(a, b, _ref(name)[0], name)
    _assert_close(b, _ref(name)[0], name)


# ---------------------------------------------------------------------------
# aliasing: a returned gradient survives the next call
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["lv", "poly"])
def test_gradient_does_not_alias_a_reused_buffer(dev, path):
    case = _case(f"{path}-reuse")
    m = _model(case, dev)
    th = [torch.as_tensor(t) for t in case["thetas"]]
    logp1, (g1,) = m.logp_grad(th[0])
    torch.cuda.synchronize()
    snap_l, snap_g = float(logp1), _np(g1).copy()
    logp2, (g2,) = m.logp_grad(th[1])
    torch.cuda.synchronize()
    assert not np.array_equal(_np(g2), snap_g)
    assert float(logp1) == snap_l
    np.testing.assert_array_equal(_np(g1), snap_g)
    assert g1.untyped_storage().data_ptr() != g2.untyped_storage().data_ptr()


@pytest.mark.parametrize("path", ["lv", "poly"])
def test_batched_results_do_not_alias_a_reused_buffer(dev, path):
    case = _case(f"{path}-reuse")
    m = _model(case, dev)
    t1 = torch.as_tensor(np.ascontiguousarray(case["thetas"][:3].T))
    t2 = torch.as_tensor(np.ascontiguousarray(case["thetas"][3:6].T))
    logps1, G1 = m.logp_grad_batched(t1)
    torch.cuda.synchronize()
    snap_l, snap_g = _np(logps1).copy(), _np(G1).copy()
    logps2, G2 = m.logp_grad_batched(t2)
    torch.cuda.synchronize()
    assert not np.array_equal(_np(G2), snap_g)
    np.testing.assert_array_equal(_np(logps1), snap_l)
    np.testing.assert_array_equal(_np(G1), snap_g)


# ---------------------------------------------------------------------------
# layout of the inputs
# ---------------------------------------------------------------------------

def _layouts(case):
    u0, y = case["u0"], case["y_obs"]
    y_perm = torch.as_tensor(np.ascontiguousarray(y.transpose(1, 0, 2))).permute(1, 0, 2)
    assert not y_perm.is_contiguous() and tuple(y_perm.shape) == y.shape
    u0_f, y_f = np.asfortranarray(u0), np.asfortranarray(y)
    assert not y_f.flags.c_contiguous
    return {"fortran_numpy": (u0_f, y_f), "permuted_torch": (torch.as_tensor(u0), y_perm)}


# B=64: one block on the LV single path, one wave per chain elsewhere, so the
# summation order is fixed and equal inputs give equal bits.
@pytest.mark.parametrize("variant", ["fortran_numpy", "permuted_torch"])
@pytest.mark.parametrize("name", ["lv-B64", "poly-B64"])
def test_non_contiguous_inputs_match_contiguous_copies(dev, name, variant):
    case = _case(name)
    u0, y = _layouts(case)[variant]
    m = _model(case, dev, u0=u0, y_obs=y)
    base = _model(case, dev)
    assert m._native_kind() == case["path"]
    assert m._u0.is_contiguous() and m._y.is_contiguous()
    ref = _ref(name)[0]
    got, want = _single(m, case), _single(base, case)
    np.testing.assert_array_equal(
        _slab(m, case, batched=False), _slab(base, case, batched=False)
    )
    _assert_close(got, ref, f"{name} {variant}")
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    (got_b,), (want_b,) = _batched(m, case), _batched(base, case)
    _assert_close(got_b, ref, f"{name} {variant} batched")
    assert got_b[0] == want_b[0]
    np.testing.assert_array_equal(got_b[1], want_b[1])
