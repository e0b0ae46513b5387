"""Premises of the ODE kernel tests, checked without a GPU.

* the long-double reference (tests/ode_reference.py) really is extended
  precision, and its own float64 instance stays within the measured ``W``;
* the tolerance the GPU tests hold the kernels to is one that honest float64
  code meets: the torch path of ODEModel on the CPU stays inside it;
* the cases are tame (finite, states within [1e-3, 1e3]);
* ODEModel's constructor and theta-size validation, and the contiguity of the
  buffers whose pointers the kernels receive.  All of these act before the
  native/eager split, so they need no GPU.
"""
import functools

import numpy as np
import pytest
import torch

import ode_reference as R
from pytensor_federated_amd.models import ODEModel
from pytensor_federated_amd.models.ode import PolynomialRHS, lotka_volterra_rhs

SMALL = R.small_case_names(4096)


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.case_reference(_case(name))


def _model(case, **kw):
    f = (
        lotka_volterra_rhs
        if case["path"] == "lv"
        else PolynomialRHS(case["terms"], case["D"], case["P"])
    )
    return ODEModel(
        f, case["u0"], 0.0, case["t1"], case["n_steps"], case["obs"], case["y_obs"],
        case["sigma"], **kw,
    )


def test_longdouble_is_extended_precision():
    """Where long double is plain double the reference proves nothing."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_case_list_is_the_issue_list():
    assert set(SMALL) == set(R.CASES) - {"lv-stride", "lv-stride-batched", "poly-stride"}
    for table in R.POLY_TABLE_NAMES:
        terms, D, P = R.TABLES[table]
        assert PolynomialRHS(terms, D, P).native_ok(), table
    for table in R.OVER_LIMIT_NAMES:
        terms, D, P = R.TABLES[table]
        assert not PolynomialRHS(terms, D, P).native_ok(), table
    for c in R.CASES.values():
        assert c["n_steps"] <= 8 and R.STEP <= 0.25


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_is_tame(name):
    case = _case(name)
    assert 0.2 <= case["thetas"].min() and case["thetas"].max() <= 1.0
    assert case["h"] <= 0.25
    for ref in _ref(name):
        s = ref["states"]
        assert np.all(np.isfinite(s))
        assert 1e-3 <= s.min() and s.max() <= 1e3
        assert np.all(np.isfinite(ref["G"])) and np.all(np.isfinite(ref["q"]))


@pytest.mark.parametrize("name", SMALL)
def test_float64_reference_within_w(name):
    """The measured W as a regression check: the reference alone, run in
    float64, stays within ``W u scale`` of its long-double instance."""
    case = _case(name)
    for r64, ref in zip(R.case_reference(case, np.float64), _ref(name)):
        w = R.w_of(r64, ref)
        print(f"{name}: W = {w:.2f}")
        assert w <= R.W
        # and so do the sums the kernels are compared on
        s_q, s_g = R.scales(ref)
        assert abs(np.longdouble(r64["logp_quad"]) - ref["logp_quad"]) <= R.W * R.U * s_q
        assert np.all(np.abs(r64["grad"].astype(np.longdouble) - ref["grad"]) <= R.W * R.U * s_g)


@pytest.mark.parametrize("name", SMALL)
def test_torch_path_meets_kernel_tolerance(name):
    """Honest float64 code (the torch adjoint sweep, on the CPU) meets the
    bound the kernels are held to."""
    case = _case(name)
    m = _model(case, use_kernels=False)
    assert m._native_kind() is None
    const = R.logp_const(case["y_obs"].size, case["sigma"])
    if case["C"] is None:
        logp, (g,) = m.logp_grad(torch.as_tensor(case["thetas"][0]))
        got = [(float(logp), g.numpy())]
    else:
        logps, G = m.logp_grad_batched(torch.as_tensor(case["thetas"].T.copy()))
        got = [(float(logps[c]), G[:, c].numpy()) for c in range(case["C"])]
    for (logp, g), ref in zip(got, _ref(name)):
        tol_q, tol_g = R.kernel_tol(ref)
        err_q = abs(np.longdouble(logp - const) - ref["logp_quad"])
        err_g = np.abs(g.astype(np.longdouble) - ref["grad"])
        print(f"{name}: logp err/tol {float(err_q)}/{tol_q}, grad err/tol {err_g}/{tol_g}")
        assert err_q <= tol_q
        assert np.all(err_g <= tol_g)


# ---------------------------------------------------------------------------
# constructor validation
# ---------------------------------------------------------------------------

def _args(n_steps=6, B=5, D=2, obs=(2, 4, 6)):
    rng = np.random.RandomState(3)
    u0 = rng.uniform(0.5, 1.5, size=(B, D))
    y = rng.uniform(0.5, 1.5, size=(len(obs), B, D))
    return u0, list(obs), y


@pytest.mark.parametrize(
    "obs",
    [
        (2, 2, 6),     # duplicate
        (4, 2, 6),     # unsorted
        (-1, 2, 6),    # negative: would wrap to the last step
        (2, 4, 7),     # beyond n_steps
    ],
)
def test_obs_indices_must_be_strictly_ascending_in_range(obs):
    u0, _, y = _args()
    with pytest.raises(ValueError, match="obs_indices"):
        ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, list(obs), y, 0.1)


def test_obs_indices_bounds_are_inclusive():
    u0, _, y = _args(obs=(0, 3, 6))
    ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, [0, 3, 6], y, 0.1)


@pytest.mark.parametrize(
    "shape",
    [
        (2, 5, 2),   # fewer rows than obs_indices
        (4, 5, 2),   # more rows
        (3, 4, 2),   # another B
        (3, 5, 3),   # another D
        (3, 10),     # flattened
    ],
)
def test_y_obs_shape_is_checked(shape):
    u0, obs, _ = _args()
    with pytest.raises(ValueError, match="y_obs"):
        ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, obs, np.ones(shape), 0.1)


def test_y_obs_shape_follows_obs_components():
    u0, obs, y = _args()
    ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, obs, y[..., :1], 0.1, obs_components=[1])
    with pytest.raises(ValueError, match="y_obs"):
        ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, obs, y, 0.1, obs_components=[1])


@pytest.mark.parametrize("shape", [(2,), (5, 2, 1), ()])
def test_u0_must_be_2d(shape):
    _, obs, y = _args()
    with pytest.raises(ValueError, match="u0"):
        ODEModel(lotka_volterra_rhs, np.ones(shape), 0.0, 1.0, 6, obs, y, 0.1)


@pytest.mark.parametrize("size", [0, 3, 5])
def test_lv_theta_size_is_checked(size):
    u0, obs, y = _args()
    m = ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, obs, y, 0.1)
    with pytest.raises(ValueError, match="theta"):
        m.logp_grad(torch.full((size,), 0.5, dtype=torch.float64))
    with pytest.raises(ValueError, match="theta"):
        m.logp_grad_batched(torch.full((size, 2), 0.5, dtype=torch.float64))


@pytest.mark.parametrize("size", [1, 3])
def test_poly_theta_size_is_checked(size):
    rng = np.random.RandomState(4)
    u0 = rng.uniform(0.5, 1.5, size=(5, 3))
    y = rng.uniform(0.5, 1.5, size=(2, 5, 3))
    m = ODEModel(PolynomialRHS.sir(), u0, 0.0, 1.0, 6, [3, 6], y, 0.1)
    with pytest.raises(ValueError, match="theta"):
        m.logp_grad(torch.full((size,), 0.5, dtype=torch.float64))
    with pytest.raises(ValueError, match="theta"):
        m.logp_grad_batched(torch.full((size, 2), 0.5, dtype=torch.float64))
    m.logp_grad(torch.full((2,), 0.5, dtype=torch.float64))


def test_right_sized_theta_passes_tensor_and_numpy_edge():
    u0, obs, y = _args()
    m = ODEModel(lotka_volterra_rhs, u0, 0.0, 1.0, 6, obs, y, 0.1)
    a, (ga,) = m.logp_grad(torch.full((4,), 0.5, dtype=torch.float64))
    b, (gb,) = m(np.full(4, 0.5))
    assert float(a) == float(b)
    np.testing.assert_array_equal(ga.numpy(), gb)


# ---------------------------------------------------------------------------
# layout: what the kernels get pointers to is C-contiguous
# ---------------------------------------------------------------------------

def _layout_variants():
    case = _case("lv-obs_mid")
    u0, y = case["u0"], case["y_obs"]
    y_perm = torch.as_tensor(np.ascontiguousarray(y.transpose(1, 0, 2))).permute(1, 0, 2)
    assert not y_perm.is_contiguous() and tuple(y_perm.shape) == y.shape
    return case, {
        "fortran_numpy": (np.asfortranarray(u0), np.asfortranarray(y)),
        "permuted_torch": (torch.as_tensor(u0).t().contiguous().t(), y_perm),
    }


@pytest.mark.parametrize("variant", ["fortran_numpy", "permuted_torch"])
def test_inputs_are_made_contiguous(variant):
    case, variants = _layout_variants()
    u0, y = variants[variant]
    m = ODEModel(lotka_volterra_rhs, u0, 0.0, case["t1"], case["n_steps"], case["obs"], y,
                 case["sigma"])
    assert m._u0.is_contiguous() and m._y.is_contiguous()
    np.testing.assert_array_equal(m._u0.numpy(), case["u0"])
    np.testing.assert_array_equal(m._y.numpy(), case["y_obs"])
    base = _model(case)
    theta = torch.as_tensor(case["thetas"][0])
    logp, (g,) = m.logp_grad(theta)
    logp0, (g0,) = base.logp_grad(theta)
    assert float(logp) == float(logp0)
    np.testing.assert_array_equal(g.numpy(), g0.numpy())
