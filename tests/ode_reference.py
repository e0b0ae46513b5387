"""Independent high-precision reference for the ODE logp+grad kernels, and the
deterministic cases the ODE tests share.

Plain numpy, no torch.  The kernels (ops/csrc/ode_lv.hip, ode_poly.hip) and the
torch path (models/ode.py) both obtain the gradient by the discrete ADJOINT:
one forward sweep, then vector-Jacobian products backward.  This module gets
the same discretised quantity by FORWARD SENSITIVITIES instead: it integrates
``u[B, D]`` and ``S = du/dtheta [B, D, P]`` together through RK4, each stage
being ``f(u)`` and ``J_u(u) . S + J_theta(u)`` with both Jacobians formed
explicitly from the term table, and at an observed step accumulates
``-1/2 sigma^-2 sum r^2`` and ``sigma^-2 r^T S``.  It shares no code and no
derivation with the autograd adjoint or the hand-written VJPs.

Everything is elementwise ``+ - *`` (powers by repeated multiplication, no
einsum, no libm), so a given dtype gives the same numbers on every platform.

Tolerance (see ``kernel_tol``).  For an output component with per-experiment
contributions ``c_b`` let ``scale = sum_b |c_b|`` and ``u = 2^-53``; a kernel
result must satisfy ``|kernel - ref| <= (8 W + B) u scale``:

* ``B u scale`` is the first-order worst case of summing B terms in any order
  (the kernels sum by wave shuffle plus atomics);
* ``W`` is measured: the worst error of this module's own float64 instance
  against its long-double instance, per-lane values, summed over the lanes of
  a component and taken in units of ``u scale`` (for the trajectory: per
  element in units of ``u max(1, |state|)``), over every case in ``CASES``;
* 8 is the margin a kernel gets over honest float64 code for contracting
  FMAs, ``ipow`` by repeated multiplication and another association of
  ``(h/6) (...)``.

``W`` was produced by ``python tests/ode_reference.py`` (prints the worst
figure per case and the maximum); the constant is that maximum rounded up to
the next integer.  test_ode_reference_cpu.py holds every small case to it.
"""
import zlib

import numpy as np

__all__ = [
    "W", "U", "CASES", "TABLES", "LV_TERMS", "make_case", "reference", "reference_chains",
    "kernel_tol", "state_tol", "logp_const",
]

#: measured (see module docstring): max over CASES was 75.52, in "poly-B1xC16"
#: (one lane, so a gradient component that cancels inside the lane has
#: nothing to hide behind); cases with B >= 63 stay below 12
W = 76.0
U = 2.0 ** -53

LV_TERMS = [
    (0, 0, 1.0, (1, 0)),   # +alpha * prey
    (0, 1, -1.0, (1, 1)),  # -beta  * prey * pred
    (1, 3, 1.0, (1, 1)),   # +delta * prey * pred
    (1, 2, -1.0, (0, 1)),  # -gamma * pred
]


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------

def _ipow(x, n):
    r = np.ones_like(x)
    for _ in range(n):
        r = r * x
    return r


def _field(terms, D, P, u, theta):
    """f[B, D], J_u[B, D, D] = df_d/du_k, J_theta[B, D, P] = df_d/dtheta_p."""
    dt = u.dtype
    B = u.shape[0]
    f = np.zeros((B, D), dtype=dt)
    Ju = np.zeros((B, D, D), dtype=dt)
    Jt = np.zeros((B, D, P), dtype=dt)
    for d, j, c, e in terms:
        e = tuple(e) + (0,) * (D - len(e))
        c = dt.type(c)
        mon = np.ones(B, dtype=dt)
        for i in range(D):
            mon = mon * _ipow(u[:, i], e[i])
        coef = c * theta[j] if j >= 0 else c
        f[:, d] += coef * mon
        if j >= 0:
            Jt[:, d, j] += c * mon
        for k in range(D):
            if e[k] == 0:
                continue
            dm = dt.type(e[k]) * _ipow(u[:, k], e[k] - 1)
            for i in range(D):
                if i != k:
                    dm = dm * _ipow(u[:, i], e[i])
            Ju[:, d, k] += coef * dm
    return f, Ju, Jt


def _stage(terms, D, P, u, S, theta):
    f, Ju, Jt = _field(terms, D, P, u, theta)
    K = Jt.copy()
    for k in range(D):
        K += Ju[:, :, k, None] * S[:, None, k, :]
    return f, K


def reference(terms, D, P, u0, theta, h, n_steps, obs_idx, y_obs, sigma, dtype=np.longdouble):
    """One chain.  Returns a dict with ``logp_quad`` (no normalisation
    constant), ``grad[P]``, the per-experiment ``q[B]`` and ``G[B, P]``, and
    ``states[n_steps + 1, B, D]``, all in ``dtype``."""
    dt = np.dtype(dtype)
    u = np.array(u0, dtype=dt)
    B = u.shape[0]
    assert u.shape == (B, D)
    theta = np.array(theta, dtype=dt).reshape(P)
    y = np.array(y_obs, dtype=dt).reshape(len(obs_idx), B, D)
    h = dt.type(h)
    sigma = dt.type(sigma)
    inv_sig2 = dt.type(1) / (sigma * sigma)
    half, two, six = dt.type(0.5), dt.type(2), dt.type(6)
    obs_of_step = {int(s): j for j, s in enumerate(obs_idx)}
    assert len(obs_of_step) == len(obs_idx)

    S = np.zeros((B, D, P), dtype=dt)
    q = np.zeros(B, dtype=dt)
    G = np.zeros((B, P), dtype=dt)
    states = np.empty((n_steps + 1, B, D), dtype=dt)
    for s in range(n_steps + 1):
        if s > 0:
            k1, K1 = _stage(terms, D, P, u, S, theta)
            k2, K2 = _stage(terms, D, P, u + half * h * k1, S + half * h * K1, theta)
            k3, K3 = _stage(terms, D, P, u + half * h * k2, S + half * h * K2, theta)
            k4, K4 = _stage(terms, D, P, u + h * k3, S + h * K3, theta)
            u = u + (h / six) * (k1 + two * k2 + two * k3 + k4)
            S = S + (h / six) * (K1 + two * K2 + two * K3 + K4)
        states[s] = u
        if s in obs_of_step:
            r = y[obs_of_step[s]] - u
            q -= half * inv_sig2 * (r * r).sum(axis=1)
            for d in range(D):
                G += inv_sig2 * r[:, d, None] * S[:, d, :]
    return {"logp_quad": q.sum(), "grad": G.sum(axis=0), "q": q, "G": G, "states": states}


def reference_chains(terms, D, P, u0, thetas, h, n_steps, obs_idx, y_obs, sigma,
                     dtype=np.longdouble):
    """``thetas[C, P]`` -> list of per-chain ``reference`` results, one theta at a time."""
    return [
        reference(terms, D, P, u0, th, h, n_steps, obs_idx, y_obs, sigma, dtype)
        for th in np.asarray(thetas)
    ]


def scales(ref):
    """(scale of logp_quad, scale[P] of the gradient): sum_b |c_b| in float64."""
    return float(np.abs(ref["q"]).sum()), np.abs(ref["G"]).sum(axis=0).astype(np.float64)


def kernel_tol(ref):
    """(tol for logp_quad, tol[P] for the gradient) = (8 W + B) u scale."""
    B = ref["q"].shape[0]
    s_q, s_g = scales(ref)
    k = (8.0 * W + B) * U
    return k * s_q, k * s_g


def state_tol(ref):
    """Per-element tolerance of the states slab: 8 W u max(1, |state|)."""
    return 8.0 * W * U * np.maximum(1.0, np.abs(ref["states"]).astype(np.float64))


def logp_const(n_vals, sigma):
    """The normalisation constant exactly as models/ode.py computes it."""
    import math

    return -0.5 * n_vals * math.log(2.0 * math.pi * float(sigma) ** 2)


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------

def _over17():
    terms = list(LV_TERMS)
    for i in range(13):
        terms.append((i % 2, i % 4, -0.01 * (i + 1), ((i % 3), (i + 1) % 3)))
    return terms


#: name -> (terms, D, P).  Signs and sizes keep trajectories tame.
TABLES = {
    "lv": (LV_TERMS, 2, 4),
    # D=1, P=1, one term: exponential decay
    "minimal": ([(0, 0, -1.0, (1,))], 1, 1),
    # exponents 2 and 3: ipow(n >= 2) and the ek * u^(ek-1) derivative
    "exp23": ([
        (0, 0, 1.0, (1, 0)),
        (0, 1, -0.5, (2, 1)),
        (1, 2, -0.3, (0, 3)),
        (1, 1, 0.4, (2, 0)),
    ], 2, 3),
    # one exponent of 15 (the native limit)
    "exp15": ([
        (0, 0, -0.1, (15, 0)),
        (0, 1, 0.2, (0, 1)),
        (1, 1, -1.0, (1, 1)),
    ], 2, 2),
    # terms without a theta factor
    "jminus1": ([
        (0, 0, 1.0, (1, 0)),
        (0, -1, -0.7, (1, 1)),
        (1, 1, -1.0, (0, 1)),
        (1, -1, 0.3, (2, 0)),
    ], 2, 2),
    # constant terms (all exponents zero), with and without theta
    "constant": ([
        (0, 0, 0.5, (0, 0)),
        (0, 1, -1.0, (1, 0)),
        (1, -1, 0.25, (0, 0)),
        (1, 0, -0.8, (0, 1)),
    ], 2, 2),
    # theta[1] is referenced by no term: its gradient is exactly 0.0
    "unused_theta": ([
        (0, 0, 1.0, (1, 0)),
        (0, 2, -1.0, (1, 1)),
        (1, 2, 0.5, (1, 1)),
        (1, 0, -0.6, (0, 1)),
    ], 2, 3),
    # two terms with the same (d, j, exponents)
    "duplicate": ([
        (0, 0, 0.6, (1, 0)),
        (0, 0, 0.3, (1, 0)),
        (0, 1, -0.8, (1, 1)),
        (1, 1, 0.4, (1, 1)),
        (1, 1, 0.4, (1, 1)),
        (1, 0, -0.7, (0, 1)),
    ], 2, 2),
    # exponent tuples shorter than D (missing trailing exponents are 0)
    "short": ([
        (0, 0, -1.0, (1,)),
        (1, 1, 1.0, (1, 1)),
        (1, 0, -0.5, (0, 1)),
        (2, 1, -0.6, (0, 0, 1)),
        (2, -1, 0.2, (2,)),
        (2, 0, 0.1, ()),
    ], 3, 2),
    # 16 terms, D=4, P=8, all of the above mixed; theta[7] unreferenced
    "full16": ([
        (0, 0, 1.0, (1, 0, 0, 0)),
        (0, 1, -0.5, (1, 1)),
        (0, -1, -0.05, (3,)),
        (0, 2, 0.1, ()),
        (1, 3, 0.4, (1, 1, 0, 0)),
        (1, 2, -0.9, (0, 1)),
        (1, 2, -0.1, (0, 1)),
        (1, 4, -0.02, (0, 15)),
        (2, 5, -0.6, (0, 0, 2)),
        (2, 4, 0.3, (1, 0, 0, 1)),
        (2, -1, 0.2, (0, 0, 0, 0)),
        (2, 0, -0.1, (0, 1, 1, 1)),
        (3, 6, -0.7, (0, 0, 0, 1)),
        (3, 5, 0.2, (2, 0, 1, 0)),
        (3, 6, -0.05, (0, 0, 0, 3)),
        (3, 1, 0.1, (0, 0, 1)),
    ], 4, 8),
    # over the native limits: served by the torch path
    "over17": (_over17(), 2, 4),
    "exp16": ([
        (0, 0, -0.1, (16, 0)),
        (0, 1, 0.2, (0, 1)),
        (1, 1, -1.0, (1, 1)),
    ], 2, 2),
}
assert len(TABLES["full16"][0]) == 16 and len(TABLES["over17"][0]) == 17

POLY_TABLE_NAMES = (
    "minimal", "exp23", "exp15", "jminus1", "constant", "unused_theta", "duplicate",
    "short", "full16",
)
OVER_LIMIT_NAMES = ("over17", "exp16")


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

SIGMA = 0.4  # log(2 pi sigma^2) ~ 0.005: the constant does not swamp the quadratic part
STEP = 0.2   # h <= 0.25

SINGLE_B = (1, 63, 64, 65, 255, 256, 257, 1000)
BATCHED_BC = ((1, 1), (1, 16), (100, 17), (257, 3), (256, 16), (64, 33))
OBS_LAYOUTS = {
    "first": (0,),
    "last": (7,),
    "first_last": (0, 7),
    "mid": (2, 5),
    "all": tuple(range(8)),
    "none": (),
}


def _n_steps_for(i):
    return (1, 2, 7)[i % 3]


def _build_cases():
    cases = {}

    def add(name, path, table, B, C, n_steps, obs):
        assert name not in cases
        cases[name] = dict(path=path, table=table, B=B, C=C, n_steps=n_steps, obs=tuple(obs))

    # path: "lv" = lotka_volterra_rhs (hand kernels), "poly" = PolynomialRHS
    for path in ("lv", "poly"):
        for i, B in enumerate(SINGLE_B):
            n = _n_steps_for(i)
            add(f"{path}-B{B}", path, "lv", B, None, n, (0, n) if n > 1 else (1,))
        for i, (B, C) in enumerate(BATCHED_BC):
            n = _n_steps_for(i + 1)
            add(f"{path}-B{B}xC{C}", path, "lv", B, C, n, (0, n) if n > 1 else (1,))
        for lay, obs in OBS_LAYOUTS.items():
            add(f"{path}-obs_{lay}", path, "lv", 65, None, 7, obs)
            add(f"{path}-obs_{lay}-C3", path, "lv", 65, 3, 7, obs)
    # second trip through the grid-stride loops (one step, one observation)
    add("lv-stride", "lv", "lv", 262144 + 77, None, 1, (1,))
    add("lv-stride-batched", "lv", "lv", 4099, 128, 1, (1,))
    add("poly-stride", "poly", "minimal", 524288 + 77, 1, 1, (1,))
    for t in POLY_TABLE_NAMES + OVER_LIMIT_NAMES:
        add(f"table-{t}", "poly", t, 65, None, 5, (0, 2, 5))
        add(f"table-{t}-C3", "poly", t, 65, 3, 5, (0, 2, 5))
    # reuse: one model, several chain counts
    add("lv-reuse", "lv", "lv", 65, 16, 7, (0, 3, 7))
    add("poly-reuse", "poly", "lv", 65, 16, 7, (0, 3, 7))
    return cases


CASES = _build_cases()


def small_case_names(limit=4096):
    return [n for n, c in CASES.items() if c["B"] * (c["C"] or 1) <= limit]


def make_case(name):
    """Deterministic inputs of a case: ``u0[B, D]``, ``thetas[C, P]`` (C=1 for a
    single-theta case), ``y_obs[n_obs, B, D]``, ``t1``, and ``h`` exactly as
    ODEModel derives it from ``(t0=0, t1, n_steps)``."""
    spec = CASES[name]
    terms, D, P = TABLES[spec["table"]]
    B, n_steps, obs = spec["B"], spec["n_steps"], spec["obs"]
    C = spec["C"] or 1
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    high = max((max(e) if len(e) else 0) for *_x, e in terms) >= 15
    u0 = rng.uniform(0.9, 1.1, size=(B, D)) if high else rng.uniform(0.5, 1.5, size=(B, D))
    thetas = rng.uniform(0.2, 1.0, size=(C, P))
    theta_true = rng.uniform(0.2, 1.0, size=P)
    t1 = STEP * n_steps
    h = (float(t1) - 0.0) / int(n_steps)
    truth = reference(terms, D, P, u0, theta_true, h, n_steps, (), np.zeros((0, B, D)),
                      SIGMA, dtype=np.float64)["states"]
    y = truth[list(obs)] + SIGMA * rng.standard_normal((len(obs), B, D))
    return dict(
        spec, name=name, terms=terms, D=D, P=P, u0=u0, thetas=thetas, y_obs=y,
        t1=t1, h=h, sigma=SIGMA, obs=list(obs),
    )


def case_reference(case, dtype=np.longdouble):
    return reference_chains(
        case["terms"], case["D"], case["P"], case["u0"], case["thetas"], case["h"],
        case["n_steps"], case["obs"], case["y_obs"], case["sigma"], dtype,
    )


def w_of(ref64, ref):
    """Worst error of a float64 result against the long-double one: per-lane
    values summed over a component's lanes in units of ``u scale``; trajectory
    per element in units of ``u max(1, |state|)``."""
    worst = 0.0
    pairs = [(ref64["q"][:, None], ref["q"][:, None]), (ref64["G"], ref["G"])]
    for a, b in pairs:
        err = np.abs(a.astype(np.longdouble) - b).sum(axis=0)
        scale = np.abs(b).sum(axis=0)
        ok = scale > 0
        assert np.all(err[~ok] == 0)
        if ok.any():
            worst = max(worst, float((err[ok] / (U * scale[ok])).max()))
    s_err = np.abs(ref64["states"].astype(np.longdouble) - ref["states"])
    worst = max(worst, float((s_err / (U * np.maximum(1, np.abs(ref["states"])))).max()))
    return worst


if __name__ == "__main__":
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    top = 0.0
    for case_name in CASES:
        cs = make_case(case_name)
        w = max(
            w_of(r64, r)
            for r64, r in zip(case_reference(cs, np.float64), case_reference(cs))
        )
        top = max(top, w)
        print(f"{case_name:28s} {w:8.2f}")
    print(f"max W = {top:.2f}")
