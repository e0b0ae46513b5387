"""MAP estimation by truncated Newton-CG on federated shards.

``find_map_newton`` solves each Newton step with the dense Fisher matrix:
``K^2`` numbers leave every worker per step.  Here the step ``(H + P) d = g``
is solved by preconditioned conjugate gradients on the Fisher-vector product
``H v = X^T (w * (X v))``, which a shard answers with one pass over its data
and a K-vector (``model.as_fisher_vector_func()``).  Only K-vectors cross the
wire, a few tens of them for a whole MAP, and the product exists where the
dense matrix does not (the logistic model, f32 shards, K = 2048).

The inner solve is inexact on purpose: far from the mode an accurate Newton
direction buys nothing, so CG stops at ``|r| <= eta |r0|`` with
``eta = min(0.5, sqrt(|g| / |g_init|))``, which tightens as the gradient
falls and keeps the superlinear convergence of Newton's method near the mode.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence, Union

import numpy as np

__all__ = ["NewtonCGResult", "find_map_newton_cg"]


class NewtonCGResult(NamedTuple):
    theta: np.ndarray   #: the mode, fp64[K]
    logp: float         #: logp (incl. the prior term) at ``theta``
    n_steps: int        #: outer (Newton) steps taken
    n_products: int     #: Fisher-vector products taken, summed over the steps
    converged: bool     #: the gradient criterion was met within ``max_steps``


def _as_list(funcs) -> list:
    return [funcs] if callable(funcs) else list(funcs)


def find_map_newton_cg(
    logp_grad_funcs: Union[Callable, Sequence[Callable]],
    fisher_vector_funcs: Union[Callable, Sequence[Callable]],
    init,
    *,
    fisher_diagonal_funcs: Union[None, Callable, Sequence[Callable]] = None,
    prior_precision=None,
    max_steps: int = 50,
    gtol: float = 1e-9,
    max_cg: Optional[int] = None,
    max_halvings: int = 30,
) -> NewtonCGResult:
    """Newton-CG MAP of one parameter vector ``theta[K]``.

    ``logp_grad_funcs`` and ``fisher_vector_funcs`` hold one callable per
    shard (a single callable is accepted too): ``theta -> (logp, [grad])``
    and ``(theta, v) -> [H v]`` (``model.as_fisher_vector_func()``, local or
    served).  ``fisher_diagonal_funcs``, optional, holds ``theta ->
    [diag(H)]`` per shard (``model.as_fisher_diagonal_func()``).  The shard
    results are summed.  One product of the count ``n_products`` is one call
    of every shard's product function.

    ``prior_precision`` is ``find_map_newton``'s: a scalar ``tau`` or a
    ``[K,K]`` matrix ``P`` of a zero-mean Gaussian prior; it adds ``P v`` to
    the product, ``-P theta`` to the gradient and ``-theta^T P theta / 2``
    to logp.

    Each outer step solves ``(H + P) d = g`` by preconditioned CG from
    ``d = 0``.  The preconditioner ``M`` is the summed shard diagonals plus
    ``diag(P)`` where diagonal functions are given (one more pass per outer
    step), the identity otherwise.  CG stops at ``|r| <= eta |r0|`` with
    ``eta = min(0.5, sqrt(|g| / |g_init|))``, after ``max_cg`` products
    (default ``2 K``), or on a non-positive curvature ``p^T (H + P) p``
    (rounding, or an overflowed weight): the direction reached so far is
    used, the preconditioned gradient if that is the first.

    The step is then halved while logp fails to increase (or is not finite),
    as in ``find_map_newton``, with the same allowance for a logp summed
    from f32 terms: a step that changes logp by no more than ``2^-20 |logp|``
    either way is one logp cannot judge, and is taken when it lowers
    ``g^T M^-1 g``, which stands in for the Newton decrement (no factor of
    ``H`` exists here).  It stops when ``max|g| <= gtol * max(1, |logp|)``.

    On a model that sums in f32 the gradient has a noise floor above that
    criterion, and a driver that went on would spend products on steps that
    only shuffle the noise.  A step that logp cannot judge and that lowers
    ``g^T M^-1 g`` by less than a factor of 4 (the gradient by less than 2,
    where CG alone promises ``eta <= 1/2`` and delivers far more that close to
    the mode) is therefore the last one: it is taken, and the result has
    ``converged = False`` unless the criterion happens to hold.

    There is no covariance in the result: forming ``(H + P)^-1`` needs the
    dense matrix.  Take the Laplace covariance from ``find_map_newton``
    started at this mode, or from ``model.fisher_information(theta)``.
    """
    lg_funcs, hv_funcs = _as_list(logp_grad_funcs), _as_list(fisher_vector_funcs)
    if not lg_funcs or len(lg_funcs) != len(hv_funcs):
        raise ValueError(
            "need one logp+grad function and one Fisher-vector function per shard"
        )
    d_funcs = None if fisher_diagonal_funcs is None else _as_list(fisher_diagonal_funcs)
    if d_funcs is not None and len(d_funcs) != len(lg_funcs):
        raise ValueError("need one Fisher-diagonal function per shard, or none")
    theta = np.array(init, dtype=np.float64)
    if theta.ndim != 1:
        raise ValueError("init must be a vector")
    K = theta.shape[0]
    if prior_precision is None:
        P = None
    else:
        P = np.asarray(prior_precision, dtype=np.float64)
        if P.ndim == 0:
            P = float(P) * np.eye(K)
        if P.shape != (K, K):
            raise ValueError(f"prior_precision must be a scalar or [{K}, {K}]")
    if max_cg is None:
        max_cg = 2 * K
    if max_cg < 1:
        raise ValueError("max_cg must be at least 1")

    def logp_grad(t):
        logp, g = 0.0, np.zeros(K)
        for f in lg_funcs:
            lp, grads = f(t)
            logp += float(lp)
            g = g + np.asarray(grads[0], dtype=np.float64).reshape(K)
        if P is None:
            return logp, g
        Pt = P @ t
        return logp - 0.5 * float(t @ Pt), g - Pt

    n_products = 0

    def product(t, p):
        nonlocal n_products
        n_products += 1
        Hp = np.zeros(K) if P is None else P @ p
        for f in hv_funcs:
            Hp = Hp + np.asarray(f(t, p)[0], dtype=np.float64).reshape(K)
        return Hp

    def preconditioner(t):
        if d_funcs is None:
            return np.ones(K)
        M = np.zeros(K) if P is None else np.diag(P).copy()
        for f in d_funcs:
            M = M + np.asarray(f(t)[0], dtype=np.float64).reshape(K)
        if not (np.all(np.isfinite(M)) and np.all(M > 0.0)):
            raise ValueError("the Fisher diagonal must be finite and positive")
        return M

    logp, g = logp_grad(theta)
    if not np.isfinite(logp):
        raise ValueError("logp is not finite at init")
    g_init = float(np.linalg.norm(g))
    n_steps, converged, stalled = 0, False, False
    while True:
        converged = bool(np.max(np.abs(g)) <= gtol * max(1.0, abs(logp)))
        if converged or stalled or n_steps >= max_steps:
            break
        M = preconditioner(theta)
        # -- inner solve: (H + P) delta = g ---------------------------------
        eta = min(0.5, float(np.sqrt(np.linalg.norm(g) / g_init)))
        delta = np.zeros(K)
        r = g.copy()
        z = r / M
        p = z.copy()
        rz = float(r @ z)
        r0 = float(np.linalg.norm(r))
        for it in range(max_cg):
            with np.errstate(all="ignore"):
                Ap = product(theta, p)
                curv = float(p @ Ap)
            if not (np.isfinite(curv) and curv > 0.0):
                if it == 0:
                    delta = z
                break
            alpha = rz / curv
            delta = delta + alpha * p
            r = r - alpha * Ap
            if float(np.linalg.norm(r)) <= eta * r0:
                break
            z = r / M
            rz_new = float(r @ z)
            p = z + (rz_new / rz) * p
            rz = rz_new
        # -- halving line search -------------------------------------------
        dec = float(g @ (g / M))
        slack = 2.0 ** -20 * max(1.0, abs(logp))  # what an f32-summed logp resolves
        step, accepted = 1.0, False
        for _ in range(max_halvings + 1):
            cand = theta + step * delta
            with np.errstate(all="ignore"):
                c_logp, c_g = logp_grad(cand)
            if np.isfinite(c_logp) and np.all(np.isfinite(c_g)):
                if c_logp > logp + slack:
                    accepted = True  # an ascent that logp resolves
                    break
                if c_logp >= logp - slack:
                    # logp cannot tell: the gradient decides
                    c_dec = float(c_g @ (c_g / M))
                    if c_dec < dec:
                        accepted = True
                        stalled = c_dec > 0.25 * dec
                        break
            step *= 0.5
        n_steps += 1
        if not accepted:
            break  # no ascent along the direction: at the resolution of logp
        theta, logp, g = cand, c_logp, c_g
    return NewtonCGResult(theta, float(logp), n_steps, n_products, converged)
