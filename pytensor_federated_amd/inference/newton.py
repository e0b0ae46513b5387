"""MAP estimation by Fisher scoring (Newton / IRLS) on federated shards.

A canonical-link GLM has a concave logp whose negative Hessian is the
Fisher information ``H = X^T diag(w) X``, so Newton's method converges in a
handful of steps where Adam ascent (``find_map``) takes hundreds; a Gaussian
model converges in exactly one.  ``logp``, its gradient and ``H`` are sums
over rows, so every shard contributes its own and the driver adds them: only
``1 + K + K^2`` numbers leave a worker per step.

The inverse of ``H`` (plus the prior precision) at the mode is the Laplace
covariance: its square-rooted diagonal gives the standard errors, and
``laplace_mass`` hands it to ``NUTS.set_dense_mass`` as a metric that needs
no warm-up draws.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence, Union

import numpy as np

__all__ = ["NewtonResult", "find_map_newton", "laplace_mass"]


class NewtonResult(NamedTuple):
    theta: np.ndarray   #: the mode, fp64[K]
    logp: float         #: logp (incl. the prior term) at ``theta``
    cov: np.ndarray     #: Laplace covariance (H + P)^-1 at ``theta``, fp64[K,K]
    n_steps: int        #: Newton steps taken
    converged: bool     #: the gradient criterion was met within ``max_steps``


def _as_list(funcs) -> list:
    return [funcs] if callable(funcs) else list(funcs)


def find_map_newton(
    logp_grad_funcs: Union[Callable, Sequence[Callable]],
    fisher_funcs: Union[Callable, Sequence[Callable]],
    init,
    *,
    prior_precision=None,
    max_steps: int = 25,
    gtol: float = 1e-9,
    max_halvings: int = 30,
) -> NewtonResult:
    """Newton MAP of one parameter vector ``theta[K]``.

    ``logp_grad_funcs`` and ``fisher_funcs`` hold one callable per shard (a
    single callable is accepted too): ``theta -> (logp, [grad])`` (the
    ``LogpGradFunc`` signature; ``model.as_logp_grad_func()`` or a remote
    client's ``evaluate``) and ``theta -> [H]`` (``model.as_fisher_func()``,
    local or served).  The shard results are summed.

    ``prior_precision`` is an optional zero-mean Gaussian prior, a scalar
    ``tau`` (``P = tau * I``) or a ``[K,K]`` matrix: it adds ``P`` to ``H``,
    ``-P theta`` to the gradient and ``-theta^T P theta / 2`` to logp.

    Each step solves ``(H + P) delta = g`` by Cholesky and halves the step
    while logp fails to increase (or is not finite), which keeps a poor
    start from overflowing the Poisson link.  Close to the mode the gain of
    a step falls below the resolution of a logp summed from f32 terms;
    a step that loses no more than ``2^-20 |logp|`` is therefore also taken
    when it lowers the Newton decrement ``g^T (H + P)^-1 g``, so the last
    digits come from the gradient.  It
    stops when ``max|g| <= gtol * max(1, |logp|)``.

    Example: the Laplace covariance as the dense metric of NUTS::

        res = find_map_newton(model.as_logp_grad_func(), model.as_fisher_func(),
                              np.zeros(K))
        stderr = np.sqrt(np.diag(res.cov))
        sampler = NUTS(model.as_logp_grad_func(), [res.theta], seed=1)
        sampler.set_dense_mass(laplace_mass(res))
        # ... or let sample_nuts start at the mode:
        draws = sample_nuts(model.as_logp_grad_func(), [res.theta], mass="dense")
    """
    lg_funcs, h_funcs = _as_list(logp_grad_funcs), _as_list(fisher_funcs)
    if not lg_funcs or len(lg_funcs) != len(h_funcs):
        raise ValueError("need one logp+grad function and one Fisher function per shard")
    theta = np.array(init, dtype=np.float64)
    if theta.ndim != 1:
        raise ValueError("init must be a vector")
    K = theta.shape[0]
    if prior_precision is None:
        P = np.zeros((K, K))
    else:
        P = np.asarray(prior_precision, dtype=np.float64)
        if P.ndim == 0:
            P = float(P) * np.eye(K)
        if P.shape != (K, K):
            raise ValueError(f"prior_precision must be a scalar or [{K}, {K}]")

    def logp_grad(t):
        logp, g = 0.0, np.zeros(K)
        for f in lg_funcs:
            lp, grads = f(t)
            logp += float(lp)
            g = g + np.asarray(grads[0], dtype=np.float64).reshape(K)
        Pt = P @ t
        return logp - 0.5 * float(t @ Pt), g - Pt

    def fisher(t):
        H = P.copy()
        for f in h_funcs:
            H = H + np.asarray(f(t)[0], dtype=np.float64).reshape(K, K)
        return H

    logp, g = logp_grad(theta)
    if not np.isfinite(logp):
        raise ValueError("logp is not finite at init")
    n_steps, converged = 0, False
    while True:
        converged = bool(np.max(np.abs(g)) <= gtol * max(1.0, abs(logp)))
        if converged or n_steps >= max_steps:
            break
        L = np.linalg.cholesky(fisher(theta))
        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
        dec = float(g @ delta)  # Newton decrement squared, in the metric of this step
        slack = 2.0 ** -20 * max(1.0, abs(logp))  # what an f32-summed logp resolves
        step, accepted = 1.0, False
        for _ in range(max_halvings + 1):
            cand = theta + step * delta
            with np.errstate(all="ignore"):
                c_logp, c_g = logp_grad(cand)
            if np.isfinite(c_logp) and np.all(np.isfinite(c_g)):
                if c_logp >= logp:
                    accepted = True
                    break
                if c_logp >= logp - slack:
                    c_dec = float(c_g @ np.linalg.solve(L.T, np.linalg.solve(L, c_g)))
                    if c_dec < dec:
                        accepted = True
                        break
            step *= 0.5
        n_steps += 1
        if not accepted:
            break  # no ascent along the Newton direction: at the resolution of logp
        theta, logp, g = cand, c_logp, c_g
    cov = np.linalg.inv(fisher(theta))
    cov = 0.5 * (cov + cov.T)
    return NewtonResult(theta, float(logp), cov, n_steps, converged)


def laplace_mass(result: NewtonResult) -> np.ndarray:
    """The Laplace covariance of ``result`` in the form
    ``NUTS.set_dense_mass`` takes: a symmetric positive-definite fp64[K,K]
    estimate of the posterior covariance."""
    cov = np.array(result.cov, dtype=np.float64)
    return 0.5 * (cov + cov.T)
