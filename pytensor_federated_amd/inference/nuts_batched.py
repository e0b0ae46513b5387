"""Lockstep multi-chain NUTS over a batched logp+grad function.

C independent NUTS chains (same math as :mod:`nuts` -- Hoffman & Gelman
2014, Algorithm 6 with dual-averaging + diagonal mass adaptation) advance
together: every "round" gathers the ONE pending gradient request of each
chain into a single batched call ``theta[K, C] -> (logp[C], grad[K, C])``.
On an MI355X shard that is one batched-kernel sweep for all chains
(``logp_grad_batched`` of ``LogisticGLMModel``, ``PoissonGLMModel``,
``GaussianGLMModel`` and ``ODEModel``),
so C chains cost close to one.

Mechanically each chain's transition is written as a *generator* that
yields ``q`` whenever the recursive tree build needs a gradient and
receives ``(logp, grad)`` back -- the driver below runs C such generators
in lockstep.  This keeps the per-chain semantics EXACTLY those of the
sequential sampler: with ``C == 1`` and the same seed, draws are
bit-identical to ``sample_nuts`` (asserted in tests/test_inference.py).
Chains that finish a transition early immediately begin the next one, so
lanes never idle across draw boundaries; tree-depth variance across chains
only pads the current round.

The multi-chain analog of the reference's ``pm.sample(cores=N)``
process-parallel chains (reference test_wrapper_ops.py:305-317), mapped
GPU-first instead of process-first.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from .nuts import _DELTA_MAX, _MAX_DEPTH

__all__ = ["sample_nuts_batched"]


class _ChainNUTS:
    """One NUTS chain whose transition is a generator (yields q, receives
    (logp, grad)).  RNG consumption order mirrors nuts.NUTS.step exactly."""

    def __init__(self, q, seed, step_size, target_accept, max_depth=_MAX_DEPTH):
        self.q = np.array(q, dtype=np.float64)
        self.rng = np.random.default_rng(seed)
        self.step_size = float(step_size)
        self.target_accept = float(target_accept)
        self.max_depth = int(max_depth)
        self.inv_mass = np.ones_like(self.q)
        self._mu = np.log(10 * self.step_size)
        self._log_eps_bar = 0.0
        self._h_bar = 0.0
        self._t0 = 10.0
        self._gamma = 0.05
        self._kappa = 0.75
        self._adapt_count = 0
        self.n_divergent = 0
        self.logp: float = 0.0
        self.grad: np.ndarray = np.zeros_like(self.q)
        self._last_accept_stat = 1.0
        # dense mass (Stan-style metric): M^-1 = Sigma (posterior covariance
        # estimate); None = diagonal metric via inv_mass
        self.mass_sigma: Optional[np.ndarray] = None
        self._mass_chol: Optional[np.ndarray] = None

    def _vel(self, p):
        """dq/dt = M^-1 p."""
        if self.mass_sigma is None:
            return self.inv_mass * p
        return self.mass_sigma @ p

    def _kinetic(self, p):
        if self.mass_sigma is None:
            # keep the exact summation order of nuts.NUTS._kinetic: the
            # C == 1 bit-identity test depends on it
            return 0.5 * float(np.sum(self.inv_mass * p * p))
        return 0.5 * float(p @ self._vel(p))

    def _sample_momentum(self):
        z = self.rng.normal(size=self.q.shape)
        if self.mass_sigma is None:
            return z / np.sqrt(self.inv_mass)
        # p ~ N(0, Sigma^-1): with Sigma = L L^T, p = L^-T z
        return np.linalg.solve(self._mass_chol.T, z)

    def set_dense_mass(self, sigma: np.ndarray) -> None:
        self.mass_sigma = sigma
        self._mass_chol = np.linalg.cholesky(sigma)

    def _leapfrog(self, q, p, grad, eps):
        p = p + 0.5 * eps * grad
        if self.mass_sigma is None:
            # exact expression grouping of nuts.NUTS._leapfrog (bit-identity)
            q = q + eps * self.inv_mass * p
        else:
            q = q + eps * (self.mass_sigma @ p)
        logp, grad = yield q
        p = p + 0.5 * eps * grad
        return q, p, logp, grad

    def transition(self):
        q0, logp0, grad0 = self.q, self.logp, self.grad
        p0 = self._sample_momentum()
        joint0 = logp0 - self._kinetic(p0)
        log_u = joint0 + np.log(self.rng.uniform())

        q_minus = q_plus = q0
        p_minus = p_plus = p0
        grad_minus = grad_plus = grad0
        q_new, logp_new, grad_new = q0, logp0, grad0
        j, n, s = 0, 1, True
        alpha_sum, n_alpha = 0.0, 0

        while s and j < self.max_depth:
            v = 1 if self.rng.uniform() < 0.5 else -1
            if v == -1:
                (q_minus, p_minus, grad_minus, _, _, _, q_prop, logp_prop, grad_prop,
                 n_prime, s_prime, a, na) = yield from self._build_tree(
                    q_minus, p_minus, grad_minus, log_u, v, j, joint0)
            else:
                (_, _, _, q_plus, p_plus, grad_plus, q_prop, logp_prop, grad_prop,
                 n_prime, s_prime, a, na) = yield from self._build_tree(
                    q_plus, p_plus, grad_plus, log_u, v, j, joint0)
            if s_prime and self.rng.uniform() < n_prime / max(n, 1):
                q_new, logp_new, grad_new = q_prop, logp_prop, grad_prop
            n += n_prime
            alpha_sum += a
            n_alpha += na
            dq = q_plus - q_minus
            s = s_prime and (dq @ self._vel(p_minus) >= 0) and (
                dq @ self._vel(p_plus) >= 0
            )
            j += 1

        self.q, self.logp, self.grad = q_new, logp_new, grad_new
        self._last_accept_stat = alpha_sum / max(n_alpha, 1)

    def _build_tree(self, q, p, grad, log_u, v, j, joint0):
        if j == 0:
            q1, p1, logp1, grad1 = yield from self._leapfrog(
                q, p, grad, v * self.step_size)
            joint = logp1 - self._kinetic(p1)
            if not np.isfinite(joint):
                joint = -np.inf  # out of support / overflow: reject cleanly
            n_prime = 1 if log_u <= joint else 0
            s_prime = log_u < joint + _DELTA_MAX
            if not s_prime:
                self.n_divergent += 1
            alpha = min(1.0, np.exp(min(joint - joint0, 0.0)))
            return (q1, p1, grad1, q1, p1, grad1, q1, logp1, grad1,
                    n_prime, s_prime, alpha, 1)
        (q_minus, p_minus, grad_minus, q_plus, p_plus, grad_plus, q_prop,
         logp_prop, grad_prop, n_prime, s_prime, a, na) = yield from self._build_tree(
            q, p, grad, log_u, v, j - 1, joint0)
        if s_prime:
            if v == -1:
                (q_minus, p_minus, grad_minus, _, _, _, q_pp, logp_pp, grad_pp,
                 n_pp, s_pp, a2, na2) = yield from self._build_tree(
                    q_minus, p_minus, grad_minus, log_u, v, j - 1, joint0)
            else:
                (_, _, _, q_plus, p_plus, grad_plus, q_pp, logp_pp, grad_pp,
                 n_pp, s_pp, a2, na2) = yield from self._build_tree(
                    q_plus, p_plus, grad_plus, log_u, v, j - 1, joint0)
            if n_pp > 0 and self.rng.uniform() < n_pp / max(n_prime + n_pp, 1):
                q_prop, logp_prop, grad_prop = q_pp, logp_pp, grad_pp
            n_prime += n_pp
            a += a2
            na += na2
            dq = q_plus - q_minus
            s_prime = s_pp and (dq @ self._vel(p_minus) >= 0) and (
                dq @ self._vel(p_plus) >= 0
            )
        return (q_minus, p_minus, grad_minus, q_plus, p_plus, grad_plus,
                q_prop, logp_prop, grad_prop, n_prime, s_prime, a, na)

    # -- adaptation (identical math to nuts.NUTS) -------------------------
    def adapt_step_size(self):
        self._adapt_count += 1
        m = self._adapt_count
        eta = 1.0 / (m + self._t0)
        self._h_bar = (1 - eta) * self._h_bar + eta * (
            self.target_accept - self._last_accept_stat)
        log_eps = self._mu - np.sqrt(m) / self._gamma * self._h_bar
        log_eps = float(np.clip(log_eps, self._mu - 20.0, self._mu + 20.0))
        w = m ** (-self._kappa)
        self._log_eps_bar = w * log_eps + (1 - w) * self._log_eps_bar
        self.step_size = float(np.exp(log_eps))

    def freeze_step_size(self):
        self.step_size = float(np.exp(self._log_eps_bar))

    def reset_step_size_adaptation(self, step_size: float) -> None:
        """Restart dual averaging at a fresh (whitened-units) step size --
        required after every metric update; see nuts.NUTS for rationale."""
        self.step_size = float(step_size)
        self._mu = np.log(10 * self.step_size)
        self._log_eps_bar = 0.0
        self._h_bar = 0.0
        self._adapt_count = 0


def metric_window_ends(tune: int, base_window: int = 25,
                       init_buffer: Optional[int] = None,
                       term_buffer: Optional[int] = None) -> List[int]:
    """Stan-style expanding adaptation windows: transition indices (1-based)
    at which the metric is re-estimated and step-size adaptation restarts.

    Layout: [init_buffer: step size only][w][2w][4w]...[term_buffer: step
    size only]; the last window is extended to absorb any remainder."""
    if init_buffer is None:
        init_buffer = max(20, int(0.15 * tune))
    if term_buffer is None:
        term_buffer = max(25, int(0.1 * tune))
    ends: List[int] = []
    pos, w = init_buffer, base_window
    while pos + w + term_buffer <= tune:
        nxt = pos + w
        if nxt + 2 * w + term_buffer > tune:
            nxt = tune - term_buffer  # absorb the remainder
        ends.append(nxt)
        pos, w = nxt, w * 2
    return ends


def _estimate_metric(ch, w: np.ndarray, mass: str) -> None:
    """Set ch's metric from window draws w[n, K] (shrunk toward diagonal)."""
    if mass == "dense":
        n_w = w.shape[0]
        cov = np.atleast_2d(np.cov(w.T))
        lam = n_w / (n_w + 5.0)
        diag = np.diag(np.maximum(np.diag(cov), 1e-12))
        ch.set_dense_mass(lam * cov + (1 - lam) * diag
                          + 1e-12 * np.eye(cov.shape[0]))
    else:
        ch.inv_mass = np.maximum(np.var(w, axis=0), 1e-10)


def sample_nuts_batched(
    batched_logp_grad: Callable[[np.ndarray], Tuple[np.ndarray, np.ndarray]],
    init: np.ndarray,
    *,
    draws: int = 1000,
    tune: int = 500,
    step_size: float = 0.1,
    target_accept: float = 0.8,
    seed: Optional[int] = None,
    adapt_mass: bool = True,
    mass: str = "diag",
    adaptation: str = "windowed",
    max_depth: int = _MAX_DEPTH,
) -> Tuple[np.ndarray, dict]:
    """Run C lockstep NUTS chains over one batched evaluator.

    Parameters
    ----------
    batched_logp_grad : callable(theta[K, C]) -> (logp[C], grad[K, C])
        Batched evaluation (e.g. ``model.logp_grad_batched``); arrays may be
        numpy or torch -- converted via ``np.asarray``.
    init : array [K, C]
        Initial states of the C chains (chain c uses seed ``seed + c``, so
        C == 1 reproduces ``sample_nuts(..., seed=seed)`` exactly).
    mass : "diag" (default, matches ``sample_nuts``) or "dense"
        "dense" adapts a full covariance metric from the tuning window --
        required for strongly correlated posteriors (e.g. ODE parameters),
        where a diagonal metric mixes arbitrarily slowly.
    adaptation : "windowed" (default) or "simple"
        "windowed" is Stan-style expanding metric windows with a step-size
        restart at each boundary -- measured 2193 vs 1680 draws/s at equal
        split-R-hat (1.006 vs 1.008) on the 16-chain dense-metric LV
        posterior (profiles/raw_r2/r2c4_nuts_*.json), so it is the default from
        round 2; "simple" keeps the single mid-tune metric update
        "simple" = one metric update at 60% of tune (matches
        ``sample_nuts``, keeps C=1 bit-identity).  "windowed" = Stan-style
        expanding windows (``metric_window_ends``): the metric is
        re-estimated several times with step-size restarts, so early
        burn-in never contaminates the final metric.

    Returns
    -------
    (chain, stats): chain has shape [draws, K, C]; stats carries rounds
    (batched calls), total leapfrogs (what a sequential run would have
    paid), per-chain step sizes and divergence counts.
    """
    init = np.array(init, dtype=np.float64)
    if init.ndim != 2:
        raise ValueError(f"init must be [K, C], got shape {init.shape}")
    K, C = init.shape
    chains = [
        _ChainNUTS(init[:, c], None if seed is None else seed + c,
                   step_size, target_accept, max_depth)
        for c in range(C)
    ]

    def ev(theta):
        logp, grad = batched_logp_grad(theta)
        return (
            np.asarray(logp, dtype=np.float64).reshape(C),
            np.asarray(grad, dtype=np.float64).reshape(K, C),
        )

    # initial evaluation at the start points (mirrors NUTS.__init__)
    theta = np.ascontiguousarray(init)
    logp, G = ev(theta)
    for c, ch in enumerate(chains):
        ch.logp, ch.grad = float(logp[c]), G[:, c].copy()

    total = tune + draws
    samples = np.empty((draws, K, C))
    accept_stats = [[] for _ in range(C)]
    n_done = [0] * C
    windows: List[List[np.ndarray]] = [[] for _ in range(C)]
    mass_update_at = int(tune * 0.6)
    if adaptation not in ("simple", "windowed"):
        raise ValueError(f"unknown adaptation schedule: {adaptation!r}")
    win_ends = metric_window_ends(tune) if adaptation == "windowed" else []
    win_ptr = [0] * C
    init_buffer = max(20, int(0.15 * tune))
    gens = [ch.transition() for ch in chains]
    pending: List[Optional[np.ndarray]] = [next(g) for g in gens]
    rounds = 0
    leapfrogs = 0

    def finish_transition(c: int):
        """Bookkeeping after chain c completes one transition; returns the
        first pending q of its next transition (or None if fully done)."""
        ch = chains[c]
        i = n_done[c]
        n_done[c] += 1
        if i < tune:
            ch.adapt_step_size()
            if adapt_mass and adaptation == "windowed":
                if i >= init_buffer:
                    windows[c].append(ch.q.copy())
                if (win_ptr[c] < len(win_ends)
                        and n_done[c] == win_ends[win_ptr[c]]):
                    if len(windows[c]) > 10:
                        _estimate_metric(ch, np.stack(windows[c]), mass)
                        ch.reset_step_size_adaptation(0.25)
                    windows[c].clear()
                    win_ptr[c] += 1
            elif adapt_mass:
                windows[c].append(ch.q.copy())
                if i == mass_update_at and len(windows[c]) > 10:
                    w = np.stack(windows[c][len(windows[c]) // 2:])
                    _estimate_metric(ch, w, mass)
                    windows[c].clear()
                    ch.reset_step_size_adaptation(0.25)
            if n_done[c] == tune:
                ch.freeze_step_size()
                # report post-warmup divergences only (Stan/arviz semantics;
                # windowed adaptation's step-size restarts make transient
                # TUNE-phase divergences normal and meaningless)
                ch.n_divergent = 0
        else:
            samples[i - tune, :, c] = ch.q
            accept_stats[c].append(ch._last_accept_stat)
        if n_done[c] >= total:
            gens[c] = None
            return None
        gens[c] = ch.transition()
        return next(gens[c])

    while any(d < total for d in n_done):
        # pad finished lanes with their current position (cost-free for the
        # batched kernels, keeps theta shape fixed)
        theta = np.stack(
            [pending[c] if pending[c] is not None else chains[c].q
             for c in range(C)], axis=1)
        logp, G = ev(theta)
        rounds += 1
        for c in range(C):
            if pending[c] is None:
                continue
            leapfrogs += 1
            try:
                pending[c] = gens[c].send((float(logp[c]), G[:, c].copy()))
            except StopIteration:
                pending[c] = finish_transition(c)

    return samples, {
        "chains": C,
        "rounds": rounds,
        "leapfrogs": leapfrogs,
        "step_sizes": [ch.step_size for ch in chains],
        "divergences": [ch.n_divergent for ch in chains],
        "accept_stat": [float(np.mean(a)) if a else float("nan")
                        for a in accept_stats],
    }
