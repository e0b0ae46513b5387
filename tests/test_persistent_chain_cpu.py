"""Premise checks for test_gpu_persistent_chain.py (no GPU needed).

The GPU tests hold the persistent Gaussian server to the fp64 numpy reference
bit-tight (gradients ``==``, logp within 2 ulp) over 80 thetas.  That is only
fair if, for those thetas and shard sizes, every sum is exact in the kernel's
own scheme: the residual in fp64, the r*x and r^2 products summed sequentially
in fp32 per lane, fp64 across lanes.  Checked here with integer arithmetic:

* r, r*x and r^2 are integers in units of 2^-5, 2^-8 and 2^-10, and the fp32
  products the kernel forms are those integers exactly;
* per lane (the kernel's lane -> element mapping: vector i of the shard goes
  to lane i % lanes, tail row g to lane g) the sum of MAGNITUDES stays below
  2^24 units, so every fp32 partial sum of every lane is an exact integer in
  whatever order it is formed, and the lane's fp32 sum is the integer sum;
* the totals stay below 2^53 units, so the fp64 sums are exact in any order
  and the reference's gradients equal the integer sums.

A size or theta that fails here gets changed, not given a tolerance.
"""
import numpy as np
import pytest

import chain_probes as cp
import exact_probes as ep

F32 = np.float32


def test_thetas_are_the_80_quarter_pairs_and_consecutive_ones_differ():
    assert len(cp.THETAS) == len(set(cp.THETAS)) == 80
    for a, b in cp.THETAS:
        assert (a, b) != (0.0, 0.0)
        assert abs(a) <= 1 and abs(b) <= 1
        assert float(int(a * 4)) == a * 4 and float(int(b * 4)) == b * 4
    # cycling: the last is followed by the first
    for prev, cur in zip(cp.THETAS, cp.THETAS[1:] + cp.THETAS[:1]):
        assert prev != cur


def test_every_element_is_exact_for_every_theta():
    """The probe's x and y are j/8 with |j| <= 32, so the element-wise
    premises depend on (x, y, a, b) alone: check them on the whole 65 x 65
    value grid once instead of on every row of every shard."""
    j = np.arange(-32, 33, dtype=np.int64)
    x8, y8 = (g.ravel() for g in np.meshgrid(j, j, indexing="ij"))
    x, y = x8 / 8.0, y8 / 8.0
    x32 = x.astype(F32)
    for a, b in cp.THETAS:
        a4, b4 = int(a * 4), int(b * 4)
        # integer arithmetic: r in units of 2^-5, r*x of 2^-8, r^2 of 2^-10
        r_i = 4 * y8 - 8 * a4 - b4 * x8
        r = y - (a + b * x)
        assert np.array_equal(r, r_i / 32.0)
        r32 = r.astype(F32)
        # the fp32 products the kernel forms are exact
        assert np.array_equal((r32 * x32).astype(np.float64), (r_i * x8) / 256.0)
        assert np.array_equal((r32 * r32).astype(np.float64), (r_i * r_i) / 1024.0)


def _lane_magnitudes(units, n, vec, lanes):
    """Per-lane sum of |units| (int64) under the kernel's mapping."""
    nvec = n // vec
    iters = -(-nvec // lanes) if nvec else 0
    body = np.zeros(iters * lanes * vec, dtype=np.int64)
    body[: nvec * vec] = np.abs(units[: nvec * vec])
    mag = body.reshape(iters, lanes, vec).sum(axis=(0, 2)) if iters else np.zeros(lanes, np.int64)
    ntail = n - nvec * vec
    assert ntail < vec <= lanes
    mag[:ntail] += np.abs(units[nvec * vec:])
    return mag


@pytest.mark.parametrize(
    "dtype,grid,n", [pytest.param(*c, id=f"{c[0]}-grid{c[1]}-{c[2]}") for c in cp.CASES]
)
def test_chain_probe_is_exact(dtype, grid, n):
    vec = ep.GAUSS_VEC[dtype]
    lanes = cp.lanes_of(grid)
    p = ep.gaussian_probe(n)
    x, y = p["x"], p["y"]
    assert ep.is_bf16_exact(x) and ep.is_bf16_exact(y)
    x8 = np.rint(x * 8).astype(np.int64)
    y8 = np.rint(y * 8).astype(np.int64)
    assert np.array_equal(x8 / 8.0, x) and np.array_equal(y8 / 8.0, y)
    assert np.abs(x8).max() <= 32 and np.abs(y8).max() <= 32  # the values checked above
    refs = cp.references(n)
    for (a, b), (logp, ga, gb) in zip(cp.THETAS, refs):
        a4, b4 = int(a * 4), int(b * 4)
        r_i = 4 * y8 - 8 * a4 - b4 * x8
        rx_i = r_i * x8
        r2_i = r_i * r_i
        if vec != 2:  # f64 inputs: fp64 products and sums throughout
            for v_i in (rx_i, r2_i):
                assert int(_lane_magnitudes(v_i, n, vec, lanes).max()) < 2 ** 24
        for v_i in (r_i, rx_i, r2_i):
            assert int(np.abs(v_i).sum()) < 2 ** 53
        assert ga == int(r_i.sum()) / 32.0
        assert gb == int(rx_i.sum()) / 256.0
        sum_r2 = int(r2_i.sum()) / 1024.0
        logp_exact = -0.5 * n * np.log(2.0 * np.pi) - 0.5 * sum_r2
        assert abs(logp - logp_exact) <= np.spacing(abs(logp_exact))
