"""Premise checks for test_gpu_persistent_resident.py (no GPU needed).

The GPU tests hold the persistent Gaussian server to the fp64 numpy
reference bit-tight at sizes that cross its register-resident capacity.
That is only fair if at those sizes every sum is exact in the kernel's own
scheme: per lane, fp64 for the residual and sequential fp32 for the r*x and
r^2 products (resident slots first, then the streamed sweeps, then the one
tail row), fp64 across lanes.  Here that scheme is replayed in numpy with the
kernel's lane -> element mapping and must agree with integer arithmetic and
with the reference bit for bit.

A size that fails here gets changed, not given a tolerance.
"""
import numpy as np
import pytest

import exact_probes as ep
import persistent_probes as pp

F32 = np.float32


def _cases():
    for dtype in sorted(ep.GAUSS_VEC):
        for n in pp.resident_sizes(dtype):
            yield pytest.param(dtype, n, pp.LANES, id=f"{dtype}-{n}")
    dtype, n = pp.DEFAULT_GRID_CASE
    yield pytest.param(dtype, n, 512 * 256, id=f"{dtype}-{n}-grid512")


def _lane_partials(v, n, vec, lanes):
    """Sequential fp32 sum per lane in the kernel's order: vector i of the
    shard belongs to lane i % lanes as its iteration i // lanes; the tail row
    nvec*vec + g goes to lane g last.  Also returns each lane's sum of
    magnitudes (fp64)."""
    nvec = n // vec
    iters = -(-nvec // lanes) if nvec else 0
    body = np.zeros(iters * lanes * vec)
    body[: nvec * vec] = v[: nvec * vec]
    body = body.reshape(iters, lanes, vec)  # padding adds exact zeros
    acc = np.zeros(lanes, dtype=F32)
    mag = np.zeros(lanes)
    for k in range(iters):
        for j in range(vec):
            acc += body[k, :, j].astype(F32)
            mag += np.abs(body[k, :, j])
    ntail = n - nvec * vec
    assert ntail < vec <= lanes
    acc[:ntail] += v[nvec * vec :].astype(F32)
    mag[:ntail] += np.abs(v[nvec * vec :])
    assert acc.dtype == F32
    return acc, mag


def test_capacity_matches_kernel_source():
    assert pp.source_pk_cap() == pp.PK_CAP >= 10


@pytest.mark.parametrize("dtype,n,lanes", list(_cases()))
def test_resident_probe_is_exact(dtype, n, lanes):
    vec = ep.GAUSS_VEC[dtype]
    p = ep.gaussian_probe(n)
    x, y = p["x"], p["y"]
    assert ep.is_bf16_exact(x) and ep.is_bf16_exact(y)
    x8 = np.rint(x * 8).astype(np.int64)
    y8 = np.rint(y * 8).astype(np.int64)
    assert np.array_equal(x8 / 8.0, x) and np.array_equal(y8 / 8.0, y)
    for a, b in ep.GAUSS_THETAS:
        a4, b4 = int(a * 4), int(b * 4)
        assert a4 / 4.0 == a and b4 / 4.0 == b
        # integer arithmetic: r in units of 2^-5, r*x of 2^-8, r^2 of 2^-10
        r_i = 4 * y8 - 8 * a4 - b4 * x8
        rx_i = r_i * x8
        r2_i = r_i * r_i
        r = y - (a + b * x)
        assert np.array_equal(r, r_i / 32.0)
        r32 = r.astype(F32)
        x32 = x.astype(F32)
        # the fp32 products the kernel forms are exact
        assert np.array_equal((r32 * x32).astype(np.float64), rx_i / 256.0)
        assert np.array_equal((r32 * r32).astype(np.float64), r2_i / 1024.0)
        for v_i, unit in ((rx_i, 2.0 ** -8), (r2_i, 2.0 ** -10)):
            acc, mag = _lane_partials(v_i * unit, n, vec, lanes)
            # every fp32 partial of every lane stays an exact integer of units
            assert np.max(mag) / unit < 2 ** 24
            total = int(v_i.sum())
            assert abs(total) < 2 ** 53
            assert float(np.sum(acc.astype(np.float64))) == total * unit
        # fp64 sums (the residual; all three for f64 inputs) are exact in
        # any order
        for v_i in (r_i, rx_i, r2_i):
            assert int(np.abs(v_i).sum()) < 2 ** 53
        logp, ga, gb = ep.gaussian_reference(x, y, a, b)
        assert ga == int(r_i.sum()) / 32.0
        assert gb == int(rx_i.sum()) / 256.0
        sum_r2 = int(r2_i.sum()) / 1024.0
        assert float(np.sum(r * r)) == sum_r2
        logp_exact = -0.5 * n * np.log(2.0 * np.pi) - 0.5 * sum_r2
        assert abs(logp - logp_exact) <= np.spacing(abs(logp_exact))
