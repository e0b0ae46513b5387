"""GPU (MI355X) tests: the persistent Gaussian server's register-resident
slice against fp64 numpy, bit-tight, at the sizes where a shard crosses the
per-lane capacity.

At ``FED_PERSIST_GRID=8`` the server has 2048 lanes, so shards of a few
hundred thousand rows fill the resident slots exactly, leave the last one
partly predicated off, or spill over into one or two streamed sweeps.  The
inputs are ``exact_probes.gaussian_probe`` shards: every sum is exact (checked
without a GPU in test_persistent_resident_cpu.py), so a dropped, doubled or
mis-addressed row or slot moves a gradient by a whole unit.
"""
import numpy as np
import pytest
import torch

import exact_probes as ep
import persistent_probes as pp

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.ops import PersistentLinearEngine


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _check_engine(dev, dtype, n):
    p = ep.gaussian_probe(n)
    tdtype = getattr(torch, dtype)
    # torch.tensor copies: the cached probe arrays are read-only
    x = torch.tensor(p["x"], dtype=tdtype, device=dev)
    y = torch.tensor(p["y"], dtype=tdtype, device=dev)
    refs = [ep.gaussian_reference(p["x"], p["y"], a, b) for a, b in ep.GAUSS_THETAS]
    eng = PersistentLinearEngine(x, y, 1.0)
    try:
        for rnd in range(3):
            for (a, b), (logp_r, ga_r, gb_r) in zip(ep.GAUSS_THETAS, refs):
                logp_k, ga_k, gb_k = eng.logp_grad_sync(a, b)
                msg = f"{dtype} n={n} round {rnd} a={a} b={b}"
                assert ga_k == ga_r, f"{msg}: d/da {ga_k!r} != {ga_r!r}"
                assert gb_k == gb_r, f"{msg}: d/db {gb_k!r} != {gb_r!r}"
                assert abs(logp_k - logp_r) <= 2 * np.spacing(abs(logp_r)), (
                    f"{msg}: logp {logp_k!r} vs {logp_r!r}"
                )
    finally:
        eng.close()


def _cases():
    for dtype in sorted(ep.GAUSS_VEC):
        for n in pp.resident_sizes(dtype):
            yield pytest.param(dtype, n, id=f"{dtype}-{n}")


@pytest.mark.parametrize("dtype,n", list(_cases()))
def test_resident_slice_capacity_boundary(dev, monkeypatch, dtype, n):
    """2048 lanes: one slot without / with a tail, the last slot partly
    predicated off, exactly full, one row over, one full streamed sweep plus
    a tail, a ragged second sweep."""
    monkeypatch.setenv("FED_PERSIST_GRID", str(pp.SMALL_GRID))
    _check_engine(dev, dtype, n)


def test_resident_slice_mostly_empty_default_grid(dev, monkeypatch):
    """Default grid (131072 lanes), 512 whole vectors and one tail row: only
    the first two blocks hold a slot, every other block contributes zero."""
    monkeypatch.delenv("FED_PERSIST_GRID", raising=False)
    dtype, n = pp.DEFAULT_GRID_CASE
    _check_engine(dev, dtype, n)


@pytest.mark.parametrize("seqlock", ["0", "1"])
def test_resident_slice_both_request_readers(dev, monkeypatch, seqlock):
    """FED_PK_SEQLOCK picks how block 0 reads the request mailbox (one
    wave-wide read carrying the payload, or detect-then-read); both serve a
    shard with resident slots, a streamed sweep and a tail."""
    monkeypatch.setenv("FED_PERSIST_GRID", str(pp.SMALL_GRID))
    monkeypatch.setenv("FED_PK_SEQLOCK", seqlock)
    dtype = "bfloat16"
    _check_engine(dev, dtype, pp.resident_sizes(dtype)[-2])
