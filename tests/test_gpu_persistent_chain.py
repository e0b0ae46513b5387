"""GPU (MI355X) tests: the persistent Gaussian server's hand-off chain.

Theta, the per-block partials and the result travel as tagged 8-byte
granules, with no flag, drain, ticket or completion barrier between calls.
What could go wrong is a value accepted from the PREVIOUS call.  Every case
therefore cycles 80 thetas, consecutive ones different, on
``exact_probes.gaussian_probe`` shards whose sums are exact (checked without
a GPU in test_persistent_chain_cpu.py): a stale theta, partial or result
moves a gradient by whole units.  Gradients are compared with ``==`` and logp
within 2 ulp of the fp64 numpy reference, as in
test_gpu_persistent_resident.py.
"""
import time

import numpy as np
import pytest
import torch

import chain_probes as cp
import exact_probes as ep

pytestmark = pytest.mark.gpu

from pytensor_federated_amd.ops import PersistentLinearEngine


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("FED_PERSIST_GRID", raising=False)
    else:
        monkeypatch.setenv("FED_PERSIST_GRID", str(grid))


def _open(dev, dtype, n):
    p = ep.gaussian_probe(n)
    tdtype = getattr(torch, dtype)
    # torch.tensor copies: the cached probe arrays are read-only
    x = torch.tensor(p["x"], dtype=tdtype, device=dev)
    y = torch.tensor(p["y"], dtype=tdtype, device=dev)
    return PersistentLinearEngine(x, y, 1.0)


def _serve(eng, refs, calls, first=0, what=""):
    """`calls` consecutive calls walking the thetas from position `first`."""
    for c in range(first, first + calls):
        a, b = cp.THETAS[c % len(cp.THETAS)]
        logp_r, ga_r, gb_r = refs[c % len(cp.THETAS)]
        logp_k, ga_k, gb_k = eng.logp_grad_sync(a, b)
        msg = f"{what} call {c} a={a} b={b}"
        assert ga_k == ga_r, f"{msg}: d/da {ga_k!r} != {ga_r!r}"
        assert gb_k == gb_r, f"{msg}: d/db {gb_k!r} != {gb_r!r}"
        assert abs(logp_k - logp_r) <= 2 * np.spacing(abs(logp_r)), (
            f"{msg}: logp {logp_k!r} vs {logp_r!r}"
        )


def _run(dev, monkeypatch, case, calls):
    dtype, grid, n = case
    _set_grid(monkeypatch, grid)
    refs = cp.references(n)
    eng = _open(dev, dtype, n)
    try:
        _serve(eng, refs, calls, what=f"{dtype} grid {grid} n={n}")
    finally:
        eng.close()


@pytest.mark.parametrize(
    "case", [cp.STALE_SMALL, cp.STALE_DEFAULT], ids=["grid8", "default-grid"]
)
def test_no_value_of_the_previous_call_is_accepted(dev, monkeypatch, case):
    """4,000 consecutive calls on one engine: 8 blocks with resident slots, a
    streamed sweep and a tail; and the default 512 blocks, most of them
    contributing zero."""
    _run(dev, monkeypatch, case, 4000)


def test_uneven_load_across_blocks(dev, monkeypatch):
    """64 blocks (8 per XCD): the first 20 stream one extra vector, the rest
    work from registers only, and there is a scalar tail -- blocks finish at
    different times."""
    _run(dev, monkeypatch, cp.UNEVEN, 400)


@pytest.mark.parametrize("case", cp.DTYPES, ids=[c[0] for c in cp.DTYPES])
def test_other_instantiations(dev, monkeypatch, case):
    _run(dev, monkeypatch, case, 400)


def test_tag_wrap(dev, monkeypatch):
    """The tags are the low 32 bits of the sequence: start 200 calls below
    the wrap and serve 400."""
    monkeypatch.setenv("FED_PK_SEQ0", str(2 ** 32 - 200))
    _run(dev, monkeypatch, cp.STALE_SMALL, 400)


def test_relaunch_serves_the_pending_request_once(dev, monkeypatch):
    """After an idle self-exit the next call relaunches the server at the
    host's sequence with every tag re-initialised: that call and the 599
    after it are exact, although the partial slots and the result line still
    held the exited kernel's granules."""
    dtype, grid, n = cp.STALE_SMALL
    _set_grid(monkeypatch, grid)
    refs = cp.references(n)
    eng = _open(dev, dtype, n)
    try:
        _serve(eng, refs, 300, what="before idle")
        assert eng.relaunch_count == 0
        time.sleep(2.5)  # past the 1.5 s idle lifetime
        _serve(eng, refs, 1, first=300, what="first after idle")
        if eng.relaunch_count == 0:
            pytest.skip("the server had not exited after 2.5 s idle; nothing relaunched")
        assert eng.relaunch_count >= 1
        _serve(eng, refs, 599, first=301, what="after relaunch")
    finally:
        eng.close()
