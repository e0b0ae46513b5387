"""Thetas and shard sizes for the persistent Gaussian server's hand-off chain.

Plain helper module (imported by ``test_persistent_chain_cpu.py`` and
``test_gpu_persistent_chain.py``).  The server hands theta, the per-block
partials and the result from one party to the next as tagged 8-byte granules;
a value taken from the PREVIOUS call must show.  So consecutive calls use
different thetas, and the data are ``exact_probes.gaussian_probe`` shards on
which every sum is exact: a stale theta, partial or result then moves a
gradient by whole units instead of hiding in a tolerance.
"""
from __future__ import annotations

import functools
from typing import Tuple

import numpy as np

import exact_probes as ep
import persistent_probes as pp


def _thetas() -> Tuple[Tuple[float, float], ...]:
    """Every (a, b) with a, b multiples of 1/4 in [-1, 1] except (0, 0): 80
    pairs, in a fixed shuffled order."""
    q = [k / 4.0 for k in range(-4, 5)]
    pairs = [(a, b) for a in q for b in q if (a, b) != (0.0, 0.0)]
    order = np.random.RandomState(20240).permutation(len(pairs))
    return tuple(pairs[i] for i in order)


THETAS = _thetas()

#: (dtype, FED_PERSIST_GRID or None for the default 512, n)
STALE_SMALL = ("bfloat16", pp.SMALL_GRID, pp.resident_sizes("bfloat16")[-2])
STALE_DEFAULT = ("bfloat16", None, 4097)
#: 64 blocks: the first 20 stream one vector beyond the 16 resident ones, the
#: rest are register-only, and there is a 5-row scalar tail
UNEVEN = ("bfloat16", 64, 64 * 256 * 16 * 8 + 8 * 256 * 20 + 5)
DTYPES = (
    ("float32", pp.SMALL_GRID, pp.resident_sizes("float32")[-1]),
    ("float64", pp.SMALL_GRID, pp.resident_sizes("float64")[-1]),
)
CASES = (STALE_SMALL, STALE_DEFAULT, UNEVEN) + DTYPES


def lanes_of(grid) -> int:
    return (512 if grid is None else grid) * 256


@functools.lru_cache(maxsize=None)
def references(n: int):
    """fp64 numpy reference (logp, d/da, d/db) for every theta, computed once
    per shard size and shared."""
    p = ep.gaussian_probe(n)
    return tuple(ep.gaussian_reference(p["x"], p["y"], a, b) for a, b in THETAS)
