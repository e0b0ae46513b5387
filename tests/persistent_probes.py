"""Probe sizes for the persistent Gaussian server's register-resident slice.

Plain helper module (imported by ``test_persistent_resident_cpu.py`` and
``test_gpu_persistent_resident.py``).  The server keeps the first ``PK_CAP``
16-byte vectors of every lane in registers and streams the rest; at
``FED_PERSIST_GRID=8`` (2048 lanes) small shards cross that boundary.  The
data are ``exact_probes.gaussian_probe`` shards, so every sum is exact and
the kernel is held to the fp64 numpy reference bit-tight.
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import Tuple

import exact_probes as ep

#: resident vector pairs per lane -- must equal PK_CAP in glm_gaussian.hip
#: (checked by test_persistent_resident_cpu.py)
PK_CAP = 16
#: lanes at FED_PERSIST_GRID=8
SMALL_GRID = 8
LANES = SMALL_GRID * 256

#: default grid (512 blocks): most blocks hold nothing
DEFAULT_GRID_CASE = ("bfloat16", 4097)

KERNEL_SOURCE = (
    Path(__file__).resolve().parent.parent
    / "pytensor_federated_amd" / "ops" / "csrc" / "glm_gaussian.hip"
)


def source_pk_cap() -> int:
    m = re.search(r"^#define\s+PK_CAP\s+(\d+)\s*$", KERNEL_SOURCE.read_text(), re.M)
    assert m, "PK_CAP not found in glm_gaussian.hip"
    return int(m.group(1))


def resident_sizes(dtype_name: str) -> Tuple[int, ...]:
    """With V rows per 16-byte vector, S lanes and full = PK_CAP*S*V rows of
    capacity: a single slot without and with a tail; the last slot partly
    predicated off plus a scalar tail; exactly full; one row over; one full
    streamed sweep plus a tail; a ragged second sweep."""
    v, s = ep.GAUSS_VEC[dtype_name], LANES
    full = PK_CAP * s * v
    return (
        1,
        v * s + 3,
        full - 1,
        full,
        full + 1,
        full + v * s + 3,
        full + 2 * v * s + v + 1,
    )
