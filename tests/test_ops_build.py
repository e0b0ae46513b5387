"""Staleness check of the HIP extension build (no GPU, no compiler needed).

The GLM kernels are several ``.hip`` units sharing ``fed_common.hpp``, so a
header edit must trigger a rebuild just like a source edit does.  A
temporary directory stands in for ``csrc`` and the built library.
"""
import os

from pytensor_federated_amd.ops.build import needs_rebuild


def _touch(path, mtime):
    path.write_text("")
    os.utime(path, (mtime, mtime))


def _tree(tmp_path, hip_mtime, hpp_mtime, lib_mtime):
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    _touch(csrc / "a.hip", hip_mtime)
    _touch(csrc / "common.hpp", hpp_mtime)
    lib = tmp_path / "libfedops.so"
    if lib_mtime is not None:
        _touch(lib, lib_mtime)
    return csrc, lib


def test_fresh_when_nothing_touched(tmp_path):
    csrc, lib = _tree(tmp_path, 1000, 1000, 2000)
    assert needs_rebuild(csrc, lib) is False


def test_stale_when_header_is_newer(tmp_path):
    csrc, lib = _tree(tmp_path, 1000, 3000, 2000)
    assert needs_rebuild(csrc, lib) is True


def test_stale_when_source_is_newer(tmp_path):
    csrc, lib = _tree(tmp_path, 3000, 1000, 2000)
    assert needs_rebuild(csrc, lib) is True


def test_stale_when_library_missing(tmp_path):
    csrc, lib = _tree(tmp_path, 1000, 1000, None)
    assert needs_rebuild(csrc, lib) is True
