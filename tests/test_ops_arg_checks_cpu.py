"""The argument checks the GLM entry points of ``ops`` share, called directly.

They are pure torch, so everything here runs on CPU tensors; the entry
points themselves are exercised on a device by the GPU dispatch tests.
"""
from unittest import mock

import pytest
import torch

from pytensor_federated_amd.ops import (
    _check_design,
    _check_rows,
    _check_sigma,
    _design_shape,
    _out_buffer,
)

N, K = 4, 8


def _design():
    return torch.zeros((N, K), dtype=torch.bfloat16)


def test_design_shape():
    assert _design_shape(_design()) == (N, K)
    for bad in (torch.zeros(K), torch.zeros((2, N, K))):
        with pytest.raises(ValueError, match=r"X must be \[N, K\]"):
            _design_shape(bad)


def test_check_design():
    # accepted: a well-formed shard on a device (is_cuda is all that tells a
    # CPU tensor from one)
    with mock.patch.object(
        torch.Tensor, "is_cuda", new_callable=mock.PropertyMock, return_value=True
    ):
        _check_design(_design())
    with pytest.raises(ValueError, match="ROCm device"):
        _check_design(_design())
    with pytest.raises(ValueError, match="X must be contiguous"):
        _check_design(torch.zeros((K, N), dtype=torch.bfloat16).t())
    with pytest.raises(ValueError, match="X must be contiguous"):
        _check_design(torch.zeros((N, 2 * K), dtype=torch.bfloat16)[:, ::2])
    base = torch.zeros(N * K + 4, dtype=torch.bfloat16)
    assert base.data_ptr() % 16 == 0
    shifted = base[4:].view(N, K)  # contiguous, 8 bytes past a 16-byte boundary
    assert shifted.is_contiguous()
    with pytest.raises(ValueError, match="16-byte aligned"):
        _check_design(shifted)


def test_check_rows():
    X = _design()
    _check_rows("y", torch.zeros(N), X)
    _check_rows("offset", torch.zeros(N), X)
    for name in ("y", "offset"):
        with pytest.raises(ValueError, match=f"{name} must be f32"):
            _check_rows(name, torch.zeros(N, dtype=torch.float64), X)
        with pytest.raises(ValueError, match=f"{name} must be f32"):
            _check_rows(name, torch.zeros(N + 1), X)
        with pytest.raises(ValueError, match=f"{name} must be f32"):
            _check_rows(name, torch.zeros((N, 1)), X)
        with pytest.raises(ValueError, match=f"{name} must be contiguous"):
            _check_rows(name, torch.zeros(2 * N)[::2], X)


def test_check_sigma():
    _check_sigma(1.0)
    _check_sigma(1e-30)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma must be positive"):
            _check_sigma(bad)


@pytest.mark.parametrize("shape", [(1 + K,), (K, K)])
def test_out_buffer(shape):
    X = _design()
    fresh = _out_buffer(None, shape, X)
    assert fresh.dtype == torch.float64 and tuple(fresh.shape) == shape
    assert fresh.device == X.device and fresh.is_contiguous()
    given = torch.zeros(shape, dtype=torch.float64)
    assert _out_buffer(given, shape, X) is given

    dims = ", ".join(str(d) for d in shape)
    msg = rf"out must be a contiguous fp64\[{dims}\] on X's device"
    with pytest.raises(ValueError, match=msg):
        _out_buffer(torch.zeros(shape, dtype=torch.float32), shape, X)
    with pytest.raises(ValueError, match=msg):
        _out_buffer(torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=torch.float64), shape, X)
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=torch.float64)
    with pytest.raises(ValueError, match=msg):
        _out_buffer(wide[..., ::2], shape, X)
