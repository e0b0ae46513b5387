"""What the three GLM shard models share, on a tiny fp64 CPU shard: the
``out=`` seam, batched against per-chain evaluation, the parameter-shape
messages and the shape properties.  Parametrised over the logistic model, the
two link families and the softmax model (N = 5, K = 3, C = 3).
"""
import re

import numpy as np
import pytest
import torch

from pytensor_federated_amd.models import (
    GaussianGLMModel,
    LogisticGLMModel,
    PoissonGLMModel,
    SoftmaxGLMModel,
)

N, K, C = 5, 3, 3


def _shard():
    rng = np.random.RandomState(7)
    return rng.standard_normal((N, K)) / np.sqrt(K), rng


def _logistic():
    X, rng = _shard()
    return LogisticGLMModel(X, (rng.uniform(size=N) < 0.5).astype(np.float64)), (K,)


def _poisson():
    X, rng = _shard()
    offset = np.log(rng.uniform(0.5, 2.0, size=N))
    return PoissonGLMModel(X, rng.poisson(2.0, size=N).astype(np.float64), offset=offset), (K,)


def _gaussian():
    X, rng = _shard()
    return GaussianGLMModel(X, rng.standard_normal(N), 0.7), (K,)


def _softmax():
    X, rng = _shard()
    return SoftmaxGLMModel(X, np.array([0, 2, 1, 1, 0]), C), (K, C)


MODELS = {"logistic": _logistic, "poisson": _poisson, "gaussian": _gaussian, "softmax": _softmax}


@pytest.fixture(params=sorted(MODELS))
def case(request):
    model, shape = MODELS[request.param]()
    return request.param, model, shape


def _params(shape, n, seed=3):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.standard_normal(shape + (n,)) * 0.5)


def test_out_receives_the_fused_result(case):
    _, model, shape = case
    beta = _params(shape, 1)[..., 0]
    logp_ref, (g_ref,) = model.logp_grad(beta)
    assert logp_ref.dtype == torch.float64 and g_ref.dtype == torch.float64
    assert tuple(g_ref.shape) == shape
    buf = torch.full((model.fused_size,), float("nan"), dtype=torch.float64)
    logp, (g,) = model.logp_grad(beta, out=buf)
    # views of buf, not copies
    assert logp.data_ptr() == buf.data_ptr()
    assert g.data_ptr() == buf[1:].data_ptr()
    assert tuple(g.shape) == shape
    torch.testing.assert_close(logp, logp_ref, rtol=0, atol=0)
    torch.testing.assert_close(g, g_ref, rtol=0, atol=0)
    torch.testing.assert_close(buf[0], logp_ref, rtol=0, atol=0)
    torch.testing.assert_close(buf[1:], g_ref.reshape(-1), rtol=0, atol=0)
    buf[1] = 123.0
    assert float(g.reshape(-1)[0]) == 123.0


@pytest.mark.parametrize("B", [1, 3])
def test_batched_equals_per_chain(case, B):
    _, model, shape = case
    theta = _params(shape, B)
    logp, G = model.logp_grad_batched(theta)
    assert tuple(logp.shape) == (B,) and tuple(G.shape) == shape + (B,)
    assert logp.dtype == torch.float64 and G.dtype == torch.float64
    for b in range(B):
        logp_b, (g_b,) = model.logp_grad(theta[..., b])
        np.testing.assert_allclose(logp[b].numpy(), logp_b.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(G[..., b].numpy(), g_b.numpy(), rtol=1e-12, atol=1e-12)


def test_wrong_shapes_raise_the_models_messages(case):
    name, model, shape = case
    if name == "softmax":
        single = "beta must have shape (3, 3), got (4, 3)."
        batched = "theta must be [9, B] or [3, 3, B], got (4, 2)"
    else:
        single = "beta must have shape (3,), got (4,)."
        batched = "theta must be [3, B], got (4, 2)"
    with pytest.raises(ValueError, match="^" + re.escape(single) + "$"):
        model.logp_grad(torch.zeros((4,) + shape[1:], dtype=torch.float64))
    with pytest.raises(ValueError, match="^" + re.escape(batched) + "$"):
        model.logp_grad_batched(torch.zeros((4, 2), dtype=torch.float64))


def test_shape_properties(case):
    name, model, _ = case
    assert model.n_rows == N and type(model.n_rows) is int
    assert model.n_features == K and type(model.n_features) is int
    assert model.fused_size == (1 + K * C if name == "softmax" else 1 + K)
    # a CPU shard is never padded
    assert model._k_eff == K and model._k_pad == 0
    assert model.device == torch.device("cpu")
    assert not model._kernel_path()


@pytest.mark.parametrize(
    "make",
    [
        lambda X, y: LogisticGLMModel(X, y),
        lambda X, y: PoissonGLMModel(X, y),
        lambda X, y: GaussianGLMModel(X, y, 1.0),
        lambda X, y: SoftmaxGLMModel(X, y, 2),
    ],
    ids=["logistic", "poisson", "gaussian", "softmax"],
)
def test_shard_shape_message(make):
    for X, y in [(np.zeros((5, 3)), np.zeros(4)), (np.zeros(5), np.zeros(5)),
                 (np.zeros((5, 3)), np.zeros((5, 1)))]:
        with pytest.raises(ValueError, match=r"^X must be \[N,K\] and y \[N\]\.$"):
            make(X, y)
