#!/usr/bin/env python3
"""GLM Fisher-information kernel (csrc/glm_family_fisher.hip): time per
evaluation of ``H = X^T diag(w) X``, effective FLOP/s and the re-read
factor; one JSON line per K.

Poisson, bf16, K in {16, 128, 512, 1024}, three paths alternating in one
process on the same model:

``kernel``        ``model.fisher_information`` on the MFMA kernel;
``eager``         the same model's eager path (f32 batched matmuls over
                  128-row chains, added in fp64: what meets the accuracy
                  bound of the tests on the GPU);
``plain_matmul``  what a torch user writes first: one f32 ``X^T @ (w X)``
                  per 2^21-row chunk of the up-cast shard (on the accuracy
                  sets its error is up to 133 units of 2^-24 * H_scale,
                  against 16 allowed for the eager path).

Times are device events around ``--inner`` back-to-back evaluations, after
``--warmup`` untimed ones; medians and the p10-p90 spread are reported.
``flops`` is 2*N*K^2 (the full product, as the eager paths compute it; the
kernel computes the upper panel pairs with three bf16 pieces).  ``reread``
is the multiple of the shard the kernel reads (HBM, L2 or Infinity Cache).

    python benchmarks/bench_glm_fisher.py --rows 2000000
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from pytensor_federated_amd.models import PoissonGLMModel

DEV = "cuda:0"


def device_ms(fns, steps, warmup, inner):
    """Per-evaluation milliseconds of each fn, the fns alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    events = [[] for _ in fns]
    for _ in range(steps):
        for i, fn in enumerate(fns):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                fn()
            end.record()
            events[i].append((start, end))
    torch.cuda.synchronize()
    return [np.array([s.elapsed_time(e) / inner for s, e in ev]) for ev in events]


def summary(ms, flops):
    med = float(np.median(ms))
    return {
        "ms_per_eval": med,
        "ms_p10": float(np.percentile(ms, 10)),
        "ms_p90": float(np.percentile(ms, 90)),
        "effective_TFLOPs": flops / (med * 1e-3) / 1e12,
    }


def random_X(n, K, gen):
    X = torch.empty((n, K), device=DEV, dtype=torch.bfloat16)
    step = 1 << 18
    for s in range(0, n, step):
        rows = min(step, n - s)
        X[s : s + rows] = (torch.randn((rows, K), device=DEV, generator=gen) / K ** 0.5).to(
            torch.bfloat16
        )
    return X


def reread_factor(K):
    """Panels of 128 columns: NP per column over the pairs, plus the weights pass."""
    return 1 if K <= 128 else K // 128 + 1


def fisher_case(n, K, args):
    gen = torch.Generator(device=DEV).manual_seed(4000 + K)
    X = random_X(n, K, gen)
    beta = torch.randn(K, device=DEV, generator=gen) * 0.5
    offset = torch.log(torch.rand(n, device=DEV, generator=gen) * 1.5 + 0.5)
    y = torch.poisson(torch.exp(X.float() @ beta + offset), generator=gen)
    m = PoissonGLMModel(X, y, offset=offset, use_kernels=True)
    assert m._fisher_kernel_path() and m._k_pad == 0
    out = torch.empty((K, K), dtype=torch.float64, device=DEV)

    def plain():
        H = torch.zeros((K, K), dtype=torch.float64, device=DEV)
        for s in range(0, n, 1 << 21):
            Xf = X[s : s + (1 << 21)].float()
            w = torch.exp(Xf @ beta + offset[s : s + (1 << 21)])
            H += (Xf.t() @ (w[:, None] * Xf)).double()
        return H

    # the wide cases take tens of milliseconds per evaluation
    steps = args.steps if K <= 128 else max(args.steps // 3, 5)
    inner = args.inner if K <= 128 else 1
    ms_k, ms_e, ms_p = device_ms(
        [lambda: m.fisher_information(beta, out=out), lambda: m._fisher_eager(beta), plain],
        steps, args.warmup, inner,
    )
    H_k = m.fisher_information(beta).clone()
    H_e, H_p = m._fisher_eager(beta), plain()
    torch.cuda.synchronize()
    flops = 2.0 * n * K * K
    scale = float(H_e.abs().max())
    return {
        "link": "poisson", "dtype": "bf16", "rows": n, "K": K,
        "kernel": summary(ms_k, flops), "eager": summary(ms_e, flops),
        "plain_matmul": summary(ms_p, flops),
        "eager_over_kernel": float(np.median(ms_e) / np.median(ms_k)),
        "plain_over_kernel": float(np.median(ms_p) / np.median(ms_k)),
        "reread": reread_factor(K),
        "shard_bytes": n * K * 2,
        "kernel_read_GBps": reread_factor(K) * n * K * 2 / (float(np.median(ms_k)) * 1e-3) / 1e9,
        "symmetric": bool(torch.equal(H_k, H_k.t())),
        "max_abs": scale,
        "kernel_vs_eager_max_abs_diff": float((H_k - H_e).abs().max()),
        "plain_vs_eager_max_abs_diff": float((H_p - H_e).abs().max()),
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=2_000_000)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--inner", type=int, default=4)
    parser.add_argument("--k", default="16,128,512,1024")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for K in (int(k) for k in args.k.split(",")):
        print(json.dumps(fisher_case(args.rows, K, args)), flush=True)


if __name__ == "__main__":
    main()
