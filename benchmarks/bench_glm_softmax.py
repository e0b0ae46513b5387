#!/usr/bin/env python3
"""Softmax (multinomial) GLM on the 16-column MFMA kernel
(csrc/glm_family_batched.hip, SoftmaxStage): time per evaluation against two
yardsticks taken in the same run; one JSON line per (K, C).

For bf16 rows, K in {8, ..., 1024} and C in {4, 16}, five things alternate
in one process:

* ``kernel_1``    one ``logp_grad`` on the kernel path (one launch, one of
                  its ``16 // CP`` chain groups in use);
* ``eager_1``     the same evaluation on the model's own eager path;
* ``kernel_16``   ``logp_grad_batched`` at B = 16 on the kernel path:
                  ``ceil(16 / (16 // CP))`` launches (4 at C = 4, 16 at
                  C = 16), packing included;
* ``eager_16``    the same on the eager path;
* ``poisson_16``  ``glm_family_logp_grad_batched`` (Poisson, 16 chains) at
                  the same N and K: one launch that moves the same bytes
                  through the same MFMA phases, so ``kernel_1`` over it is
                  the price of the row-coupled stage.

Times are device events around ``--inner`` back-to-back evaluations, after
``--warmup`` untimed ones; medians and the p10-p90 spread are reported.
``bytes`` is what one pass has to read: X as stored plus y.

    python benchmarks/bench_glm_softmax.py --rows 2000000
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from pytensor_federated_amd.models import SoftmaxGLMModel
from pytensor_federated_amd.ops import glm_family_logp_grad_batched

DEV = "cuda:0"
CHAINS = 16


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


def summary(ms, nbytes, passes=1):
    med = float(np.median(ms))
    return {
        "ms_per_eval": med,
        "ms_p10": float(np.percentile(ms, 10)),
        "ms_p90": float(np.percentile(ms, 90)),
        "passes_over_X": passes,
        "effective_GBps": passes * nbytes / (med * 1e-3) / 1e9,
    }


def random_X(n, K, gen):
    """bf16 [n, K], N(0, 1/K) with an intercept column."""
    X = torch.empty((n, K), device=DEV, dtype=torch.bfloat16)
    step = 1 << 18
    for s in range(0, n, step):
        rows = min(step, n - s)
        X[s : s + rows] = (
            torch.randn((rows, K), device=DEV, generator=gen) / K ** 0.5
        ).to(torch.bfloat16)
    X[:, 0] = 1.0
    return X


def one_config(n, K, C, args):
    gen = torch.Generator(device=DEV).manual_seed(4000 + K + C)
    X = random_X(n, K, gen)
    beta = torch.randn((K, C), device=DEV, generator=gen)
    y = torch.empty(n, dtype=torch.int64, device=DEV)
    step = 1 << 18
    for s in range(0, n, step):
        P = torch.softmax(X[s : s + step].float() @ beta, dim=1)
        y[s : s + step] = torch.multinomial(P, 1, generator=gen)[:, 0]
    m = SoftmaxGLMModel(X, y, C, use_kernels=True)
    assert m._kernel_path() and m._k_pad == 0
    scales = torch.linspace(-1.0, 1.0, CHAINS, device=DEV)
    theta = (beta[:, :, None] * scales[None, None, :]).contiguous()   # [K, C, 16]
    th1 = beta.reshape(K, C, 1)
    # the Poisson yardstick: same X, counts of the same order, 16 chains
    theta_p = (beta[:, 0, None] * 0.5 * scales[None, :]).contiguous()
    y_p = torch.poisson(torch.exp(X.float() @ theta_p[:, -1]), generator=gen)

    fns = [
        lambda: m._eval_kernel(th1),
        lambda: m._eval_eager(th1),
        lambda: m._eval_kernel(theta),
        lambda: m._eval_eager(theta),
        lambda: glm_family_logp_grad_batched(X, y_p, theta_p, link="poisson"),
    ]
    ms = device_ms(fns, args.steps, args.warmup, args.inner)
    logp_k, G_k = m._eval_kernel(theta)
    logp_e, G_e = m._eval_eager(theta)
    torch.cuda.synchronize()
    nbytes = n * K * 2 + n * 4
    launches = -(-CHAINS // m.chains_per_launch)
    med = [float(np.median(v)) for v in ms]
    return {
        "model": "softmax", "dtype": "bf16", "rows": n, "K": K, "C": C,
        "chains_per_launch": m.chains_per_launch, "bytes": int(nbytes),
        "kernel_1": summary(ms[0], nbytes),
        "eager_1": summary(ms[1], nbytes),
        "kernel_16": summary(ms[2], nbytes, launches),
        "eager_16": summary(ms[3], nbytes),
        "poisson_16": summary(ms[4], nbytes),
        "eager_1_over_kernel_1": med[1] / med[0],
        "eager_16_over_kernel_16": med[3] / med[2],
        "kernel_1_over_poisson_16": med[0] / med[4],
        "kernel_16_per_launch_over_poisson_16": med[2] / launches / med[4],
        "logp_max_rel_diff_vs_eager": float(((logp_k - logp_e) / logp_e).abs().max()),
        "grad_max_abs_diff_vs_eager": float((G_k - G_e).abs().max()),
        "grad_max_abs": float(G_e.abs().max()),
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=2_000_000)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--inner", type=int, default=2)
    parser.add_argument("--ks", default="8,16,32,64,128,256,512,1024")
    parser.add_argument("--classes", default="4,16")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for K in (int(k) for k in args.ks.split(",")):
        for C in (int(c) for c in args.classes.split(",")):
            print(json.dumps(one_config(args.rows, K, C, args)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
