#!/usr/bin/env python3
"""Row-group GLM family kernel (csrc/glm_family.hip): time per evaluation,
bytes and effective bandwidth; one JSON line per config.

(a) Poisson, bf16, K in {16, 64, 512}: the fused kernel against the same
    model's eager torch path.
(b) Logistic link at K = 100 (zero-padded to 128) against the existing
    wave-per-row ``logistic_glm_logp_grad`` on the same data padded to 512.
(c) Both kernels at K = 512 (the same layout in both).
(d) 16 chains, Poisson and Gaussian, bf16, K in {16, 128, 512, 1024}: the
    MFMA batched kernel (``logp_grad_batched``'s kernel path) against the
    eager batched path and against 16 back-to-back single-chain kernel
    calls, the three alternating in one process.

Times are device events around ``--inner`` back-to-back evaluations, after
``--warmup`` untimed ones.  In (b) and (c) the two kernels alternate in one
process, and medians, the p10-p90 spread and the difference of their
outputs are reported.  ``bytes`` is what the algorithm has to read,
computed from the shapes: X as stored (padding included) plus y and offset.

    python benchmarks/bench_glm_family.py --rows 2000000
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from pytensor_federated_amd.models import GaussianGLMModel, PoissonGLMModel
from pytensor_federated_amd.ops import glm_family_logp_grad, logistic_glm_logp_grad

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


def summary(ms, nbytes):
    med = float(np.median(ms))
    return {
        "ms_per_eval": med,
        "ms_p10": float(np.percentile(ms, 10)),
        "ms_p90": float(np.percentile(ms, 90)),
        "bytes": int(nbytes),
        "effective_GBps": nbytes / (med * 1e-3) / 1e9,
    }


def random_X(n, K, k_store, gen):
    """bf16 [n, k_store], the first K columns N(0, 1/K), the rest zero."""
    X = torch.zeros((n, k_store), device=DEV, dtype=torch.bfloat16)
    step = 1 << 18
    for s in range(0, n, step):
        rows = min(step, n - s)
        X[s : s + rows, :K] = (
            torch.randn((rows, K), device=DEV, generator=gen) / K ** 0.5
        ).to(torch.bfloat16)
    return X


def poisson_vs_eager(n, K, args):
    gen = torch.Generator(device=DEV).manual_seed(1000 + K)
    X = random_X(n, K, K, gen)
    beta = torch.randn(K, device=DEV, generator=gen) * 0.5
    offset = torch.log(torch.rand(n, device=DEV, generator=gen) * 1.5 + 0.5)
    y = torch.poisson(torch.exp(X.float() @ beta + offset), generator=gen)
    m = PoissonGLMModel(X, y, offset=offset, use_kernels=True)
    assert m._kernel_path() and m._k_pad == 0
    out = torch.empty(1 + K, dtype=torch.float64, device=DEV)
    ms_k, ms_e = device_ms(
        [lambda: m.logp_grad(beta, out=out), lambda: m._logp_grad_eager(beta)],
        args.steps, args.warmup, args.inner,
    )
    logp_k, (g_k,) = m.logp_grad(beta)
    logp_e, (g_e,) = m._logp_grad_eager(beta)
    nbytes = n * K * 2 + 2 * n * 4
    return {
        "config": "a", "link": "poisson", "dtype": "bf16", "rows": n, "K": K,
        "kernel": summary(ms_k, nbytes), "eager": summary(ms_e, nbytes),
        "eager_over_kernel": float(np.median(ms_e) / np.median(ms_k)),
        "logp_rel_diff": abs(float(logp_k) - float(logp_e)) / abs(float(logp_e)),
        "grad_max_abs_diff": float((g_k - g_e).abs().max()),
        "grad_max_abs": float(g_e.abs().max()),
    }


def family_vs_wave_per_row(n, K, k_family, k_wave, label, args):
    gen = torch.Generator(device=DEV).manual_seed(2000 + K)
    Xw = random_X(n, K, k_wave, gen)
    Xf = Xw if k_family == k_wave else Xw[:, :k_family].contiguous()
    beta_w = torch.zeros(k_wave, device=DEV)
    beta_w[:K] = torch.randn(K, device=DEV, generator=gen) * 0.5
    beta_f = beta_w[:k_family].contiguous()
    p = torch.sigmoid(Xw.float() @ beta_w)
    y32 = (torch.rand(n, device=DEV, generator=gen) < p).float()
    y16 = y32.to(torch.bfloat16)
    out_f = torch.empty(1 + k_family, dtype=torch.float64, device=DEV)
    out_w = torch.empty(1 + k_wave, dtype=torch.float64, device=DEV)
    ms_f, ms_w = device_ms(
        [lambda: glm_family_logp_grad(Xf, y32, beta_f, link="logistic", out=out_f),
         lambda: logistic_glm_logp_grad(Xw, y16, beta_w, out=out_w)],
        args.steps, args.warmup, args.inner,
    )
    torch.cuda.synchronize()
    return {
        "config": label, "link": "logistic", "dtype": "bf16", "rows": n, "K": K,
        "family_K": k_family, "wave_per_row_K": k_wave,
        "family": summary(ms_f, n * k_family * 2 + n * 4),
        "wave_per_row": summary(ms_w, n * k_wave * 2 + n * 2),
        "wave_per_row_over_family": float(np.median(ms_w) / np.median(ms_f)),
        "logp_rel_diff": abs(float(out_f[0]) - float(out_w[0])) / abs(float(out_w[0])),
        "grad_max_abs_diff": float((out_f[1 : 1 + K] - out_w[1 : 1 + K]).abs().max()),
        "grad_max_abs": float(out_w[1 : 1 + K].abs().max()),
    }


def batched_vs_eager_vs_single(n, K, family, args):
    gen = torch.Generator(device=DEV).manual_seed(3000 + K)
    X = random_X(n, K, K, gen)
    beta = torch.randn(K, device=DEV, generator=gen) * 0.5
    scales = torch.linspace(-1.0, 1.0, 16, device=DEV)
    theta = (beta[:, None] * scales[None, :]).contiguous()
    if family == "poisson":
        offset = torch.log(torch.rand(n, device=DEV, generator=gen) * 1.5 + 0.5)
        y = torch.poisson(torch.exp(X.float() @ beta + offset), generator=gen)
        m = PoissonGLMModel(X, y, offset=offset, use_kernels=True)
        nbytes = n * K * 2 + 2 * n * 4
    else:
        y = X.float() @ beta + 0.5 * torch.randn(n, device=DEV, generator=gen)
        m = GaussianGLMModel(X, y, 0.5, use_kernels=True)
        nbytes = n * K * 2 + n * 4
    assert m._batched_kernel_path() and m._k_pad == 0
    out1 = torch.empty(1 + K, dtype=torch.float64, device=DEV)
    cols = [theta[:, b].contiguous() for b in range(16)]

    def single16():
        for b in range(16):
            m.logp_grad(cols[b], out=out1)

    steps = max(args.steps // 3, 5)
    ms_k, ms_e, ms_s = device_ms(
        [lambda: m._logp_grad_batched_kernel(theta),
         lambda: m._logp_grad_batched_eager(theta), single16],
        steps, args.warmup, max(args.inner // 2, 1),
    )
    logp_k, G_k = m._logp_grad_batched_kernel(theta)
    logp_e, G_e = m._logp_grad_batched_eager(theta)
    single = [m.logp_grad(cols[b]) for b in range(16)]
    logp_s = torch.stack([s[0] for s in single])
    G_s = torch.stack([s[1][0] for s in single], dim=1)
    torch.cuda.synchronize()
    return {
        "config": "d", "link": family, "dtype": "bf16", "rows": n, "K": K, "chains": 16,
        "batched_kernel": summary(ms_k, nbytes),
        "eager_batched": summary(ms_e, nbytes),
        "single_chain_x16": summary(ms_s, 16 * nbytes),
        "eager_over_kernel": float(np.median(ms_e) / np.median(ms_k)),
        "single_x16_over_kernel": float(np.median(ms_s) / np.median(ms_k)),
        "logp_max_rel_diff_vs_eager": float(((logp_k - logp_e) / logp_e).abs().max()),
        "logp_max_rel_diff_vs_single": float(((logp_k - logp_s) / logp_s).abs().max()),
        "grad_max_abs_diff_vs_eager": float((G_k - G_e).abs().max()),
        "grad_max_abs_diff_vs_single": float((G_k - G_s).abs().max()),
        "grad_max_abs": float(G_s.abs().max()),
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=2_000_000)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--inner", type=int, default=4)
    parser.add_argument("--configs", default="a,b,c")
    parser.add_argument("--batched-k", default="16,128,512,1024",
                        help="feature counts of config d")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    configs = args.configs.split(",")
    if "a" in configs:
        for K in (16, 64, 512):
            print(json.dumps(poisson_vs_eager(args.rows, K, args)), flush=True)
    if "b" in configs:
        print(json.dumps(family_vs_wave_per_row(args.rows, 100, 128, 512, "b", args)), flush=True)
    if "c" in configs:
        print(json.dumps(family_vs_wave_per_row(args.rows, 512, 512, 512, "c", args)), flush=True)
    if "d" in configs:
        for family in ("poisson", "gaussian"):
            for K in (int(k) for k in args.batched_k.split(",")):
                print(json.dumps(batched_vs_eager_vs_single(args.rows, K, family, args)),
                      flush=True)


if __name__ == "__main__":
    main()
