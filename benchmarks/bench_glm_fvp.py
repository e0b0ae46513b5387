#!/usr/bin/env python3
"""GLM Fisher-vector kernel (csrc/glm_family_fvp.hip): time per product
``H v = X^T (w * (X v))`` and per diagonal, against one ``logp_grad`` on the
same shard; one JSON line per case.

Poisson, bf16, K in {16, 128, 512, 1024, 2048}; the paths alternate in one
process on the same model:

``product``     ``model.fisher_vector_product`` on the row-group kernel;
``diagonal``    ``model.fisher_diagonal`` on the same kernel;
``logp_grad``   ``model.logp_grad`` (csrc/glm_family.hip): the yardstick, one
                pass over X in the same geometry;
``eager``       the same model's eager product (two f32 matmuls per
                2^21-row chunk of the up-cast shard);
``fisher``      ``model.fisher_information`` on the MFMA kernel, where it has
                one (K <= 1024): what a dense Newton step pays.

Times are device events around ``--inner`` back-to-back evaluations, after
``--warmup`` untimed ones; medians and the p10-p90 spread are reported.
``read_GBps`` is the shard's bytes over the median time: every path but
``fisher`` reads X once.

A last line (``"case": "map"``) times a whole MAP at K = 512 from zero on
the kernel model, host clock around a run that ends on the host:
``find_map_newton_cg`` with the Jacobi preconditioner against
``find_map_newton``.

    python benchmarks/bench_glm_fvp.py --rows 2000000
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from pytensor_federated_amd.inference import find_map_newton, find_map_newton_cg
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


def summary(ms, shard_bytes):
    med = float(np.median(ms))
    return {
        "ms_per_eval": med,
        "ms_p10": float(np.percentile(ms, 10)),
        "ms_p90": float(np.percentile(ms, 90)),
        "read_GBps": shard_bytes / (med * 1e-3) / 1e9,
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


def poisson_model(n, K):
    gen = torch.Generator(device=DEV).manual_seed(4000 + K)
    X = random_X(n, K, gen)
    beta = torch.randn(K, device=DEV, generator=gen) * 0.5
    offset = torch.log(torch.rand(n, device=DEV, generator=gen) * 1.5 + 0.5)
    y = torch.poisson(torch.exp(X.float() @ beta + offset), generator=gen)
    m = PoissonGLMModel(X, y, offset=offset, use_kernels=True)
    assert m._fvp_kernel_path() and m._k_pad == 0
    return m, beta, gen


def fvp_case(n, K, args):
    m, beta, gen = poisson_model(n, K)
    v = torch.randn(K, device=DEV, generator=gen)
    out = torch.empty(K, dtype=torch.float64, device=DEV)
    out_lg = torch.empty(1 + K, dtype=torch.float64, device=DEV)
    with_fisher = m._X.dtype == torch.bfloat16 and K <= 1024
    names = ["product", "diagonal", "logp_grad", "eager"]
    fns = [
        lambda: m.fisher_vector_product(beta, v, out=out),
        lambda: m.fisher_diagonal(beta, out=out),
        lambda: m.logp_grad(beta, out=out_lg),
        lambda: m._fisher_vector_eager(beta, v),
    ]
    if with_fisher:
        assert m._fisher_kernel_path()
        out_H = torch.empty((K, K), dtype=torch.float64, device=DEV)
        names.append("fisher")
        fns.append(lambda: m.fisher_information(beta, out=out_H))
    all_ms = device_ms(fns, args.steps, args.warmup, args.inner)
    Hv_k = m.fisher_vector_product(beta, v).clone()
    Hv_e = m._fisher_vector_eager(beta, v)
    torch.cuda.synchronize()
    shard_bytes = n * K * 2
    res = {"case": "product", "link": "poisson", "dtype": "bf16", "rows": n, "K": K,
           "shard_bytes": shard_bytes}
    for name, ms in zip(names, all_ms):
        res[name] = summary(ms, shard_bytes)
    med = {name: float(np.median(ms)) for name, ms in zip(names, all_ms)}
    res["product_over_logp_grad"] = med["product"] / med["logp_grad"]
    res["diagonal_over_logp_grad"] = med["diagonal"] / med["logp_grad"]
    res["eager_over_product"] = med["eager"] / med["product"]
    if with_fisher:
        res["fisher_over_product"] = med["fisher"] / med["product"]
    res["max_abs"] = float(Hv_e.abs().max())
    res["kernel_vs_eager_max_abs_diff"] = float((Hv_k - Hv_e).abs().max())
    return res


def map_case(n, K, args):
    m, _, _ = poisson_model(n, K)
    lg, hv, dg, H = (m.as_logp_grad_func(), m.as_fisher_vector_func(),
                     m.as_fisher_diagonal_func(), m.as_fisher_func())

    def run_cg():
        return find_map_newton_cg(lg, hv, np.zeros(K), fisher_diagonal_funcs=dg)

    def run_newton():
        return find_map_newton(lg, H, np.zeros(K))

    res = {"case": "map", "link": "poisson", "dtype": "bf16", "rows": n, "K": K}
    results = {}
    for name, run in (("newton_cg", run_cg), ("newton", run_newton)):
        run()  # warm-up
        times = []
        for _ in range(args.map_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        results[name] = r
        res[name] = {
            "seconds": float(np.median(times)), "seconds_min": float(np.min(times)),
            "n_steps": int(r.n_steps), "converged": bool(r.converged), "logp": float(r.logp),
        }
    cg, nt = results["newton_cg"], results["newton"]
    res["newton_cg"]["n_products"] = int(cg.n_products)
    res["newton_cg"]["wire_doubles"] = int(K * (cg.n_products + cg.n_steps))
    res["newton"]["wire_doubles"] = int(K * K * (nt.n_steps + 1))
    res["newton_over_newton_cg"] = res["newton"]["seconds"] / res["newton_cg"]["seconds"]
    res["theta_max_abs_diff"] = float(np.max(np.abs(cg.theta - nt.theta)))
    return res


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=2_000_000)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--inner", type=int, default=4)
    parser.add_argument("--k", default="16,128,512,1024,2048")
    parser.add_argument("--map-k", type=int, default=512, help="0 skips the MAP case")
    parser.add_argument("--map-repeats", type=int, default=3)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for K in (int(k) for k in args.k.split(",") if k):
        print(json.dumps(fvp_case(args.rows, K, args)), flush=True)
        torch.cuda.empty_cache()
    if args.map_k:
        print(json.dumps(map_case(args.rows, args.map_k, args)), flush=True)


if __name__ == "__main__":
    main()
