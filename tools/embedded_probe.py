"""Throughput of the embedded-GP sampler (fokl_embedded_hmc) on a CSTR-shaped problem: chains x draws on the device,
gradient passes per second per chain and in total, and the time per 1000 draws next to embedded.full_sample_host.

    python tools/embedded_probe.py [--rows 4000] [--terms 10] [--chains 1 8 64 256] [--draws 1000] [--host-draws 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
from fokl_gpy_amd import embedded, getKernels  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4000)
    ap.add_argument('--terms', type=int, default=10)
    ap.add_argument('--chains', type=int, nargs='+', default=[1, 8, 64, 256])
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--host-draws', type=int, default=50)
    ap.add_argument('--leapfrog', type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = args.rows
    inv_t = 1 / 600 + (1 / 300 - 1 / 600) * rng.random(n)
    x = (inv_t - 1 / 600) / (1 / 300 - 1 / 600)
    ca, cb, cc = (0.2 + rng.random(n) for _ in range(3))
    model = embedded.Embedded_GP_Model(embedded.GP(), embedded.GP())
    model.inputs, model.phis = x[:, None], getKernels.sp500()
    model.data = -(np.exp(-100 * inv_t) * ca * cb - np.exp(-200 * inv_t) * cc) + 1e-3 * rng.standard_normal(n)
    model.set_equation(lambda: -(np.exp(-model.Processed_GPs[0]) * ca * cb - np.exp(-model.Processed_GPs[1]) * cc))
    model.discmtx = np.arange(1, args.terms + 1)[:, None]
    model.full_sample(50)                                              # context, upload, first launch
    print(f"{n} rows, {args.terms} terms, D = {2 * (args.terms + 1) + 1}, leapfrog {args.leapfrog}")
    for chains in args.chains:
        t0 = time.perf_counter()
        model.full_sample(args.draws, chains=chains, leapfrog=args.leapfrog)
        dt = time.perf_counter() - t0
        passes = args.draws * args.leapfrog
        print(f"device  {chains:4d} chains x {args.draws} draws: {dt:8.3f} s  = {1e3 * dt / args.draws:7.3f} s per 1000 draws, "
              f"{passes / dt:10.0f} passes/s per chain, {chains * passes / dt:12.0f} in total, acceptance "
              f"{model.diagnostics['acceptance_rate'].mean():.2f}")
    t0 = time.perf_counter()
    model.full_sample_host(args.host_draws, leapfrog=args.leapfrog)
    dt = time.perf_counter() - t0
    print(f"host       1 chain  x {args.host_draws} draws: {dt:8.3f} s  = {1e3 * dt / args.host_draws:7.3f} s per 1000 draws, "
          f"{args.host_draws * args.leapfrog / dt:10.0f} passes/s")


if __name__ == '__main__':
    main()
