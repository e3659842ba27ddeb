"""Kernel and call time of fokl_resample_chains for chains in {1, 64, 1024, 4096} x 10 000 iterations at P + 1 in {28, 100, 300},
with rows kept (what keep='betas' moves) and without (keep=None), next to (a) the host statement resample.chains_host
(timed on a few hundred iterations of one chain, scaled) and (b) the only other route to the same draws: _capi.gibbs_chain
on a LegacyStream, once per chain, one thread (one chain timed, scaled by the number of chains).

Asserted: at every P + 1, 1 024 chains take less than 4 x the kernel time of one chain of the same length -- they occupy one
wavefront slot each on 256 CUs x 4 SIMDs; anything worse means the chains are serialised somewhere.

    python tools/resample_probe.py [--iterations 10000] [--columns 28 100 300] [--chains 1 64 1024 4096] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
from fokl_gpy_amd import _capi  # noqa: E402
from fokl_gpy_amd import resample as R  # noqa: E402

ROW_LIMIT = 4 << 30             # rows are copied to the host: larger sets are timed without rows only


def spectrum(p1, n=100_000):
    rng = np.random.default_rng(p1)
    lamb = n * np.sort(rng.uniform(0.01, 1.0, p1))
    beta = rng.standard_normal(p1)
    return dict(lamb=lamb, qty=lamb * beta, shift=beta, dtd=float(np.sum(lamb * beta * beta) + n * 0.04),
                astar=4 + 1 + n / 2 + p1 / 2, atau_star=4 + (p1 - 1) / 2, b=0.8, btau=3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=10000)
    ap.add_argument('--columns', type=int, nargs='+', default=[28, 100, 300])
    ap.add_argument('--chains', type=int, nargs='+', default=[1, 64, 1024, 4096])
    ap.add_argument('--host-iterations', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    its = args.iterations
    lines = [f"fokl_resample_chains, {its} iterations per chain; times in ms",
             "  P+1 chains rows | instance grid | kernel_ms  us/iteration  call_ms | statement_ms (scaled)  gibbs_chain_ms "
             "(one thread, scaled) | attempts  most"]
    ratios = {}
    for p1 in args.columns:
        s = spectrum(p1)
        model = (s['lamb'], s['qty'], s['shift'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'])
        ctx.resample_chains(*model, [0.16], [0.6], 0, 8, 1, 0, rows=False)                 # code object
        t0 = time.perf_counter()
        R.chains_host(*model, [0.16], [0.6], 0, args.host_iterations, 1, 0, rows=False)
        host_one = (time.perf_counter() - t0) * its / args.host_iterations
        np.random.seed(0)
        t0 = time.perf_counter()
        _capi.gibbs_chain(s['lamb'], s['qty'], s['astar'], s['atau_star'], s['b'], s['btau'], s['dtd'], 0.16, 0.6, its,
                          _capi.LegacyStream())
        parent_one = time.perf_counter() - t0
        kernel = {}
        for chains in args.chains:
            sig0, tau0 = np.full(chains, 0.16), np.full(chains, 0.6)
            for rows in (False, True):
                if rows and chains * its * p1 * 8 > ROW_LIMIT:
                    lines.append(f"{p1:5d} {chains:6d}  yes | rows of {chains * its * p1 * 8 / 2 ** 30:.1f} GiB: not timed")
                    continue
                t0 = time.perf_counter()
                ctx.resample_chains(*model, sig0, tau0, 0, its, 1, 0, rows=rows)
                call = time.perf_counter() - t0
                rep = ctx.resample_report()
                if not rows:
                    kernel[chains] = rep['kernel_ms']
                lines.append(f"{p1:5d} {chains:6d} {'yes' if rows else ' no':>4s} | {rep['instance']:8d} {rep['grid']:4d} | "
                             f"{rep['kernel_ms']:9.2f} {1e3 * rep['kernel_ms'] / its:13.3f} {1e3 * call:8.1f} | "
                             f"{1e3 * host_one * chains:14.0f} {1e3 * parent_one * chains:22.0f} | {rep['attempts']:9d} "
                             f"{rep['attempts_max']:5d}")
                print(lines[-1], flush=True)
        if 1 in kernel and 1024 in kernel:
            ratios[p1] = kernel[1024] / kernel[1]
            lines.append(f"{p1:5d} : 1 024 chains take {ratios[p1]:.2f} x the kernel time of one chain")
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    ctx.close()
    for p1, ratio in ratios.items():
        assert ratio < 4.0, f"P + 1 = {p1}: 1 024 chains take {ratio:.2f} x the time of one -- the chains are serialised somewhere"


if __name__ == '__main__':
    main()
