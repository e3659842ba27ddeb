"""Time of one fokl_population_stats launch (population_kernel + population_reduce_kernel) by the context's own event
timers, as a fraction of the fp64 matrix peak (78.6 TFLOP/s, 2 S ncp E flops), next to population.population_stats_host on
a slice of the rows.

    python tools/propagate_probe.py [--rows 1000000] [--columns 100] [--draws 1000] [--cuts 0 1 32] [--repeat 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
from fokl_gpy_amd import _capi, getKernels  # noqa: E402
from fokl_gpy_amd import population as pop  # noqa: E402

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--columns', type=int, nargs='+', default=[100])
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--cuts', type=int, nargs='+', default=[0, 1, 32])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--host-rows', type=int, default=20000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    S, E = args.rows, args.draws
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    y = rng.standard_normal(S)
    ctx.upload(rng.random((S, 1)), y, getKernels.KERNEL_BERNOULLI, packed, nb, width)
    lines = []
    for nc in args.columns:
        ctx.reserve_slots(nc + 2)
        cols = rng.standard_normal((S, nc - 1))
        for j in range(nc - 1):
            ctx.write_slot(2 + j, cols[:, j])
        slots = np.concatenate([[0], np.arange(2, nc + 1)]).astype(np.int32)
        betas = rng.standard_normal((E, nc)) / np.sqrt(nc)
        shift = betas[:, 0].copy()
        for K in args.cuts:
            cuts = shift[:, None] + rng.standard_normal((E, K))
            ctx.population_stats(slots, betas, shift, cuts, True)               # first launch: code object, buffers
            ctx.timing_enable(True)
            ctx.timing_reset()
            t0 = time.perf_counter()
            for _ in range(args.repeat):
                mom, above = ctx.population_stats(slots, betas, shift, cuts, True)
            wall = (time.perf_counter() - t0) / args.repeat
            timed = ctx.timing_get(_capi.K_POPULATION)
            ctx.timing_enable(False)
            ms = timed['ms'] / max(timed['launches'], 1)
            ncp = (nc + 3) & ~3
            hs = min(S, args.host_rows)
            X = np.concatenate([np.ones((hs, 1)), cols[:hs]], axis=1)
            t0 = time.perf_counter()
            pop.population_stats_host(X, betas, shift, cuts, y[:hs])
            host = (time.perf_counter() - t0) * S / hs
            rec = dict(rows=S, columns=nc, draws=E, cuts=K, kernel_ms=ms, call_ms=1e3 * wall,
                       fraction_of_fp64_peak=2.0 * S * ncp * E / (ms * 1e-3) / PEAK if ms > 0 else None,
                       host_ms_scaled=1e3 * host, report=ctx.population_report())
            lines.append(rec)
            print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
