"""The multistart optimiser on the device against the host statement, same box, same run.

Two models: (a) the 2-input, 12-term toy model of the tests; (b) an 8-input two-way model of the size a configs[2] fit
selects (32 main effects, orders 1-4 on every input, + 60 two-factor terms = 92 terms, 32 distinct factors).  Draws
are the mean coefficients x (1 + 0.1 N(0, 1)); starts are the deterministic sequence in the whole training range.
Per draws x starts: wall time of `optimize.optimize` (argument handling, upload, the launch, fetch and the assembly of
the per-draw optima and their bounds; one warm-up call, then `repeats` calls: median, minimum and maximum), the kernel's
device time from HIP events (the context's timing table, median), and `optimize.solve_host` -- numpy, a batch of solves
carried through every operation, BLAS held to ONE thread -- measured on at most 4 096 of the solves and scaled.

    python tools/optimize_probe.py [repeats]        (default 7)
"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np

from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd import optimize as opt


def box():
    model = 'unknown CPU'
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    return f"{model}, {len(os.sched_getaffinity(0))} usable CPUs"


def models():
    toy = np.array([[1, 0], [0, 1], [2, 0], [0, 2], [1, 1], [3, 0], [0, 3], [2, 1], [1, 2], [4, 0], [0, 4], [3, 2]])
    toy_mean = np.array([0.3, 0.8, -0.5, 1.5, -1.2, 0.9, 0.7, -0.6, 0.5, 0.4, -2.0, 1.6, 0.8])
    rng = np.random.default_rng(8)
    rows = []
    for j in range(8):
        for order in range(1, 5):
            row = np.zeros(8, dtype=int)
            row[j] = order
            rows.append(row)
    for _ in range(60):
        row = np.zeros(8, dtype=int)
        row[rng.choice(8, 2, replace=False)] = rng.integers(1, 5, 2)
        rows.append(row)
    wide = np.array(rows)
    wide_mean = rng.standard_normal(wide.shape[0] + 1)
    return (('2 inputs, 12 terms', toy, toy_mean, [[0.0, 2.0], [-1.0, 3.0]]),
            ('8 inputs two-way, 92 terms', wide, wide_mean, [[0.0, 1.0]] * 8))


def one_blas_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    phis = getKernels.bernoulli()
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    ctx.timing_enable(True)
    print(f"box: {box()}")
    print(f"device call = optimize.optimize (upload, launch, fetch, assembly), {repeats} calls after one warm-up; "
          f"host = optimize.solve_host on one thread, at most 4096 solves measured and scaled")
    for label, mtx, mean, minmax in models():
        print(f"model: {label}")
        print(f"{'draws':>6} {'starts':>6} {'call ms med':>12} {'min':>8} {'max':>8} {'kernel ms':>10} {'solves/s':>10} "
              f"{'iter mean':>9} {'iter max':>8} {'not conv.':>9} {'host s':>9} {'speed-up':>9} {'max |f - f_host|':>17}")
        for E, S in ((1, 64), (1000, 32), (1000, 64), (10000, 64)):
            rng = np.random.default_rng(E + S)
            betas = mean * (1 + 0.1 * rng.standard_normal((E, mean.shape[0])))
            opt.optimize(betas, mtx, phis, minmax, starts=S, device=ctx, ReturnBounds=E > 1)          # warm-up
            walls, kernels = [], []
            for _ in range(repeats):
                ctx.timing_reset()
                t0 = time.perf_counter()
                res = opt.optimize(betas, mtx, phis, minmax, starts=S, device=ctx, ReturnBounds=E > 1, ReturnAll=True)
                walls.append(time.perf_counter() - t0)
                kernels.append(ctx.timing_get(_capi.K_OPTIMIZE)['ms'])
            sample = min(E, max(1, 4096 // S))
            with one_blas_thread():
                t0 = time.perf_counter()
                host = opt.optimize_host(betas[:sample], mtx, phis, minmax, starts=S, ReturnBounds=False, ReturnAll=True)
                host_s = (time.perf_counter() - t0) * E / sample
            both = (res.status_all[:sample] == opt.CONVERGED) & (host.status_all == opt.CONVERGED) & \
                   (np.max(np.abs(res.x_all[:sample] - host.x_all), axis=-1) <= 1e-3)
            worst = float(np.max(np.abs(res.f_all[:sample] - host.f_all)[both])) if both.any() else float('nan')
            med = float(np.median(walls))
            print(f"{E:6d} {S:6d} {med * 1e3:12.2f} {min(walls) * 1e3:8.2f} {max(walls) * 1e3:8.2f} "
                  f"{float(np.median(kernels)):10.3f} {E * S / med:10.3g} {res.iterations_all.mean():9.1f} "
                  f"{res.iterations_all.max():8d} {int(np.sum(res.status_all != opt.CONVERGED)):9d} {host_s:9.2f} "
                  f"{host_s / med:9.0f} {worst:17.2e}", flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
