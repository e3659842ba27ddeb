"""GP_Integrate over an ensemble against the host integrator in a loop, same box, same run.

The golden's two models (tests/golden/gp_integrate.npz) stretched to the reference example's 3 750 steps; members are the
golden's mean coefficients x (1 + 0.05 N(0, 1)) from initial states spread over `norms`.  Per ensemble size: wall time of
the device call (upload and fetch included; mean + bounds, and with every member returned), member-steps per second,
the two kernel families' device time from the context's timing table, and the host loop (`GP_Integrate` per member on
ONE thread -- the only way to run it) measured on a sample of members and scaled to the ensemble.

    python tools/integrate_ensemble_probe.py [steps] [sizes ...]     (default: 3750  64 1000 10000)
"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np

from fokl_gpy_amd import _capi, getKernels
from fokl_gpy_amd.GP_Integrate import GP_Integrate, GP_Integrate_ensemble


def box():
    model = 'unknown CPU'
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    try:
        from helpers import host_fingerprint
        fp = host_fingerprint()
    except Exception as exc:                                     # scipy missing: the probe still runs
        fp = f'unavailable ({type(exc).__name__})'
    return f"{model}, {len(os.sched_getaffinity(0))} usable CPUs; numerical-stack fingerprint {fp}"


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3750
    sizes = [int(v) for v in sys.argv[2:]] or [64, 1000, 10000]
    golden = os.path.join(ROOT, 'tests', 'golden')
    g = np.load(os.path.join(golden, 'gp_integrate.npz'))
    phis = getKernels.table_to_phis(np.load(os.path.join(golden, 'spline_phis.npz'))['table'])
    means, mtx = [g['betas0'], g['betas1']], [g['mtx0'], g['mtx1']]
    h, start = float(g['h']), float(g['start'])
    stop = start + steps * h - 1e-9
    b = 0.5 + 0.45 * np.sin(np.arange(steps + 5) / 17.0)          # the golden's forcing, continued
    used = [row for row in g['used']]
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    ctx.timing_enable(True)
    print(f"box: {box()}")
    print(f"system: 2 states + 1 forcing input, models of {mtx[0].shape[0]} and {mtx[1].shape[0]} terms, {steps} steps; "
          f"host loop on 1 thread")
    print(f"{'members':>8} {'device ms':>10} {'+members ms':>12} {'Mmember-steps/s':>16} {'integrate ms':>13} {'band ms':>8} "
          f"{'launches':>9} {'host us/member-step':>20} {'host loop s':>12} {'speed-up':>9} {'max |dev - host|':>17}")
    for E in sizes:
        rng = np.random.default_rng(E)
        draws = [m * (1 + 0.05 * rng.standard_normal((E, m.shape[0]))) for m in means]
        lo, hi = g['norms']
        y0 = lo + (hi - lo) * rng.random((E, 2))
        args = (draws, mtx, b, g['norms'], phis, start, stop, y0, h, used)
        GP_Integrate_ensemble(*args, device=ctx)                  # warm-up: code objects, first allocations
        best, best_members = np.inf, np.inf
        for _ in range(3):
            ctx.timing_reset()
            t0 = time.perf_counter()
            T, mean, bounds = GP_Integrate_ensemble(*args, device=ctx)
            best = min(best, time.perf_counter() - t0)
            ti, tb = ctx.timing_get(_capi.K_INTEGRATE), ctx.timing_get(_capi.K_BAND)
        for _ in range(2):
            t0 = time.perf_counter()
            out = GP_Integrate_ensemble(*args, ReturnMembers=True, device=ctx)
            best_members = min(best_members, time.perf_counter() - t0)
        members = out[3]
        sample = np.unique(np.linspace(0, E - 1, min(E, 24)).astype(int))
        worst = 0.0
        t0 = time.perf_counter()
        for e in sample:
            Y = GP_Integrate([d[e] for d in draws], mtx, b, g['norms'], phis, start, stop, y0[e].copy(), h, used)[1]
            worst = max(worst, float(np.max(np.abs(Y - members[e]))))
        per = (time.perf_counter() - t0) / len(sample)
        print(f"{E:8d} {best * 1e3:10.2f} {best_members * 1e3:12.2f} {E * steps / best / 1e6:16.2f} {ti['ms']:13.2f} "
              f"{tb['ms']:8.2f} {ti['launches']:9d} {per / steps * 1e6:20.3f} {per * E:12.2f} {per * E / best:9.1f} "
              f"{worst:17.2e}", flush=True)
        del members, out
    ctx.close()


if __name__ == '__main__':
    main()
