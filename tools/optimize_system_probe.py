"""The constrained system optimiser on the device: time of the call and of the kernel, iterations and statuses.

Three systems: (1) one model -- the 8-input two-way model of tools/optimize_probe.py (92 terms, 32 distinct factors) --
whose first input is maximised while its output stays inside a band; (2) the two-model, 8-variable system and (3) the three-model, 16-variable system with an
intermediate of tests/test_optimize_system_gpu.py.  Draws are the mean coefficients x (1 + 0.1 N(0, 1)); starts are the
deterministic sequence in the variables' boxes.  Per system and draws x starts: wall time of `optimize.optimize_system`
(argument handling, upload, the launches, fetch, assembly; one warm-up call, then `repeats` calls: median, minimum,
maximum), the kernel's device time from HIP events (the context's timing table: sum over the call's launches, median
over the calls) and the number of launches, iterations per solve and the status histogram (0 converged ... 4 infeasible).

Every measurement is a child process of its own under a time limit; the first one that fails ends the run.

    python tools/optimize_system_probe.py [repeats]        (default 7)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

SIZES = ((1000, 32), (1000, 64))
LIMIT_S = 300


def one_model(draws):
    import numpy as np
    from fokl_gpy_amd import getKernels
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
    mtx = np.array(rows)
    mean = rng.standard_normal(mtx.shape[0] + 1)
    betas = mean * (1 + 0.1 * np.random.default_rng(draws).standard_normal((draws, mean.shape[0])))
    model = dict(betas=betas, mtx=mtx, phis=getKernels.bernoulli(), minmax=[[0.0, 1.0]] * 8, kernel='Bernoulli Polynomials')
    return ([model], [[f'x{j}' for j in range(8)]], ['y'], 'x0'), \
        dict(sense='max', constraints={'y': (float(mean[0]) - 0.5, float(mean[0]) + 0.5)})


def measure(which, E, S, repeats):
    import numpy as np
    from fokl_gpy_amd import _capi
    from fokl_gpy_amd import optimize as opt
    if which == 1:
        args, kw = one_model(E)
    else:
        import test_optimize_system_gpu as cases
        args, kw = cases.system({2: 'eight', 3: 'sixteen'}[which], E)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    ctx.timing_enable(True)
    opt.optimize_system(*args, starts=S, device=ctx, **kw)                                        # warm-up
    walls, kernels, launches = [], [], 0
    for _ in range(repeats):
        ctx.timing_reset()
        t0 = time.perf_counter()
        res = opt.optimize_system(*args, starts=S, device=ctx, ReturnAll=True, **kw)
        walls.append(time.perf_counter() - t0)
        timed = ctx.timing_get(_capi.K_OPTIMIZE_SYSTEM)
        kernels.append(timed['ms'])
        launches = timed['launches']
    med = float(np.median(walls))
    n_terms = sum(np.atleast_2d(m['mtx']).shape[0] for m in args[0])
    print(f"{which:6d} {len(res.variables):4d} {n_terms:5d} {len(res.constraint_names):4d} {E:6d} {S:6d} {med * 1e3:12.2f} "
          f"{min(walls) * 1e3:8.2f} {max(walls) * 1e3:8.2f} {float(np.median(kernels)):10.3f} {launches:8d} "
          f"{E * S / med:10.3g} {res.iterations_all.mean():9.1f} {res.iterations_all.max():8d}   "
          f"{np.bincount(res.status_all.ravel(), minlength=5).tolist()}", flush=True)
    ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--case':
        measure(*(int(a) for a in sys.argv[2:6]))
        return 0
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    print(f"device call = optimize.optimize_system (upload, launches, fetch, assembly), {repeats} calls after one warm-up")
    print(f"{'models':>6} {'vars':>4} {'terms':>5} {'cons':>4} {'draws':>6} {'starts':>6} {'call ms med':>12} {'min':>8} "
          f"{'max':>8} {'kernel ms':>10} {'launches':>8} {'solves/s':>10} {'iter mean':>9} {'iter max':>8}   statuses 0-4",
          flush=True)
    for which in (1, 2, 3):
        for E, S in SIZES:
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(which), str(E), str(S),
                                       str(repeats)], timeout=LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"system {which}, {E} x {S}: no result within {LIMIT_S} s; stopping", flush=True)
                return 124
            if done.returncode != 0:
                print(f"system {which}, {E} x {S}: exit status {done.returncode}; stopping", flush=True)
                return done.returncode if done.returncode > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
