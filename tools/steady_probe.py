"""Kernel time of dynamics.steady_states (steady_states_kernel by the context's own events) on tools/simulate_probe.py's first
system, (states, terms per model, draws) = (2, 30, 1 000), from 16 starts at (operating points, draws, starts) = (1, 1 000, 16)
and (64, 1 000, 16), next to the host statement dynamics.steady_states_host on a slice (the first point, the first 20 draws),
scaled to the whole.  With each: how the members ended, iterations and halvings per member, distinct roots per draw.

    python tools/steady_probe.py [--repeat 3] [--out FILE]

Every case runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child
that fails or runs out of time ends the probe and nothing more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.normpath(os.path.join(HERE, '..')))
sys.path.insert(0, HERE)

SYSTEM = (2, 30, 1000)
STARTS = 16
POINTS = (1, 64)
HOST_DRAWS = 20
KERNELS = ('Bernoulli Polynomials', 'Cubic Splines')
HEADER = ("# tools/steady_probe.py on one MI355X: kernel_ms = the launches of steady_states_kernel by the context's events, the best\n"
          "# of the calls; call_ms = the whole call (upload, fetch, eigenvalues and roots on the host included); host_ms_scaled = the\n"
          "# host statement on the first point and the first 20 draws, times (points x draws) / 20; status = how many members ended\n"
          "# converged, at the iteration limit, stalled, not finite; roots = how many (point, draw) have 0, 1, 2, ... distinct roots\n")


def one(args):
    from fokl_gpy_amd import _capi, dynamics
    from simulate_probe import system

    n_states, n_terms, draws = SYSTEM
    Q, kernel = POINTS[args.case], KERNELS[args.kernel]
    full = system(n_states, n_terms, draws, Q, kernel, np.random.default_rng(0))
    sysargs = dict(models=full['models'], states=full['states'], inputs=full['inputs'])
    at = {'u': np.linspace(1.5, 8.5, Q) if Q > 1 else np.array([5.0])}
    rec = dict(states=n_states, terms=n_terms, points=Q, draws=draws, starts=STARTS, kernel=kernel)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    call = lambda: dynamics.steady_states(**sysargs, at=at, starts=STARTS, device=ctx)
    call()                                                             # first launch: code object
    ctx.timing_enable(True)
    kernel_ms, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = call()
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    call_ms = 1e3 * (time.perf_counter() - t0) / args.repeat
    ctx.timing_enable(False)
    rep = ctx.steady_report()
    ctx.close()
    members = Q * draws * STARTS
    rec.update(kernel_ms=min(kernel_ms), call_ms=call_ms, launches=rep['launches'], workgroups=rep['workgroups'],
               lds_bytes=rep['lds_bytes'], status=np.bincount(res.status.ravel(), minlength=4).tolist(),
               iterations_mean=rep['iterations'] / members, iterations_max=int(res.iterations.max()),
               halvings_mean=rep['halvings'] / members, on_wall_fraction=float(res.on_wall.any(axis=-1).mean()),
               roots=np.bincount(res.n_roots.ravel()).tolist(), stable_roots_mean=float(res.n_stable.mean()),
               unique_fraction_mean=float(res.unique_fraction.mean()))
    small = {name: values[:1] for name, values in at.items()}
    t0 = time.perf_counter()
    host = dynamics.steady_states_host(**sysargs, at=small, starts=STARTS, draws=np.arange(HOST_DRAWS))
    rec.update(host_ms_scaled=1e3 * (time.perf_counter() - t0) * Q * draws / HOST_DRAWS,
               host_slice_equal=bool(np.array_equal(host.y, res.y[:1, :HOST_DRAWS], equal_nan=True) and
                                     np.array_equal(host.status, res.status[:1, :HOST_DRAWS])))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--case', type=int, default=None, help='run the single case given (0: 1 point, 1: 64 points), in this process')
    ap.add_argument('--kernel', type=int, default=0, help='with --case: 0 Bernoulli Polynomials, 1 Cubic Splines')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.case is not None:
        return one(args)
    lines = []
    for kernel in range(len(KERNELS)):
        for case in range(len(POINTS)):
            cmd = [sys.executable, os.path.abspath(__file__), '--case', str(case), '--kernel', str(kernel), '--repeat',
                   str(args.repeat)]
            what = f"{KERNELS[kernel]}, {POINTS[case]} points"
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"steady_probe: {what} ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"steady_probe: {what} ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + f'# python tools/steady_probe.py --repeat {args.repeat}\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
