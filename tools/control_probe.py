"""Kernel time per iteration of dynamics.control (control_iterate_kernel by the context's own events) for random Bernoulli
systems of (states, terms per model, draws, starts, steps, decision values D: one control over D holds that begin at steps
floor(k steps / D)); next to each dynamics.control_host on a slice of the draws and steps, scaled up to all of them.

    python tools/control_probe.py [--repeat 2] [--host-draws 2] [--host-steps 50] [--out FILE]

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

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

from simulate_probe import KERNELS, system                            # the same random systems: 'u' becomes the control

CASES = ((2, 30, 1000, 1, 200, 8), (2, 30, 1000, 4, 1000, 16), (4, 92, 1000, 1, 200, 32))
HEADER = ("# tools/control_probe.py on one MI355X: kernel_ms = the launches of control_iterate_kernel and the trajectory launch by\n"
          "# the context's events, the best of the calls; ms_per_iteration = kernel_ms / launches that found a running solve;\n"
          "# call_ms = the whole call (upload and fetch included); host_ms_scaled = dynamics.control_host on host_draws draws and\n"
          "# host_steps steps, scaled to all of them\n")


def one(args):
    from fokl_gpy_amd import _capi, dynamics

    n_states, n_terms, draws, starts, steps, D = args.case
    rec = dict(states=n_states, terms=n_terms, draws=draws, starts=starts, steps=steps, D=D)
    rng = np.random.default_rng(0)
    sysargs = system(n_states, n_terms, draws, steps, KERNELS[0], rng)
    sysargs['y0'] = sysargs['y0'][0]
    del sysargs['forcing']
    call = dict(sysargs, controls=['u'], segments=np.arange(D) * steps // D, targets={'x0': 0.1}, terminal={'x0': 1.0},
                move_weight={'u': 1e-3}, limits={name: (-0.8, 0.8) for name in sysargs['states']}, starts=starts, max_iter=20)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    dynamics.control(**call, device=ctx)                               # first launch: code object
    ctx.timing_enable(True)
    kernel_ms, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.control(**call, device=ctx)
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    wall = (time.perf_counter() - t0) / args.repeat
    report = ctx.control_report()
    rec.update(report, kernel_ms=min(kernel_ms), ms_per_iteration=min(kernel_ms) / max(1, report['launches_with_work']),
               call_ms=1e3 * wall, converged=int((res.status == 0).sum()), mean_iterations=float(res.iterations.mean()),
               saturated=int((res.first_saturation >= 0).sum()))
    ctx.close()
    hd, hs = min(draws, args.host_draws), min(steps, args.host_steps)
    small = dict(call, t=(0.0, (hs - 0.5) * sysargs['t'][2], sysargs['t'][2]), draws=np.arange(hd),
                 segments=np.arange(min(D, hs)) * hs // min(D, hs), max_iter=3)
    t0 = time.perf_counter()
    host = dynamics.control_host(**small)
    per_iteration = (time.perf_counter() - t0) / max(1, int(host.iterations.max()) + 1)
    rec.update(host_draws=hd, host_steps=hs, host_ms_per_iteration_scaled=1e3 * per_iteration * (draws / hd) * (steps / hs))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-draws', type=int, default=2)
    ap.add_argument('--host-steps', type=int, default=50)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--case', type=int, nargs=6, default=None,
                    help='run the single (states, terms, draws, starts, steps, D) given, in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.case:
        return one(args)
    lines = []
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), '--case', *map(str, case), '--repeat', str(args.repeat),
               '--host-draws', str(args.host_draws), '--host-steps', str(args.host_steps)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"control_probe: {case} ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"control_probe: {case} ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + f'# python tools/control_probe.py --repeat {args.repeat} --host-draws {args.host_draws} '
                                  f'--host-steps {args.host_steps}\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
