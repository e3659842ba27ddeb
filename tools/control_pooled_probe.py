"""Kernel time per iteration of dynamics.control_pooled, split by kernel (the launches' own events, read from
DeviceContext.control_pooled_report), for tools/control_probe.py's three systems at 1 000 draws; next to each,
dynamics.control's time per iteration for the same system on the same device (control_iterate_kernel by the context's
events) and dynamics.control_pooled_host on a slice of the draws and steps, scaled up to all of them.

    python tools/control_pooled_probe.py [--repeat 2] [--host-draws 2] [--host-steps 50] [--out FILE]

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

from control_probe import CASES                                       # (states, terms per model, draws, starts, steps, D)
from simulate_probe import KERNELS, system

KINDS = ('tangent', 'chunk', 'step', 'trial', 'accept')
HEADER = ("# tools/control_pooled_probe.py on one MI355X: <kind>_ms_per_iteration = the launches of that kind of kernel by their\n"
          "# own events (the two chunk-sum launches together), the best of the calls, over the iterations that found a running\n"
          "# start; kernel_ms = all launches of the call by the context's events; call_ms = the whole call (upload and fetch\n"
          "# included); control_ms_per_iteration = dynamics.control on the same system and device; host_ms_scaled =\n"
          "# dynamics.control_pooled_host on host_draws draws and host_steps steps, scaled to all of them\n")


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
    dynamics.control_pooled(**call, device=ctx)                        # first launch: code objects
    dynamics.control(**call, device=ctx)
    ctx.timing_enable(True)
    best, t0 = None, time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.control_pooled(**call, device=ctx)
        ctx.sync()
        report = dict(ctx.control_pooled_report(), kernel_ms=ctx.timing_get(_capi.K_INTEGRATE)['ms'])
        if best is None or report['kernel_ms'] < best['kernel_ms']:
            best = report
    wall = (time.perf_counter() - t0) / args.repeat
    worked = max(1, best['iterations_with_work'])
    rec.update({key: best[key] for key in ('chunks', 'lds_bytes', 'step_lds_bytes', 'iterations_queued', 'iterations_with_work')})
    rec.update({f'{kind}_ms_per_iteration': 1e-6 * best[f'{kind}_ns'] / worked for kind in KINDS})
    rec.update(kernel_ms=best['kernel_ms'], ms_per_iteration=1e-6 * sum(best[f'{kind}_ns'] for kind in KINDS) / worked,
               call_ms=1e3 * wall, status=int(res.status), iterations=int(res.iterations),
               saturated=int((res.first_saturation >= 0).sum()))
    own_ms = []
    for _ in range(args.repeat):
        ctx.timing_reset()
        dynamics.control(**call, device=ctx)
        ctx.sync()
        own_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    rec.update(control_ms_per_iteration=min(own_ms) / max(1, ctx.control_report()['launches_with_work']))
    ctx.close()
    hd, hs = min(draws, args.host_draws), min(steps, args.host_steps)
    small = dict(call, t=(0.0, (hs - 0.5) * sysargs['t'][2], sysargs['t'][2]), draws=np.arange(hd),
                 segments=np.arange(min(D, hs)) * hs // min(D, hs), max_iter=3)
    t0 = time.perf_counter()
    host = dynamics.control_pooled_host(**small)
    per_iteration = (time.perf_counter() - t0) / max(1, int(host.iterations) + 1)
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
            sys.exit(f"control_pooled_probe: {case} ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"control_pooled_probe: {case} ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + f'# python tools/control_pooled_probe.py --repeat {args.repeat} --host-draws {args.host_draws} '
                                  f'--host-steps {args.host_steps}\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
