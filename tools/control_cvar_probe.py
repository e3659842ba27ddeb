"""Kernel time per iteration of dynamics.control_cvar at alpha 0.9, split by kind of launch (the launches' own events, read
from DeviceContext.control_cvar_report), for tools/control_probe.py's three systems at 1 000 draws; next to each,
dynamics.control_pooled's time per iteration for the same system on the same device and build.

    python tools/control_cvar_probe.py [--repeat 2] [--alpha 0.9] [--out FILE]

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

KINDS = ('tangent', 'risk', 'chunk', 'step', 'trial', 'accept')
POOLED_KINDS = ('tangent', 'chunk', 'step', 'trial', 'accept')
HEADER = ("# tools/control_cvar_probe.py on one MI355X: <kind>_ms_per_iteration = the launches of that kind of kernel by their own\n"
          "# events (the two risk launches together), the best of the calls, over the iterations that found a running start;\n"
          "# extra_share = (risk + chunk + step + accept) / all; kernel_ms = all launches of the call by the context's events;\n"
          "# call_ms = the whole call (upload and fetch included); pooled_* = dynamics.control_pooled on the same system, device\n"
          "# and build, by its own report\n")


def one(args):
    from fokl_gpy_amd import _capi, dynamics

    n_states, n_terms, draws, starts, steps, D = args.case
    rec = dict(states=n_states, terms=n_terms, draws=draws, starts=starts, steps=steps, D=D, alpha=args.alpha)
    rng = np.random.default_rng(0)
    sysargs = system(n_states, n_terms, draws, steps, KERNELS[0], rng)
    sysargs['y0'] = sysargs['y0'][0]
    del sysargs['forcing']
    call = dict(sysargs, controls=['u'], segments=np.arange(D) * steps // D, targets={'x0': 0.1}, terminal={'x0': 1.0},
                move_weight={'u': 1e-3}, limits={name: (-0.8, 0.8) for name in sysargs['states']}, starts=starts, max_iter=20)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    dynamics.control_cvar(**call, alpha=args.alpha, device=ctx)       # first launch: code objects
    dynamics.control_pooled(**call, device=ctx)
    ctx.timing_enable(True)
    best, t0 = None, time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.control_cvar(**call, alpha=args.alpha, device=ctx)
        ctx.sync()
        report = dict(ctx.control_cvar_report(), kernel_ms=ctx.timing_get(_capi.K_INTEGRATE)['ms'])
        if best is None or report['kernel_ms'] < best['kernel_ms']:
            best = report
    wall = (time.perf_counter() - t0) / args.repeat
    worked = max(1, best['iterations_with_work'])
    rec.update({key: best[key] for key in ('chunks', 'lds_bytes', 'step_lds_bytes', 'risk_lds_bytes', 'risk_threads',
                                           'iterations_queued', 'iterations_with_work')})
    rec.update({f'{kind}_ms_per_iteration': 1e-6 * best[f'{kind}_ns'] / worked for kind in KINDS})
    total = sum(best[f'{kind}_ns'] for kind in KINDS)
    rec.update(kernel_ms=best['kernel_ms'], ms_per_iteration=1e-6 * total / worked,
               extra_share=(total - best['tangent_ns'] - best['trial_ns']) / max(1, total), call_ms=1e3 * wall,
               status=int(res.status), iterations=int(res.iterations), cvar=float(res.cvar), expected_cost=float(res.expected_cost),
               epsilon=float(res.epsilon))
    pooled_best, pooled = None, None
    for _ in range(args.repeat):
        ctx.timing_reset()
        pooled = dynamics.control_pooled(**call, device=ctx)
        ctx.sync()
        report = dict(ctx.control_pooled_report(), kernel_ms=ctx.timing_get(_capi.K_INTEGRATE)['ms'])
        if pooled_best is None or report['kernel_ms'] < pooled_best['kernel_ms']:
            pooled_best = report
    worked = max(1, pooled_best['iterations_with_work'])
    rec.update({f'pooled_{kind}_ms_per_iteration': 1e-6 * pooled_best[f'{kind}_ns'] / worked for kind in POOLED_KINDS})
    rec.update(pooled_ms_per_iteration=1e-6 * sum(pooled_best[f'{kind}_ns'] for kind in POOLED_KINDS) / worked,
               pooled_iterations=int(pooled.iterations), pooled_status=int(pooled.status),
               pooled_cvar=float(dynamics.cvar_exact(pooled.cost_draws, pooled.draw_weights, args.alpha)[0]),
               pooled_expected_cost=float(pooled.cost))
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--alpha', type=float, default=0.9)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--case', type=int, nargs=6, default=None,
                    help='run the single (states, terms, draws, starts, steps, D) given, in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.case:
        return one(args)
    lines = []
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), '--case', *map(str, case), '--repeat', str(args.repeat), '--alpha',
               str(args.alpha)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"control_cvar_probe: {case} ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"control_cvar_probe: {case} ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + f'# python tools/control_cvar_probe.py --repeat {args.repeat} --alpha {args.alpha}\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
