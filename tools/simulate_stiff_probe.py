"""Kernel time of dynamics.simulate_stiff next to dynamics.simulate_adaptive (simulate_stiff_kernel and
simulate_adaptive_kernel by the context's own events), both at rtol = 1e-4, on three versions of
tools/simulate_adaptive_probe.py's system, (states, terms per model, members, steps) = (2, 30, 1 000, 3 750): as it is, with a
tenth of the draws 16 times stiffer, and with a tenth of the draws 256 times stiffer (their coefficients times the factor).
With each: accepted steps / pairs per member, rejected trials and the histogram of the members' deepest levels.

    python tools/simulate_stiff_probe.py [--repeat 2] [--steps 3750] [--out FILE]

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

CASE = (2, 30, 1000, 3750)
RTOL = 1e-4
VARIANTS = (('as it is', 1.0), ('a tenth of the draws 16 times stiffer', 16.0), ('a tenth of the draws 256 times stiffer', 256.0))
KERNELS = ('Bernoulli Polynomials', 'Cubic Splines')
HEADER = ("# tools/simulate_stiff_probe.py on one MI355X, both functions at rtol = 1e-4: *_kernel_ms = the launches of\n"
          "# simulate_stiff_kernel / simulate_adaptive_kernel by the context's events, the best of the calls; *_call_ms = the whole\n"
          "# call; stiff_steps_* = accepted Rodas3 steps per member, adaptive_pairs_* = accepted pairs of half steps per member;\n"
          "# *_levels = how many members have their deepest level at 0, 1, 2, ...\n")


def measure(ctx, call, report, repeat):
    from fokl_gpy_amd import _capi
    call()                                                             # first launch: code object
    ctx.timing_enable(True)
    kernel_ms, t0 = [], time.perf_counter()
    for _ in range(repeat):
        ctx.timing_reset()
        res = call()
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    wall = (time.perf_counter() - t0) / repeat
    ctx.timing_enable(False)
    return res, report(), min(kernel_ms), 1e3 * wall


def one(args):
    from fokl_gpy_amd import _capi, dynamics
    from simulate_probe import system

    n_states, n_terms, members, _ = CASE
    steps = args.steps
    kernel = KERNELS[args.kernel]
    name, factor = VARIANTS[args.variant]
    rec = dict(states=n_states, terms=n_terms, members=members, steps=steps, kernel=kernel, variant=name, rtol=RTOL)
    sysargs = system(n_states, n_terms, members, steps, kernel, np.random.default_rng(0))
    for model in sysargs['models']:
        model['betas'][::10] *= factor
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    res, rep, kernel_ms, call_ms = measure(ctx, lambda: dynamics.simulate_stiff(**sysargs, rtol=RTOL, device=ctx),
                                           ctx.simulate_stiff_report, args.repeat)
    deepest = int(res.max_level.max())
    rec.update(stiff_kernel_ms=kernel_ms, stiff_call_ms=call_ms, stiff_launches=rep['launches'], stiff_lds_bytes=rep['lds_bytes'],
               stiff_steps_mean=float(res.steps.mean()), stiff_steps_max=int(res.steps.max()),
               stiff_rejected_mean=float(res.rejected.mean()), stiff_swaps=rep['swaps'],
               stiff_levels=np.bincount(res.max_level, minlength=deepest + 1).tolist(),
               stiff_saturated_fraction=res.saturated_fraction, stiff_unresolved_fraction=res.unresolved_fraction)
    res, rep, kernel_ms, call_ms = measure(ctx, lambda: dynamics.simulate_adaptive(**sysargs, rtol=RTOL, device=ctx),
                                           ctx.simulate_adaptive_report, args.repeat)
    ctx.close()
    deepest = int(res.max_level.max())
    rec.update(adaptive_kernel_ms=kernel_ms, adaptive_call_ms=call_ms, adaptive_launches=rep['launches'],
               adaptive_pairs_mean=float(res.pairs.mean()), adaptive_pairs_max=int(res.pairs.max()),
               adaptive_rejected_mean=float(res.rejected.mean()),
               adaptive_levels=np.bincount(res.max_level, minlength=deepest + 1).tolist(),
               adaptive_saturated_fraction=res.saturated_fraction, adaptive_unresolved_fraction=res.unresolved_fraction)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--steps', type=int, default=CASE[3], help='output steps of the horizon')
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--variant', type=int, default=None, help='run the single variant given (0, 1, 2), in this process')
    ap.add_argument('--kernel', type=int, default=0, help='with --variant: 0 Bernoulli Polynomials, 1 Cubic Splines')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.variant is not None:
        return one(args)
    lines = []
    for kernel in range(len(KERNELS)):
        for variant in range(len(VARIANTS)):
            cmd = [sys.executable, os.path.abspath(__file__), '--variant', str(variant), '--kernel', str(kernel), '--repeat',
                   str(args.repeat), '--steps', str(args.steps)]
            what = f"{KERNELS[kernel]}, {VARIANTS[variant][0]}"
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"simulate_stiff_probe: {what} ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"simulate_stiff_probe: {what} ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + f'# python tools/simulate_stiff_probe.py --repeat {args.repeat} --steps {args.steps}\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
