"""Kernel time and pairs per member of dynamics.simulate_adaptive (simulate_adaptive_kernel by the context's own events) for
tools/simulate_probe.py's first system, (states, terms per model, members, steps) = (2, 30, 1 000, 3 750), in two variants:
as it is, and with a tenth of the draws made 16 times stiffer (their coefficients times 16).  Next to each: dynamics.simulate
on the uniform grid at the deepest level any member reached -- what a user without error control has to pay for the same
resolution -- and dynamics.simulate_adaptive_host on a slice of the members scaled up to all of them.

    python tools/simulate_adaptive_probe.py [--repeat 2] [--host-members 8] [--host-steps 50] [--out FILE]

Every case runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child
that fails or runs out of time ends the probe and nothing more is started on the device.  The uniform grid is run over at
most --uniform-steps refined steps (from the start of the horizon) and its kernel time scaled to the whole horizon; the
record says how many were run.
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
VARIANTS = ('as it is', 'a tenth of the draws 16 times stiffer')
KERNELS = ('Bernoulli Polynomials', 'Cubic Splines')
HEADER = ("# tools/simulate_adaptive_probe.py on one MI355X: kernel_ms = the launches of simulate_adaptive_kernel by the context's\n"
          "# events, band_ms = those of ensemble_band_kernel, the best of the calls; call_ms = the whole call; pairs_* = accepted\n"
          "# pairs of half steps per member; uniform_kernel_ms = dynamics.simulate's kernel on the grid h / 2^(max_level + 1),\n"
          "# run over uniform_steps_run refined steps and scaled to all of them; host_ms_scaled = simulate_adaptive_host on\n"
          "# host_members members and host_steps steps, scaled to all of them\n")


def one(args):
    from fokl_gpy_amd import _capi, dynamics
    from simulate_probe import system

    n_states, n_terms, members, steps = CASE
    kernel = KERNELS[args.kernel]
    rec = dict(states=n_states, terms=n_terms, members=members, steps=steps, kernel=kernel, variant=VARIANTS[args.variant])
    sysargs = system(n_states, n_terms, members, steps, kernel, np.random.default_rng(0))
    if args.variant == 1:
        for model in sysargs['models']:
            model['betas'][::10] *= 16.0
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    dynamics.simulate_adaptive(**sysargs, device=ctx)                  # first launch: code object
    ctx.timing_enable(True)
    kernel_ms, band_ms, t0 = [], [], time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.simulate_adaptive(**sysargs, device=ctx)
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
        band_ms.append(ctx.timing_get(_capi.K_BAND)['ms'])
    wall = (time.perf_counter() - t0) / args.repeat
    rep = ctx.simulate_adaptive_report()
    deepest = int(res.max_level.max())
    rec.update(rep, kernel_ms=min(kernel_ms), band_ms=min(band_ms), call_ms=1e3 * wall, pairs_mean=float(res.pairs.mean()),
               pairs_min=int(res.pairs.min()), pairs_max=int(res.pairs.max()), rejected_mean=float(res.rejected.mean()),
               max_level=deepest, levels=np.bincount(res.max_level, minlength=deepest + 1).tolist(),
               saturated_fraction=res.saturated_fraction, unresolved_fraction=res.unresolved_fraction)
    # simulate on the uniform grid every member would need: h / 2^(deepest + 1), every forcing row repeated
    n = 2 ** (deepest + 1)
    h = sysargs['t'][2]
    run = max(1, min(steps, args.uniform_steps // n))
    fine = dict(sysargs, t=(0.0, (run * n - 0.5) * (h / n), h / n),
                forcing={name: np.repeat(values[:run], n) for name, values in sysargs['forcing'].items()})
    dynamics.simulate(**fine, device=ctx)
    uniform_ms = []
    for _ in range(args.repeat):
        ctx.timing_reset()
        dynamics.simulate(**fine, device=ctx)
        ctx.sync()
        uniform_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    ctx.close()
    rec.update(uniform_steps=steps * n, uniform_steps_run=run * n, uniform_kernel_ms=min(uniform_ms) * steps / run)
    he, hs = min(members, args.host_members), min(steps, args.host_steps)
    small = dict(sysargs, y0=sysargs['y0'][:he], t=(0.0, (hs - 0.5) * h, h))
    t0 = time.perf_counter()
    dynamics.simulate_adaptive_host(**small, draws=np.arange(he), ReturnBounds=False)
    rec.update(host_members=he, host_steps=hs, host_ms_scaled=1e3 * (time.perf_counter() - t0) * (members / he) * (steps / hs))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-members', type=int, default=8)
    ap.add_argument('--host-steps', type=int, default=50)
    ap.add_argument('--uniform-steps', type=int, default=1 << 18, help='refined steps the uniform grid is run over at most')
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--variant', type=int, default=None, help='run the single variant given (0, 1), in this process')
    ap.add_argument('--kernel', type=int, default=0, help='with --variant: 0 Bernoulli Polynomials, 1 Cubic Splines')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.variant is not None:
        return one(args)
    lines = []
    for kernel in range(len(KERNELS)):
        for variant in range(len(VARIANTS)):
            cmd = [sys.executable, os.path.abspath(__file__), '--variant', str(variant), '--kernel', str(kernel), '--repeat',
                   str(args.repeat), '--host-members', str(args.host_members), '--host-steps', str(args.host_steps),
                   '--uniform-steps', str(args.uniform_steps)]
            what = f"{KERNELS[kernel]}, {VARIANTS[variant]}"
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"simulate_adaptive_probe: {what} ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"simulate_adaptive_probe: {what} ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + f'# python tools/simulate_adaptive_probe.py --repeat {args.repeat} --host-members '
                                      f'{args.host_members} --host-steps {args.host_steps} --uniform-steps {args.uniform_steps}\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
