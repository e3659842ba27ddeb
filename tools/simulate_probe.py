"""Kernel time of dynamics.simulate (simulate_ensemble_kernel by the context's own events, and the band kernel) for random
systems of (states, terms per model, members, steps), for both kernels, next to dynamics.simulate_host on a slice of the
members scaled up to all of them.

    python tools/simulate_probe.py [--repeat 2] [--host-members 8] [--host-steps 50] [--out FILE]

Every case runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child
that fails or runs out of time ends the probe and nothing more is started on the device.  A case the call refuses (the
coefficients and factors of a system must fit a wavefront's LDS) is reported as refused, with the call's message.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

CASES = ((2, 30, 1000, 3750), (4, 92, 10000, 1000), (8, 92, 1000, 1000))
KERNELS = ('Bernoulli Polynomials', 'Cubic Splines')
HEADER = ("# tools/simulate_probe.py on one MI355X: kernel_ms = the launches of simulate_ensemble_kernel by the context's events,\n"
          "# band_ms = those of ensemble_band_kernel, the best of the calls; call_ms = the whole call (upload and fetch included);\n"
          "# host_ms_scaled = dynamics.simulate_host on host_members members and host_steps steps, scaled to all of them\n")


def system(n_states, n_terms, members, steps, kernel, rng):
    """Model k reads every state and one forcing input through ranges of its own; n_terms terms of one to three factors of
    orders 1..3; small coefficients, so that the members stay inside the box."""
    from fokl_gpy_amd import getKernels
    phis = getKernels.bernoulli() if kernel == KERNELS[0] else getKernels.sp500()
    states = [f'x{k}' for k in range(n_states)]
    models, inputs = [], []
    for k in range(n_states):
        names = states + ['u']
        mtx = np.zeros((n_terms, len(names)), dtype=int)
        for t in range(n_terms):
            cols = rng.choice(len(names), size=min(len(names), 1 + t % 3), replace=False)
            mtx[t, cols] = 1 + rng.integers(0, 3, size=cols.shape[0])
        mean = 0.2 * rng.standard_normal(n_terms + 1) / np.sqrt(n_terms + 1)
        models.append(dict(betas=mean * (1.0 + 0.05 * rng.standard_normal((members, n_terms + 1))), mtx=mtx, phis=phis,
                           minmax=[[-1.0 - 0.1 * k, 1.0 + 0.1 * k]] * n_states + [[0.0, 10.0]], kernel=kernel))
        inputs.append(names)
    h = 0.01
    return dict(models=models, states=states, inputs=inputs, forcing={'u': 5.0 + 4.0 * np.sin(np.arange(steps) / 30.0)},
                y0=rng.uniform(-0.3, 0.3, (members, n_states)), t=(0.0, (steps - 0.5) * h, h))


def one(args):
    from fokl_gpy_amd import _capi, dynamics

    n_states, n_terms, members, steps = args.case
    kernel = KERNELS[args.kernel]
    rec = dict(states=n_states, terms=n_terms, members=members, steps=steps, kernel=kernel)
    sysargs = system(n_states, n_terms, members, steps, kernel, np.random.default_rng(0))
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    try:
        dynamics.simulate(**sysargs, device=ctx)                       # first launch: code object
    except ValueError as refusal:
        ctx.close()
        print(json.dumps(dict(rec, refused=str(refusal))))
        return
    ctx.timing_enable(True)
    kernel_ms, band_ms, t0 = [], [], time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.simulate(**sysargs, device=ctx)
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
        band_ms.append(ctx.timing_get(_capi.K_BAND)['ms'])
    wall = (time.perf_counter() - t0) / args.repeat
    rep = ctx.simulate_report()
    ctx.close()
    rec.update(rep, kernel_ms=min(kernel_ms), band_ms=min(band_ms), call_ms=1e3 * wall,
               us_per_step=1e3 * min(kernel_ms) / steps, saturated_fraction=res.saturated_fraction)
    he, hs = min(members, args.host_members), min(steps, args.host_steps)
    small = dict(sysargs, y0=sysargs['y0'][:he], t=(0.0, (hs - 0.5) * sysargs['t'][2], sysargs['t'][2]))
    t0 = time.perf_counter()
    dynamics.simulate_host(**small, draws=np.arange(he), ReturnBounds=False)
    rec.update(host_members=he, host_steps=hs, host_ms_scaled=1e3 * (time.perf_counter() - t0) * (members / he) * (steps / hs))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-members', type=int, default=8)
    ap.add_argument('--host-steps', type=int, default=50)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--case', type=int, nargs=4, default=None, help='run the single (states, terms, members, steps) given, in this process')
    ap.add_argument('--kernel', type=int, default=0, help='with --case: 0 Bernoulli Polynomials, 1 Cubic Splines')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.case:
        return one(args)
    lines = []
    for case in CASES:
        for kernel in range(len(KERNELS)):
            cmd = [sys.executable, os.path.abspath(__file__), '--case', *map(str, case), '--kernel', str(kernel), '--repeat',
                   str(args.repeat), '--host-members', str(args.host_members), '--host-steps', str(args.host_steps)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"simulate_probe: {case} {KERNELS[kernel]} ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"simulate_probe: {case} {KERNELS[kernel]} ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + f'# python tools/simulate_probe.py --repeat {args.repeat} --host-members {args.host_members} '
                                      f'--host-steps {args.host_steps}\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
