"""Kernel time of dynamics.assimilate (assimilate_kernel by the context's own events) for random Bernoulli systems of
(states, terms per model, draws, steps, observations); next to each the kernel time of dynamics.simulate for 64 x draws
members of the same system where simulate accepts it (the same number of trajectories, without the filter), and
dynamics.assimilate_host on a slice of the draws scaled up to all of them.

    python tools/assimilate_probe.py [--repeat 2] [--host-draws 4] [--host-steps 50] [--out FILE]

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

from simulate_probe import KERNELS, system                            # the same random systems

CASES = ((2, 30, 1000, 3750, 375), (4, 92, 1000, 1000, 100), (8, 92, 1000, 1000, 100))
HEADER = ("# tools/assimilate_probe.py on one MI355X: kernel_ms = the launches of assimilate_kernel by the context's events, the\n"
          "# best of the calls; call_ms = the whole call (upload and fetch included); simulate_kernel_ms = simulate_ensemble_kernel\n"
          "# for 64 x draws members of the same system (or simulate_refused); host_ms_scaled = dynamics.assimilate_host on\n"
          "# host_draws draws and host_steps steps, scaled to all of them\n")


def one(args):
    from fokl_gpy_amd import _capi, dynamics

    n_states, n_terms, draws, steps, n_obs = args.case
    rec = dict(states=n_states, terms=n_terms, draws=draws, steps=steps, observations=n_obs)
    rng = np.random.default_rng(0)
    sysargs = system(n_states, n_terms, draws, steps, KERNELS[0], rng)
    sysargs['y0'] = sysargs['y0'][0]
    every = steps // n_obs
    # draw 0's trajectory by the host statement's own step (simulate_host refuses what exceeds simulate's LDS)
    plan = dynamics._prepare(sysargs['models'], sysargs['states'], sysargs['inputs'], sysargs['forcing'], sysargs['y0'],
                             sysargs['t'], np.array([0]), None, False, 'members', lds_per_member=False)
    truth = dynamics._run_host(plan)[0][0]
    points = np.arange(every, every * (n_obs + 1), every)
    data = truth[:1, points].T + 0.02 * rng.standard_normal((n_obs, 1))
    call = dict(sysargs, observe=['x0'], data=data, obs_points=points, obs_sd=[0.02], process_sd=[0.05] * n_states,
                y0_sd=[0.01] * n_states, resample_below=0.5, seed=1)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    dynamics.assimilate(**call, device=ctx)                            # first launch: code object
    ctx.timing_enable(True)
    kernel_ms, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        ctx.timing_reset()
        res = dynamics.assimilate(**call, device=ctx)
        ctx.sync()
        kernel_ms.append(ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    wall = (time.perf_counter() - t0) / args.repeat
    rec.update(ctx.assimilate_report(), kernel_ms=min(kernel_ms), call_ms=1e3 * wall, us_per_step=1e3 * min(kernel_ms) / steps,
               resampled_fraction=float(res.resampled.mean()), ess_draws=res.ess_draws,
               collapsed=int((res.collapsed >= 0).sum()), saturated=int((res.first_saturation >= 0).sum()))
    # the same number of trajectories through simulate: every draw 64 times
    wide = dict(sysargs, draws=np.repeat(np.arange(draws), 64))
    try:
        dynamics.simulate(**wide, ReturnBounds=False, device=ctx)
        ctx.timing_reset()
        dynamics.simulate(**wide, ReturnBounds=False, device=ctx)
        ctx.sync()
        rec.update(simulate_members=64 * draws, simulate_kernel_ms=ctx.timing_get(_capi.K_INTEGRATE)['ms'])
    except ValueError as refusal:
        rec.update(simulate_refused=str(refusal))
    ctx.close()
    hd, hs = min(draws, args.host_draws), min(steps, args.host_steps)
    keep = points[points <= hs]
    small = dict(call, t=(0.0, (hs - 0.5) * sysargs['t'][2], sysargs['t'][2]), draws=np.arange(hd), data=data[:keep.shape[0]],
                 obs_points=keep)
    t0 = time.perf_counter()
    dynamics.assimilate_host(**small)
    rec.update(host_draws=hd, host_steps=hs, host_ms_scaled=1e3 * (time.perf_counter() - t0) * (draws / hd) * (steps / hs))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-draws', type=int, default=4)
    ap.add_argument('--host-steps', type=int, default=50)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--case', type=int, nargs=5, default=None,
                    help='run the single (states, terms, draws, steps, observations) given, in this process')
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
            sys.exit(f"assimilate_probe: {case} ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"assimilate_probe: {case} ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + f'# python tools/assimilate_probe.py --repeat {args.repeat} --host-draws {args.host_draws} '
                                  f'--host-steps {args.host_steps}\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
