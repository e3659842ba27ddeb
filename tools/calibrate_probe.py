"""Kernel time of dynamics.calibrate (calibrate_kernel by the call's own events) and its trajectory steps per second for
tools/simulate_probe.py's first system, the forcing input u as an unknown parameter next to the initial value of x0, at
(draws, steps, iterations) = (1 000, 200, 500); next to it dynamics.simulate's kernel time per member-step on the same
system, and dynamics.calibrate_host on a slice of the draws and iterations scaled up to all of them.

    python tools/calibrate_probe.py [--draws 1000] [--steps 200] [--iterations 500] [--repeat 2] [--host-draws 2]
                                    [--host-iterations 10] [--out FILE]

The measurement runs in a child process of its own under a time limit (--limit seconds); if it fails or runs out of time the
probe ends and nothing more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

from simulate_probe import CASES, KERNELS, system  # noqa: E402

HEADER = ("# tools/calibrate_probe.py on one MI355X: kernel_ms = the launches of calibrate_kernel by the call's own events, the\n"
          "# best of the calls (kernel_ms_runs: each of them, after a first call that loads the code object);\n"
          "# trajectory_steps_per_s = evaluations x steps / kernel time; simulate_ns_per_member_step = simulate_ensemble_kernel on\n"
          "# 128 x draws members of the same system; host_ms_scaled = dynamics.calibrate_host on host_draws draws and\n"
          "# host_iterations iterations, scaled to all of them; rhat_max is the worst of all draws after iterations / 2 kept\n"
          "# iterations of a random system -- the probe times the kernel, it does not tune a sampler\n")


def problem(draws, steps, iterations, rng):
    n_states, n_terms = CASES[0][:2]
    sysargs = system(n_states, n_terms, draws, steps, KERNELS[0], rng)
    forcing = sysargs.pop('forcing')
    truth = dict(sysargs, forcing={'u': np.full(steps, 6.0)}, draws=np.array([0]), y0=[0.1] * n_states)
    from fokl_gpy_amd import dynamics
    members = dynamics.simulate_host(**truth, ReturnBounds=False, keep='members').members
    points = np.arange(20, steps + 1, 20)
    data = members[0, :, points] + 0.02 * rng.standard_normal((points.shape[0], n_states))
    call = dict(sysargs, y0=sysargs['y0'], unknown=['u', 'y0:x0'], observe=sysargs['states'], data=data, obs_points=points,
                obs_sd=[0.02] * n_states, prior={'u': (5.0, 3.0)}, burnin=iterations // 2,
                draws_kept=iterations - iterations // 2, thin=10)
    return call, dict(sysargs, forcing=forcing)


def one(args):
    from fokl_gpy_amd import _capi, dynamics

    call, sim = problem(args.draws, args.steps, args.iterations, np.random.default_rng(0))
    rec = dict(draws=args.draws, steps=args.steps, iterations=args.iterations, unknowns=2)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    dynamics.calibrate(**dict(call, burnin=0, draws_kept=1, thin=1), device=ctx)      # first launch: code object
    runs, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        res = dynamics.calibrate(**call, device=ctx)
        runs.append(ctx.calibrate_report())
    wall = (time.perf_counter() - t0) / args.repeat
    rep = min(runs, key=lambda r: r['kernel_us'])
    trajectory_steps = rep['evaluations'] * args.steps
    rec.update(rep, kernel_ms=rep['kernel_us'] / 1e3, kernel_ms_runs=[r['kernel_us'] / 1e3 for r in runs], call_ms=1e3 * wall,
               trajectory_steps_per_s=trajectory_steps / (rep['kernel_us'] * 1e-6),
               ns_per_trajectory_step=1e3 * rep['kernel_us'] / trajectory_steps, rhat_max=res.rhat_max,
               accept_stretch=float(res.accept[:, 0].mean()), saturated_fraction=float(res.saturated.mean()))
    # simulate on as many members as a half step of every draw integrates twice over: 128 x draws
    members = 128 * args.draws
    wide = dict(sim, y0=np.tile(sim['y0'], (128, 1)), draws=np.tile(np.arange(args.draws), 128), ReturnBounds=False)
    dynamics.simulate(**wide, device=ctx)
    ctx.timing_enable(True)
    ctx.timing_reset()
    dynamics.simulate(**wide, device=ctx)
    ctx.sync()
    sim_ms = ctx.timing_get(_capi.K_INTEGRATE)['ms']
    ctx.close()
    rec.update(simulate_members=members, simulate_kernel_ms=sim_ms, simulate_ns_per_member_step=1e6 * sim_ms / (members * args.steps))
    he, hi = min(args.draws, args.host_draws), min(args.iterations, args.host_iterations)
    small = dict(call, y0=call['y0'][:he], draws=np.arange(he), burnin=hi // 2, draws_kept=hi - hi // 2, thin=1)
    t0 = time.perf_counter()
    dynamics.calibrate_host(**small)
    rec.update(host_draws=he, host_iterations=hi,
               host_ms_scaled=1e3 * (time.perf_counter() - t0) * (args.draws / he) * (args.iterations / hi))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--iterations', type=int, default=500)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-draws', type=int, default=2)
    ap.add_argument('--host-iterations', type=int, default=10)
    ap.add_argument('--limit', type=int, default=400)
    ap.add_argument('--child', action='store_true', help='run the measurement in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        return one(args)
    options = ['--draws', args.draws, '--steps', args.steps, '--iterations', args.iterations, '--repeat', args.repeat,
               '--host-draws', args.host_draws, '--host-iterations', args.host_iterations]
    cmd = [sys.executable, os.path.abspath(__file__), '--child', *map(str, options)]
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"calibrate_probe: ran out of its {args.limit} s; nothing more is started")
    if done.returncode != 0:
        sys.exit(f"calibrate_probe: ended with status {done.returncode}; nothing more is started\n" + done.stderr[-2000:])
    line = done.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(HEADER + '# python tools/calibrate_probe.py ' + ' '.join(map(str, options)) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
