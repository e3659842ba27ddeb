"""Time of fokl_infer_inputs' launches (infer_inputs_kernel) by their own events and target evaluations per second, for
random models of (d unknowns, K observations, T terms) over E posterior draws, next to infer.sample_host on a slice of the
draws and iterations scaled up to all of them.

    python tools/infer_probe.py [--iterations 500] [--draws 1000] [--repeat 2] [--out FILE]

Every shape runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child
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

SHAPES = ((2, 3, 30), (8, 20, 92), (16, 50, 150))
HEADER = ("# tools/infer_probe.py on one MI355X: kernel_ms = the launches of infer_inputs_kernel by their own events, the best "
          "of the calls;\n# evaluations_per_s = target evaluations (one walker, all K observations) / kernel time; "
          "host_ms_scaled = infer.sample_host on host_draws\n# draws and host_iterations iterations scaled to all of them\n")


def problem(d, K, T, E, rng):
    """A random model over d unknowns with T terms of one to three factors of orders 1..2, K observations near its surface."""
    from fokl_gpy_amd import getKernels
    mtx = np.zeros((T, d), dtype=np.int32)
    for t in range(T):
        cols = rng.choice(d, size=min(d, 1 + t % 3), replace=False)
        mtx[t, cols] = 1 + rng.integers(0, 2, size=cols.shape[0])
    table, n_basis, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    mean = rng.standard_normal(T + 1) / np.sqrt(T + 1)
    betas = mean * (1.0 + 0.05 * rng.standard_normal((E, T + 1)))
    P = np.concatenate([np.ones((K, 1)), 0.5 + rng.random((K, T))], axis=1)
    return dict(mtx_u=mtx, betas=betas, h=np.full(E, 0.5 / 0.05 ** 2), table=table, lo=np.zeros(d), hi=np.ones(d),
                prior_mean=np.full(d, 0.5), prior_prec=np.zeros(d), y=P @ mean * 0.9, P=P)


def one(args):
    from fokl_gpy_amd import _capi, infer, optimize

    d, K, T = args.shape
    E, iterations = args.draws, args.iterations
    p = problem(d, K, T, E, np.random.default_rng(0))
    starts = optimize.start_points(64, p['lo'], p['hi'])
    order = ('mtx_u', 'betas', 'h', 'table', 'lo', 'hi', 'prior_mean', 'prior_prec', 'y', 'P')
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    run = lambda: ctx.infer_inputs(*[p[k] for k in order], starts, 0, iterations, 1, 8, 0, rows=False)
    run()                                                              # first launch: code object
    us, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        out = run()
        us.append(ctx.infer_report()['kernel_us'])
    wall = (time.perf_counter() - t0) / args.repeat
    rep = ctx.infer_report()
    ctx.close()
    best = min(us)
    rec = dict(d=d, K=K, T=T, draws=E, iterations=iterations, mapping=rep['mapping'], lds_rows=rep['lds_rows'],
               launches=rep['launches'], grid=rep['grid'], kernel_ms=best / 1e3, kernel_us_all=us, call_ms=1e3 * wall,
               evaluations=rep['evaluations'], evaluations_per_s=rep['evaluations'] / (best * 1e-6),
               stretch_acceptance=float(out[3][:, :, 0].sum()) / (E * 64.0 * (iterations - iterations // 8)))
    he, hi_ = min(E, args.host_draws), min(iterations, args.host_iterations)
    q = dict(p, betas=p['betas'][:he], h=p['h'][:he])
    t0 = time.perf_counter()
    infer.sample_host(*[q[k] for k in order], starts, 0, hi_, 1, 8, 0, rows=False)
    rec['host_ms_scaled'] = 1e3 * (time.perf_counter() - t0) * (E / he) * (iterations / hi_)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=500)
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-draws', type=int, default=4)
    ap.add_argument('--host-iterations', type=int, default=10)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--shape', type=int, nargs=3, default=None, help='run the single (d, K, T) given, in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.shape:
        return one(args)
    lines = []
    given, skip = [], False                                  # the command as given, without where its output went
    for a in sys.argv[1:]:
        if skip or a == '--out':
            skip = not skip
            continue
        given.append(a)
    for d, K, T in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--shape', str(d), str(K), str(T), '--iterations', str(args.iterations),
               '--draws', str(args.draws), '--repeat', str(args.repeat), '--host-draws', str(args.host_draws),
               '--host-iterations', str(args.host_iterations)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"infer_probe: (d, K, T) = ({d}, {K}, {T}) ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"infer_probe: (d, K, T) = ({d}, {K}, {T}) ended with status {done.returncode}; nothing more is started\n"
                     + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + '# python tools/infer_probe.py' + ''.join(' ' + a for a in given) + '\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
