"""Time of the Student-t instances of score_kernel and predictive_kernel next to the Gaussian instances ON THE SAME DRAWS, by
the kernels' own events (score_report / predictive_report), for (rows, columns, draws) = (1e6, 100, 1 000) and (1e6, 300,
1 000): 'waic', 'waic' + 'loo', the PIT alone and 3 quantiles.  The t instances run unweighted and with row precisions.

    python tools/student_probe.py [--rows 1000000] [--repeat 2] [--nu 4] [--out FILE]

Every shape runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child that
fails or runs out of time ends the probe and nothing more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

SHAPES = ((100, 1000), (300, 1000))                          # columns, draws
QUANTILES = (0.025, 0.5, 0.975)
HEADER = ("# tools/student_probe.py on one MI355X: kernel milliseconds by the kernels' own events, the best of the launches, of the\n"
          "# Gaussian instance (fokl_score_rows / fokl_predictive_rows), the Student-t instance without weights and with row\n"
          "# precisions (fokl_score_rows_noise / fokl_predictive_rows_noise), on the same rows and draws; passes = the mean number\n"
          "# of passes per 16-row tile (pass 0 and the t instance's PIT pass not counted)\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import predictive as pd

    S, nc, E, nu = args.rows, args.columns, args.draws, args.nu
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    mean = rng.standard_normal(nc) / np.sqrt(nc)
    betas = mean + 0.05 * rng.standard_normal((E, nc)) / np.sqrt(nc)
    sig = 0.25 * (1.0 + 0.2 * rng.random(E))
    y = mean[0] + 0.5 * rng.standard_normal(S)
    ctx.upload(rng.random((S, 1)), np.zeros(S), getKernels.KERNEL_BERNOULLI, packed, nb, width)
    ctx.reserve_slots(nc + 2)
    for j in range(nc - 1):                                  # a column at a time: 300 columns of 1e6 rows are 2.4 GB
        col = rng.standard_normal(S)
        y += mean[j + 1] * col
        ctx.write_slot(2 + j, col)
    ctx.write_slot(_capi.SLOT_Y, y)
    slots = np.concatenate([[0], np.arange(2, nc + 1)]).astype(np.int32)
    sd, rinv = pd.scales(sig)
    sw = np.sqrt(rng.choice([0.25, 1.0, 4.0], S))
    p = np.array(QUANTILES)
    zs = {'gaussian': np.array([pd.normal_quantile(v) for v in p]), 'student': np.array([pd.student_quantile(v, nu) for v in p])}
    noises = (('gaussian', np.inf, None), ('student', nu, None), ('student_weighted', nu, sw))

    def best(call, report):
        call()                                               # first launch: code object
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(report()['kernel_ms'])
        return min(ms), report()

    rec = dict(rows=S, columns=nc, draws=E, nu=nu)
    for name, nu_, sw_ in noises:
        for label, want_loo in (('waic', False), ('waic_loo', True)):
            ms, rep = best(lambda: ctx.score_rows_noise(slots, betas, sig, want_loo, nu=nu_, sw=sw_), ctx.score_report)
            rec[f'{label}_{name}_ms'] = ms
            rec.setdefault('instances', {})[f'{label}_{name}'] = (rep['instance'], rep['noise'])
        z = zs['gaussian' if name == 'gaussian' else 'student']
        for label, pp, zz in (('pit', [], []), ('q3', p, z)):
            ms, rep = best(lambda: ctx.predictive_rows_noise(slots, betas, sd, rinv, True, pp, zz, nu=nu_, sw=sw_),
                           ctx.predictive_report)
            rec[f'{label}_{name}_ms'] = ms
            rec['instances'][f'{label}_{name}'] = (rep['instance'], rep['noise'])
            if label == 'q3':
                rec[f'q3_{name}_passes'] = rep['passes_sum'] / rep['row_tiles']
                rec[f'q3_{name}_unresolved'] = rep['unresolved']
    for label in ('waic', 'waic_loo', 'pit', 'q3'):
        rec[f'{label}_student_over_gaussian'] = rec[f'{label}_student_ms'] / rec[f'{label}_gaussian_ms']
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--nu', type=float, default=4.0)
    ap.add_argument('--limit', type=int, default=400)
    ap.add_argument('--one', action='store_true', help='run the single shape given by --columns --draws, in this process')
    ap.add_argument('--columns', type=int, default=100)
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.one:
        return one(args)
    lines = []
    given, skip = [], False                                  # the command as given, without where its output went
    for a in sys.argv[1:]:
        if skip or a == '--out':
            skip = not skip
            continue
        given.append(a)
    for nc, E in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '--rows', str(args.rows), '--columns', str(nc), '--draws', str(E),
               '--repeat', str(args.repeat), '--nu', str(args.nu)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"student_probe: {nc} columns x {E} draws ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"student_probe: {nc} columns x {E} draws ended with status {done.returncode}; nothing more is started\n" +
                     done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + '# python tools/student_probe.py' + ''.join(' ' + a for a in given) + '\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
