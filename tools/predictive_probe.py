"""Time of one fokl_predictive_rows launch (predictive_kernel) by its own events and the passes it ran, for (rows, columns,
draws, Q) = (1e6, 100, 1 000, 3), (1e6, 300, 1 000, 3) and (1e6, 100, 4 000, 8) and for the PIT-only call of the first shape,
next to predictive.predictive_rows_host on a slice of the rows scaled up to all of them.

    python tools/predictive_probe.py [--rows 1000000] [--repeat 2] [--host-rows 200] [--out FILE]

Every shape runs in a child process of its own under a time limit (--limit seconds), one after the other; the first child that
fails or runs out of time ends the probe and nothing more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

PEAK = 78.6e12
SHAPES = ((100, 1000, 3), (300, 1000, 3), (100, 4000, 8), (100, 1000, 0))     # columns, draws, Q (0: the PIT only)
QUANTILES = {0: (), 3: (0.025, 0.5, 0.975), 8: (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 0.9)}
HEADER = ("# tools/predictive_probe.py on one MI355X: kernel_ms = predictive_kernel by its own events, the best of the launches;\n"
          "# passes_max / passes_sum = the most passes a 16-row tile ran and their sum over the tiles (pass 0 not counted);\n"
          "# product_fraction_of_fp64_peak counts the products of the passes that ran, 2 x 16 ncp E per tile and pass;\n"
          "# host_ms_scaled = predictive.predictive_rows_host on a slice of the rows scaled to all of them; the errors are the\n"
          "# device against that slice\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import predictive as pd

    S, nc, E, Q = args.rows, args.columns, args.draws, args.quantiles
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    mean = rng.standard_normal(nc) / np.sqrt(nc)
    betas = mean + 0.05 * rng.standard_normal((E, nc)) / np.sqrt(nc)
    sig = 0.25 * (1.0 + 0.2 * rng.random(E))
    y = mean[0] + 0.5 * rng.standard_normal(S)
    head = np.empty((min(S, args.host_rows), nc - 1))
    ctx.upload(rng.random((S, 1)), np.zeros(S), getKernels.KERNEL_BERNOULLI, packed, nb, width)
    ctx.reserve_slots(nc + 2)
    for j in range(nc - 1):                                  # a column at a time: 300 columns of 1e6 rows are 2.4 GB
        col = rng.standard_normal(S)
        y += mean[j + 1] * col
        head[:, j] = col[:head.shape[0]]
        ctx.write_slot(2 + j, col)
    ctx.write_slot(_capi.SLOT_Y, y)
    slots = np.concatenate([[0], np.arange(2, nc + 1)]).astype(np.int32)
    ncp = (nc + 3) & ~3
    sd, rinv = pd.scales(sig)
    p = np.array(QUANTILES[Q])
    z = np.array([pd.normal_quantile(v) for v in p])
    block = ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)              # first launch: code object
    ms, t0 = [], time.perf_counter()
    for _ in range(args.repeat):
        block = ctx.predictive_rows(slots, betas, sd, rinv, True, p, z)
        ms.append(ctx.predictive_report()['kernel_ms'])
    wall = (time.perf_counter() - t0) / args.repeat
    rep = ctx.predictive_report()
    best = min(ms)
    rec = dict(rows=S, columns=nc, draws=E, quantiles=Q, kernel_ms=best, kernel_ms_all=ms, call_ms=1e3 * wall,
               passes_max=rep['passes_max'], passes_sum=rep['passes_sum'], passes_mean=rep['passes_sum'] / rep['row_tiles'],
               unresolved=rep['unresolved'],
               product_fraction_of_fp64_peak=2.0 * 16 * ncp * E * (rep['row_tiles'] + rep['passes_sum']) / (best * 1e-3) / PEAK,
               report=rep)
    hs = head.shape[0]
    X = np.concatenate([np.ones((hs, 1)), head], axis=1)
    t0 = time.perf_counter()
    ref = pd.predictive_rows_host(X, betas, sd, rinv, y[:hs], p, z)
    rec['host_ms_scaled'] = 1e3 * (time.perf_counter() - t0) * S / hs
    rec['pit_error_on_slice'] = float(np.abs(block[:hs, 5] - ref[:, 5]).max())
    if Q:
        rec['quantile_error_on_slice'] = float(np.abs(block[:hs, 6::5] - ref[:, 6::5]).max())
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-rows', type=int, default=200)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--one', action='store_true', help='run the single shape given by --columns --draws --quantiles, in this process')
    ap.add_argument('--columns', type=int, default=100)
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--quantiles', type=int, default=3, choices=sorted(QUANTILES))
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
    for nc, E, Q in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '--rows', str(args.rows), '--columns', str(nc), '--draws', str(E),
               '--quantiles', str(Q), '--repeat', str(args.repeat), '--host-rows', str(args.host_rows)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"predictive_probe: {nc} columns x {E} draws x {Q} quantiles ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"predictive_probe: {nc} columns x {E} draws x {Q} quantiles ended with status {done.returncode}; nothing more "
                     f"is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + '# python tools/predictive_probe.py' + ''.join(' ' + a for a in given) + '\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
