"""Time of one fokl_score_rows launch (score_kernel) by its own events, for 'waic' alone and for 'waic' plus 'loo', as a
fraction of the fp64 matrix peak (78.6 TFLOP/s, 2 S ncp E flops), next to score.score_rows_host on a slice of the rows
scaled up to all of them.

    python tools/score_probe.py [--rows 1000000] [--columns 100 300] [--draws 1000 4000] [--repeat 3] [--out FILE]

Every (columns, draws) pair runs in a child process of its own under a time limit (--limit seconds), one after the other; the
first child that fails or runs out of time ends the probe and nothing more is started on the device.
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
HEADER = ("# tools/score_probe.py on one MI355X: kernel_ms = score_kernel by its own events, the best of the launches; "
          "host_ms_scaled = score.score_rows_host\n# ('waic' + 'loo') on a slice of the rows scaled to all of them; the errors "
          "are the device against that slice\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import score as sc

    S, nc, E = args.rows, args.columns[0], args.draws[0]
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
    rec = dict(rows=S, columns=nc, draws=E, tail=sc.tail_len(E))
    for name, want_loo in (('waic', False), ('waic_loo', True)):
        stats = ctx.score_rows(slots, betas, sig, want_loo)                      # first launch: code object
        ms, t0 = [], time.perf_counter()
        for _ in range(args.repeat):
            stats = ctx.score_rows(slots, betas, sig, want_loo)
            ms.append(ctx.score_report()['kernel_ms'])
        wall = (time.perf_counter() - t0) / args.repeat
        best = min(ms)
        rec[name] = dict(kernel_ms=best, kernel_ms_all=ms, call_ms=1e3 * wall,
                         fraction_of_fp64_peak=2.0 * S * ncp * E / (best * 1e-3) / PEAK, report=ctx.score_report())
    hs = head.shape[0]
    X = np.concatenate([np.ones((hs, 1)), head], axis=1)
    t0 = time.perf_counter()
    ref = sc.score_rows_host(X, y[:hs], betas, sig)
    rec['host_ms_scaled'] = 1e3 * (time.perf_counter() - t0) * S / hs
    finite = np.isfinite(ref[:, 4])
    rec['elpd_loo_error_on_slice'] = float(np.abs(stats[:hs, 3] - ref[:, 3]).max())
    rec['khat_error_on_slice'] = float(np.abs(stats[:hs, 4] - ref[:, 4])[finite].max())
    rec['khat_max'] = float(stats[np.isfinite(stats[:, 4]), 4].max())
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--columns', type=int, nargs='+', default=[100, 300])
    ap.add_argument('--draws', type=int, nargs='+', default=[1000, 4000])
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-rows', type=int, default=200)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--one', action='store_true', help='run the single (columns, draws) pair given, in this process')
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
    for nc in args.columns:
        for E in args.draws:
            cmd = [sys.executable, os.path.abspath(__file__), '--one', '--rows', str(args.rows), '--columns', str(nc),
                   '--draws', str(E), '--repeat', str(args.repeat), '--host-rows', str(args.host_rows)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"score_probe: {nc} columns x {E} draws ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"score_probe: {nc} columns x {E} draws ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + '# python tools/score_probe.py' + ''.join(' ' + a for a in given) + '\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
