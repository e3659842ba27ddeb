"""Kernel time of one fokl_design_select call split by kernel (the quadratic-form launches, the step launches, the pivot
launches, by the call's own events with the context's timing on), for both criteria, next to design.select_host on a slice
of the pool scaled up to all of it.

    python tools/design_probe.py [--cases 1000000,29,64 1000000,101,256 200000,601,64] [--repeat 2] [--out FILE]

A case is rows,columns,picks.  Every (case, criterion) pair runs in a child process of its own under a time limit (--limit
seconds), one after the other; the first child that fails or runs out of time ends the probe and nothing more is started
on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

HEADER = ("# tools/design_probe.py on one MI355X: microseconds of the kernels of one fokl_design_select call by its own events "
          "(the best call by its\n# total): quadform = first pass + refreshes, step and pivot = all picks; host_ms_scaled = "
          "design.select_host on a slice of the pool,\n# its time scaled to all rows; refresh_every = 64\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import design as dg

    S, nc, picks = (int(v) for v in args.cases[0].split(','))
    ivr = args.criterion == 'ivr'
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    hs = min(S, args.host_rows)
    head = np.ones((hs, nc))
    ctx.upload(rng.random((S, 1)), np.zeros(S), getKernels.KERNEL_BERNOULLI, packed, nb, width)
    ctx.reserve_slots(nc + 2)
    for j in range(nc - 1):                                  # a column at a time: 600 columns of 2e5 rows are 1 GB
        col = rng.random(S) - 0.5
        head[:, j + 1] = col[:hs]
        ctx.write_slot(2 + j, col)
    slots = np.concatenate([[0], np.arange(2, nc + 1)]).astype(np.int32)
    G = np.array(ctx.gram(slots, slots), dtype=np.float64)
    G = 0.5 * (G + G.T)
    C0 = dg.information_inverse(G / 100.0, 1.0)              # a training set a hundredth of the pool, tau^2 = 1
    CMC0 = C0 @ (G / S) @ C0 if ivr else None
    CMC0 = None if CMC0 is None else 0.5 * (CMC0 + CMC0.T)
    ctx.timing_enable(True)
    res = ctx.design_select(slots, C0, CMC0, picks, False, 64)                   # first call: code object
    best, calls = None, []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        res = ctx.design_select(slots, C0, CMC0, picks, False, 64)
        wall = time.perf_counter() - t0
        rep = ctx.design_report()
        calls.append(rep['kernel_us'])
        if best is None or rep['kernel_us'] < best['kernel_us']:
            best = dict(rep, call_ms=1e3 * wall)
    t0 = time.perf_counter()
    ref = dg.select_host(head, C0, CMC0, picks, False, 64)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rec = dict(rows=S, columns=nc, picks=picks, criterion=args.criterion, kernel_us=best['kernel_us'],
               quadform_us=best['quadform_us'], step_us=best['step_us'], pivot_us=best['pivot_us'], call_ms=best['call_ms'],
               us_per_pick=(best['step_us'] + best['pivot_us']) / picks, kernel_us_all=calls, refreshes=best['refreshes'],
               launches=best['launches'], grid=best['grid'], step_grid=best['step_grid'], lds_bytes=best['lds_bytes'],
               host_rows=hs, host_ms_on_slice=host_ms, host_ms_scaled=host_ms * S / hs,
               first_gain=float(res['gain'][0]), first_gain_host_slice=float(ref['gain'][0]))
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['1000000,29,64', '1000000,101,256', '200000,601,64'])
    ap.add_argument('--criterion', default=None, help="'variance' or 'ivr' (default: both, one after the other)")
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-rows', type=int, default=20000)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--one', action='store_true', help='run the single (case, criterion) pair given, in this process')
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
    for case in args.cases:
        for criterion in ([args.criterion] if args.criterion else ['variance', 'ivr']):
            cmd = [sys.executable, os.path.abspath(__file__), '--one', '--cases', case, '--criterion', criterion,
                   '--repeat', str(args.repeat), '--host-rows', str(args.host_rows)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"design_probe: {case} '{criterion}' ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"design_probe: {case} '{criterion}' ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + '# python tools/design_probe.py' + ''.join(' ' + a for a in given) + '\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
