"""Kernel time of one fokl_acquire_select call split by kernel (the pass launches, the bound launches, the pivot launches, by
the call's own events with the context's timing on) and the 16-row tiles evaluated per pick, for both criteria, lazy on and
off, next to acquire.select_host on a 200-row slice of the pool scaled up to all of it.

    python tools/acquire_probe.py [--cases 1000000,29,1000,16 1000000,101,1000,16 200000,601,1000,8] [--repeat 2] [--out FILE]

A case is rows,columns,draws,picks.  Every (case, criterion) pair runs in a child process of its own under a time limit
(--limit seconds), lazy and full one after the other in it; the first child that fails or runs out of time ends the probe
and nothing more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

HEADER = ("# tools/acquire_probe.py on one MI355X: microseconds of the kernels of one fokl_acquire_select call by its own events "
          "(the best call by its\n# total) for lazy = true and false: pass, bound and pivot = all picks; tiles = 16-row tiles "
          "evaluated per pick; same_bits = lazy and full returned the same\n# index and gain bytes; host_ms_scaled = "
          "acquire.select_host (lazy) on a slice of the pool, its time scaled to all rows\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import acquire as aq

    S, nc, E, picks = (int(v) for v in args.cases[0].split(','))
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
    betas = rng.standard_normal(nc) + 0.3 * rng.standard_normal((E, nc))
    train = np.concatenate([np.ones((2000, 1)), rng.random((2000, nc - 1)) - 0.5], axis=1)
    b0 = (train @ betas.T).max(axis=0)                       # what incumbent='training' is to a model: 2 000 other rows
    ctx.timing_enable(True)
    rec = dict(rows=S, columns=nc, draws=E, picks=picks, criterion=args.criterion)
    results = {}
    for lazy in (True, False):
        res = ctx.acquire_select(slots, betas, b0, picks, args.criterion, lazy)         # first call: code object
        best, calls = None, []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            res = ctx.acquire_select(slots, betas, b0, picks, args.criterion, lazy)
            wall = time.perf_counter() - t0
            rep = ctx.acquire_report()
            calls.append(rep['kernel_us'])
            if best is None or rep['kernel_us'] < best['kernel_us']:
                best = dict(rep, call_ms=1e3 * wall)
        results[lazy] = res
        rec['lazy' if lazy else 'full'] = dict(
            kernel_us=best['kernel_us'], pass_us=best['pass_us'], bound_us=best['bound_us'], pivot_us=best['pivot_us'],
            call_ms=best['call_ms'], kernel_us_all=calls, launches=best['launches'], tiles=res['tiles_evaluated'].tolist(),
            tiles_evaluated=best['tiles_evaluated'])
        rec.update(grid=best['grid'], bound_grid=best['bound_grid'], row_tiles=best['row_tiles'], lds_bytes=best['lds_bytes'],
                   dt=best['dt'])
    rec['same_bits'] = bool(results[True]['index'].tobytes() == results[False]['index'].tobytes() and
                            results[True]['gain'].tobytes() == results[False]['gain'].tobytes())
    rec['full_over_lazy'] = rec['full']['kernel_us'] / max(rec['lazy']['kernel_us'], 1)
    t0 = time.perf_counter()
    ref = aq.select_host(head, betas, b0, min(picks, hs), args.criterion, True)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rec.update(host_rows=hs, host_ms_on_slice=host_ms, host_ms_scaled=host_ms * S / hs, gains=results[True]['gain'].tolist(),
               first_gain_host_slice=float(ref['gain'][0]))
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['1000000,29,1000,16', '1000000,101,1000,16', '200000,601,1000,8'])
    ap.add_argument('--criterion', default=None, help="'ei' or 'pi' (default: both, one after the other)")
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-rows', type=int, default=200)
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
        for criterion in ([args.criterion] if args.criterion else ['ei', 'pi']):
            cmd = [sys.executable, os.path.abspath(__file__), '--one', '--cases', case, '--criterion', criterion,
                   '--repeat', str(args.repeat), '--host-rows', str(args.host_rows)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"acquire_probe: {case} '{criterion}' ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"acquire_probe: {case} '{criterion}' ended with status {done.returncode}; nothing more is started\n"
                         + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + '# python tools/acquire_probe.py' + ''.join(' ' + a for a in given) + '\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
