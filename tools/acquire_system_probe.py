"""Kernel time of one fokl_acquire_system_select call split by kernel (by the call's own events with the context's timing
on) and the 16-row tiles evaluated per pick, for both criteria, lazy on and off, next to fokl_acquire_select on the same
objective and the same pool in the same process.

    python tools/acquire_system_probe.py [--cases 1000000,29,29,16 1000000,101,29+29,16 200000,601,101,8] [--draws 1000]
                                         [--repeat 2] [--out FILE]

A case is rows,objective columns,constraint columns (several models joined with +),picks.  The expectation to measure
against: a full pass costs about sum ncp_k / ncp_0 times the unconstrained pass (``columns_ratio``), because the matrix
work scales that way.  Each constraint model's limits are the 15 % and 85 % quantiles of its own values over 2 000 rows and
all draws, so about 70 % of the (row, draw) pairs satisfy one model.  Every (case, criterion) pair runs in a child process
of its own under a time limit (--limit seconds); the first child that fails or runs out of time ends the probe and nothing
more is started on the device.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

HEADER = ("# tools/acquire_system_probe.py on one MI355X: microseconds of the kernels of one fokl_acquire_system_select call "
          "('system') and of one\n# fokl_acquire_select call on the same objective and pool ('free') by their own events (the "
          "best call by its total), lazy = true and false;\n# tiles = 16-row tiles evaluated per pick; columns_ratio = sum of "
          "the models' padded columns / the objective's: what a full pass is expected\n# to cost over the unconstrained one; "
          "full_ratio, lazy_ratio = system / free kernel time; share = feasible (row, draw) pairs on a 2 000-row sample\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels

    S, nc0, cons, picks = args.cases[0].split(',')
    S, nc0, picks, E = int(S), int(nc0), int(picks), args.draws
    widths = [nc0] + [int(v) for v in cons.split('+')]
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    hs = min(S, 2000)
    ctx.upload(rng.random((S, 1)), np.zeros(S), getKernels.KERNEL_BERNOULLI, packed, nb, width)
    ctx.reserve_slots(sum(widths) + 2)
    slots, heads, at = [], [], _capi.SLOT_FIRST_FREE
    for nc in widths:
        head = np.ones((hs, nc))
        for j in range(nc - 1):                              # a column at a time
            col = rng.random(S) - 0.5
            head[:, j + 1] = col[:hs]
            ctx.write_slot(at + j, col)
        slots.append(np.concatenate([[_capi.SLOT_ONES], np.arange(at, at + nc - 1)]).astype(np.int32))
        heads.append(head)
        at += nc - 1
    betas = [rng.standard_normal(nc) + 0.3 * rng.standard_normal((E, nc)) for nc in widths]
    train = np.concatenate([np.ones((2000, 1)), rng.random((2000, nc0 - 1)) - 0.5], axis=1)
    b0 = (train @ betas[0].T).max(axis=0)
    lo, hi, ok = [], [], np.ones((hs, E), dtype=bool)
    for head, B in zip(heads[1:], betas[1:]):
        G = head @ B.T
        lo.append(float(np.quantile(G, 0.15)))
        hi.append(float(np.quantile(G, 0.85)))
        ok &= (G >= lo[-1]) & (G <= hi[-1])
    padded = [-(-nc // 4) * 4 for nc in widths]
    ctx.timing_enable(True)
    rec = dict(rows=S, columns=widths, draws=E, picks=picks, criterion=args.criterion, share=float(ok.mean()),
               columns_ratio=sum(padded) / padded[0])
    runs = {'system': (lambda lazy: ctx.acquire_system_select(slots, betas, b0, lo, hi, picks, args.criterion, lazy),
                       ctx.acquire_system_report),
            'free': (lambda lazy: ctx.acquire_select(slots[0], betas[0], b0, picks, args.criterion, lazy), ctx.acquire_report)}
    results = {}
    for name, (call, report) in runs.items():
        rec[name] = {}
        for lazy in (True, False):
            res = call(lazy)                                 # first call: code object
            best, calls = None, []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                res = call(lazy)
                wall = time.perf_counter() - t0
                rep = report()
                calls.append(rep['kernel_us'])
                if best is None or rep['kernel_us'] < best['kernel_us']:
                    best = dict(rep, call_ms=1e3 * wall)
            results[name, lazy] = res
            rec[name]['lazy' if lazy else 'full'] = dict(
                kernel_us=best['kernel_us'], pass_us=best['pass_us'], bound_us=best['bound_us'], pivot_us=best['pivot_us'],
                call_ms=best['call_ms'], kernel_us_all=calls, launches=best['launches'], tiles=res['tiles_evaluated'].tolist(),
                tiles_evaluated=best['tiles_evaluated'])
            rec[name].update(grid=best['grid'], bound_grid=best['bound_grid'], row_tiles=best['row_tiles'],
                             lds_bytes=best['lds_bytes'])
        rec[name]['same_bits'] = bool(results[name, True]['index'].tobytes() == results[name, False]['index'].tobytes() and
                                      results[name, True]['gain'].tobytes() == results[name, False]['gain'].tobytes())
        rec[name]['gains'] = results[name, True]['gain'].tolist()
    rec['feasible_draws'] = results['system', True]['feasible'].tolist()
    rec['full_ratio'] = rec['system']['full']['kernel_us'] / max(rec['free']['full']['kernel_us'], 1)
    rec['lazy_ratio'] = rec['system']['lazy']['kernel_us'] / max(rec['free']['lazy']['kernel_us'], 1)
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['1000000,29,29,16', '1000000,101,29+29,16', '200000,601,101,8'])
    ap.add_argument('--criterion', default=None, help="'ei' or 'pi' (default: both, one after the other)")
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--repeat', type=int, default=2)
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
                   '--repeat', str(args.repeat), '--draws', str(args.draws)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"acquire_system_probe: {case} '{criterion}' ran out of its {args.limit} s; nothing more is started")
            if done.returncode != 0:
                sys.exit(f"acquire_system_probe: {case} '{criterion}' ended with status {done.returncode}; nothing more is "
                         f"started\n" + done.stderr[-2000:])
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, 'w') as fh:
                    fh.write(HEADER + '# python tools/acquire_system_probe.py' + ''.join(' ' + a for a in given) + '\n')
                    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
