"""Kernel time of one fokl_drawbest_rows call (the whole queue by the call's own events, and with the context's timing on the
passes and the merges apart), next to one fokl_population_stats call without cuts at the same shape: the same product
reduced in the same direction, moments in the place of (value, row).

    python tools/optimize_pool_probe.py [--cases 1000000,29,1000,1 1000000,101,1000,1 1000000,101,1000,4 200000,601,1000,1]
                                        [--repeat 2] [--out FILE]

A case is rows,columns,draws,ranks.  Every case runs in a child process of its own under a time limit (--limit seconds); the
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

HEADER = ("# tools/optimize_pool_probe.py on one MI355X: microseconds of the kernels of one fokl_drawbest_rows call by its own "
          "events (the better of the calls\n# by its total): kernel_us = the whole queue of 2 * ranks launches, pass_us and "
          "merge_us = the passes and the merges; population_us = both kernels\n# of one fokl_population_stats call without "
          "cuts on the same columns and draws (the better of the calls); rank0_over_population = kernel_us / ranks\n# over "
          "population_us; host_ms_scaled = pooloptimum.ranks_host on a slice of the pool, its time scaled to all rows\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import pooloptimum as po

    S, nc, E, ranks = (int(v) for v in args.cases[0].split(','))
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
    ctx.timing_enable(True)
    rec = dict(rows=S, columns=nc, draws=E, ranks=ranks)

    res = ctx.drawbest_rows(slots, betas, None, ranks)      # first call: code object
    best, calls = None, []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        res = ctx.drawbest_rows(slots, betas, None, ranks)
        wall = time.perf_counter() - t0
        rep = ctx.drawbest_report()
        calls.append(rep['kernel_us'])
        if best is None or rep['kernel_us'] < best['kernel_us']:
            best = dict(rep, call_ms=1e3 * wall)
    rec.update(kernel_us=best['kernel_us'], pass_us=best['pass_us'], merge_us=best['merge_us'], call_ms=best['call_ms'],
               kernel_us_all=calls, launches=best['launches'], grid=best['grid'], row_chunks=best['row_chunks'],
               draw_blocks=best['draw_blocks'], row_tiles=best['row_tiles'], lds_bytes=best['lds_bytes'],
               coefficients=best['coefficients'])

    shift = betas[:, 0].copy()
    ctx.population_stats(slots, betas, shift, None, False)
    pop = []
    for _ in range(args.repeat):
        ctx.timing_reset()
        mom, _ = ctx.population_stats(slots, betas, shift, None, False)
        pop.append(1e3 * ctx.timing_get(_capi.K_POPULATION)['ms'])
    rec.update(population_us=min(pop), population_us_all=pop, population_coefficients=ctx.population_report()['coefficients'],
               rank0_over_population=best['kernel_us'] / ranks / max(min(pop), 1e-9),
               same_maximum=bool(np.array_equal(mom[:, 3], res['value'][0])))

    t0 = time.perf_counter()
    ref = po.ranks_host(head, betas, ranks)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rec.update(host_rows=hs, host_ms_on_slice=host_ms, host_ms_scaled=host_ms * S / hs,
               distinct_best_rows=int(np.unique(res['index'][0]).shape[0]),
               best_value_range=[float(res['value'][0].min()), float(res['value'][0].max())],
               best_value_range_host_slice=[float(ref['value'][0].min()), float(ref['value'][0].max())])
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+',
                    default=['1000000,29,1000,1', '1000000,101,1000,1', '1000000,101,1000,4', '200000,601,1000,1'])
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--host-rows', type=int, default=2000)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--one', action='store_true', help='run the single case given, in this process')
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
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '--cases', case, '--repeat', str(args.repeat),
               '--host-rows', str(args.host_rows)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"optimize_pool_probe: {case} ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"optimize_pool_probe: {case} ended with status {done.returncode}; nothing more is started\n"
                     + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + '# python tools/optimize_pool_probe.py' + ''.join(' ' + a for a in given) + '\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
