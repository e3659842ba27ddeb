"""Kernel time per iteration of fokl_robust_chains split by kernel (pass, reduce, step; by the launches' own events over the
last iterations of a short run) for (rows, columns, chains) = (1e6, 28, 4), (1e6, 100, 4) and (2e5, 127, 4), next to
robust.pass_host on a slice of the rows scaled up to all of them.

    python tools/robust_probe.py [--iterations 12] [--host-rows 20000] [--out FILE]

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

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12
SHAPES = ((1_000_000, 28, 4), (1_000_000, 100, 4), (200_000, 127, 4))          # rows, columns P + 1, chains
HEADER = ("# tools/robust_probe.py on one MI355X: *_ms_per_iteration = the kernel's launches by their own events, summed over the\n"
          "# timed iterations and divided by them (all chains together; per chain: divide by chains); run_ms_per_iteration = the\n"
          "# whole run by its two events over its iterations; column_read_fraction_of_hbm_peak and product_fraction_of_fp64_peak are\n"
          "# the pass's 8 n (P + 2) chains bytes and 2 n 256 pairs chains flops over pass time; host_pass_ms_scaled = one\n"
          "# robust.pass_host of ONE chain on a slice of the rows scaled to all of them\n")


def one(args):
    from fokl_gpy_amd import _capi, getKernels
    from fokl_gpy_amd import robust as rb

    n, nc, chains = args.rows, args.columns, args.chains
    rng = np.random.default_rng(0)
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    packed, nb, width = getKernels.pack_phis(getKernels.bernoulli(), getKernels.KERNEL_BERNOULLI)
    truth = rng.standard_normal(nc) / np.sqrt(nc)
    y = truth[0] + 0.1 * rng.standard_normal(n)
    hs = min(n, args.host_rows)
    head = np.empty((hs, nc - 1))
    ctx.upload(rng.random((n, 1)), np.zeros(n), getKernels.KERNEL_BERNOULLI, packed, nb, width)
    ctx.reserve_slots(nc + 2)
    for j in range(nc - 1):                                  # a column at a time
        col = rng.uniform(-1.0, 1.0, n)
        y += truth[j + 1] * col
        head[:, j] = col[:hs]
        ctx.write_slot(2 + j, col)
    y[::50] += 2.0
    ctx.write_slot(_capi.SLOT_Y, y)
    slots = np.concatenate([[0], np.arange(2, nc + 1)]).astype(np.int32)
    hyper = rb.hyper_of(4.0, 0.05, 4.0, 1.0, n, nc - 1)
    sig0, tau0 = np.full(chains, 0.01), np.full(chains, 0.5)
    ctx.robust_chains(slots, None, 4.0, hyper, truth, sig0, tau0, 0, 2, 1, 0, rows=False)          # first launch: code object
    t0 = time.perf_counter()
    raw = ctx.robust_chains(slots, None, 4.0, hyper, truth, sig0, tau0, 0, args.iterations, 1, 0, rows=True)
    wall = time.perf_counter() - t0
    rep = ctx.robust_report()
    timed, blocks = rep['timed_iterations'], rep['blocks']
    pairs = blocks * (blocks + 1) // 2
    pass_ms = rep['pass_ms'] / timed
    rec = dict(rows=n, columns=nc, chains=chains, iterations=rep['iterations'], timed_iterations=timed,
               pass_ms_per_iteration=pass_ms, reduce_ms_per_iteration=rep['reduce_ms'] / timed,
               step_ms_per_iteration=rep['step_ms'] / timed, run_ms_per_iteration=rep['total_ms'] / rep['iterations'],
               call_ms=1e3 * wall, column_read_fraction_of_hbm_peak=8.0 * n * (nc + 2) * chains / (pass_ms * 1e-3) / PEAK_BYTES,
               product_fraction_of_fp64_peak=2.0 * n * 256 * pairs * chains / (pass_ms * 1e-3) / PEAK_FLOPS,
               attempts_per_variate=rep['attempts'] / (chains * (rep['iterations'] - 1) * (n + 2) + 2 * chains), flagged=rep['flagged'],
               sd=float(np.sqrt(raw['sigsqd'][:, -1].mean())), report=rep)
    X = np.concatenate([np.ones((hs, 1)), head], axis=1)
    t0 = time.perf_counter()
    rb.pass_host(X, y[:hs], None, raw['betas'][0, -1], raw['sigsqd'][0, -1], 4.0, 0, 0, 1)
    rec['host_pass_ms_scaled'] = 1e3 * (time.perf_counter() - t0) * n / hs
    ctx.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=12)
    ap.add_argument('--host-rows', type=int, default=20000)
    ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--one', action='store_true', help='run the single shape given by --rows --columns --chains, in this process')
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--columns', type=int, default=100)
    ap.add_argument('--chains', type=int, default=4)
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
    for n, nc, chains in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '--rows', str(n), '--columns', str(nc), '--chains', str(chains),
               '--iterations', str(args.iterations), '--host-rows', str(args.host_rows)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"robust_probe: {n} rows x {nc} columns x {chains} chains ran out of its {args.limit} s; nothing more is started")
        if done.returncode != 0:
            sys.exit(f"robust_probe: {n} rows x {nc} columns x {chains} chains ended with status {done.returncode}; nothing more "
                     f"is started\n" + done.stderr[-2000:])
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(HEADER + '# python tools/robust_probe.py' + ''.join(' ' + a for a in given) + '\n')
                fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
