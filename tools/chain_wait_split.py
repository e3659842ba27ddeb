"""Where the wait for a sub-stage model's host chain goes, from the stderr of a run under FOKL_CHAIN_PROFILE=1
FOKL_SEARCH_PROFILE=1 (the second delimits the fits):

    FOKL_CHAIN_PROFILE=1 FOKL_SEARCH_PROFILE=1 python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-microbench \
        --no-throughput --no-parity 2> err.txt
    python tools/chain_wait_split.py err.txt

Per chain: microseconds between submission and a chain thread taking it, standing in front of blocks of the tape that
were not finished yet, in the recursion itself, and in the statistics behind it; next to them what the driver thread
waited for that chain.  One table for the last fit of the file, then the sums per fit over all fits but the first."""
import re
import sys

CHAIN = re.compile(r'fokl_chain: p1 (\d+) draws (\d+) queued ([\d.]+) us, waited for the tape ([\d.]+) us, recursion ([\d.]+) us, '
                   r'statistics ([\d.]+) us, recut (\d)')
WAIT = re.compile(r'fokl_search: waited ([\d.]+) us for the host chain of p1 (\d+)')


def main(path):
    fits, chains, waits = [], [], []
    for line in open(path):
        m = CHAIN.search(line)
        if m:
            chains.append([int(m.group(1))] + [float(m.group(i)) for i in (3, 4, 5, 6)] + [int(m.group(7))])
        m = WAIT.search(line)
        if m:
            waits.append((int(m.group(2)), float(m.group(1))))
        if line.startswith('fokl_search teardown'):
            if chains:
                fits.append((chains, waits))
            chains, waits = [], []
    if not fits:
        sys.exit('no fit found (FOKL_CHAIN_PROFILE=1 FOKL_SEARCH_PROFILE=1?)')
    chains, waits = fits[-1]
    print(f'{len(fits)} fits; the last one, chain by chain (us):')
    print('   p1   queued  tape not there  recursion  statistics  recut | driver waited')
    by_p1 = {}
    for p1, us in waits:
        by_p1.setdefault(p1, []).append(us)
    for p1, queued, tape, rec, stat, recut in chains:
        waited = by_p1.get(p1, [])
        print(f'{p1:5d} {queued:8.1f} {tape:15.1f} {rec:10.1f} {stat:11.1f} {recut:6d} | '
              + (f'{waited.pop(0):8.1f}' if waited else '    never (started ahead, not used)'))
    rest = fits[1:] or fits
    n = len(rest)
    tot = [sum(c[i] for ch, _ in rest for c in ch) / n for i in range(1, 5)]
    print(f'per fit, mean of {n} fits: {sum(len(ch) for ch, _ in rest) / n:.1f} chains, queued {tot[0] / 1e3:.2f} ms, tape not there '
          f'{tot[1] / 1e3:.2f} ms, recursion {tot[2] / 1e3:.2f} ms, statistics {tot[3] / 1e3:.2f} ms, recuts '
          f'{sum(c[5] for ch, _ in rest for c in ch) / n:.2f}; the driver waited {sum(w for _, ws in rest for _, w in ws) / n / 1e3:.2f} ms '
          f'in {sum(len(ws) for _, ws in rest) / n:.1f} waits')


if __name__ == '__main__':
    main(sys.argv[1])
