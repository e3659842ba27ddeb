"""bench.py --dump-outputs: the files hold what the fits of the last timed step returned, in float64, the same from run to
run and never more than bench.DUMP_BYTES in all.  The writer is plain numpy (CPU); that a benchmark run hands it the timed
fits' own results is checked on the GPU against the oracle's golden of a configs[4] unit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.abspath(bench.__file__))


def load_dir(path):
    return {name[:-4]: np.load(os.path.join(path, name), allow_pickle=False) for name in sorted(os.listdir(path))}


def test_dump_writes_every_result_of_every_unit_as_float64(tmp_path):
    rng = np.random.default_rng(3)
    results = {5: (rng.standard_normal((40, 7)), rng.integers(0, 4, (6, 3)), rng.standard_normal(9)),
               2: (rng.standard_normal((40, 4)), rng.integers(0, 4, (3, 3)), rng.standard_normal((5, 1)))}
    bench.dump_outputs(str(tmp_path / 'out'), results)
    got = load_dir(tmp_path / 'out')
    assert sorted(got) == ['unit2_betas', 'unit2_evs', 'unit2_mtx', 'unit5_betas', 'unit5_evs', 'unit5_mtx']
    for unit, fit in results.items():
        for name, want in zip(('betas', 'mtx', 'evs'), fit):
            have = got[f'unit{unit}_{name}']
            assert have.dtype == np.float64 and have.shape == want.shape and np.array_equal(have, want)


def test_dump_beyond_the_cap_keeps_the_same_rows_in_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 16)
    rng = np.random.default_rng(4)
    results = {u: (rng.standard_normal((500, 12)), rng.integers(0, 4, (11, 8)), rng.standard_normal(30)) for u in range(4)}
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), results)
    a, b = load_dir(tmp_path / 'a'), load_dir(tmp_path / 'b')
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    on_disk = sum(os.path.getsize(tmp_path / 'a' / name) for name in os.listdir(tmp_path / 'a'))
    assert 0.8 * bench.DUMP_BYTES < on_disk <= bench.DUMP_BYTES
    for u, (betas, _, _) in results.items():
        kept = a[f'unit{u}_betas']
        rows = [int(np.flatnonzero((betas == row).all(axis=1))[0]) for row in kept]       # rows of the result, in its order
        assert 0 < len(rows) < betas.shape[0] and rows == sorted(set(rows))


def test_dump_needs_a_timed_step(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0', '--dump-outputs', str(tmp_path / 'd')],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and '--steps' in out.stderr
    assert not os.path.exists(tmp_path / 'd')


@pytest.mark.gpu
@pytest.mark.parametrize('fits_per_step,procs', [(1, 1), (2, 2)])
def test_benchmark_dumps_what_its_timed_fits_returned(tmp_path, fits_per_step, procs):
    """configs[4] with its fits in the reporting process (1 fit per step) and dealt over worker processes (2 over 2): unit 0
    of the dump is the fit of tests/golden/cfg4_unit0_n1e5_m8.npz, to the tolerances of tests/test_config_goldens.py."""
    golden = os.path.join(GOLDEN, 'cfg4_unit0_n1e5_m8.npz')
    if not os.path.exists(golden):
        pytest.skip('cfg4_unit0_n1e5_m8.npz has not been generated (tests/golden/make_config_golden.py)')
    g = np.load(golden, allow_pickle=False)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                          '--config', '4', '--fits-per-step', str(fits_per_step), '--procs', str(procs), '--no-cpu-baseline',
                          '--no-microbench', '--no-parity', '--dump-outputs', str(tmp_path / 'out')],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['steps'] == 2 and line['fits_per_s'] > 0
    got = load_dir(tmp_path / 'out')
    assert sorted(got) == sorted(f'unit{u}_{name}' for u in range(fits_per_step) for name in ('betas', 'mtx', 'evs'))
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got['unit0_mtx'], g['mtx'])
    np.testing.assert_allclose(got['unit0_evs'], g['evs'], rtol=1e-9)
    assert got['unit0_betas'].shape == g['betas'].shape
    assert np.max(np.abs(got['unit0_betas'] - g['betas']) / np.max(np.abs(g['betas']), axis=0)) < 1e-9
