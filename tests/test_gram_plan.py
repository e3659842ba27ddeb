"""
The launch plan of the tile-list Gram kernel (fokl_gram path 2, csrc/fokl_hip.hip: plan_gram) is host arithmetic:
replayed here with numpy -- every tile list executed as the kernel executes it (staged column tiles, the k-steps of a
wavefront team, the slab reduction with the column permutation and the mirror image of the tiles below the diagonal) --
the result must be the block X_r' X_c exactly (integer data), for every shape the search produces and a few it does not.
No device needed.
"""
import numpy as np
import pytest

from fokl_gpy_amd import _capi


def replay(cols, rs, cs, kind=0):
    n = cols.shape[0]
    pl = _capi.gram_plan(rs, cs, kind)
    ks, IT, JT, nci = pl['ks'], pl['i_tiles'], pl['j_tiles'], pl['nci']
    assert pl['rows_per_chunk'] in (32, 64, 128, 256, 512) and pl['ct'] * pl['rows_per_chunk'] // 32 <= 16
    assert 1 <= pl['nt'] <= (4 if kind else 8 if pl['half'].any() else 10) and 1 <= pl['ct'] <= (8 if kind else 16)
    assert ks in (1, 2, 4) and (ks == 1 or pl['nt'] == 1) and pl['waves'] == 4 and (ks == 1 or not kind)
    assert np.array_equal(pl['icols'][:len(rs)], rs)
    X = np.zeros((n, 16 * JT))
    X[:, :nci] = cols[:, pl['icols']]
    slab = np.full((ks, 16 * IT, 16 * JT), np.nan)             # positions nobody computes stay NaN
    rows = np.arange(n)
    written = set()
    for g in range(pl['tiles'].shape[0]):
        st = pl['staged'][g]
        assert np.all(st[pl['ct']:] == -1)
        for w in range(4):
            for k in range(10):
                a, b, oi, oj = pl['tiles'][g, w, k]
                if oi < 0:
                    assert 0 <= a < pl['ct'] and 0 <= b < pl['ct']        # padding tiles still read valid LDS
                    continue
                half_slots = bool(pl['half'].any())                       # entries 0, 1 of every list: half-tile slots
                assert st[a] == oi and st[b] == oj and oj >= oi and (k - 2 if half_slots else k) < pl['nt']
                phase = w % ks
                assert (oi, oj, phase) not in written
                written.add((oi, oj, phase))
                sel = ((rows % 32) // 4) % ks == phase                    # the k-steps this wavefront multiplies
                if pl['half'][g, w, k]:
                    # formed as an 8 x 16 half tile: only where rows 8 .. 15 of the tile are nobody's (they stay NaN here)
                    assert k < 2 and oi == IT - 1 and 1 <= len(rs) % 16 <= 8 and ks == 1 and not kind
                    slab[phase, 16 * oi:16 * oi + 8, 16 * oj:16 * oj + 16] = \
                        X[sel][:, 16 * oi:16 * oi + 8].T @ X[sel][:, 16 * oj:16 * oj + 16]
                    continue
                assert not (half_slots and k < 2)
                slab[phase, 16 * oi:16 * oi + 16, 16 * oj:16 * oj + 16] = \
                    X[sel][:, 16 * oi:16 * oi + 16].T @ X[sel][:, 16 * oj:16 * oj + 16]
    total = slab.sum(axis=0)
    out = np.empty((len(rs), len(cs)))
    for i in range(len(rs)):
        for j in range(len(cs)):
            c, r = int(pl['perm'][j]), i
            if (c >> 4) < (r >> 4):
                r, c = c, r
            out[i, j] = total[r, c]
    return out, pl



def _kinds():
    """Tile-list kinds the library plans: 0 (16x16x4 MFMA, the product) and -- development builds only (make DEV=1) -- 1, the
    retired 4x4x4 form."""
    try:
        _capi.gram_plan(np.array([2], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32), kind=1)
        return (0, 1)
    except _capi.FoklNativeError as exc:
        assert 'development build' in str(exc)
        return (0,)


KINDS = _kinds()

SHAPES = [(1, 1), (2, 3), (8, 10), (16, 16), (17, 33), (28, 38), (56, 58), (56, 66), (65, 131), (70, 150), (56, 176),
          (33, 40), (48, 48), (200, 60), (120, 300)]
# the widths models have today (586, 768 and 1000 columns): 12 to 16 staged column tiles per group, ten tiles per list, up
# to 24 groups and 16 row tiles (four bands of four) -- the plans tests/test_fit_kernels_device.py runs on the device
WIDE_SHAPES = [(1, 1000), (8, 1000), (24, 768), (32, 150), (48, 150), (40, 180), (48, 586), (72, 768), (100, 586), (104, 300),
               (160, 768), (200, 202), (256, 1000)]


@pytest.mark.parametrize('nr,nc', WIDE_SHAPES)
def test_wide_tile_lists_reproduce_the_block(nr, nc):
    """The search's pattern and a disjoint column list at the wide shapes, on 20-bit integers (64 rows: exact in double)."""
    rng = np.random.default_rng(nr * 1000 + nc)
    n, pool = 64, nr + nc + 4
    cols = rng.integers(-2 ** 20 + 1, 2 ** 20, size=(n, pool)).astype(np.float64)
    rs = (2 + rng.permutation(pool - 2)[:nr]).astype(np.int32)
    rest = np.setdiff1d(np.arange(2, pool), rs)
    search = np.concatenate([[0], rest[:nc - nr - 2], rs, [1]]).astype(np.int32)
    assert search.shape[0] == nc
    seen = dict(ct=0, nt=0)
    for cs in (search, rest[:nc].astype(np.int32), rng.integers(0, pool, nc).astype(np.int32)):
        out, pl = replay(cols, rs, cs)
        assert np.array_equal(out, cols[:, rs].T @ cols[:, cs])
        seen = dict(ct=max(seen['ct'], pl['ct']), nt=max(seen['nt'], pl['nt']))
    if nc >= 586:
        assert seen['ct'] >= 14 and (seen['nt'] >= 9 or nr <= 24)


@pytest.mark.parametrize('nr,nc', SHAPES)
def test_tile_lists_reproduce_the_block(nr, nc):
    rng = np.random.default_rng(nr * 1000 + nc)
    n = 96
    cols = rng.integers(-3, 4, size=(n, 400)).astype(np.float64)
    # (a) the search's own pattern [ones | model | new | y] with the new columns on the row side, (b) unrelated random
    # lists with partial overlap, (c) lists with repeated slots
    new = rng.permutation(400)[:nr]
    rest = np.setdiff1d(np.arange(400), new)
    search = np.concatenate([rest[:max(nc - nr, 0) // 2], new, rest[200:200 + max(nc - nr, 0)]])[:nc]
    cases = [(new, search), (rng.permutation(400)[:nr], rng.permutation(400)[:nc]),
             (rng.integers(0, 40, nr), rng.integers(0, 40, nc))]
    for rs, cs in cases:
        rs, cs = rs.astype(np.int32), cs.astype(np.int32)
        for kind in KINDS:
            out, _ = replay(cols, rs, cs, kind)
            assert np.array_equal(out, cols[:, rs].T @ cols[:, cs]), kind


def test_symmetric_part_is_computed_once_and_work_is_balanced():
    # 56 new columns against [ones | 118 model columns | the 56 | y]: 4 x 11 tiles, the 6 below the diagonal skipped
    rs = np.arange(100, 156, dtype=np.int32)
    cs = np.concatenate([[0], np.arange(200, 318), rs, [1]]).astype(np.int32)
    pl = _capi.gram_plan(rs, cs)
    real = pl['tiles'][..., 2] >= 0
    assert pl['i_tiles'] == 4 and pl['j_tiles'] == 11 and int(real.sum()) == 38
    per_wave = real.sum(axis=2)
    assert per_wave.max() - per_wave.min() <= 1
    # its last row tile holds 8 of the 56 columns: the 8 tiles of that row sit in the half-tile slots (entries 0 and 1 of
    # the four lists; half the matrix-pipe time each in gram_tiles_dma_kernel), the 30 others follow from entry 2 -- 8 of
    # them per list at most -- and the lists carry 9, 9, 8, 8 tiles' worth of work where plain dealing gives 10, 10, 9, 9
    assert int(pl['half'].sum()) == 8 and np.all(pl['half'][0, :, :2]) and np.all(pl['tiles'][0, :, :2, 2] == 3)
    assert pl['nt'] == 8 and not pl['half'][0, :, 2:].any()
    work = 2 * real.sum(axis=2) - pl['half'].sum(axis=2)
    assert sorted(work[0].tolist()) == [16, 16, 18, 18]
    # the same block for the 4x4x4 kernel: 16 tiles per group at most, lists packed (the kernel skips the MFMAs of
    # padding entries by counting the real ones)
    if 1 in KINDS:
        p4 = _capi.gram_plan(rs, cs, kind=1)
        real4 = p4['tiles'][..., 2] >= 0
        assert int(real4.sum()) == 38 and p4['nt'] <= 4 and p4['ct'] <= 8 and p4['tiles'].shape[0] >= 3
        assert np.all(np.diff(real4.astype(int), axis=2) <= 0)
    # a big block (configs[3]): every group within the kernel's limits, nearly half of the square part skipped
    rs = np.arange(1000, 1560, dtype=np.int32)
    cs = np.concatenate([[0], np.arange(2, 26), rs, [1]]).astype(np.int32)
    pl = _capi.gram_plan(rs, cs)
    real = pl['tiles'][..., 2] >= 0
    full = pl['i_tiles'] * pl['j_tiles']
    assert pl['i_tiles'] == 35 and pl['j_tiles'] == 37 and int(real.sum()) == full - 35 * 34 // 2
    assert pl['ks'] == 1 and pl['rows_per_chunk'] == 32


def test_narrow_blocks_split_the_k_steps_over_wavefronts():
    pl = _capi.gram_plan(np.arange(2, 10, dtype=np.int32), np.concatenate([[0], np.arange(2, 10), [1]]).astype(np.int32))
    assert pl['i_tiles'] == 1 and pl['j_tiles'] == 1 and pl['ks'] == 4 and pl['nt'] == 1
    assert np.all(pl['tiles'][0, :, 0, 2:] == 0)              # all four wavefronts work on the one tile


# the (nr, nc) of tests/test_fit_kernels_device.py's table that the lists above do not have
DEVICE_SHAPES = [(16, 30), (52, 120), (120, 122), (104, 300)]
KNOBS = ['FOKL_GRAM_PATH', 'FOKL_GRAM_MFMA4', 'FOKL_GRAM_DMA', 'FOKL_GRAM_HALF', 'FOKL_GRAM_BUFS', 'FOKL_GRAM_LOADERS',
         'FOKL_GRAM_RB', 'FOKL_GRAM_DEPTH', 'FOKL_GRAM_WGS']


def test_every_plan_stays_within_the_kernels_the_product_instantiates(monkeypatch):
    """The product library holds gram_tiles_kernel only as the k-split teams <NT 1, P 4, DEPTH 1, KS 2 | 4> and
    gram_tiles_dma_kernel as <NT8 1 .. 5> plain and <NT8 1 .. 4> with half-tile slots (csrc/fokl_hip.hip: ksplit_kernel,
    tiles_dma_kernel); a plan outside them is refused, not served by another instance.  The planner never makes one: every
    nr up to 80 against every nc up to 200 and the shapes of the lists above, as the search's pattern and as disjoint lists."""
    for name in KNOBS:                                    # a development build plans what its knobs say: none set
        monkeypatch.delenv(name, raising=False)
    seen = set()
    shapes = [(nr, nc) for nr in range(1, 81) for nc in range(1, 201)] + SHAPES + WIDE_SHAPES + DEVICE_SHAPES
    for nr, nc in shapes:
        rs = np.arange(2, 2 + nr, dtype=np.int32)
        model = np.arange(2 + nr, 2 + nr + max(nc - nr - 2, 0))
        search = np.concatenate([[0], model, rs, [1]])[:nc] if nc >= nr + 2 else np.concatenate([rs, [0, 1]])[:nc]
        for cs in (search.astype(np.int32), np.arange(2 + nr, 2 + nr + nc, dtype=np.int32)):
            pl = _capi.gram_plan(rs, cs)
            if pl['ks'] > 1:
                assert pl['nt'] == 1 and pl['depth'] == 1 and pl['rows_per_chunk'] == 32, (nr, nc, pl['nt'], pl['depth'])
                assert pl['ct'] <= 4, (nr, nc, pl['ks'], pl['ct'])                # P = 4 staging passes
                seen.add(('tiles', pl['ks'], int(pl['ct'])))
            else:
                half = bool(pl['half'].any())
                assert pl['depth'] == 1 and pl['rows_per_chunk'] == 32 and 1 <= pl['nt'] <= (8 if half else 10), (nr, nc, pl['nt'])
                seen.add(('dma', (pl['nt'] + 1) // 2, half))
    # and it reaches every one of them
    assert {s for s in seen if s[0] == 'dma'} == {('dma', k, h) for k in (1, 2, 3, 4, 5) for h in (False, True)} - {('dma', 5, True)}
    assert {s[1:] for s in seen if s[0] == 'tiles'} == {(4, 1), (2, 2)}       # one tile on one column tile, two tiles on two
