"""The three kernels every fit lives on -- basis build (K1), Gram block (K2), residual moments (K3) -- over the launch plans
the product runs, each against a plain numpy statement of the same operation.

* The reference is exact wherever it can be: integer columns whose every partial sum stays below 2^53 make a Gram block
  and the residual moments independent of the order of summation, so the device must return the same bits
  (``array_equal`` / ``==``).  A term lost, doubled, mirrored to the wrong place or formed in lower precision changes them.
* Where it cannot be exact (real-valued columns) the reference is ``np.longdouble`` and the bound is per element,
  proportional to sum |a_i b_i|, with the constant taken from the longest chain of roundings the launch report gives.
* Which kernel instance a launch took is READ from ``DeviceContext.gram_report`` / ``resid_report`` / ``basis_report`` and
  held against the planner (``_capi.gram_plan``) and against the table below, so a shape that silently moves to another
  instance fails here instead of leaving one untested.

Nothing here is meant to make a kernel fault: every shape is one ``engine`` can produce, every refusal returns before a launch.
"""
import os

import numpy as np
import pytest

from helpers import OracleBackend, upload, load_columns
from fokl_gpy_amd import _capi, getKernels
from oracle import fokl_oracle as O

pytestmark = pytest.mark.gpu

BERN = getKernels.bernoulli()
RS_BATCH = 256                      # columns per table load of resid_kernel (csrc/fokl_kernels.hip.h)


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------

def int_bits(n):
    """Largest b <= 20 with 9 n 2^(2 b) <= 2^53: products of two b-bit integers summed over n rows, in any order and with
    a margin of 9, stay exact in double."""
    b = 20
    while 9 * n * 4 ** b > 2 ** 53:
        b -= 1
    return b


def integer_dataset(ctx, rng, n, k):
    """Dataset of n rows with integer y and k integer columns in slots 2 .. ; -> full [n, 2 + k] indexed by slot."""
    bits = int_bits(n)
    y = rng.integers(-2 ** bits + 1, 2 ** bits, n).astype(np.float64)
    cols = rng.integers(-2 ** bits + 1, 2 ** bits, size=(n, k)).astype(np.float64)
    upload(ctx, rng.random((n, 1)), y, O.KERNEL_BERNOULLI)
    load_columns(ctx, cols)
    return np.concatenate([np.ones((n, 1)), y[:, None], cols], axis=1)


def search_lists(nr, nc, first=2):
    """The search's pattern: new columns on the row side, [ones | model | new | y] on the column side."""
    rs = np.arange(first, first + nr, dtype=np.int32)
    if nc - nr >= 2:
        others = np.arange(first + nr, first + nr + (nc - nr - 2))
        cs = np.concatenate([[0], others, rs, [1]]).astype(np.int32)
    else:
        cs = np.concatenate([rs, np.arange(first + nr, first + nc)]).astype(np.int32)
    assert cs.shape[0] == nc
    return rs, cs


def exact_block(full, rs, cs):
    """X_r' X_c of integer columns: every partial sum of the products is an integer below 2^53 (int_bits), so the double
    product is the integer result whatever the order BLAS sums in (held against int64 where that is cheap)."""
    want = full[:, rs].T @ full[:, cs]
    if full.shape[0] <= 64:
        exact = full[:, rs].astype(np.int64).T @ full[:, cs].astype(np.int64)
        assert np.array_equal(want, exact.astype(np.float64))
    return want


def planned(rs, cs):
    """What the planner says the launch of this block is: the fields the report must repeat."""
    pl = _capi.gram_plan(rs, cs)
    dma = pl['ks'] == 1
    return dict(kernel='dma' if dma else 'tiles', nt8=(pl['nt'] + 1) // 2 if dma else pl['nt'], half=bool(pl['half'].any()),
                ks=pl['ks'], ct=pl['ct'], nt=pl['nt'], groups=pl['tiles'].shape[0], row_tiles=pl['i_tiles'],
                col_tiles=pl['j_tiles'], depth=pl['depth'], rows_per_chunk=pl['rows_per_chunk'])


def check_report(ran, rs, cs, n):
    want = planned(rs, cs)
    for key, value in want.items():
        assert ran[key] == value, (key, ran, want)
    assert ran['nr_pad'] == 16 * want['row_tiles'] and ran['nc_pad'] == 16 * want['col_tiles']
    chunks = -(-n // ran['rows_per_chunk'])
    assert 1 <= ran['S'] <= chunks and ran['chunks_per_workgroup'] == -(-chunks // ran['S'])
    assert ran['slabs'] == ran['S'] * ran['ks']
    if ran['kernel'] == 'dma':
        assert ran['pieces'] == -(-ran['ct'] * 16 * 34 * 8 // 1024) and ran['lds_buffers'] == 2
        assert ran['lds_bytes'] == 2 * 1024 * ran['pieces'] <= 160 * 1024
        assert ran['loaders'] in (0, 4) and ran['lanes'] == 512 + 64 * ran['loaders']
    return ran


# (nr, nc) -> kernel, NT8 (tiles: NT), HALF, ks, ct, nt, groups, row tiles -- read from the planner for the search's
# pattern, pinned here so that the table keeps reaching every product instance <NT8 1..5, HALF off | on>, both k-split
# widths, ct = 12 .. 16, nt = 10, 8 and more groups and 7, 8, 13, 16 row tiles
GRAM_TABLE = {
    (8, 10): ('tiles', 1, False, 4, 1, 1, 1, 1),
    (16, 30): ('tiles', 1, False, 2, 2, 1, 1, 1),
    (28, 38): ('dma', 1, False, 1, 3, 2, 1, 2),
    (1, 1000): ('dma', 2, False, 1, 14, 4, 5, 1),
    (8, 1000): ('dma', 2, False, 1, 14, 4, 5, 1),
    (32, 150): ('dma', 3, False, 1, 10, 5, 1, 2),
    (48, 150): ('dma', 4, False, 1, 10, 7, 1, 3),
    (48, 586): ('dma', 5, False, 1, 15, 9, 3, 3),
    (17, 33): ('dma', 1, True, 1, 3, 1, 1, 2),
    (24, 768): ('dma', 2, True, 1, 15, 4, 4, 2),
    (52, 120): ('dma', 3, True, 1, 8, 6, 1, 4),
    (40, 180): ('dma', 4, True, 1, 12, 7, 1, 3),
    (200, 202): ('dma', 4, True, 1, 10, 8, 5, 13),
    (120, 122): ('dma', 4, True, 1, 8, 7, 2, 8),
    (104, 300): ('dma', 5, False, 1, 13, 9, 4, 7),
    (100, 586): ('dma', 5, False, 1, 15, 9, 7, 7),
    (72, 768): ('dma', 5, False, 1, 16, 10, 8, 5),
    (160, 768): ('dma', 5, False, 1, 15, 10, 13, 10),
    (256, 1000): ('dma', 5, False, 1, 15, 10, 24, 16),
}
NARROW = [s for s in GRAM_TABLE if s[1] <= 202]
WIDE = [s for s in GRAM_TABLE if s[1] > 202]
POOL = 1260                         # stored columns: 256 + 1000 disjoint ones and a few to spare
SEEN = {}                           # (kernel, nt8, half, loaders) -> a shape that ran it, over the whole module


def test_the_table_reaches_what_it_claims():
    """The table against the planner (host arithmetic: no launch) and against the list of what it must reach."""
    for (nr, nc), row in GRAM_TABLE.items():
        p = planned(*search_lists(nr, nc))
        assert (p['kernel'], p['nt8'], p['half'], p['ks'], p['ct'], p['nt'], p['groups'], p['row_tiles']) == row, (nr, nc, p)
    rows = list(GRAM_TABLE.values())
    assert {(r[1], r[2]) for r in rows if r[0] == 'dma'} == {(k, h) for k in (1, 2, 3, 4, 5) for h in (False, True)} - {(5, True)}
    assert {r[3] for r in rows} == {1, 2, 4}
    assert {12, 13, 14, 15, 16} <= {r[4] for r in rows} and max(r[5] for r in rows) == 10
    assert max(r[6] for r in rows) >= 8 and {7, 8, 13, 16} <= {r[7] for r in rows}


def run_shapes(ctx, full, shapes, n):
    for nr, nc in shapes:
        rs, cs = search_lists(nr, nc)
        got = ctx.gram(rs, cs)
        ran = check_report(ctx.gram_report(), rs, cs, n)
        assert np.array_equal(got, exact_block(full, rs, cs)), (nr, nc, n, 'search pattern')
        row = GRAM_TABLE[(nr, nc)]
        assert (ran['kernel'], ran['nt8'], ran['half'], ran['ks'], ran['ct'], ran['nt'], ran['groups'], ran['row_tiles']) == row
        SEEN.setdefault((ran['kernel'], ran['nt8'], ran['half'], ran['loaders']), (nr, nc, n))
        # a column list that shares nothing with the row side: no tile is mirrored, the internal order is rows | columns
        cd = np.arange(2 + nr, 2 + nr + nc, dtype=np.int32)
        got = ctx.gram(rs, cd)
        ran = check_report(ctx.gram_report(), rs, cd, n)
        assert ran['col_tiles'] == -(-(nr + nc) // 16)
        assert np.array_equal(got, exact_block(full, rs, cd)), (nr, nc, n, 'disjoint')
        SEEN.setdefault((ran['kernel'], ran['nt8'], ran['half'], ran['loaders']), (nr, nc, n))
        yield (nr, nc), ran


@pytest.mark.parametrize('n', [1, 33, 4099])
def test_gram_exact_over_the_table(device_ctx, n):
    rng = np.random.default_rng(n)
    full = integer_dataset(device_ctx, rng, n, POOL)
    most = dict(ct=0, nt=0, groups=0, row_tiles=0, pieces=0)
    for _, ran in run_shapes(device_ctx, full, GRAM_TABLE, n):
        for key in most:
            most[key] = max(most[key], ran[key])
    # the limits of the kernel are reached, not only approached: 16 staged tiles (68 pieces: nine per wavefront for some),
    # ten entries per list
    assert most['ct'] == 16 and most['nt'] == 10 and most['pieces'] == 68 and most['groups'] >= 24 and most['row_tiles'] == 16
    # the 8 x 8 corner of the seed Gram is a VALU launch (64 elements or fewer)
    g = device_ctx.gram([0, 1, 2], [0, 1, 2])
    assert device_ctx.gram_report()['kernel'] == 'valu'
    assert np.array_equal(g, exact_block(full, np.array([0, 1, 2]), np.array([0, 1, 2])))


def test_gram_exact_when_every_workgroup_walks_several_chunks(device_ctx):
    """Row counts at which the row cut S leaves every workgroup three chunks or more, the last round ragged (some workgroups
    have a chunk less) and the last chunk short of 32 rows: 50 021 rows for the blocks of one or two groups (S up to 768),
    12 003 for the wide ones (S up to 170)."""
    for n, shapes, pool in ((50021, NARROW, 410), (12003, WIDE, POOL)):
        rng = np.random.default_rng(n)
        full = integer_dataset(device_ctx, rng, n, pool)
        assert n % 32 != 0
        ragged = []
        for shape, ran in run_shapes(device_ctx, full, shapes, n):
            assert ran['chunks_per_workgroup'] >= 3, (shape, ran)
            ragged.append((-(-n // ran['rows_per_chunk'])) % ran['S'] != 0)
        assert sum(ragged) > len(ragged) // 2                    # the last round leaves some workgroups a chunk short


def test_gram_instances_and_loaders_seen(device_ctx):
    """Over the table (33 rows are enough: the instance does not depend on the row count) every product instance of
    gram_tiles_dma_kernel has run, and both loader variants: LW = 4 where a CU hosts as many of the 12-wavefront
    workgroups as the row cut puts on it, LW = 0 elsewhere -- which is the occupancy query's answer on the card, so the
    test says which shapes took which instead of forcing one."""
    rng = np.random.default_rng(5)
    full = integer_dataset(device_ctx, rng, 33, POOL)
    for _ in run_shapes(device_ctx, full, GRAM_TABLE, 33):
        pass
    dma = {k[1:3] for k in SEEN if k[0] == 'dma'}
    assert dma >= {(k, h) for k in (1, 2, 3, 4, 5) for h in (False, True)} - {(5, True)}, SEEN
    assert any(k[0] == 'tiles' for k in SEEN)
    loaders = {k[3] for k in SEEN if k[0] == 'dma'}
    print('gram instances seen (kernel, NT8, HALF, LW) -> first shape:', sorted(SEEN.items()))
    assert loaders == {0, 4}, SEEN


def test_gram_repeats_rows_wider_than_columns_and_the_launch_form(device_ctx):
    n = 4099
    rng = np.random.default_rng(77)
    full = integer_dataset(device_ctx, rng, n, 640)
    # a slot repeated inside row_slots and inside col_slots ("first occurrence wins" in the planner), wide block
    rs = np.concatenate([np.arange(2, 50), [7, 7, 30], np.arange(50, 95)]).astype(np.int32)
    cs = np.concatenate([[0], np.arange(100, 600), [120, 120, 0], rs, [1, 1]]).astype(np.int32)
    got = device_ctx.gram(rs, cs)
    assert device_ctx.gram_report()['kernel'] == 'dma'
    assert np.array_equal(got, exact_block(full, rs, cs))
    # slots 0 and 1 on the row side of a wide block
    rs = np.concatenate([[1, 0], np.arange(2, 70)]).astype(np.int32)
    cs = np.concatenate([np.arange(100, 640), rs]).astype(np.int32)
    got = device_ctx.gram(rs, cs)
    assert device_ctx.gram_report()['ct'] >= 12
    assert np.array_equal(got, exact_block(full, rs, cs))
    # nr > nc, with and without shared columns
    for rs, cs in ((np.arange(2, 302), np.arange(250, 290)), (np.arange(2, 202), np.arange(300, 317)),
                   (np.arange(2, 130), np.array([0, 5, 1]))):
        rs, cs = rs.astype(np.int32), cs.astype(np.int32)
        assert np.array_equal(device_ctx.gram(rs, cs), exact_block(full, rs, cs)), (rs.shape, cs.shape)
        check_report(device_ctx.gram_report(), rs, cs, n)
    # the same block through gram_launch / gram_fetch, with another block and a residual pass launched behind it
    rs, cs = search_lists(100, 586)
    want = exact_block(full, rs, cs)
    shape = device_ctx.gram_launch(rs, cs)
    ran = device_ctx.gram_report()
    assert np.array_equal(device_ctx.gram(rs[:9], cs[:40]), want[:9, :40])
    device_ctx.bic_resid([0, 2], [1.0, 2.0])
    assert np.array_equal(device_ctx.gram_fetch(shape), want)
    assert (ran['kernel'], ran['nt8'], ran['ct'], ran['groups']) == ('dma', 5, 15, 7)
    # repeatability, and both explicit paths exact on integers
    first = device_ctx.gram(rs, cs, path=2)
    assert np.array_equal(first, want) and np.array_equal(device_ctx.gram(rs, cs, path=2), first)
    valu = device_ctx.gram(rs, cs, path=1)
    ran = device_ctx.gram_report()
    assert ran['kernel'] == 'valu' and ran['groups'] == 25 * 147 and ran['nr_pad'] == 100 and ran['nc_pad'] == 588
    assert np.array_equal(valu, want) and np.array_equal(device_ctx.gram(rs, cs, path=1), valu)


def test_gram_state_carried_across_calls():
    """Slab and argument buffers grow and are reused: a wide block after a narrow one and a narrow one after a wide one on
    a context of its own.  Then a dataset with fewer rows on the context that held a longer one (the same leading
    dimension, so the columns may well land on the longer one's memory): rows past the end of a column are not seen."""
    ctx = _capi.DeviceContext(int(os.environ.get('FOKL_DEVICE', '0')))
    try:
        rng = np.random.default_rng(31)
        n_long, n_short = 4160, 4099
        full = integer_dataset(ctx, rng, n_long, 800)
        narrow, wide = search_lists(8, 10), search_lists(160, 768)
        for rs, cs in (narrow, wide, narrow, wide, search_lists(28, 38)):
            assert np.array_equal(ctx.gram(rs, cs), exact_block(full, rs, cs)), (rs.shape, cs.shape)
        sl = np.arange(2, 602, dtype=np.int32)
        ctx.bic_resid(sl, np.arange(1, 601) / 8.0)               # (grows the argument buffer between the blocks)
        full = integer_dataset(ctx, rng, n_short, 800)
        for rs, cs in (wide, narrow, search_lists(100, 586), search_lists(17, 33)):
            got = ctx.gram(rs, cs)
            assert ctx.gram_report()['chunks_per_workgroup'] >= 1 and n_short % 32 != 0
            assert np.array_equal(got, exact_block(full, rs, cs)), (rs.shape, cs.shape)
        y = full[:, 1]
        assert ctx.bic_resid([0], [0.0]) == (y.sum(), y @ y)     # K3 on the shorter dataset: the moments of y, exactly
    finally:
        ctx.close()


def test_gram_rounding_against_longdouble(device_ctx):
    """Real-valued columns of very different scales at 100 x 586 and 160 x 768.  Bound per element:
        |G_ij - sum_k a_k b_k| <= L u (1 + L u) sum_k |a_k b_k|,   u = 2^-53,   L = 32 c + s + 1
    where c = chunks the busiest workgroup walks and s = slabs the reduction sums (both from the report): an accumulator
    of the matrix pipe takes the 32 products of a chunk one after the other (at most one rounding each, as a fused
    multiply-add; 32 c along a workgroup's rows), the reduction adds at most s partial sums in a chain, and one more
    rounding allows for a product rounded on its own.  The standard bound for a sum whose every term passes through at most
    L roundings.  The longdouble reference's own error (2^-64 per operation) is four orders below u."""
    rng = np.random.default_rng(9)
    n = 4099
    y = rng.standard_normal(n)
    upload(device_ctx, rng.random((n, 1)), y, O.KERNEL_BERNOULLI)
    cols = rng.standard_normal((n, 800)) * np.exp(2.0 * rng.standard_normal(800))
    load_columns(device_ctx, cols)
    full = np.concatenate([np.ones((n, 1)), y[:, None], cols], axis=1)
    u = 2.0 ** -53
    for nr, nc in ((100, 586), (160, 768)):
        rs, cs = search_lists(nr, nc)
        got = device_ctx.gram(rs, cs)
        ran = check_report(device_ctx.gram_report(), rs, cs, n)
        L = 32 * ran['chunks_per_workgroup'] + ran['slabs'] + 1
        A, B = full[:, rs], full[:, cs]
        want = A.astype(np.longdouble).T @ B.astype(np.longdouble)
        mass = np.abs(A).T @ np.abs(B)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        assert np.all(err <= L * u * (1 + L * u) * mass), (nr, nc, L, float(np.max(err / mass)) / u)
        assert np.array_equal(got, device_ctx.gram(rs, cs))
        # the VALU path on the same block: chains of n / S rows per thread and S slabs
        got1 = device_ctx.gram(rs, cs, path=1)
        ran1 = device_ctx.gram_report()
        L1 = ran1['rows_per_chunk'] * ran1['chunks_per_workgroup'] + ran1['slabs'] + 1
        err1 = np.abs(got1.astype(np.longdouble) - want).astype(np.float64)
        assert np.all(err1 <= L1 * u * (1 + L1 * u) * mass), (nr, nc, 'valu')


# ---------------------------------------------------------------------------------------------------------
# K3 residual moments
# ---------------------------------------------------------------------------------------------------------

def exact_residual_case(ctx, rng, n, stored=8):
    """Integer y and `stored` integer columns in [-3, 3]; -> (y, cols) as int64."""
    y = rng.integers(-50, 51, n)
    cols = rng.integers(-3, 4, size=(n, stored))
    upload(ctx, rng.random((n, 1)), y.astype(np.float64), O.KERNEL_BERNOULLI)
    load_columns(ctx, cols.astype(np.float64))
    return y, cols


def exact_moments(y, cols, slots, eighths):
    """sum r and sum r^2 of r = y - sum_j (eighths_j / 8) column(slots_j), in integers: 8 r and 64 r^2 are integers, and
    so is every partial sum of theirs on the device, far below 2^53 (asserted) -- the doubles are exact whatever the order.
    A slot that appears several times contributes the sum of its coefficients (what summing its column several times gives)."""
    per_col = np.zeros(cols.shape[1] + 2, dtype=np.int64)
    np.add.at(per_col, slots, eighths)
    r8 = 8 * y - cols @ per_col[2:] - per_col[0] - per_col[1] * y
    s1, s2 = int(r8.sum()), int((r8 * r8).sum())
    assert s2 < 2 ** 53
    return s1 / 8.0, s2 / 64.0


def slot_list(rng, width, stored=8):
    """`width` slots over ones + the stored columns, each repeated many times in a shuffled order (check_slots asks only
    for slots inside the table), with coefficients that are multiples of 1/8 and differ from batch to batch."""
    slots = np.concatenate([[0], 2 + rng.integers(0, stored, width - 1)]).astype(np.int32)
    eighths = rng.integers(-8, 9, width)
    eighths[eighths == 0] = 3
    return slots, eighths


@pytest.mark.parametrize('n', [1, 511, 512, 513])
def test_resid_exact_at_every_width(device_ctx, n):
    rng = np.random.default_rng(100 + n)
    y, cols = exact_residual_case(device_ctx, rng, n)
    for width in (1, 2, 255, 256, 257, 512, 513, 586, 769):
        slots, eighths = slot_list(rng, width)
        want = exact_moments(y, cols, slots, eighths)
        got = device_ctx.bic_resid(slots, eighths / 8.0)
        ran = device_ctx.resid_report()
        assert got == want, (n, width, got, want)
        assert ran == dict(kernel='columns', columns=width, batches=-(-width // RS_BATCH), grid=-(-n // 512),
                           row_tiles=-(-n // 512), layout=(0, 0), order_class=0, inputs=0)
        # the launch / fetch form gives the same bits; a second launch without a fetch is refused and leaves 'none'
        device_ctx.bic_resid_launch(slots, eighths / 8.0)
        with pytest.raises(_capi.FoklNativeError) as e:
            device_ctx.bic_resid_launch(slots, eighths / 8.0)
        assert e.value.code == -3 and device_ctx.resid_report()['kernel'] == 'none'
        assert device_ctx.bic_resid_fetch() == want


def test_resid_exact_when_the_tile_loop_goes_round(device_ctx):
    """An odd row count above 8 x CUs x 512 rows: more row tiles than workgroups (the report says so), so the tile loop goes
    round -- narrow, and with more than 256 columns, where the column table is reloaded for every tile between two barriers."""
    rng = np.random.default_rng(8)
    n = 1048576 + 2561
    y, cols = exact_residual_case(device_ctx, rng, n)
    for width in (3, 257, 586):
        slots, eighths = slot_list(rng, width)
        want = exact_moments(y, cols, slots, eighths)
        got = device_ctx.bic_resid(slots, eighths / 8.0)
        ran = device_ctx.resid_report()
        assert ran['kernel'] == 'columns' and ran['row_tiles'] == -(-n // 512) > ran['grid'], ran
        assert ran['batches'] == -(-width // RS_BATCH)
        assert got == want, (width, got, want)
        device_ctx.bic_resid_launch(slots, eighths / 8.0)
        assert device_ctx.bic_resid_fetch() == want


def test_resid_rounding_against_longdouble(device_ctx):
    """One model of 586 real-valued columns.  With u = 2^-53, P columns and d_i = P u sum_j |beta_j x_ij| + u |r_i| (the
    fit is a chain of P fused multiply-adds, the subtraction rounds once), and L = row tiles per workgroup + 1 + 6 + 4 + slabs
    (a lane's running sum and its two rows, the wavefront's butterfly, the workgroup's four wavefronts, the slab reduction):
        |s1 - sum r_i|   <= sum_i d_i + L u sum_i |r_i|
        |s2 - sum r_i^2| <= sum_i (2 |r_i| d_i + d_i^2) + (L + 2) u sum_i r_i^2
    each times (1 + 1e-6) for the second-order terms."""
    rng = np.random.default_rng(12)
    n, P = 20001, 586
    y = rng.standard_normal(n)
    upload(device_ctx, rng.random((n, 1)), y, O.KERNEL_BERNOULLI)
    cols = rng.standard_normal((n, P - 1)) * np.exp(rng.standard_normal(P - 1))
    load_columns(device_ctx, cols)
    beta = rng.standard_normal(P) / np.sqrt(P)
    slots = np.concatenate([[0], np.arange(2, P + 1)]).astype(np.int32)
    X = np.concatenate([np.ones((n, 1)), cols], axis=1)
    s1, s2 = device_ctx.bic_resid(slots, beta)
    ran = device_ctx.resid_report()
    assert ran['batches'] == 3 and ran['columns'] == P
    r = y.astype(np.longdouble) - X.astype(np.longdouble) @ beta.astype(np.longdouble)
    u = 2.0 ** -53
    absr = np.abs(r).astype(np.float64)
    d = P * u * (np.abs(X) @ np.abs(beta)) + u * absr
    L = -(-ran['row_tiles'] // ran['grid']) + 1 + 6 + 4 + ran['grid']
    assert abs(float(np.longdouble(s1) - r.sum())) <= (d.sum() + L * u * absr.sum()) * (1 + 1e-6)
    assert abs(float(np.longdouble(s2) - (r * r).sum())) <= ((2 * absr * d + d * d).sum() + (L + 2) * u * (absr ** 2).sum()) * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------------------
# K1 basis build
# ---------------------------------------------------------------------------------------------------------

def oracle_columns(x, kid, phis, terms):
    if kid == O.KERNEL_SPLINES:
        phind, xsm = O.inputs_to_phind(x, len(phis[0][0]))
    else:
        phind, xsm = None, x
    return O.build_columns_c(xsm, phind, phis, kid, np.asarray(terms, dtype=np.int32))


def bernoulli_bound(x, terms):
    """prod over the term's inputs of sum_j |c_j| |x|^j -- the magnitude one ulp of a monomial is measured against."""
    out = np.ones((x.shape[0], len(terms)))
    for j, term in enumerate(terms):
        for k, o in enumerate(term):
            if o:
                c = np.abs(np.asarray(BERN[o - 1]))
                out[:, j] *= sum(c[p] * np.abs(x[:, k]) ** p for p in range(len(c)))
    return out


def build_and_check(ctx, x, kid, phis, terms):
    terms = np.asarray(terms, dtype=np.int32)
    T = terms.shape[0]
    ctx.reserve_slots(2 + T)
    slots = np.arange(2, 2 + T, dtype=np.int32)
    ctx.build_terms(terms, slots)
    ran = ctx.basis_report()
    got = np.stack([ctx.read_slot(int(s)) for s in slots], axis=1)          # every row of every built column
    want = oracle_columns(x, kid, phis, terms)
    assert got.shape == want.shape
    if kid == O.KERNEL_SPLINES:
        assert np.array_equal(got, want)
    else:
        assert np.all(np.abs(got - want) <= 2.0 ** -50 * bernoulli_bound(x, terms))
    return ran


def split_terms(m, wide):
    """Terms that fokl_build_terms splits into three launches: eight two-factor terms on 16 distinct factors (register
    table), one term of `wide` factors (more than 16: the LDS table, alone in its launch), ordinary terms behind it."""
    terms = np.zeros((8 + 1 + 4, m), dtype=np.int32)
    for j in range(8):
        terms[j, 2 * j], terms[j, 2 * j + 1] = 3, 3
    terms[8, :wide] = [1 + (k % 2) for k in range(wide)]
    terms[9, m - 1] = 4
    terms[10, 0], terms[10, m - 1] = 4, 2
    terms[11, 1] = 5
    terms[12, 2], terms[12, 3], terms[12, 4] = 1, 2, 4
    return terms


# (splines: the four staged slabs leave the LDS table 20 factors, so the 24-factor term is a Bernoulli case)
@pytest.mark.parametrize('kid,m,wide', [(O.KERNEL_BERNOULLI, 17, 17), (O.KERNEL_BERNOULLI, 20, 20), (O.KERNEL_BERNOULLI, 24, 24),
                                        (O.KERNEL_SPLINES, 17, 17), (O.KERNEL_SPLINES, 20, 20)])
def test_basis_lds_table_next_to_ordinary_terms(device_ctx, kid, m, wide):
    """A term of 17 and more factors takes basis_build_kernel (factor table in LDS), alone in its launch; the terms around
    it take the register-table kernel.  Lanes per workgroup follow the occupancy arithmetic of launch_basis: for Bernoulli
    (no spline slabs) 17 factors -> 64 lanes, 20 -> 256, 24 -> 128."""
    rng = np.random.default_rng(m)
    n = 3001
    x = rng.random((n, m))
    x[:3] = [[0.0] * m, [1.0] * m, [0.5] * m]
    phis = upload(device_ctx, x, np.zeros(n), kid)
    ran = build_and_check(device_ctx, x, kid, phis, split_terms(m, wide))
    assert ran['launches'] == 3 and ran['lds_table'] == 1
    assert ran['first']['kernel'] == 'reg_table' and ran['first']['factors'] == 16 and ran['first']['lanes'] == 256
    assert ran['last']['kernel'] == 'reg_table' and ran['last']['factors'] <= 16
    lds = ran['last_lds']
    assert lds['kernel'] == 'lds_table' and lds['factors'] == wide and lds['splines'] == (kid == O.KERNEL_SPLINES)
    assert lds['row_tiles'] == -(-n // (2 * lds['lanes'])) and lds['grid'] == lds['row_tiles']
    if kid == O.KERNEL_BERNOULLI:
        assert lds['lanes'] == {17: 64, 20: 256, 24: 128}[wide] and lds['slabs'] == 0
    else:
        assert lds['lanes'] in (64, 128, 256) and lds['slabs'] == 2
    # the wide term alone: one launch
    ran = build_and_check(device_ctx, x, kid, phis, split_terms(m, wide)[8:9])
    assert ran['launches'] == 1 and ran['lds_table'] == 1 and ran['first'] == ran['last'] == ran['last_lds']


@pytest.mark.parametrize('kid', [O.KERNEL_BERNOULLI, O.KERNEL_SPLINES])
def test_basis_rows_beyond_both_grid_caps(device_ctx, kid):
    """700 001 rows: above the register-table kernel's grid (5 workgroups per CU x 512 rows) and the LDS-table kernel's, so
    both grid-stride loops go round -- the report says so -- and every row of every built column is compared."""
    rng = np.random.default_rng(70)
    n, m = 700001, 17
    x = rng.random((n, m))
    phis = upload(device_ctx, x, np.zeros(n), kid)
    terms = split_terms(m, 17)[[0, 8, 10, 12]]
    ran = build_and_check(device_ctx, x, kid, phis, terms)
    assert ran['launches'] == 3 and ran['lds_table'] == 1
    for which in ('first', 'last', 'last_lds'):
        one = ran[which]
        assert one['row_tiles'] == -(-n // (2 * one['lanes'])) > one['grid'], (which, one)


def test_basis_derivative_through_the_lds_table(device_ctx):
    """build_terms_deriv of a 17-factor term (and an ordinary one) against the oracle's scalar statement, the formula
    tests/test_derivatives.py holds the host logic to."""
    rng = np.random.default_rng(3)
    n, m = 257, 17
    x = rng.random((n, m))
    upload(device_ctx, x, np.zeros(n), O.KERNEL_BERNOULLI)
    terms = np.zeros((2, m), dtype=np.int32)
    terms[0, :] = 1                                    # B1(x) = x - 1/2 sixteen times: no factor cancels ...
    terms[0, 4] = 3                                    # ... around the differentiated one
    terms[1, 4], terms[1, 9] = 3, 2
    ref = OracleBackend()
    packed, nb, width = getKernels.pack_phis(BERN, O.KERNEL_BERNOULLI)
    ref.upload(x, np.zeros(n), O.KERNEL_BERNOULLI, packed, nb, width)
    ref.reserve_slots(8)
    device_ctx.reserve_slots(8)
    for order, divisor in ((1, 2.5), (2, 6.25)):
        device_ctx.build_terms_deriv(terms, [2, 3], 4, order, divisor)
        ran = device_ctx.basis_report()
        assert ran['launches'] == 2 and ran['first']['kernel'] == 'lds_table' and ran['last']['kernel'] == 'reg_table'
        ref.build_terms_deriv(terms, [2, 3], 4, order, divisor)
        # absolute bounds, as the differentiated factor (and B2 in the second term) may cancel to nothing: its value is of
        # order one and good to a few ulps of one, the sixteen B1 factors are good to an ulp of themselves each
        others = np.prod(np.abs(np.delete(x, 4, axis=1) - 0.5), axis=1)
        tol = (1e-13 * others, 1e-13 * bernoulli_bound(x, terms)[:, 1])
        for j, s in enumerate((2, 3)):
            got, want = device_ctx.read_slot(s), ref.read_slot(s)
            assert np.all(np.abs(got - want) <= tol[j]), (order, s)
            assert np.median(np.abs(want) / tol[j]) > 1e9          # (the bound is far below the values it guards)


# ---------------------------------------------------------------------------------------------------------
# refusals: before anything is launched, and the report says so
# ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_reports_empty(device_ctx):
    rng = np.random.default_rng(0)
    n, m = 600, 40
    x = rng.random((n, m))
    upload(device_ctx, x, rng.standard_normal(n), O.KERNEL_BERNOULLI)
    device_ctx.reserve_slots(20)
    good = np.zeros((2, m), dtype=np.int32)
    good[0, 0], good[1, 1] = 1, 2

    def gram_is_none():
        ran = device_ctx.gram_report()
        return ran['kernel'] == 'none' and not any(v for k, v in ran.items() if k != 'kernel')

    def basis_is_none():
        ran = device_ctx.basis_report()
        return ran['launches'] == 0 and ran['first']['kernel'] == ran['last']['kernel'] == ran['last_lds']['kernel'] == 'none'

    device_ctx.build_terms(good, [2, 3])
    assert device_ctx.basis_report()['launches'] == 1
    device_ctx.gram([2, 3], [0, 2, 3, 1])
    assert device_ctx.gram_report()['kernel'] == 'valu'
    for rs, cs in (([], [0, 1]), ([0], []), ([0, 99999], [0]), ([0], [-1])):      # empty block, slot out of range
        with pytest.raises(_capi.FoklNativeError) as e:
            device_ctx.gram(np.array(rs, dtype=np.int32), np.array(cs, dtype=np.int32))
        assert e.value.code == -2 and gram_is_none()
        device_ctx.gram([2, 3], [0, 2, 3, 1])
        assert not gram_is_none()
    with pytest.raises(_capi.FoklNativeError):
        device_ctx.gram_launch(np.array([0, 99999], dtype=np.int32), np.array([0], dtype=np.int32))
    assert gram_is_none()
    # path 3 on a product build (development builds run their panel kernel and say so)
    try:
        device_ctx.gram([2, 3], [0, 2, 3, 1], path=3)
        assert device_ctx.gram_report()['kernel'] == 'panel'
    except _capi.FoklNativeError as exc:
        assert exc.code == -2 and 'development build' in str(exc) and gram_is_none()
    # a term with more factors than LDS holds (36 Bernoulli factors fit): refused before the terms in front of it are
    # built -- slot 2 keeps what the last good call left there
    before = device_ctx.read_slot(2)
    too_wide = np.zeros((2, m), dtype=np.int32)
    too_wide[0, 0] = 3
    too_wide[1, :37] = 1
    with pytest.raises(_capi.FoklNativeError) as e:
        device_ctx.build_terms(too_wide, [2, 4])
    assert e.value.code == -2 and 'more factors than fit in LDS' in str(e.value) and basis_is_none()
    assert np.array_equal(device_ctx.read_slot(2), before)
    fits = np.zeros((1, m), dtype=np.int32)
    fits[0, :36] = 1
    ran = build_and_check(device_ctx, x, O.KERNEL_BERNOULLI, BERN, fits)
    assert ran['launches'] == 1 and ran['first']['kernel'] == 'lds_table' and ran['first']['factors'] == 36
    for bad_terms, bad_slots in ((good, [1, 2]), (good * 30, [2, 3]), (good * 0, [2, 3]), (good, [2, 99999])):
        with pytest.raises(_capi.FoklNativeError):
            device_ctx.build_terms(bad_terms, bad_slots)
        assert basis_is_none()
    # residual passes
    device_ctx.bic_resid([0, 2], [0.5, 1.0])
    assert device_ctx.resid_report()['kernel'] == 'columns'
    with pytest.raises(_capi.FoklNativeError):
        device_ctx.bic_resid([0, 99999], [0.5, 1.0])
    assert device_ctx.resid_report()['kernel'] == 'none'
    device_ctx.bic_resid_terms_launch(good, [0.5, 1.0, -1.0])
    ran = device_ctx.resid_report()
    assert ran['kernel'] == 'matrix_free' and ran['columns'] == 2 and ran['layout'] == (8, 1) and ran['order_class'] == 2
    assert ran['inputs'] == 2 and ran['grid'] == ran['row_tiles'] == 2
    device_ctx.bic_resid_fetch()
    three_way = np.zeros((1, m), dtype=np.int32)
    three_way[0, :3] = 1
    with pytest.raises(_capi.FoklNativeError):
        device_ctx.bic_resid_terms_launch(three_way, [0.0, 1.0])
    assert device_ctx.resid_report()['kernel'] == 'none'
    fresh = _capi.DeviceContext(device_ctx.device)
    try:
        assert fresh.gram_report()['kernel'] == 'none' and fresh.resid_report()['kernel'] == 'none'
        assert fresh.basis_report()['launches'] == 0
    finally:
        fresh.close()
