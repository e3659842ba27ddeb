"""What ensemble_band_kernel (csrc/fokl_integrate_device.inc) promises about a (state, point) row of members, stated in
numpy: the bounds as numpy's order statistics and the mean in the kernel's own order of additions.  The GPU tests compare
the kernel with these bit for bit; tests/test_band_reference.py pins them without a device."""
import numpy as np

BAND_THREADS = 256


def band_rows(members, cut):
    """members [E, ...] -> (lower, upper) = np.sort(members, axis=0) at [cut] and [E - cut]: numpy's order, in which NaN
    sorts after +inf and -0.0 == 0.0.  Compare with ``same_rows``."""
    members = np.asarray(members, dtype=np.float64)
    E = members.shape[0]
    if not 1 <= cut < E:
        raise ValueError(f"bounds need 1 <= cut < members, got cut {cut} of {E}")
    srt = np.sort(members, axis=0)
    return srt[cut], srt[E - cut]


def mean_rows(members):
    """members [E, ...] -> the kernel's mean, operation for operation: partial[t] starts at 0.0 and adds members t, t + 256,
    ... in ascending order; partial[t] += partial[t + half] for half = 128 ... 1; partial[0] / E.  Additions only (the
    kernel is compiled without contraction), so float64 numpy reproduces every rounding."""
    members = np.asarray(members, dtype=np.float64)
    E = members.shape[0]
    partial = np.zeros((BAND_THREADS,) + members.shape[1:])
    with np.errstate(invalid='ignore', over='ignore'):
        for first in range(0, E, BAND_THREADS):
            block = members[first:first + BAND_THREADS]
            partial[:block.shape[0]] = partial[:block.shape[0]] + block
        half = BAND_THREADS // 2
        while half:
            partial[:half] = partial[:half] + partial[half:2 * half]
            half //= 2
        return partial[0] / float(E)


def same_rows(a, b):
    """Bit-equal up to what numpy's order cannot tell apart: NaN equals NaN, -0.0 equals 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def band_next_to_nan(members, mean, bounds, nan_members, cut):
    """What a band next to members that turn NaN looks like (fewer than E - cut of them), per (state, point) row with n NaN
    among its members: the mean is NaN from n = 1, the upper bound is the largest finite value at n = cut - 1 and NaN from
    n = cut, the lower bound stays finite.  Asserts it of members [E, K, P], mean [K, P], bounds [K, P, 2]."""
    n = np.isnan(members).sum(axis=0)
    assert n.max() == len(nan_members) and n[:, 0].max() == 0
    assert np.isfinite(np.delete(members, list(nan_members), axis=0)).all()
    assert np.array_equal(np.isnan(mean), n >= 1) and np.isfinite(bounds[..., 0]).all()
    assert np.array_equal(np.isnan(bounds[..., 1]), n >= cut)
    largest = np.sort(members, axis=0)[members.shape[0] - 1 - n, np.arange(n.shape[0])[:, None], np.arange(n.shape[1])]
    assert np.array_equal(bounds[..., 1][n == cut - 1], largest[n == cut - 1])


FINITE_ROWS = ('permutation', 'ties', 'sorted', 'reversed', 'signed_zeros')
EDGE_ROWS = ('plus_inf', 'minus_inf', 'both_inf', 'nan_first', 'nan_last', 'nan_middle', 'nan_cut_minus_1', 'nan_cut',
             'nan_cut_plus_1', 'nan_all_but_cut', 'all_nan', 'mixed')


def designed_row(kind, E, cut, rng):
    """One row of E members designed for the band: distinct integers (every sum exact, every misplaced element shows) in
    an order or with the special values that ``kind`` names.  nan_cut_minus_1 / nan_cut / nan_cut_plus_1 hold that many NaN
    at random places, so that sorted[E - cut] is the largest finite value, then the first NaN, then a NaN; nan_all_but_cut
    leaves ``cut`` finite values, so that sorted[cut] is the first NaN."""
    row = rng.permutation(E).astype(np.float64) - float(E // 3)

    def put(value, count):
        row[rng.choice(E, size=min(max(count, 0), E), replace=False)] = value

    if kind == 'permutation':
        pass
    elif kind == 'ties':
        row = rng.choice(np.array([-3.0, -1.0, -0.0, 0.0, 0.5, 2.0, 7.0]), size=E)
    elif kind == 'sorted':
        row = np.sort(row)
    elif kind == 'reversed':
        row = np.sort(row)[::-1].copy()
    elif kind == 'signed_zeros':
        row = np.where(rng.random(E) < 0.5, -0.0, 0.0)
        row[rng.integers(E)] = -1.0
    elif kind == 'plus_inf':
        put(np.inf, 1 + E // 5)
    elif kind == 'minus_inf':
        put(-np.inf, 1 + E // 5)
    elif kind == 'both_inf':
        put(np.inf, 1 + E // 7)
        put(-np.inf, 1 + E // 7)
    elif kind == 'nan_first':
        row[0] = np.nan
    elif kind == 'nan_last':
        row[E - 1] = np.nan
    elif kind == 'nan_middle':
        row[E // 2] = np.nan
    elif kind == 'nan_cut_minus_1':
        put(np.nan, cut - 1)
    elif kind == 'nan_cut':
        put(np.nan, cut)
    elif kind == 'nan_cut_plus_1':
        put(np.nan, cut + 1)
    elif kind == 'nan_all_but_cut':
        put(np.nan, E - cut)
    elif kind == 'all_nan':
        row[:] = np.nan
    elif kind == 'mixed':
        row = rng.choice(np.array([-np.inf, -2.0, -0.0, 0.0, 1.0, 1.0, 3.0, np.inf, np.nan]), size=E)
        row[rng.integers(E)] = np.nan
    else:
        raise ValueError(kind)
    return row


def bitonic_rows(members, cut, count_nan=True):
    """The kernel's sort restated step for step for one row: the bitonic network over the next power of two (>= 2), padded
    with +inf, a exchanging with b on ``(a > b) == ascending``.  ``count_nan``: a NaN enters the list as +inf and is
    counted, and sorted[k] is NaN from k = E - count on -- the kernel as it is.  Without: the NaN enters the list itself,
    where ``>`` is no order, and the row comes out unsorted -- the kernel as it was, kept to show what the count is for."""
    row = np.asarray(members, dtype=np.float64).reshape(-1)
    E = row.shape[0]
    n = 2
    while n < E:
        n *= 2
    lds = np.full(n, np.inf)
    lds[:E] = row
    first_nan = E
    if count_nan:
        first_nan = E - int(np.isnan(row).sum())
        lds[np.isnan(lds)] = np.inf
    i = np.arange(n // 2)
    size = 2
    while size <= n:
        stride = size // 2
        while stride:
            a = 2 * i - (i & (stride - 1))
            b = a + stride
            up = (a & size) == 0
            va, vb = lds[a], lds[b]
            with np.errstate(invalid='ignore'):
                swap = (va > vb) == up
            lds[a], lds[b] = np.where(swap, vb, va), np.where(swap, va, vb)
            stride //= 2
        size *= 2
    return tuple(lds[k] if k < first_nan else np.nan for k in (cut, E - cut))
