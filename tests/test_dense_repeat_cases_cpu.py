"""The cohort helper of tests/test_gpu_dense_repeats.py (tests/dense_repeat_cases.py) without a GPU: the marked columns are
a clear factor under COLLINEAR_TAU and all others a factor 10 above it, and ``repeat_runs`` -- the documented rule of the
collapsed scan's dense repeats (csrc/scan.hip: scan_core) -- at its edges."""
import numpy as np
import pytest

import dense_repeat_cases as drc


@pytest.mark.parametrize("name", sorted(drc.LAYOUTS))
def test_share_margins(name):
    lay = drc.layout(name)
    p, marked, first, count = drc.LAYOUTS[name]
    assert lay.G.shape == (203, p) and lay.Gd.shape == (9, p) and first + count <= p
    assert np.array_equal(lay.G, lay.Gd[lay.donor])                       # donor-constant, exactly
    assert sorted(np.bincount(lay.donor)) == sorted(drc.CELLS) and np.any(np.diff(lay.donor) < 0)     # shuffled
    s = drc.check_margins(lay)
    # (independently of the helper's own assertions: the projection by QR instead of lstsq)
    Qw, _ = np.linalg.qr(lay.W)
    R = lay.G - Qw @ (Qw.T @ lay.G)
    s2 = np.sum(R * R, 0) / np.sum(lay.G * lay.G, 0)
    assert np.allclose(s, s2, rtol=1e-8, atol=0)
    is_marked = np.isin(np.arange(p), marked)
    assert s[is_marked].max() < 0.7 * drc.TAU and s[~is_marked].min() >= 10 * drc.TAU
    if name == "dosages":
        assert lay.dosage.dtype == np.int8 and lay.W.shape[1] == 1 and len(marked) >= 3
        assert np.all(np.abs(s[is_marked] - 4.877 / 797) < 1e-5)          # g = 2 on 198 cells, 1 on 5: 0.6 %
        assert all(p // 4 <= j < 3 * p // 4 for j in marked)              # mid-panel
    else:
        assert np.allclose(s[is_marked], drc.MARKED_SHARE, rtol=1e-6, atol=0)
        assert lay.W.shape[1] == 3 and np.all(lay.W[:, 0] == 1.0)
        for d in range(9):                                               # w is donor-level, z is not
            assert np.ptp(lay.W[lay.donor == d, 1]) == 0.0 and np.ptp(lay.W[lay.donor == d, 2]) > 0.0
        # every marked column has its own coefficients on [1, w]
        coef = np.linalg.lstsq(lay.W, lay.G[:, list(marked)], rcond=None)[0][:2]
        assert np.unique(np.round(coef, 6), axis=1).shape[1] == len(marked)


def test_the_layouts_give_the_runs_they_are_named_for():
    assert drc.layout("scattered").runs == [(3, 32), (67, 1), (127, 2), (299, 1)]
    win = drc.layout("window")
    assert win.in_range == (1, 132) and win.runs == [(1, 1), (132, 1)] and all(off > 0 for off, _ in win.runs)
    assert drc.layout("quarter").runs == [(0, 40)] and len(drc.layout("quarter").marked) == 11
    assert drc.layout("dosages").runs == [(9, 6)]
    # "window" holds the columns of "scattered" wherever neither is marked
    free = np.setdiff1d(np.arange(300), win.marked)
    assert np.array_equal(win.Gd[:, free], drc.layout("scattered").Gd[:, free])


def test_repeat_runs_at_the_edges():
    assert drc.repeat_runs([], 10) == []
    assert drc.repeat_runs([], 0) == []
    assert drc.repeat_runs([5], 100) == [(5, 1)]
    assert drc.repeat_runs([0], 1) == [(0, 1)]                            # (1 of 1: more than a quarter, the same run)
    # gap 32 merges, gap 33 does not
    assert drc.repeat_runs([10, 42], 400) == [(10, 33)]
    assert drc.repeat_runs([10, 43], 400) == [(10, 1), (43, 1)]
    # a chain of merges: each neighbour within 32 of the one before
    assert drc.repeat_runs([0, 32, 64, 97], 400) == [(0, 65), (97, 1)]
    # exactly a quarter keeps the runs, one more scans everything
    quarter = list(range(0, 40, 4))
    assert len(quarter) * 4 == 40 and drc.repeat_runs(quarter, 40) == [(0, 37)]
    assert drc.repeat_runs(quarter + [39], 40) == [(0, 40)]
    assert drc.repeat_runs([150, 0, 100, 50, 199], 200) == [(0, 1), (50, 1), (100, 1), (150, 1), (199, 1)]   # (unsorted input)
    assert drc.repeat_runs([0, 1, 2], 12) == [(0, 3)] and drc.repeat_runs([0, 1, 2, 11], 12) == [(0, 12)]
    # marks at 0 and count - 1
    assert drc.repeat_runs([0, 99], 100) == [(0, 1), (99, 1)]
    assert drc.repeat_runs([0, 33], 34) == [(0, 1), (33, 1)]
    assert drc.repeat_runs([0, 32], 33) == [(0, 33)]
    with pytest.raises(AssertionError):
        drc.repeat_runs([100], 100)
