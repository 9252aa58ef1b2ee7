"""``_engine._walk_runs`` (the walk of ``scan_association_many`` and the context-many drivers over a panel, whole or along the
runs of ``cis_index``) with a stand-in for the device call: ``progress=True`` is ONE bar over the whole pass, advanced
through the callable every call is handed; results are scattered and gathered by ``cis_index``."""
import sys
import types

import numpy as np
import pytest

from cellregmap_amd import _engine

KEYS = (("pv", False, float), ("beta", True, float), ("status", True, np.int32))
K = 2


class _Bar:
    made = []

    def __init__(self, total=None):
        self.total, self.n, self.closed = total, 0, False
        _Bar.made.append(self)

    def update(self, by):
        self.n += by

    def close(self):
        self.closed = True


@pytest.fixture
def bars(monkeypatch):
    _Bar.made = []
    monkeypatch.setitem(sys.modules, "tqdm", types.SimpleNamespace(tqdm=_Bar))
    return _Bar.made


def _value(i, j):
    return 100.0 * i + j


def _scan(calls):
    """What a driver's ``scan`` does, without a device: fill the outputs, report as ``_progress`` reports."""
    def scan(idx, a, count, out, offset, total, progress):
        calls.append((list(idx), a, count, offset, total, progress))
        for row, i in enumerate(idx):
            for j in range(count):
                out["pv"][row, j] = _value(i, a + j)
                out["beta"][row, j, :] = _value(i, a + j) + np.arange(K) / 10
                out["status"][row, j, :] = i
        if callable(progress):
            progress(offset + count, total)
    return scan


CIS = [(0, 10), (2, 5), np.array([7, 3, 3]), (0, 0)]     # a whole panel, a stretch inside it, indices out of order, nothing


def test_one_bar_over_a_cis_walk(bars):
    calls = []
    out = _engine._walk_runs(KEYS, 4, 10, K, CIS, True, _scan(calls))
    assert len(bars) == 1 and bars[0].total == 10 and bars[0].n == 10 and bars[0].closed
    assert len(calls) > 1 and all(callable(c[5]) for c in calls)          # every call gets the bar's callable, never ``True``
    assert [c[3] for c in calls] == list(np.cumsum([0] + [c[2] for c in calls])[:-1]) and all(c[4] == 10 for c in calls)
    assert any(c[0] != [0, 1, 2] and 0 in c[0] for c in calls)            # runs hold strict subsets of the phenotypes
    columns = [np.arange(0, 10), np.arange(2, 5), np.array([7, 3, 3]), np.arange(0)]
    for i, cols in enumerate(columns):
        assert np.array_equal(out["pv"][i], [_value(i, j) for j in cols])
        assert out["beta"][i].shape == (cols.size, K) and out["status"][i].dtype == np.int32
        assert np.array_equal(out["beta"][i][:, 1], [_value(i, j) + 0.1 for j in cols])
        assert np.all(out["status"][i] == i)


def test_one_bar_over_a_whole_panel(bars):
    calls = []
    out = _engine._walk_runs(KEYS, 3, 6, K, None, True, _scan(calls))
    assert len(bars) == 1 and bars[0].total == 6 and bars[0].n == 6 and bars[0].closed
    assert len(calls) == 1 and callable(calls[0][5]) and calls[0][:5] == ([0, 1, 2], 0, 6, 0, 6)
    assert out["pv"].shape == (3, 6) and out["beta"].shape == (3, 6, K) and out["pv"][2, 5] == _value(2, 5)


def test_the_bar_is_closed_when_a_call_fails(bars):
    def scan(*args):
        raise RuntimeError("device call failed")

    with pytest.raises(RuntimeError):
        _engine._walk_runs(KEYS, 4, 10, K, CIS, True, scan)
    assert len(bars) == 1 and bars[0].closed


def test_silent_and_callable_progress_pass_through(bars):
    calls, seen = [], []
    _engine._walk_runs(KEYS, 4, 10, K, CIS, False, _scan(calls))
    assert not bars and all(c[5] is False for c in calls)
    report = lambda done, total: seen.append((done, total))
    _engine._walk_runs(KEYS, 4, 10, K, CIS, report, _scan([]))
    assert not bars and seen[-1] == (10, 10) and [d for d, _ in seen] == sorted(d for d, _ in seen)


def test_no_variants(bars):
    out = _engine._walk_runs(KEYS, 2, 0, K, None, False, _scan([]))
    assert out["pv"].shape == (2, 0) and out["status"].shape == (2, 0, K)
