"""The yardsticks that tests/test_gpu_davies_widths.py holds csrc/davies.hip to, proved on the CPU first, over the table
of tests/davies_cases.py (2 to 256 weights):

(a) the float64 and the long-double build of oracle/qfc.c take the same path;
(b) the long-double value is within AS 155's own acc = 1e-6 of the exact tail probability, and of Imhof's integral in
    mpmath at 30 digits -- which is what pins the Davies branch of the oracle;
(c) the limit per case, 32 x what the float64 oracle achieves and not below a floor derived for the device's form
    (davies_reference.davies_limit), is never set by its ceiling, and a float64 restatement of the device's form
    (tests/davies_device_form.py) stays inside it;
(d) seven imitated slips of that form fall outside it, two of which the tolerance the suite had before lets through;
(e) Liu's value: scipy's against mpmath at 40 digits, 32 x its error within the 1e-8 the suite had before.
"""
import numpy as np
import pytest

import davies_cases as dc
import davies_device_form as form
import davies_reference as dr

SET_ASIDE_CAP = 0.02
OLD_RTOL, OLD_ATOL = 1e-5, 1e-13       # tests/test_gpu_kernels.py: test_davies_matches_oracle


def _held():
    return [r for r in dr.refs() if r.same_path and r.davies_held]


def test_both_builds_take_the_same_path():
    refs = dr.refs()
    aside = [r.case.name for r in refs if not r.same_path]
    print("set aside: %d of %d cases" % (len(aside), len(refs)), aside)
    assert len(aside) <= SET_ASIDE_CAP * len(refs)


def test_the_table_reaches_every_exit_at_every_kind_of_width():
    refs = dr.refs()
    exits = {}
    for r in refs:
        exits.setdefault(r.exit, set()).add(r.r)
    print({k: sorted(v) for k, v in exits.items()})
    assert set(exits) == {"converged", "ifault 1", "early cdf 1 or 0", "single survivor"}
    for r in dc.WIDTHS:
        assert r in exits["converged"] and r in exits["early cdf 1 or 0"], r
    # the auxiliary integration, past one and two trips of the lane-strided loops too
    two = {r.r for r in refs if r.trace[2] == 2 and r.ifault == 0}
    assert set(dc.AUX_WIDTHS) <= two, two
    # both early exits, and a filter row at each width that keeps fewer weights than it was given
    early = {(r.p64 >= 1.0) for r in refs if r.exit == "early cdf 1 or 0"}
    assert early == {True, False}
    assert all(r.r < r.case.k for r in refs if r.case.kind == "filter")


def test_long_double_value_is_within_acc_of_the_exact_tail_probability():
    import tail_pvalue_prototype as tp       # (tests/test_tail_pvalue_cpu.py holds it to recorded truths)

    worst = 0.0
    for r in _held():
        p, _, status = tp.tail_pvalue(r.case.q, r.lam)
        assert status == tp.CONVERGED, r.case.name
        worst = max(worst, abs(r.p_ld - p))
        assert abs(r.p_ld - p) <= form.ACC, (r.case.name, r.p_ld, p)
    print("largest |p_LD - exact| = %.3g over %d cases" % (worst, len(_held())))


@pytest.mark.parametrize("r", dc.WIDTHS)
def test_long_double_value_against_imhofs_integral_at_30_digits(r):
    ref = next(x for x in dr.refs() if x.case.name == "gamma-r%d-q2" % r)
    assert ref.davies_held and ref.trace[2] >= 1
    exact = dr.tail_contour_mp(ref.lam, ref.case.q)
    print("r = %d: p_LD - integral = %.3g" % (r, ref.p_ld - float(exact)))
    assert abs(ref.p_ld - float(exact)) <= form.ACC
    if r == 2:      # the moved path gives what Imhof's own form on the real axis gives
        assert abs(dr.imhof_real_axis_mp(ref.lam, ref.case.q) - exact) < 1e-25


def test_the_ceiling_never_sets_a_limit():
    worst = max(32.0 * abs(r.p64 - r.p_ld) for r in _held())
    print("largest 32 |p64 - p_LD| = %.3g" % worst)
    assert worst < dr.CEILING


def test_the_device_form_takes_the_oracles_path_and_stays_inside_the_limit():
    worst = (0.0, None)
    for r in dr.refs():
        if not r.same_path or r.r < 2:
            continue
        cdf, ifault, trace = form.qfc(r.lam, r.case.q)
        assert (ifault, trace) == (r.ifault, r.trace), (r.case.name, ifault, trace, r.ifault, r.trace)
        if r.davies_held:
            share = abs((1.0 - cdf) - r.p_ld) / r.limit
            worst = max(worst, (share, r.case.name))
            assert share <= 1.0, (r.case.name, 1.0 - cdf, r.p_ld, r.limit)
    print("largest share of the limit: %.3g (%s)" % worst)


def _slip_subset():
    return [r for r in _held() if r.trace[2] >= 1 and (r.case.kind == "aux" or r.case.name.startswith(("gamma-", "dominant-")))]


_SLIP_REPORT = {}


def slip_report(slip):
    """(cases the slip changed, caught by the limit and the path, let through by the tolerance the suite had before)."""
    if slip not in _SLIP_REPORT:
        applied = caught = old_passes = 0
        missed, widths = [], {}
        for r in _slip_subset():
            cdf, ifault, trace, did = form.qfc(r.lam, r.case.q, slip)
            if not did:
                continue
            p = 1.0 - cdf
            applied += 1
            new = ifault != r.ifault or trace != r.trace or not abs(p - r.p_ld) <= r.limit
            old = ifault != r.ifault or not abs(p - r.p64) <= OLD_RTOL * r.p64 + OLD_ATOL
            caught += new
            old_passes += not old
            widths[r.r] = widths.get(r.r, False) or bool(new)
            if not new:
                missed.append(r.case.name)
        _SLIP_REPORT[slip] = (applied, caught, old_passes, missed, widths)
    return _SLIP_REPORT[slip]


# slips that the tolerance of test_davies_matches_oracle lets through on most problems (all of them at some widths)
PASSED_BEFORE = ("tail_skip64", "last_abscissa")


@pytest.mark.parametrize("slip", form.SLIPS)
def test_an_imitated_slip_falls_outside_the_limit(slip):
    applied, caught, old_passes, missed, widths = slip_report(slip)
    print("%s: changed %d problems, %d outside the limit or off the path, %d inside 1e-5 p + 1e-13; missed: %s"
          % (slip, applied, caught, old_passes, missed))
    assert applied >= 20
    # wherever the weights are of one size (the gamma rows) the slip is caught on every problem it changes, and at every
    # width on some problem.  (Where weight 64 is one of many of 3e-4 under a few of order one, leaving it out of
    # tail_bound moves the step of the trapezoid rule and nothing else: both steps integrate to the same value.)
    assert not [m for m in missed if m.startswith("gamma-")], missed
    assert all(widths.values()), widths
    assert {"tail_skip64": set(range(65, 257))}.get(slip, set(dc.WIDTHS)) >= set(widths)
    if slip in PASSED_BEFORE:
        assert old_passes > applied // 2


def test_liu_yardstick_is_within_the_tolerance_the_suite_had():
    table = dr.liu_refs()
    worst = max(table.values(), key=lambda v: v[1])
    print("largest Liu limit %.3g (scipy off by %.3g) over %d cases" % (worst[1], worst[2], len(table)))
    for name, (want, limit, err) in table.items():
        assert limit <= dr.LIU_PRESENT, (name, float(want), err)
    # the table reaches below the double range, where both values must be 0
    assert any(float(v[0]) == 0.0 for v in table.values()) and any(0.0 < float(v[0]) < 1e-250 for v in table.values())
