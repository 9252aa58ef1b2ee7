"""The two-stage family solver (eigh2_band.hip, eigh2_chase.hip, eigh2_back.hip) at the residues of its edge logic,
through ``crm_test_eigh2``.  In production the order is 64 + (non-context columns), any integer from 1024 up, so every
residue mod 64 occurs; what depends on it:

    npanels = (dim - 2 - 64) / 64 + 1, the last panel with one row (no reflector), two (one reflector) or three;
    nwg = ceil(m / 256), nch = ceil(m / 128) of a panel of m rows;  chain positions = ceil((n - 1) / 64);
    nblocks = ceil((dim - 1) / 128) of the back-transformation;  dimp = round_up(dim, 128).

  * stage 1 against the numpy statement (tools/eigh2_prototype.py: stage1), entry by entry, exact zeros below the band;
  * the chase against the prototype's, and the spectrum of its T(d, e) against the long-double reference of the scaled
    matrix under the bound of tests/eigh_reference.py;
  * the family solver end to end under that bound, also with the constructor's grid (ten points: about 25 workgroups of
    the chase per matrix) -- every grid point against its own scaled matrix;
  * orders 1025 and 1026 (the production range, dimp 1152, last panel with one and two rows) against LAPACK with the
    tolerances of test_gpu_eigh2.py::test_family_solver_against_lapack.

A chase (or panel QR) that gave up after its bounded wait (a shared device) answers CRM_ERR_UNSUPPORTED with a message that
says its workgroups "were not co-resident": the test skips, nothing retries.  Any other CRM_ERR_UNSUPPORTED is a failure.
"""
import numpy as np
import pytest

import eigh_reference as er
from cellregmap_amd import _lib
from test_gpu_eigh2 import _call, _family, proto

pytestmark = pytest.mark.gpu

CRM_ERR_UNSUPPORTED = -3


def _solve(C, rho, stage):
    rho = np.asarray(rho, float)
    try:
        return _call(C, np.sqrt(rho), np.sqrt(1 - rho), stage)
    except _lib.CrmError as err:
        if f"error {CRM_ERR_UNSUPPORTED}:" in str(err) and "were not co-resident" in str(err):
            pytest.skip(str(err))
        raise


def _scaled(C, rho):
    dsc = er.family_scaling(C.shape[0], rho)
    return C * np.outer(dsc, dsc), dsc


# (dim, k1): k1 contexts in the leading block of 64, the 64 - k1 coordinates in front of them zero rows.  With k1 < 64
# column 0 of C is zero, and at order 66 entry (65, 0) is the only one below the band: both k1 wherever that matters.
BAND_CASES = [(dim, k1) for dim in (65, 66, 67, 129, 130, 193, 194, 257, 258, 320, 321) for k1 in (10, 64)]
CHASE_CASES = [(3, 64), (64, 10), (64, 64), (65, 10), (65, 64), (66, 10), (66, 64), (129, 64), (130, 10), (193, 64), (257, 10)]
FAMILY_CASES = [(65, 10), (65, 64), (66, 10), (66, 64), (130, 10), (194, 64), (257, 64), (258, 10)]


@pytest.mark.parametrize("dim,k1", BAND_CASES)
def test_dense_to_band_at_the_panel_edges(dim, k1):
    C = _family(dim, k1, seed=dim)
    _, _, _, _, band = _solve(C, [0.5], 1)
    ref, blocks = proto.stage1(C, 64, 64)
    low = np.tril(band)
    below = np.abs(np.tril(low, -65)).max()
    err = np.abs(low - np.tril(ref)).max()
    print(f"[eigh2-band] dim={dim:<4d} k1={k1:<2d} panels {len(blocks)}  max below the band {below:.2e}  "
          f"max |band - prototype| {err:.2e}  limit {1e-11 * np.abs(ref).max():.2e}")
    assert below == 0.0
    assert err <= 1e-11 * np.abs(ref).max()


@pytest.mark.parametrize("dim,k1", CHASE_CASES)
def test_chase_at_the_chain_edges(dim, k1):
    C = _family(dim, k1, seed=dim + 1)
    rho = [0.0, 0.4, 0.9]
    _, _, d, e, _ = _solve(C, rho, 2)
    band, _ = proto.stage1(C, 64, 64)
    bad = []
    for q, r in enumerate(rho):
        A, dsc = _scaled(C, r)
        dr, er_, _ = proto.chase(band * np.outer(dsc, dsc), 64)
        scale = np.abs(dr).max()
        ed, ee = np.abs(d[q] - dr).max(), np.abs(e[q, : dim - 1] - er_).max()
        print(f"[eigh2-chase] dim={dim:<4d} k1={k1:<2d} rho={r:<4g} max |d - prototype| {ed:.2e}  max |e - prototype| {ee:.2e}  "
              f"limit {1e-10 * scale:.2e}")
        if not (ed <= 1e-10 * scale and ee <= 1e-10 * scale):
            bad.append(f"dim {dim} k1 {k1} rho {r}: d, e off the prototype by {ed:.3e}, {ee:.3e} > {1e-10 * scale:.3e}")
        # whatever the conventions: the tridiagonal has the spectrum of the scaled matrix (its own spectrum by bisection
        # in long double, so that the chase's error is all there is to see)
        bad += er.hold_spectrum(f"chase dim={dim} k1={k1} rho={r:g}", er.tridiagonal_eigenvalues(d[q], e[q]), A)
    assert not bad, "\n".join(bad)


def _hold_family(C, rho, label):
    lam, Z, _, _, _ = _solve(C, rho, 0)
    bad = []
    for q, r in enumerate(rho):
        A, _ = _scaled(C, r)
        if not np.all(np.diff(lam[q]) >= 0):
            bad.append(f"{label} rho {r}: lam not ascending")
        bad += er.hold(f"{label} rho={r:g}", A, lam[q], Z[q])
    return bad


@pytest.mark.parametrize("dim,k1", FAMILY_CASES)
def test_family_solver_at_the_edges(dim, k1):
    C = _family(dim, k1, seed=dim + 2)
    bad = _hold_family(C, [0.0, 0.1, 0.5, 0.9], f"family dim={dim} k1={k1}")
    assert not bad, "\n".join(bad)


def test_family_solver_on_the_constructors_grid():
    """Ten grid points (the eleven-point grid without rho = 1, which the constructor never sends to the two-stage form):
    the chase runs about 25 workgroups per matrix, not 64."""
    C = _family(194, 10, seed=7)
    bad = _hold_family(C, list(np.linspace(0.0, 1.0, 11)[:10]), "family grid dim=194")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dim,k1", [(1025, 64), (1026, 10)])
def test_family_solver_in_the_production_range(dim, k1):
    C = _family(dim, k1, seed=dim + 2)
    rho = [0.1, 0.9]
    lam, Z, _, _, _ = _solve(C, rho, 0)
    for q, r in enumerate(rho):
        A, _ = _scaled(C, r)
        ref = np.linalg.eigvalsh(A)
        scale = np.abs(ref).max()
        got = (np.abs(lam[q] - ref).max() / scale, np.abs(Z[q].T @ Z[q] - np.eye(dim)).max(),
               np.abs(A @ Z[q] - Z[q] * lam[q]).max() / scale)
        print(f"[eigh2-family] dim={dim} rho={r:g} against LAPACK: eig {got[0]:.2e} (2e-13)  orth {got[1]:.2e} (5e-12)  "
              f"resid {got[2]:.2e} (1e-12)")
        assert got[0] <= 2e-13
        assert got[1] <= 5e-12
        assert got[2] <= 1e-12
