"""The long-double eigenvalue reference and the bound of tests/eigh_reference.py, checked on the CPU:

  * against something else: the closed form of the 1-2-1 Toeplitz spectrum, 2 - 2 cos(k pi / (n + 1)), from mpmath at
    n = 300, and ``mpmath.eigsy`` at 40 digits on a dense matrix of order 24; the tridiagonaliser keeps the spectrum;
  * nothing excluded: LAPACK alone stays inside the bound on every case the GPU tests build (true by construction -- the
    assertion is there so that a later edit of the bound cannot silently exclude the reference solver);
  * the cases are what they are named: the library's own deflation plan (eigh_dc.hip: plan_merge through the host-only
    hook crm_test_dc_plan) of each structure's top merge leaves k = 2, 1, 0 poles for (a), (b), (c), rotates every twin
    pair of (d) into one pole (rotations == k) and deflates nothing of (g);
  * teeth: an eigenvalue moved by 1e-12 of the scale, two eigenvector columns swapped, one column rotated by 1e-11
    towards its neighbour -- each must break the bound on at least one of the three measures.
"""
import numpy as np
import pytest

import eigh_reference as er

LD = np.longdouble


def _mp_to_ld(x):
    import mpmath as mp

    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def test_toeplitz_closed_form():
    import mpmath as mp

    mp.mp.dps = 40
    n = 300
    ref = er.tridiagonal_eigenvalues(np.full(n, 2.0), np.full(n - 1, -1.0))
    exact = np.array([_mp_to_ld(2 - 2 * mp.cos(k * mp.pi / (n + 1))) for k in range(1, n + 1)], dtype=LD)
    err = float(np.abs(ref - exact).max())
    print(f"Toeplitz n = {n}: max error {err:.2e}")
    assert err <= 2e-18          # (a few units of the long double's 1.1e-19 at a scale of 4)


def test_dense_against_mpmath():
    import mpmath as mp

    mp.mp.dps = 40
    rng = np.random.default_rng(24)
    X = rng.normal(size=(24, 24))
    A = X + X.T
    E = mp.eigsy(mp.matrix(A.tolist()), eigvals_only=True)
    exact = np.sort(np.array([_mp_to_ld(v) for v in E], dtype=LD))
    ref = er.reference_eigenvalues(A)
    err = float(np.abs(ref - exact).max())
    print(f"dense n = 24: max error against mpmath.eigsy {err:.2e}")
    assert err <= 24 * 1.1e-19 * float(np.abs(exact).max())


def test_the_tridiagonaliser_keeps_the_spectrum():
    import mpmath as mp

    mp.mp.dps = 40
    rng = np.random.default_rng(7)
    X = rng.normal(size=(30, 30))
    A = X + X.T
    d, e = er.tridiagonalise(A)
    T = er.tridiag(d.astype(float), e.astype(float))      # structure only: the long-double entries go to the bisection
    assert er.is_tridiagonal(T) and not er.is_tridiagonal(A)
    exact = np.sort(np.array([_mp_to_ld(v) for v in mp.eigsy(mp.matrix(A.tolist()), eigvals_only=True)], dtype=LD))
    got = er.tridiagonal_eigenvalues(d, e)
    assert float(np.abs(got - exact).max()) <= 30 * 1.1e-19 * float(np.abs(exact).max())
    # ... and a matrix that is tridiagonal already comes back as it went in
    d0, e0 = er.dc_structure("i", 40)
    d1, e1 = er.tridiagonalise(er.tridiag(d0, e0))
    assert np.array_equal(d1.astype(float), d0) and np.array_equal(np.abs(e1.astype(float)), np.abs(e0[:39]))


def test_squares_that_underflow_in_double_count():
    """Couplings of 1e-200: the reference must not lose them where they decide the order of two equal diagonal entries
    (nothing to lose here beyond 1e-200, but the Sturm count must stay finite and monotone)."""
    d, e = er.dc_structure("h", 33)
    ref = er.tridiagonal_eigenvalues(d, e)
    assert np.all(np.isfinite(ref)) and np.all(np.diff(ref) >= 0)
    assert float(np.abs(ref - np.sort(d)).max()) <= 1e-18


def _all_cases():
    for n in er.DC_ORDERS:
        for kind, T in er.dc_cases(n).items():
            yield f"dc {kind} n={n}", T
    names, batch = er.dc_batch()
    for name, T in zip(names, batch):
        yield f"dc batch {name}", T
    for name, A in er.background_kinds().items():
        yield name, A


def test_lapack_alone_is_inside_the_bound_on_every_case():
    bad = []
    for name, A in _all_cases():
        lam, Z = np.linalg.eigh(A)
        ref = er.reference_eigenvalues(A)
        # (eigvalsh and eigh may differ in their eigenvalues: the candidate is eigh's pair, as for a device's)
        bad += er.hold(name, A, lam, Z, ref=ref)
    assert not bad, "\n".join(bad)


def _top_merge_plan(d, e):
    """(k, rotations) of the library's deflation plan for the top merge of T(d, e), the halves solved by LAPACK."""
    import ctypes

    from cellregmap_amd import _lib

    lib = _lib.load()
    lam, z, n1, beta = er.top_merge_inputs(d, e)
    n = lam.size
    k, nrot, rho = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    rows, dl, w, rots = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(4 * n)
    _lib.check(lib.crm_test_dc_plan(_lib.ptr(lam), _lib.ptr(z), n1, n, float(beta), ctypes.byref(k), ctypes.byref(rho),
                                    _lib.ptr(rows), _lib.ptr(dl), _lib.ptr(w), ctypes.byref(nrot), _lib.ptr(rots)))
    return k.value, nrot.value


@pytest.mark.parametrize("n", [n for n in er.DC_ORDERS if n > 32])      # (order 32 is one leaf: no merge)
def test_the_deflation_states_are_the_ones_named(n):
    plans = {kind: _top_merge_plan(*er.dc_structure(kind, n)) for kind in er.dc_cases(n)}
    print(f"top merge n = {n}: (k, rotations) {plans}")
    assert plans["a"] == (2, 0)
    assert plans["b"] == (1, 1)
    assert plans["c"] == (0, 0)
    k, nrot = plans["d"]
    assert nrot == k >= 8                    # every surviving pole is a twin pair rotated into one
    if "g" in plans:
        assert plans["g"] == (n, 0)          # nothing deflates
        assert plans["e"][1] >= 5 and plans["i"][0] >= n // 3      # close pairs rotate; many poles survive


def test_exact_structures():
    for name, A in (("zero", np.zeros((40, 40))), ("identity", np.eye(40)), ("diagonal", np.diag(np.arange(40.0)[::-1]))):
        ref = er.reference_eigenvalues(A)
        assert float(np.abs(ref - np.sort(np.diag(A))).max()) <= 40 * 2.0 ** -88      # (the interval after 90 halvings)
        lam, Z = np.linalg.eigh(A)
        assert not er.hold(name, A, lam, Z, ref=ref)


@pytest.mark.parametrize("slip", list(er.SLIPS))
@pytest.mark.parametrize("case", ["random dense", "D C D rho=0", "dc i n=129"])
def test_planted_slips_break_the_bound(case, slip):
    if case == "random dense":
        X = np.random.default_rng(3).normal(size=(130, 130))
        A = X + X.T
    elif case.startswith("dc"):
        A = er.dc_cases(129)["i"]
    else:
        A = er.background_kinds()[case]
    ref = er.reference_eigenvalues(A)
    lam, Z = np.linalg.eigh(A)
    scale = float(np.abs(ref).max())
    assert not er.hold(case, A, lam, Z, ref=ref)
    bad = er.hold(f"{case}: {slip}", A, *er.SLIPS[slip](lam, Z, scale), ref=ref)
    assert bad, f"{slip} on {case} passed the bound"
