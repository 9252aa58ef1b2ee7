"""The one-stage eigen-solver (eigh_trd.hip, eigh_dc.hip, eigh_bt.hip) at its size and deflation edges, through
``crm_test_eigh``, under the bound of tests/eigh_reference.py: every measure (eigenvalues, A - Z diag(lam) Z', Z'Z - I, all
formed in long double against a long-double spectrum) within 8 x max(LAPACK's own value on the same matrix, n eps scale).

  * divide and conquer alone (stage 2: lam, Z are the eigen-pairs of the returned T(d, e)) at the orders where the tree
    changes shape, with tridiagonals that put the top merge -- cut after row m - 1, m = (ceil(n / 16) / 2) 16 -- into each
    deflation state: k = 2, 1, 0 surviving poles, every surviving pole a rotated twin pair, close pairs, graded,
    constant (nothing deflates), couplings whose squares underflow, a random one (many poles, partial deflation) --
    tests/test_eigh_reference_cpu.py asserts these states on the library's own deflation plan; and one batch whose
    matrices deflate differently;
  * dense matrices of the kinds a background has, end to end at order 130;
  * the back-transformation in blocks of 256 reflectors (order >= 2048) with per-matrix reflectors and T factors: 2048
    (8 pairs, no trailing block) and batches of two different matrices at 2050 and 2052 (8 pairs and a trailing block
    that holds the last, trivial reflector alone, or two working ones beside it), against LAPACK with the tolerances of
    test_gpu_eigh.py::test_larger_matrix (long double is too slow at this order).

Every case prints the device's three measures, LAPACK's and the ratio (``pytest -s``).
"""
import numpy as np
import pytest

import eigh_reference as er
from test_gpu_eigh import _check, _eigh, ctx  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu


def _hold_dc(ctx, name, T_in):
    """Stage 2 on a tridiagonal passed as dense: (lam, Z) against the T the device itself reports."""
    T_in = np.asarray(T_in)
    batched = T_in.ndim == 3
    lam, Z, d, e = _eigh(ctx, T_in, stage=2)
    bad = []
    for b in range(lam.shape[0]):
        n = lam.shape[1]
        T = er.tridiag(d[b], e[b])
        src = T_in[b] if batched else T_in
        label = f"{name[b] if batched else name} n={n}"
        # the tridiagonaliser met a tridiagonal: it may flip signs of e, nothing else
        if not (np.array_equal(np.diag(T), np.diag(src)) and np.array_equal(np.abs(np.diag(T, -1)), np.abs(np.diag(src, -1)))):
            bad.append(f"{label}: T(d, e) is not the input up to the signs of e")
        if not (np.all(np.isfinite(lam[b])) and np.all(np.diff(lam[b]) >= 0)):
            bad.append(f"{label}: lam not ascending and finite")
        bad += er.hold("D&C " + label, T, lam[b], Z[b])
    return bad


@pytest.mark.parametrize("n", er.DC_ORDERS)
def test_divide_and_conquer_at_the_tree_edges(ctx, n):  # noqa: F811
    bad = []
    for kind, T in er.dc_cases(n).items():
        bad += _hold_dc(ctx, f"({kind})", T)
    assert not bad, "\n".join(bad)


def test_a_batch_that_deflates_differently_per_matrix(ctx):  # noqa: F811
    names, batch = er.dc_batch(97)
    bad = _hold_dc(ctx, [f"batch ({k})" for k in names], batch)
    assert not bad, "\n".join(bad)


def test_dense_kinds_a_background_has_under_the_bound(ctx):  # noqa: F811
    bad = []
    for name, A in er.background_kinds(130).items():
        lam, Z, _, _ = _eigh(ctx, A)
        if not np.all(np.diff(lam[0]) >= 0):
            bad.append(f"{name}: lam not ascending")
        bad += er.hold(name, A, lam[0], Z[0])
    assert not bad, "\n".join(bad)


def test_exact_structures_under_the_bound(ctx):  # noqa: F811
    rng = np.random.default_rng(2)
    bad = []
    for name, A in (("zero", np.zeros((130, 130))), ("identity", np.eye(130)), ("diagonal", np.diag(rng.normal(size=130)))):
        lam, Z, _, _ = _eigh(ctx, A)
        assert np.all(np.isfinite(lam[0])) and np.all(np.diff(lam[0]) >= 0), name
        bad += er.hold(name, A, lam[0], Z[0])
    assert not bad, "\n".join(bad)


def _print_against_lapack(name, A, lam, Z):
    ref = np.linalg.eigvalsh(A)
    n, scale = A.shape[0], np.abs(ref).max()
    print(f"[eigh-hold] {name:<46s} n={n:<5d} against LAPACK, in units of n scale: eig "
          f"{np.abs(lam - ref).max() / (n * scale):.2e} resid {np.abs(A @ Z - Z * lam).max() / (n * scale):.2e} "
          f"orth {np.abs(Z.T @ Z - np.eye(n)).max() / n:.2e} (tolerance 2e-13)")


def test_back_transformation_in_pairs_of_blocks(ctx):  # noqa: F811
    """2048: 16 blocks of 128 reflectors, 8 pairs, no trailing block, no padding (dimp == dim)."""
    A = er.graded_gram(2048, seed=11, decades=3)
    lam, Z, _, _ = _eigh(ctx, A)
    _print_against_lapack("pairs of blocks", A, lam[0], Z[0])
    _check(A, lam[0], Z[0], tol=2e-13)


@pytest.mark.parametrize("dim", [2050, 2052])
def test_back_transformation_in_pairs_per_matrix_reflectors(ctx, dim):  # noqa: F811
    """Two different matrices: 17 blocks, 8 pairs and a trailing block of 128; the T factors, pair Gram matrices and
    reflectors are per matrix, so a mix-up between the two shows.  At 2050 the trailing block holds the single reflector
    2048, the last one, which is the identity (tau = 0: nothing below its pivot), so that block only has to leave Z alone;
    at 2052 it holds 2048 and 2049, which do work, and the trailing block's per-matrix T and strides show too."""
    A = np.stack([er.graded_gram(dim, seed=12, decades=3), er.graded_gram(dim, seed=13, decades=1)])
    lam, Z, _, _ = _eigh(ctx, A)
    for b in range(2):
        _print_against_lapack(f"pairs + trailing block, matrix {b}", A[b], lam[b], Z[b])
    for b in range(2):
        _check(A[b], lam[b], Z[b], tol=2e-13)
