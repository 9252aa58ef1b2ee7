"""A numpy statement of what blockops.hip's donor_pairs_rotate_kernel computes, held against dense numpy: the per-donor
sums S_d = sum_c g_c e_c e_c' from the packed pair products P_d[pair(j, i)] (j <= i, row-major upper triangle), and the
rotated S, A[(i), d k2 + j] = sum_k S_d[k, i] Psi_d[k, j], with the contraction over k cut into the groups of four that one
matrix instruction takes -- the groups past k0 meet zero rows of Psi_d and drop out, and the lanes k >= k0 of the last
group read pair (0, 0) instead of the next donor's rows."""
import numpy as np


def _pair(lo, hi, k0):
    return lo * k0 - lo * (lo - 1) // 2 + (hi - lo)


def _pairs_of(S):
    k0 = S.shape[0]
    return np.array([S[j, i] for j in range(k0) for i in range(j, k0)])


def _expand(P, k0):
    """S_d from the pair row as the kernel indexes it: S[k, i] = P[pair(min(k, i), max(k, i))]."""
    S = np.empty((k0, k0))
    for k in range(k0):
        for i in range(k0):
            lo, hi = min(k, i), max(k, i)
            S[k, i] = P[_pair(lo, hi, k0)]
    return S


def _rotate_in_groups(P, U, k0, k2):
    """The kernel's contraction: k-steps of four from k = 0, lanes k >= k0 reading pair (0, 0), steps past k0 left out."""
    ks = (k0 + 3) // 4
    A = np.zeros((k0, k2))
    for s in range(ks):
        for lane_k in range(4):
            k = 4 * s + lane_k
            row = np.array([P[_pair(min(k, i), max(k, i), k0)] if k < k0 else P[0] for i in range(k0)])
            A += np.outer(row, U[k, :k2])
    return A


def test_pair_index_covers_the_upper_triangle_once():
    for k0 in (2, 5, 50, 63):
        seen = sorted(_pair(j, i, k0) for j in range(k0) for i in range(j, k0))
        assert seen == list(range(k0 * (k0 + 1) // 2))


def test_expansion_and_rotation_match_dense_numpy():
    rng = np.random.default_rng(3)
    for k0, cells in ((5, 11), (20, 40), (50, 31), (56, 80)):
        k2 = k0
        k2pad = -(-k2 // 16) * 16
        e = rng.normal(size=(cells, k0))
        g = rng.normal(size=cells)
        S_dense = (e * g[:, None]).T @ e
        S_dense = np.triu(S_dense) + np.triu(S_dense, 1).T   # (the product's two triangles differ by rounding)
        P = _pairs_of(S_dense)
        assert np.allclose(_expand(P, k0), S_dense, rtol=0, atol=0)
        # Psi_d as the background stores it: k2pad rows, zero beyond k2 rows, dropped directions zero columns
        U = np.zeros((k2pad, 128))
        U[:k2, :k2] = rng.normal(size=(k2, k2))
        U[:, 1] = 0.0
        A = _rotate_in_groups(P, U, k0, k2)
        ref = S_dense.T @ U[:k2, :k2]
        assert np.allclose(A, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        assert np.all(A[:, 1] == 0.0)


def test_steps_past_k0_only_add_zeros():
    """The launch the kernel replaces ran all k2pad rows; the rows past k0 of Psi_d are zero, so their products are zeros
    whatever the operand (finite) -- the partial sums are unchanged."""
    rng = np.random.default_rng(5)
    k0 = 50
    k2pad = 64
    U = np.zeros((k2pad, 128))
    U[:k0, :k0] = rng.normal(size=(k0, k0))
    X = rng.normal(size=(k2pad, k0))       # rows past k0: the next donor's rows in the old layout
    part = sum(np.outer(X[k], U[k, :k0]) for k in range(4 * ((k0 + 3) // 4)))
    full = part + sum(np.outer(X[k], U[k, :k0]) for k in range(4 * ((k0 + 3) // 4), k2pad))
    assert np.array_equal(part, full)
