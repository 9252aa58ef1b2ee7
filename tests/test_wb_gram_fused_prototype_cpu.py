"""The index arithmetic of wb_gram_fused_kernel, as tools/wb_gram_fused_prototype.py states it in numpy with an LDS of NaN
and bounds-checked global reads, against the two launches' arithmetic written plainly: the rotated S of every donor from its
pair products, then the weighted Gram over all donors k0 positions.  Covers the pair lookup, where A_d and the other rows
land in the LDS image, and the walk in chunks that end at multiples of four positions -- an odd last donor included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wb_gram_fused_prototype as proto  # noqa: E402


def _problem(donors, k0, c, seed, drop=()):
    """(P, U, rows, S0) as the kernel meets them: ldp and ldr rounded up to 128, zeros past the data, NaN in P's padding."""
    rng = np.random.default_rng(seed)
    npair = k0 * (k0 + 1) // 2
    ldp = -(-npair // 128) * 128
    k2pad = -(-k0 // 16) * 16
    ptot = donors * k0
    ldr = -(-ptot // 128) * 128
    P = np.full((donors, ldp), np.nan)
    P[:, :npair] = rng.normal(size=(donors, npair))
    U = np.zeros((donors, k2pad, 128))
    U[:, :k0, :k0] = rng.normal(size=(donors, k0, k0))
    S0 = np.zeros(ldr)
    S0[:ptot] = rng.uniform(0.1, 3.0, size=ptot)
    for d, j in drop:                     # a dropped direction: zero column of Psi, zero spectrum entry
        U[d, :, j] = 0.0
        S0[d * k0 + j] = 0.0
    rows = np.zeros((k0 + c + 2, ldr))
    rows[:, :ptot] = rng.normal(size=(k0 + c + 2, ptot))
    return P, U, rows, S0


def _plain(P, U, rows, S0, k0, ratio, has_A):
    donors = P.shape[0]
    ptot = donors * k0
    A = np.zeros((k0, ptot))
    for d in range(donors):
        S = np.array([[P[d, proto.pair(min(k, i), max(k, i), k0)] for i in range(k0)] for k in range(k0)])
        if has_A:
            A[:, d * k0:(d + 1) * k0] = S.T @ U[d, :k0, :k0]
    full = np.vstack([A, rows[:, :ptot]])
    s = ratio * S0[:ptot]
    return full @ (full * (s / (1.0 + s))).T


def test_layout_fits_two_workgroups_per_cu_at_the_large_configuration():
    L = proto.layout(50, 103, 1280)
    assert 2 * 8 * L["total"] <= 160 * 1024
    assert L["RS"] == 54 and L["RS"] // 2 % 2 == 1          # sixteen rows of a fragment read: distinct bank pairs
    assert L["off_U"] + (L["urows"] - 1) * L["UW"] + 64 <= L["off_d"]      # the rotation's widest fragment read stays inside
    for k0 in range(30, 56, 2):
        RS = proto.layout(k0, 2 * k0 + 3, -(-(k0 * (k0 + 1) // 2) // 128) * 128)["RS"]
        assert RS >= k0 + 4 and RS % 4 == 2 and RS <= 64


@pytest.mark.parametrize("k0,donors", [(50, 5), (50, 4), (40, 3), (54, 3), (6, 7), (6, 1), (8, 2)])
def test_chunks_tile_the_positions_in_whole_groups_of_four(k0, donors):
    at = 0
    for d in range(donors):
        start, end, c0, lim = proto.chunk(d, k0, donors)
        assert start == at and start % 4 == 0 and end % 4 == 0 and end > start
        assert c0 in (0, 2) and c0 + (end - start) <= ((k0 + 4) | 2)
        assert start - c0 + 2 == k0 * d                      # A_d[., j] at column j + 2
        at = end
    assert at == (donors * k0 + 3) // 4 * 4 and lim == donors * k0


@pytest.mark.parametrize("k0,donors,c,splits,has_A", [
    (50, 5, 1, 2, True),      # 103 rows; k0 = 2 mod 4: chunks of 48 and 52, an odd last donor with two columns of zeros
    (50, 2, 1, 1, False),     # a variant without a kinship term: rows of zeros
    (40, 3, 3, 3, True),      # k0 = 0 mod 4: whole chunks; three covariates
    (54, 4, 1, 3, True),      # the largest k0; a range of donors that holds none (4 donors in ranges of 2, 3 splits)
    (6, 3, 1, 1, True),       # small: the index arithmetic alone (the launch serves 65 rows and more)
])
def test_gw_and_donor_sums_from_the_lds_walk(k0, donors, c, splits, has_A):
    P, U, rows, S0 = _problem(donors, k0, c, 40 + k0 + donors, drop=((0, 1), (donors - 1, k0 - 1)))
    ratio = 0.7
    Gw, Psum, stats = proto.fused_gw(P, U, rows, S0, k0, c, ratio, has_A=has_A, splits=splits)
    ref = _plain(P, U, rows, S0, k0, ratio, has_A)
    assert np.all(np.isfinite(Gw))                           # (no column that nothing wrote, no read off a buffer)
    assert np.allclose(Gw, ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())
    npair = k0 * (k0 + 1) // 2
    per = -(-donors // splits)
    for s in range(splits):
        assert np.array_equal(Psum[s], sum((P[d, :npair] for d in range(s * per, min(donors, (s + 1) * per))), np.zeros(npair)))
