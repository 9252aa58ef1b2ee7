"""The background checker (tests/background_reference.py) on the CPU: LAPACK's own decompositions of every family the GPU
module builds (order up to 400) stay inside every cap with every rank margin at least 10 -- so the caps ask nothing of the
device that the reference route does not deliver itself -- and every planted defect is caught."""
import numpy as np
import pytest

import background_reference as br

GRID = br.RHO_GRID


def _families():
    """name -> (E1, B, grid, rel_tol, prescribed(rho) or None, with_mix)

    with_mix: Q0 is formed as H Mix with Mix = D(rho) V s^-1 of LAPACK's SVD, and Mix is held to the caps too.  Only for
    well-conditioned families: formed from V it satisfies Mix' C Mix = I to eps * S_max / S_min, which is the loss that
    the device's polish exists to repair, not a property of the reference's Q0 = U (which the other families check)."""
    out = {}

    def add(name, E1, B, grid=GRID, rel_tol=None, s=None, with_mix=False):
        pres = None if s is None else (lambda rho, s=s: br.prescribed_spectrum(s[0], s[1], rho))
        out[name] = (E1, B, np.asarray(grid, float), rel_tol, pres, with_mix)

    add("thin_well_97_3_20", *br.random_family(97, 3, 20, seed=1), with_mix=True)
    for n in (65, 64, 63):
        add("boundary_n%d_cols64" % n, *br.random_family(n, 5, 59, seed=2), with_mix=n == 65)
    for name, tol in (("default", None), ("1e-6", 1e-6)):
        E1, B, s1, s2 = br.rank_rule_family(tol)
        add("rank_rule_" + name, E1, B, rel_tol=tol, s=(s1, s2))
    for cols in (257, 384, 385):
        E1, B, s1, s2 = br.geometric_family(cols)
        add("polish_cols%d" % cols, E1, B, s=(s1, s2))
    for cond in (5e5, 2e6):
        E1, B, s1, s2 = br.conditioned_family(cond)
        add("seal_cond%g" % cond, E1, B, s=(s1, s2))
    add("eigh_random_60_10_100", *br.random_family(60, 10, 100, seed=3))
    E1, B, s1, s2 = br.eigh_prescribed_family()
    add("eigh_prescribed", E1, B, s=(s1, s2))
    E1, _ = br.random_family(80, 7, 0, seed=4)
    add("kb0_rho1", E1, None, grid=[1.0], with_mix=True)
    add("kb0_grid", E1, None, with_mix=True)
    E1, us, hK, B = br.hadamard_family(120, 5, 4, 9, seed=6)
    add("hadamard_thin", E1, B, with_mix=True)
    E1, us, hK, B = br.hadamard_family(120, 5, 10, 15, seed=7)
    add("hadamard_eigh", E1, B)
    return out


FAMILIES = _families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_lapack_decomposition_is_inside_every_cap(name):
    E1, B, grid, rel_tol, pres, with_mix = FAMILIES[name]
    dec = [br.lapack_decomposition(E1, B, rho, rel_tol, through_mix=with_mix) for rho in grid]
    figs = br.check_grid(E1, B, grid, lambda i: dec[i][:3], rel_tol=rel_tol, prescribed=pres,
                         mixes=[d[3] for d in dec] if with_mix and br.is_thin(E1, B) else None)
    w = br.worst(figs)
    print(name, w)
    assert w["rank_margin"] >= br.RANK_MARGIN


def test_the_families_have_the_shapes_their_cases_are_about():
    """Ranks, branches and conditioning that the GPU cases rely on, as facts about the inputs."""
    def ranks(name):
        E1, B, grid, rel_tol, _, _ = FAMILIES[name]
        return [br.rank_rule(br.reference_spectrum(E1, B, rho)[0], br.is_thin(E1, B), rel_tol)[0] for rho in grid]

    for name in ("rank_rule_default", "rank_rule_1e-6"):
        assert ranks(name) == [55] + [61] * 9 + [6]          # rank(0) = kept part of B, rank(10) = k1
    for cols in (257, 384, 385):
        assert ranks("polish_cols%d" % cols) == [cols - 5] + [cols] * 9 + [5]
    assert ranks("kb0_grid") == [0] + [7] * 10
    assert ranks("eigh_prescribed") == [47] + [56] * 9 + [9]
    assert br.is_thin(*FAMILIES["boundary_n65_cols64"][:2])
    assert not br.is_thin(*FAMILIES["boundary_n64_cols64"][:2]) and not br.is_thin(*FAMILIES["boundary_n63_cols64"][:2])
    for cond in (5e5, 2e6):      # S_max / S_min at the worst grid point, a factor 2 on either side of seal's 1e6
        E1, B, grid, _, _, _ = FAMILIES["seal_cond%g" % cond]
        kept = [s[:br.rank_rule(s, True)[0]] for s in (br.reference_spectrum(E1, B, rho)[0] for rho in grid)]
        worst = max(s.max() / s.min() for s in kept)
        assert abs(worst / cond - 1) < 1e-6
    E1, B, grid, _, _, _ = FAMILIES["polish_cols384"]
    s = br.reference_spectrum(E1, B, 0.5)[0]
    assert s.max() > 1e6 * s.min()


# ---- the checker bites ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    E1, B = br.random_family(97, 3, 20, seed=1)
    rho = 0.5
    Q0, S0, r, Mix = br.lapack_decomposition(E1, B, rho, through_mix=True)
    padded = np.zeros((128, 128))
    padded[:Mix.shape[0], :r] = Mix
    br.check(E1, B, rho, Q0, S0, r, Mix=padded)
    for a in (Q0, S0, padded):
        a.setflags(write=False)
    return E1, B, rho, Q0, S0, r, padded


def _caught(clean, match, Q0=None, S0=None, r=None, Mix=None):
    E1, B, rho, q, s, rr, m = clean
    with pytest.raises(AssertionError, match=match):
        br.check(E1, B, rho, q if Q0 is None else Q0, s if S0 is None else S0, rr if r is None else r,
                 Mix=m if Mix is None else Mix)


def test_a_rotated_column_is_caught(clean):
    Q0 = clean[3].copy()
    j = 7
    Q0[:, j] = np.cos(1e-9) * clean[3][:, j] + np.sin(1e-9) * clean[3][:, j + 1]
    _caught(clean, "orthonormality", Q0=Q0)


def test_one_wrong_eigenvalue_is_caught(clean):
    S0 = clean[4].copy()
    S0[5] += 1e-9 * S0.max()
    _caught(clean, "spectrum", S0=S0)


def test_swapped_columns_are_caught(clean):
    Q0 = clean[3].copy()
    Q0[:, [2, 3]] = Q0[:, [3, 2]]
    _caught(clean, "reconstruction", Q0=Q0)


@pytest.mark.parametrize("step", [-1, 1])
def test_a_rank_off_by_one_is_caught(clean, step):
    E1, B, rho, Q0, S0, r, Mix = clean
    if step < 0:
        q, s = Q0[:, :-1], S0[:-1]
    else:     # one more column: orthonormal to the others, with the next (zero) eigenvalue
        extra = np.linalg.svd(Q0, full_matrices=True)[0][:, r]
        q, s = np.c_[Q0, extra], np.r_[S0, 0.0]
    _caught(clean, "rank", Q0=q, S0=s, r=r + step)


def test_a_scaled_row_of_the_mixing_matrix_is_caught(clean):
    Mix = clean[6].copy()
    Mix[4, :] *= 1 + 1e-9
    _caught(clean, "mixing matrix", Mix=Mix)


@pytest.mark.parametrize("where", ["row", "column"])
def test_a_non_zero_in_the_padding_of_the_mixing_matrix_is_caught(clean, where):
    Mix = clean[6].copy()
    if where == "row":
        Mix[23, 0] = 1e-300     # first row past cols = 23
    else:
        Mix[0, 23] = 1e-300     # first column past r = 23
    _caught(clean, "padding", Mix=Mix)


def test_rows_of_B_at_rho_1_must_be_zero():
    E1, B = br.random_family(97, 3, 20, seed=1)
    Q0, S0, r, Mix = br.lapack_decomposition(E1, B, 1.0, through_mix=True)
    assert r == 3
    br.check(E1, B, 1.0, Q0, S0, r, Mix=Mix)
    Mix = Mix.copy()
    Mix[10, 1] = 1e-300
    with pytest.raises(AssertionError, match="rows of B at rho = 1"):
        br.check(E1, B, 1.0, Q0, S0, r, Mix=Mix)


def test_a_spectrum_in_the_wrong_order_is_caught(clean):
    _caught(clean, "order", Q0=clean[3][:, ::-1], S0=clean[4][::-1])


def test_an_eigenvalue_near_the_cut_is_refused():
    """A case whose rank rounding could decide is not a case: a factor 5 from the cut is refused."""
    s1 = np.array([1.0, 0.5])
    s2 = np.r_[np.linspace(1.0, 0.1, 9), 5e-12]
    E1, B = br.prescribed_family(40, s1, s2, seed=9)
    Q0, S0, r, _ = br.lapack_decomposition(E1, B, 0.0)
    with pytest.raises(br.CaseRefused):
        br.check(E1, B, 0.0, Q0, S0, r)
