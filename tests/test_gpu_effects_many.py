"""Batched effect sizes (estimate_betas_many / predict_interaction_many) against the oracle's
restatement of cellregmap/_cellregmap.py:137-205 and against the per-SNP device path (estimate_betas)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cellregmap_amd.synth import make_cohort  # noqa: E402


def _cohort(seed=3, donors=8, cells=15, k0=3, p=4, phenotypes=3):
    c = make_cohort(donors, cells, k0, p, seed=seed)
    maf = np.clip(np.minimum(c.G.mean(0) / 2, 1 - c.G.mean(0) / 2), 0.05, 0.5)
    rng = np.random.default_rng(seed + 100)
    n = c.y.shape[0]
    Y = np.column_stack([c.y] + [c.y * 0.5 + rng.normal(size=n) for _ in range(phenotypes - 1)])
    return c, maf, Y


# repeated variants, repeated pairs, arbitrary order
PAIRS = np.array([[2, 1], [0, 3], [1, 1], [0, 0], [2, 1], [1, 2], [0, 3], [2, 0]])


def _hold(dev, ora, ora_polished):
    """test_gpu_effects.py::test_estimate_betas_at_two_thousand_cells's bound through the oracle's own optimum."""
    scale = np.max(np.abs(ora_polished))
    gap = np.max(np.abs(dev - ora))
    assert gap <= 2.0 * np.max(np.abs(ora - ora_polished)) + 3e-6 * scale, (gap, np.max(np.abs(ora - ora_polished)), scale)


def _oracle_pair(Y, c, maf, i, v, hK, polish=False, **kw):
    from oracle import crm as ocrm

    return ocrm.estimate_betas(Y[:, i], c.W, c.E, c.G[:, [v]], maf=maf[[v]], hK=hK, polish=polish, **kw)


def _oracle_rho1(Y, c, i, v, hK):
    """rho* of the oracle's verbatim fit and whether its two best grid lmls are within 1e-9 relative."""
    from oracle.crm import RHO_GRID, khatri_rao_halves
    from oracle.lmm import LMM
    from oracle.sugar import economic_qs_linear

    g = c.G[:, [v]]
    M = np.concatenate((c.W, g, c.E), axis=1)
    Ls = [] if hK is None else khatri_rao_halves(hK, c.E)
    grid = [1.0] if hK is None else RHO_GRID
    lmls = []
    for rho in grid:
        hS = np.concatenate([np.sqrt(rho) * g * c.E] + [np.sqrt(1 - rho) * L for L in Ls], axis=1)
        lmm = LMM(Y[:, i], M, economic_qs_linear(hS, return_q1=False), restricted=True)
        lmm.fit(verbose=False)
        lmls.append(lmm.lml())
    lmls = np.array(lmls)
    best = int(np.argmax(lmls))
    top = np.sort(lmls)[::-1]
    close = top.size > 1 and abs(top[0] - top[1]) <= 1e-9 * abs(top[0])
    return grid[best], close


@pytest.mark.parametrize("case", ["small_kinship", "small_no_kinship", "two_thousand_cells"])
def test_pairs_hold_against_the_oracle(case):
    import cellregmap_amd as crm

    if case == "two_thousand_cells":
        c, maf, Y = _cohort(seed=29, donors=40, cells=50, k0=10, p=4)
    else:
        c, maf, Y = _cohort()
    hK = None if case == "small_no_kinship" else c.hK
    bg, bgxe, info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=hK, pairs=PAIRS, return_info=True)
    assert bg.shape == (len(PAIRS),) and bgxe.shape == (1, Y.shape[0], len(PAIRS))
    assert np.all(info["route"] == "woodbury"), info["route"]
    assert info["u"].shape == (len(PAIRS), c.E.shape[1])
    for t, (i, v) in enumerate(PAIRS):
        obg, obgxe = _oracle_pair(Y, c, maf, i, v, hK)
        pbg, pbgxe = _oracle_pair(Y, c, maf, i, v, hK, polish=True)
        _hold(bg[[t]], obg, pbg)
        _hold(bgxe[0, :, t], obgxe[0, :, 0], pbgxe[0, :, 0])
        rho, close = _oracle_rho1(Y, c, i, v, hK)
        if not close:
            assert info["rho1"][t] == rho, (t, info["rho1"][t], rho)


def test_pairs_hold_against_the_per_snp_device_path():
    """E2 != E0 and two columns of W; E1 accepted and left unused (as in the reference)."""
    import cellregmap_amd as crm

    c, maf, Y = _cohort(seed=11)
    rng = np.random.default_rng(5)
    n = Y.shape[0]
    W = np.column_stack([np.ones(n), rng.normal(size=n)])
    E2 = rng.normal(size=(n, 2))
    E1 = rng.normal(size=(n, 4))
    bg, bgxe, info = crm.estimate_betas_many(Y, W, c.E, c.G, maf=maf, E1=E1, E2=E2, hK=c.hK, pairs=PAIRS,
                                             return_info=True)
    assert np.all(info["route"] == "woodbury")
    for t, (i, v) in enumerate(PAIRS):
        dbg, dbgxe = crm.estimate_betas(Y[:, i], W, c.E, c.G[:, [v]], maf=maf[[v]], E1=E1, E2=E2, hK=c.hK)
        from oracle import crm as ocrm

        pbg, pbgxe = ocrm.estimate_betas(Y[:, i], W, c.E, c.G[:, [v]], maf=maf[[v]], E1=E1, E2=E2, hK=c.hK, polish=True)
        _hold(bg[[t]], dbg, pbg)
        _hold(bgxe[0, :, t], dbgxe[0, :, 0], pbgxe[0, :, 0])


def test_a_pair_does_not_depend_on_its_batch():
    import cellregmap_amd as crm

    c, maf, Y = _cohort(seed=29, donors=40, cells=50, k0=10, p=4)
    all_bg, all_gxe, all_info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=PAIRS,
                                                        return_info=True)
    perm = np.random.default_rng(1).permutation(len(PAIRS))
    s_bg, s_gxe = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=PAIRS[perm])
    assert np.array_equal(s_bg, all_bg[perm]) and np.array_equal(s_gxe, all_gxe[:, :, perm])
    h1 = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=PAIRS[:3])
    h2 = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=PAIRS[3:])
    assert np.array_equal(np.concatenate([h1[0], h2[0]]), all_bg)
    assert np.array_equal(np.concatenate([h1[1], h2[1]], axis=2), all_gxe)
    for t in (0, 5):
        one_bg, one_gxe, one_info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=PAIRS[[t]],
                                                            return_info=True)
        assert np.array_equal(one_bg, all_bg[[t]]) and np.array_equal(one_gxe[:, :, 0], all_gxe[:, :, t])
        assert np.array_equal(one_info["u"][0], all_info["u"][t])


def _per_snp(Y, W, c, G, maf, pairs, hK):
    import cellregmap_amd as crm

    out = [crm.estimate_betas(Y[:, i], W, c.E, G[:, [v]], maf=maf[[v]], hK=hK) for i, v in pairs]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out], axis=2)


def test_fallback_when_g_lies_in_the_span_of_w_and_e0():
    import cellregmap_amd as crm

    c, maf, Y = _cohort()
    G = c.G.copy()
    G[:, 2] = 0.5 * c.W[:, 0] + c.E @ np.array([1.0, -0.5, 0.25])
    pairs = np.array([[0, 2], [1, 0], [2, 2]])
    bg, bgxe, info = crm.estimate_betas_many(Y, c.W, c.E, G, maf=maf, hK=c.hK, pairs=pairs, return_info=True)
    assert list(info["route"]) == ["per_snp", "woodbury", "per_snp"]
    ref = _per_snp(Y, c.W, c, G, maf, pairs[[0, 2]], c.hK)
    assert np.array_equal(bg[[0, 2]], ref[0]) and np.array_equal(bgxe[:, :, [0, 2]], ref[1])


def test_fallback_when_the_cohort_is_too_small_or_too_wide():
    import cellregmap_amd as crm

    # n <= k0 + columns of L: 4 donors x 3 cells = 12 cells against k0 = 3 and L of 3 x 4 = 12 columns
    c, maf, Y = _cohort(seed=7, donors=4, cells=3, k0=3, p=2)
    pairs = np.array([[0, 1], [2, 0]])
    bg, bgxe, info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=pairs, return_info=True)
    assert np.all(info["route"] == "per_snp")
    ref = _per_snp(Y, c.W, c, c.G, maf, pairs, c.hK)
    assert np.array_equal(bg, ref[0]) and np.array_equal(bgxe, ref[1])
    # k0 = 65: c_W + 2 k0 + 2 = 133 > 130 (mode A keeps it small)
    c, maf, Y = _cohort(seed=8, donors=10, cells=20, k0=65, p=2, phenotypes=2)
    pairs = np.array([[1, 0]])
    bg, bgxe, info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, pairs=pairs, return_info=True)
    assert np.all(info["route"] == "per_snp")
    ref = _per_snp(Y, c.W, c, c.G, maf, pairs, None)
    assert np.array_equal(bg, ref[0]) and np.array_equal(bgxe, ref[1])


def test_config3_shape_through_the_route():
    import cellregmap_amd as crm
    from cellregmap_amd.synth import make_config

    c = make_config("cfg3", n_variants=2)
    maf = np.clip(np.minimum(c.G.mean(0) / 2, 1 - c.G.mean(0) / 2), 0.05, 0.5)
    rng = np.random.default_rng(3)
    n = c.y.shape[0]
    Y = np.column_stack([c.y] + [c.y * 0.5 + rng.normal(size=n) for _ in range(3)])
    pairs = np.array([[0, 0], [1, 1], [2, 0], [3, 1]])
    bg, bgxe, info = crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=pairs, return_info=True)
    assert np.all(info["route"] == "woodbury")
    assert np.all(np.isfinite(bg)) and np.all(np.isfinite(bgxe))
    for t in (0, 3):   # (two of the four against the per-SNP device path: 1.1 s a pair)
        i, v = pairs[t]
        dbg, dbgxe = crm.estimate_betas(Y[:, i], c.W, c.E, c.G[:, [v]], maf=maf[[v]], hK=c.hK)
        for a, b in ((bg[[t]], dbg), (bgxe[0, :, t], dbgxe[0, :, 0])):
            scale = np.max(np.abs(b))
            assert np.max(np.abs(a - b)) <= 1e-4 * scale, (t, np.max(np.abs(a - b)), scale)


def test_misuse_is_refused_before_device_work():
    import cellregmap_amd as crm
    from cellregmap_amd import CellRegMap, get_L_values

    c, maf, Y = _cohort()
    with pytest.raises(ValueError):
        crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=np.array([[3, 0]]))
    with pytest.raises(ValueError):
        crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=np.array([[0, 4]]))
    with pytest.raises(ValueError):
        crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf, hK=c.hK, pairs=np.array([[-1, 0]]))
    with pytest.raises(ValueError):
        crm.estimate_betas_many(Y, c.W, c.E, c.G, maf=maf[:3], hK=c.hK)
    bad = Y.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        crm.estimate_betas_many(bad, c.W, c.E, c.G, maf=maf, hK=c.hK)
    Ls = get_L_values(c.hK, c.E)
    a = CellRegMap(Y[:, 0], c.E, W=c.W, Ls=Ls)
    for other in (CellRegMap(Y[:, 1], c.E, W=np.column_stack([c.W, c.E[:, 0]]), Ls=Ls),
                  CellRegMap(Y[:, 1], c.E[:, ::-1], W=c.W, Ls=Ls),
                  CellRegMap(Y[:, 1], c.E, W=c.W, Ls=get_L_values(c.hK, c.E[:, :2]))):
        with pytest.raises(ValueError):
            crm.predict_interaction_many([a, other], c.G, maf)
