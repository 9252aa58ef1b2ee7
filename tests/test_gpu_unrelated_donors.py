"""The unrelated-donor form of the dense scan (scan.hip: kin_wb; assemble.hip: woodbury_kernel).  Where the donor-level
kinship hKd hKd' is diagonal, Q and F go through a per-donor Woodbury inverse of K0 instead of the product
A~ = MixK(rho*)'S.  Forced here (form ``kin_diag`` = 2: the cost model leaves small cohorts on the MixK route) and held
against the MixK route (``kin_diag`` = 0: the same rho*, Q and F to 1e-9, p to 1e-7), against the oracle at the north-star
tolerances, and -- per entry point and hook -- against itself bit for bit, as the MixK route is."""
import ctypes
import contextlib

import numpy as np
import pytest

import parity_bounds

pytestmark = pytest.mark.gpu


def _ragged(donors, cells, k0, variants, seed, kinship="indicator"):
    from cellregmap_amd.synth import make_cohort

    c = make_cohort(donors, cells, k0, variants, seed=seed, kinship=kinship)
    rng = np.random.default_rng(seed)
    keep = rng.random(c.y.shape[0]) > 0.35 * (np.arange(c.y.shape[0]) * 7 % donors) / donors   # unequal donor sizes
    keep[: cells] = True
    G = c.G[keep] + 0.05 * rng.normal(size=c.G[keep].shape)
    return c, keep, G


def _blocks():
    from cellregmap_amd import _engine, _lib

    out = ctypes.c_long(-1)
    _lib.check(_lib.load().crm_test_unrelated_donor_blocks(_engine._context(0), ctypes.byref(out)))
    return out.value


@contextlib.contextmanager
def _route(kernel_form, diag):
    """Kinship-structure route, folded form, unrelated-donor form `diag` (read when the structure is announced and by the
    scan: backgrounds made inside the block carry it)."""
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    kernel_form("kin_fold", 2)
    kernel_form("kin_diag", diag)
    _engine._bg_cache.clear()
    _lib.check(lib.crm_test_set_kinship_route(ctx, 2))
    try:
        yield
    finally:
        _lib.check(lib.crm_test_set_kinship_route(ctx, 1))


def _close(new, old):
    """(pv, info, stats) of the two routes: the same rho*, Q and F to 1e-9, p to 1e-7."""
    pv, info, st = new
    pv0, info0, st0 = old
    assert np.array_equal(info["rho1"], info0["rho1"])
    scale = np.maximum(np.abs(st0["Q"]), np.trace(st0["F"], axis1=1, axis2=2))
    assert np.all(np.abs(st["Q"] - st0["Q"]) <= 1e-9 * scale)
    fs = np.abs(st0["F"]).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(st["F"] - st0["F"]) <= 1e-9 * fs)
    assert np.all(np.abs(pv - pv0) <= 1e-7 * pv0 + 1e-13)


def _both_routes(kernel_form, make_obj, G, **hooks):
    """Scan with the MixK route, then with the unrelated-donor form; returns (old, new, new object, blocks it served)."""
    import cellregmap_amd as crm

    with _route(kernel_form, 0):
        old = make_obj().scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True, **hooks)
    with _route(kernel_form, 2):
        obj = make_obj()
        before = _blocks()
        new = obj.scan_interaction(crm.GenotypePanel(G, groups=None), return_stats=True, **hooks)
        served = _blocks() - before
        bp = parity_bounds.bounds(obj, crm.GenotypePanel(G, groups=None), **hooks)[1]
    return old, new, served, bp


def _oracle_p(pv, bp, sel, opv):
    parity_bounds.assert_p_within(pv[sel], opv, bp[sel])


@pytest.mark.parametrize("kinship", ["indicator", "rotated"])
@pytest.mark.parametrize("donors,cells,k0,variants,staged", [
    (7, 60, 5, 37, False),          # 5 + 3 + 5 = 13 Gram rows: the LDS-DMA Gram
    (7, 60, 5, 37, True),           # ... and the staged one (form gram_staged)
    (12, 40, 20, 70, False),
    (8, 60, 40, 40, False),         # 40 + 3 + 40 = 83 rows: the staged Gram the large configurations run
])
def test_unrelated_donors_match_the_mixk_route_and_the_oracle(donors, cells, k0, variants, staged, kinship, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    if staged:
        kernel_form("gram_staged", 1)
    c, keep, G = _ragged(donors, cells, k0, variants, 500 + k0 + cells, kinship)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    old, new, served, bp = _both_routes(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)), G)
    assert served > 0
    _close(new, old)
    sel = np.arange(0, variants, max(1, variants // 6))
    opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel])
    _oracle_p(new[0], bp, sel, opv)


def test_unrelated_donors_with_three_context_sets(kernel_form):
    """E1 != E2 != E0 (k1 = 7, k2 = 5, k0 = 6): the E1 rows, the capacitance and the per-donor basis all differ."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    c, keep, G = _ragged(9, 40, 6, 45, 123)
    rng = np.random.default_rng(4)
    n = int(keep.sum())
    y, E0, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    E1, E2 = rng.normal(size=(n, 7)), rng.normal(size=(n, 5))
    make = lambda: crm.CellRegMap(y, E0, W=W, E1=E1, Ls=crm.get_L_values(hK, E2))  # noqa: E731
    old, new, served, bp = _both_routes(kernel_form, make, G)
    assert served > 0
    _close(new, old)
    sel = np.arange(0, 45, 7)
    opv, _ = ocrm.OracleCellRegMap(y, E0, W=W, E1=E1, Ls=ocrm.khatri_rao_halves(hK, E2)).scan_interaction(G[:, sel])
    _oracle_p(new[0], bp, sel, opv)


@pytest.mark.parametrize("hook", ["E", "G"])
def test_unrelated_donors_with_the_permutation_hooks(hook, kernel_form):
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    c, keep, G = _ragged(8, 40, 5, 33, 61)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    idx = np.random.default_rng(3).permutation(y.size)
    hooks = {"idx_E": idx} if hook == "E" else {"idx_G": idx}
    old, new, served, bp = _both_routes(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)), G,
                                        **hooks)
    assert served > 0
    _close(new, old)
    sel = np.arange(0, 33, 5)
    opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel], **hooks)
    _oracle_p(new[0], bp, sel, opv)


@pytest.mark.parametrize("hook", ["E", "G", "both"])
def test_unrelated_donors_permutations_in_one_call_equal_separate_calls(hook, kernel_form):
    """crm_scan_interaction_permuted replays the first permutation's fits: the unrelated-donor form forms H'Gx again for
    Phi'gx and E1'gx -- the same bits as the separate calls."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(10, 24, 4, 29, 53)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    n = y.size
    rng = np.random.default_rng(8)
    B = 4
    perms = [rng.permutation(n) for _ in range(B)]
    perms2 = [rng.permutation(n) for _ in range(B)]
    lists = {"E": dict(idx_E_list=perms), "G": dict(idx_G_list=perms), "both": dict(idx_E_list=perms, idx_G_list=perms2)}[hook]
    with _route(kernel_form, 2):
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        panel = crm.GenotypePanel(G, groups=None)
        before = _blocks()
        pv, info, Q = obj.scan_interaction_permutations(panel, return_Q=True, **lists)
        assert _blocks() > before
        for b in range(B):
            one = {"E": dict(idx_E=perms[b]), "G": dict(idx_G=perms[b]), "both": dict(idx_E=perms[b], idx_G=perms2[b])}[hook]
            pv1, info1, st1 = obj.scan_interaction(panel, return_stats=True, **one)
            assert np.array_equal(pv[b], pv1)
            assert np.array_equal(Q[b], st1["Q"])
            for k in info1:
                assert np.array_equal(info[k], info1[k]), k


def test_unrelated_donors_many_phenotypes_in_one_pass_equal_separate_scans(kernel_form):
    """Several phenotypes: S in block order, each (gene, variant) its own weighted Gram -- bit for bit the single scans."""
    from cellregmap_amd import CellRegMap, GenotypePanel, get_L_values, scan_interaction_many

    c, keep, G = _ragged(8, 30, 4, 70, 41)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    rng = np.random.default_rng(7)
    Y = np.stack([y, y[rng.permutation(y.size)], rng.normal(size=y.size), y + rng.normal(size=y.size)], axis=1)
    with _route(kernel_form, 2):
        Ls = get_L_values(hK, E)
        first = CellRegMap(Y[:, 0], E, W=W, Ls=Ls)
        crms = [first] + [CellRegMap(Y[:, i], E, W=W, Ls=Ls, background=first._bg) for i in range(1, 4)]
        panel = GenotypePanel(G, groups=None)
        for kw in ({}, {"idx_E": rng.permutation(y.size)}, {"idx_G": rng.permutation(y.size)}):
            before = _blocks()
            pv, info = scan_interaction_many(crms, panel, **kw)
            assert _blocks() > before
            for i, one in enumerate(crms):
                spv, sinfo = one.scan_interaction(panel, **kw)
                assert np.array_equal(pv[i], spv)
                for k in sinfo:
                    assert np.array_equal(info[k][i], sinfo[k])


def test_unrelated_donors_info_flags(kernel_form):
    """scan_interaction_info: the flat-optimum probes assemble again at shifted delta through the same correction."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(8, 40, 5, 40, 17)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    res = {}
    for diag in (0, 2):
        with _route(kernel_form, diag):
            obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
            before = _blocks()
            res[diag] = obj.scan_interaction_info(crm.GenotypePanel(G, groups=None))
            assert (_blocks() > before) == (diag == 2)
    (pv, xi), (pv0, xi0) = res[2], res[0]
    assert np.all(np.abs(pv - pv0) <= 1e-7 * pv0 + 1e-13)
    for k in ("bound_Q", "bound_p"):
        assert np.all(np.abs(xi[k] - xi0[k]) <= 1e-3 * np.abs(xi0[k]) + 1e-12), k


def test_unrelated_donors_in_mode_b(kernel_form):
    """hK without Ls (K + E1E1'): the k2 = 1 case, us_d = 1."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    c, keep, G = _ragged(9, 50, 6, 40, 77)
    y, E, W, hK = c.y[keep], c.E[keep], c.W[keep], c.hK[keep]
    old, new, served, bp = _both_routes(kernel_form, lambda: crm.CellRegMap(y, E, W=W, hK=hK), G)
    assert served > 0
    _close(new, old)
    sel = np.arange(0, 40, 7)
    opv, _ = ocrm.OracleCellRegMap(y, E, W=W, hK=hK).scan_interaction(G[:, sel])
    _oracle_p(new[0], bp, sel, opv)


def test_past_the_row_limit_the_mixk_route_serves(kernel_form):
    """k0 + c + 2 + k1 > 144 (64 contexts, 16 covariate columns): even forced, the form is not taken; the scan runs and
    gives the MixK route's results."""
    import cellregmap_amd as crm

    c, keep, G = _ragged(6, 40, 64, 20, 9)
    rng = np.random.default_rng(2)
    y, E, hK = c.y[keep], c.E[keep], c.hK[keep]
    W = np.column_stack([np.ones(y.size), rng.normal(size=(y.size, 15))])
    old, new, served, _ = _both_routes(kernel_form, lambda: crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E)), G)
    assert served == 0
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[2]["Q"], old[2]["Q"])


def test_related_donors_keep_the_mixk_route(kernel_form):
    """A dense donor kinship (sib pairs plus a structure component) is not diagonal: even forced, the counter stays and the
    oracle agrees.  Positive control: the same cohort with its indicator factor moves the counter."""
    import cellregmap_amd as crm
    from oracle import crm as ocrm

    donors, cells, k0, variants = 10, 50, 6, 30
    c, keep, G = _ragged(donors, cells, k0, variants, 91)
    rng = np.random.default_rng(5)
    Kd = np.eye(donors)
    for d in range(0, donors - 1, 2):
        Kd[d, d + 1] = Kd[d + 1, d] = 0.5
    s = rng.normal(size=(donors, 1))
    Kd = Kd + 0.3 * s @ s.T
    hKd = np.linalg.cholesky(Kd)
    donor = np.argmax(c.hK, axis=1)
    y, E, W = c.y[keep], c.E[keep], c.W[keep]
    hK = hKd[donor[keep]]
    with _route(kernel_form, 2):
        panel = crm.GenotypePanel(G, groups=None)
        control = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(c.hK[keep], E))
        before = _blocks()
        control.scan_interaction(panel)
        assert _blocks() > before
        obj = crm.CellRegMap(y, E, W=W, Ls=crm.get_L_values(hK, E))
        from cellregmap_amd import _lib
        assert _lib.load().crm_background_kinship_folded(obj._bg.handle) > 0   # (the folded MixK route itself)
        before = _blocks()
        pv, info = obj.scan_interaction(panel)
        assert _blocks() == before
        bp = parity_bounds.bounds(obj, panel)[1]
    sel = np.arange(0, variants, 5)
    opv, _ = ocrm.OracleCellRegMap(y, E, W=W, Ls=ocrm.khatri_rao_halves(hK, E)).scan_interaction(G[:, sel])
    _oracle_p(pv, bp, sel, opv)
