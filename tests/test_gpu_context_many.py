"""The fixed-effect GxC tests of several phenotypes in one pass (``scan_interaction_contexts_many``,
``scan_interaction_contexts_joint_many``; crm_scan_interaction_contexts_multi, crm_scan_interaction_contexts_joint_multi;
DESIGN.md section 14) on a real MI355X.  Cohorts: tests/context_many_cases.py (conditions: tests/test_context_many_cases_cpu.py).

  accuracy      every phenotype's row of a many call, both ``fast`` values, against the longdouble references of the
                single-phenotype tests at the (rho, delta_i) the device reports, by ``_hold`` of tests/context_lrt_hold.py and
                tests/context_joint_hold.py unchanged: limit 32 x the float64 oracle's own error, floor n x 2.2e-16, ceiling
                1e-11.  Against the phenotype's single call: status, dof, dropped, rho1 and the six numbers of the gene-level
                null equal (bit for bit), the continuous outputs within the sum of the two limits.
  independence  bit for bit: a phenotype's rows do not depend on the other phenotypes of the call, on their order, on the
                window (``first > 0``), on blocks of 128 variants with room for the rotated candidates of 50, nor on whether
                the panel is donor-level or expanded.
  cis walks     overlapping windows, a scattered index array with repeats, an empty entry, a phenotype alone on a stretch:
                entry i is the many call of that phenotype on ``G[:, cis_index[i]]`` bit for bit.
  sharing       the count of timed Khatri-Rao contractions of a many call is (distinct rho*) x (sub-ranges), and their flops
                the same factor of one single call's -- against P x (sub-ranges) of P single calls.
  misuse        the error codes, with nothing launched.
"""
import ctypes

import numpy as np
import pytest

import context_block_cases as bc
import context_joint_hold as jh
import context_lrt_hold as lh
import context_many_cases as mc
import context_joint_reference as jr
import context_lrt_reference as cr

pytestmark = pytest.mark.gpu

RECORD = {}
OK = lh.OK
K3 = "k 3, c 9, mode B"
MIXED = "k 5, rank 260, mode B"
FLOAT_EACH = ("alt_lml", "beta", "beta_se", "log_pvalue", "null_lml", "null_delta")
INT_KEYS = ("status", "dof", "dropped")


def _kit(joint):
    return jh if joint else lh


def _many_call(joint):
    import cellregmap_amd as crm

    return crm.scan_interaction_contexts_joint_many if joint else crm.scan_interaction_contexts_many


_objs = {}


def _objects(name):
    """(the cohort, its phenotype views, one CellRegMap per phenotype on one background)."""
    if name not in _objs:
        import cellregmap_amd as crm

        base, views = mc.cohort(name)
        first = _kit(False)._device(views[0])
        crms = [first] + [crm.CellRegMap(v.y, v.C, W=v.W, background=first._bg, **v.device_kw()) for v in views[1:]]
        _objs[name] = (base, views, crms)
    return _objs[name]


_scans = {}


def _many(name, fast, joint=None):
    """(pv, info) of the cohort's many call with ``return_stats``; one scan per process."""
    joint = mc.is_joint(name) if joint is None else joint
    key = (name, fast, joint)
    if key not in _scans:
        base, _, crms = _objects(name)
        _scans[key] = _many_call(joint)(crms, base.G, fast=fast, return_stats=True)
    return _scans[key]


def _row(result, i):
    """Phenotype i of a many call as the (pv, info) of a single-phenotype call."""
    pv, info = result
    one = {key: (val[i] if key not in ("rho1", "e2", "g2", "eps2") else np.asarray([val[i]])) for key, val in info.items()}
    return pv[i], one


def _entry(result, i):
    """Phenotype i of a many call with ``cis_index`` (lists over the phenotypes) as the (pv, info) of a single call."""
    pv, info = result
    one = {}
    for key, val in info.items():
        one[key] = val[i] if isinstance(val, list) or key.startswith("gene_null") else np.asarray([val[i]])
    return pv[i], one


def _same_rows(a, b, what):
    """Bit equality of two single-phenotype results (every key they both hold)."""
    (pa, ia), (pb, ib) = a, b
    assert np.array_equal(pa, pb, equal_nan=True), what
    for key in ia:
        if key in ib:
            assert np.array_equal(np.asarray(ia[key]), np.asarray(ib[key]), equal_nan=key not in INT_KEYS), (what, key)


class _EachAt(lh._At):
    """``context_lrt_hold._At`` that computes every record once: they depend on the phenotype, the variant and delta alone."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._memo = {}

    def at(self, g, delta):
        key = ("at", g.tobytes(), delta)
        if key not in self._memo:
            self._memo[key] = super().at(g, delta)
        return self._memo[key]

    def refit(self, g):
        key = ("refit", g.tobytes())
        if key not in self._memo:
            self._memo[key] = super().refit(g)
        return self._memo[key]


class _JointAt(jh._At):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._memo = {}

    def at(self, g, delta, keep=None):
        key = (g.tobytes(), delta, None if keep is None else tuple(keep))
        if key not in self._memo:
            self._memo[key] = super().at(g, delta, keep=keep)
        return self._memo[key]


_ats = {}


def _at(joint, name, i, view, rho):
    key = (joint, name, i, float(rho))
    if key not in _ats:
        _ats[key] = (_JointAt if joint else _EachAt)(view, view.y, rho)
    return _ats[key]


def _hold(name, i, result, fast, tag):
    base, views, _ = _objects(name)
    joint = mc.is_joint(name)
    pv, info = result
    at = _at(joint, name, i, views[i], info["rho1"][0])
    label = "many %s %s, %s, phenotype %d%s" % ("joint" if joint else "each", "fast" if fast else "refit", name, i, tag)
    return _kit(joint)._hold(label, views[i], views[i].y, base.G, pv, info, fast, at=at, record=RECORD)


PHENOTYPES = [(name, i) for name in mc.COHORTS for i in range(len(mc.COHORTS[name][1]))]


# ---- B: accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name,i", PHENOTYPES)
def test_every_phenotypes_row_against_the_reference_and_its_single_call(name, i, fast):
    base, views, crms = _objects(name)
    joint = mc.is_joint(name)
    pv, info = _row(_many(name, fast), i)
    _, lim = _hold(name, i, (pv, info), fast, "")
    assert np.all(info["status"] == OK), (name, i)
    # the single-phenotype call (the many call bound the context gene: the same handle, the same null fit)
    single = (crms[i].scan_interaction_contexts_joint if joint else crms[i].scan_interaction_contexts)(base.G, fast=fast,
                                                                                                      return_stats=True)
    _, lim1 = _hold(name, i, single, fast, " (single call)")
    pv1, info1 = single
    for key in ("status",) + (("dof", "dropped") if joint else ()):
        assert np.array_equal(info[key], info1[key]), (name, i, key)
    for key in ("rho1", "e2", "g2", "eps2", "gene_null_lml", "gene_null_delta"):
        assert np.array_equal(np.asarray(info[key]), np.asarray(info1[key])), (name, i, key)
    for j in range(base.G.shape[1]):
        got = {key: info[key][j] for key in ("null_lml", "alt_lml", "beta", "beta_se")}
        ref = {key: np.asarray(info1[key][j], lh.LD) for key in ("null_lml", "alt_lml", "beta", "beta_se")}
        gap = jr.errors(got, ref) if joint else cr.errors(got, ref)
        for key, v in gap.items():
            assert v <= lim[key] + lim1[key], (name, i, j, key, v, lim[key], lim1[key])
    if fast:
        assert np.array_equal(info["null_delta"], info1["null_delta"])


def test_the_many_calls_results_have_a_leading_phenotype_axis():
    base, views, crms = _objects(K3)
    P, p, k = len(crms), base.G.shape[1], base.k
    pv, info = _many(K3, True)
    assert pv.shape == (P, p, k) and info["status"].shape == (P, p, k) and info["status"].dtype == np.int32
    assert info["null_lml"].shape == (P, p) and info["gene_null_lml"].shape == (P,)
    for key in ("rho1", "e2", "g2", "eps2"):
        assert info[key].shape == (P,)
    pv, info = _many(K3, True, joint=True)
    assert pv.shape == (P, p) and info["beta"].shape == (P, p, k) and info["dropped"].dtype == bool
    assert info["dof"].shape == (P, p) and info["dof"].dtype == np.int32 and np.all(info["dof"] == k)
    # without return_stats: the keys of the single-phenotype calls
    pv2, info2 = _many_call(False)(crms, base.G)
    assert sorted(info2) == ["beta", "beta_se", "e2", "eps2", "g2", "log_pvalue", "rho1", "status"]
    assert np.array_equal(pv2, _many(K3, True)[0])
    # a panel without variants: the nulls are still fitted and reported
    pv0, info0 = _many_call(False)(crms, np.zeros((base.n, 0)), return_stats=True)
    assert pv0.shape == (P, 0, k) and info0["status"].shape == (P, 0, k) and info0["null_lml"].shape == (P, 0)
    assert np.array_equal(info0["gene_null_lml"], _many(K3, True)[1]["gene_null_lml"])


def test_the_mixed_cohorts_form_several_rho_groups_on_the_device():
    """What the CPU test asserts of the oracle's nulls, here of the device's: a grid point shared by several phenotypes and
    one held by exactly one, in one call."""
    for name in mc.MIXED:
        rho = list(_many(name, True)[1]["rho1"])
        counts = sorted(rho.count(r) for r in set(rho))
        assert len(counts) >= 2 and counts[0] == 1 and counts[-1] >= 2, (name, rho)


# ---- C: independence, bit for bit -----------------------------------------------------------------------------------------------
def _wide_panel(cs, p=150):
    Gd = np.random.default_rng(11).normal(size=(cs.donors, p))
    return Gd, Gd[cs.donor_of_cell]


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name,joint", [(MIXED, False), (MIXED, True), (K3, False)])
def test_a_phenotypes_rows_do_not_depend_on_the_call_around_them(name, joint, fast):
    from cellregmap_amd import GenotypePanel
    from test_gpu_context_blocks import _cut

    base, views, crms = _objects(name)
    call = _many_call(joint)
    P = len(crms)
    Gd, G = _wide_panel(base)
    dense = GenotypePanel(G, groups=None)
    whole = call(crms, dense, fast=fast, return_stats=True)
    assert np.all(whole[1]["status"] == OK)
    # the gene alone, through the multi entry
    for i in (0, P - 1):
        alone = call([crms[i]], dense, fast=fast, return_stats=True)
        _same_rows(_row(alone, 0), _row(whole, i), ("alone", i))
    # the gene order
    order = list(range(P))[::-1]
    order = order[1:] + order[:1]
    shuffled = call([crms[i] for i in order], dense, fast=fast, return_stats=True)
    for at, i in enumerate(order):
        _same_rows(_row(shuffled, at), _row(whole, i), ("order", i))
    # blocks of 128 variants, room for the rotated candidates of 50; the donor-level panel
    with _cut(crms[0], base, block=bc.BLOCK, sub=bc.SUB):
        cut = call(crms, dense, fast=fast, return_stats=True)
        donors = call(crms, GenotypePanel.from_donors(Gd, base.donor_of_cell), fast=fast, return_stats=True)
    for i in range(P):
        _same_rows(_row(cut, i), _row(whole, i), ("blocks", i))
        _same_rows(_row(donors, i), _row(whole, i), ("donors", i))
    # a window (first > 0) against the sliced matrix
    first, count = 37, 101
    window = call(crms, dense, cis_index=[(first, first + count)] * P, fast=fast, return_stats=True)
    part = call(crms, G[:, first:first + count], fast=fast, return_stats=True)
    for i in range(P):
        _same_rows(_entry(window, i), _row(part, i), ("window", i))
        sl = (whole[0][i][first:first + count], {key: whole[1][key][i][first:first + count] for key in FLOAT_EACH + ("status",)})
        _same_rows(sl, _row(part, i), ("slice of the whole", i))


# ---- D: cis walks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True])
def test_a_cis_walk_equals_the_many_call_of_each_phenotype_on_its_columns(joint):
    from cellregmap_amd import GenotypePanel

    base, views, crms = _objects(MIXED)
    call = _many_call(joint)
    P = len(crms)
    _, G = _wide_panel(base, p=60)
    mask = np.zeros(60, bool)
    mask[[3, 4, 5, 30, 31]] = True
    cis = [(0, 25), slice(10, 40), np.array([50, 7, 7, 59, 12, 50]), np.array([], np.int64), mask, (45, 60)][:P]
    assert len(cis) == P and P >= 6
    # [40, 45) is tested by nobody, [55, 59) by phenotype 5 alone; phenotype 3 has no variants
    seen = []
    walk = call(crms, GenotypePanel(G, groups=None), cis_index=cis, fast=True, return_stats=True,
                progress=lambda done, total: seen.append((done, total)))
    assert seen and seen[-1][0] == seen[-1][1] == 55
    pv, info = walk
    assert isinstance(pv, list) and len(pv) == P and info["rho1"].shape == (P,)
    for i in range(P):
        cols = np.arange(60)[cis[i]] if isinstance(cis[i], slice) else (np.arange(*cis[i]) if isinstance(cis[i], tuple)
                                                                         else np.flatnonzero(cis[i]) if cis[i].dtype == bool else cis[i])
        got, want = _entry(walk, i), _row(call([crms[i]], G[:, cols], fast=True, return_stats=True), 0)
        assert got[0].shape == want[0].shape == ((len(cols),) if joint else (len(cols), base.k)), i
        _same_rows(got, want, ("cis", i))
    assert pv[3].shape[0] == 0 and info["status"][3].dtype == np.int32


def test_the_wrappers_bind_the_cohort_and_call_the_scans():
    import cellregmap_amd as crm

    base, views, _ = _objects(K3)
    Y = np.column_stack([v.y for v in views[:3]])
    Ls = crm.get_L_values(base.hK, base.C)
    first = crm.CellRegMap(y=Y[:, 0], E=base.C, W=base.W, E1=base.C, Ls=Ls)
    crms = [first] + [crm.CellRegMap(y=Y[:, i], E=base.C, W=base.W, E1=base.C, Ls=Ls, background=first._bg) for i in (1, 2)]
    for joint, run in ((False, crm.run_interaction_contexts_many), (True, crm.run_interaction_contexts_joint_many)):
        for fast in (True, False):
            pv, info = run(Y, base.C, base.G, W=base.W, hK=base.hK, fast=fast)
            want = _many_call(joint)(crms, base.G, fast=fast)
            assert np.array_equal(pv, want[0]) and sorted(info) == sorted(want[1])
            for key in info:
                assert np.array_equal(info[key], want[1][key], equal_nan=True), key
    pvj, infoj = crm.run_interaction_contexts_joint_many(Y, base.C, base.G, W=base.W, hK=base.hK, cis_index=[(0, 2)] * 3)
    assert isinstance(pvj, list) and pvj[0].shape == (2,) and np.all(infoj["dof"][0] == base.k)


# ---- E: the sharing is real ---------------------------------------------------------------------------------------------------
def _timed(run):
    from cellregmap_amd import _engine, _lib

    lib, ctx = _lib.load(), _engine._context(0)
    _lib.check(lib.crm_kernel_timer_reset(ctx))
    try:
        run()
        ms, launches, flops = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
        _lib.check(lib.crm_kernel_timer_read(ctx, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(flops), None))
    finally:
        _lib.check(lib.crm_kernel_timer_stop(ctx))
    return launches.value, flops.value


@pytest.mark.parametrize("joint", [False, True])
def test_one_contraction_per_rho_group_and_sub_range(joint):
    from cellregmap_amd import GenotypePanel
    from test_gpu_context_blocks import _cut

    base, views, crms = _objects(MIXED)
    call = _many_call(joint)
    P = len(crms)
    _, G = _wide_panel(base)                                      # 150 variants: blocks of 128 + 22, sub-ranges of 50, 50, 28 and 22
    panel = GenotypePanel(G, groups=None)
    subranges = 4
    with _cut(crms[0], base, block=bc.BLOCK, sub=bc.SUB):
        out = {}
        many = _timed(lambda: out.update(r=call(crms, panel, fast=True)))
        rho = list(out["r"][1]["rho1"])
        singles = [_timed(lambda c=c: (c.scan_interaction_contexts_joint if joint else c.scan_interaction_contexts)(panel, fast=True))
                   for c in crms]
    groups = len(set(rho))
    assert 2 <= groups < P, rho
    assert all(n == subranges for n, _ in singles), singles
    assert many[0] == groups * subranges, (many, groups)
    assert sum(n for n, _ in singles) == P * subranges
    # the flops: one single call's per group -- 2 n r(rho*) k per variant, r by the group's grid point
    by_rho = {}
    for r, (_, fl) in zip(rho, singles):
        assert by_rho.setdefault(r, fl) == fl, (r, fl)
    assert many[1] == sum(by_rho.values()), (many, by_rho)
    assert many[1] < sum(fl for _, fl in singles)


# ---- F: misuse ------------------------------------------------------------------------------------------------------------------
def _handles(crms, C, own=True):
    from cellregmap_amd import _engine

    genes = _engine._bind_context_genes(crms, C, own)
    return genes, (ctypes.c_void_p * len(genes))(*[g.value for g in genes])


def _nulls(hs, n):
    from cellregmap_amd import _lib

    null = np.empty((n, 6))
    _lib.check(_lib.load().crm_association_null_multi(hs, n, _lib.ptr(null)))
    return null


def test_misuse_returns_the_error_codes_and_launches_nothing():
    import cellregmap_amd as crm
    from cellregmap_amd import GenotypePanel, _lib

    lib = _lib.load()
    base, views, crms = _objects(K3)
    P = len(crms)
    panel = GenotypePanel(base.G, groups=None)
    genes, hs = _handles(crms, base.C)
    null = _nulls(hs, P)
    # other contexts, other covariates: bound on the same background
    rng = np.random.default_rng(5)
    otherC = crm.CellRegMap(views[1].y, base.C, W=base.W, background=crms[0]._bg, **base.device_kw())
    gC = otherC._bind_context_gene(base.C + 0.01 * rng.normal(size=base.C.shape), False)
    otherW = crm.CellRegMap(views[1].y, base.C, W=base.W + 0.01 * rng.normal(size=base.W.shape), background=crms[0]._bg,
                            **base.device_kw())
    gW = otherW._bind_context_gene(base.C, True)
    seen = []

    def refused(rc, code, text):
        seen.append((rc, code, text, lib.crm_last_error()))

    def misuse():
        for entry, outs in ((lib.crm_scan_interaction_contexts_multi, [None] * 8),
                            (lib.crm_scan_interaction_contexts_joint_multi, [None] * 10)):
            refused(entry(hs, 0, panel.handle, 0, 3, 1, _lib.ptr(null), *outs), -2, b"no genes")
            refused(entry(None, P, panel.handle, 0, 3, 1, _lib.ptr(null), *outs), -2, b"no genes")
            refused(entry(hs, P, panel.handle, 2, 2, 1, _lib.ptr(null), *outs), -2, b"outside the panel")
            refused(entry(hs, P, panel.handle, 0, 3, 1, None, *outs), -2, b"NULL")
            off = null.copy()
            off[1, 0] = 0.55
            refused(entry(hs, P, panel.handle, 0, 3, 1, _lib.ptr(off), *outs), -2, b"not a point of the background's grid")
            off = null.copy()
            off[P - 1, 4] = np.nan
            refused(entry(hs, P, panel.handle, 0, 3, 1, _lib.ptr(off), *outs), -2, b"non-finite lml")
            mixed = (ctypes.c_void_p * 2)(genes[0].value, gC.value)
            refused(entry(mixed, 2, panel.handle, 0, 3, 1, _lib.ptr(null), *outs), -2, b"same contexts C")
            mixed = (ctypes.c_void_p * 2)(genes[0].value, gW.value)
            refused(entry(mixed, 2, panel.handle, 0, 3, 1, _lib.ptr(null), *outs), -2, b"same covariates X0")
            assert entry(hs, P, panel.handle, 1, 0, 1, _lib.ptr(null), *outs) == 0          # count = 0 is no error

    assert _timed(misuse) == (0, 0.0)                                # no contraction was launched
    assert len(seen) == 16
    for rc, code, text, message in seen:
        assert rc == code and text in message, (rc, code, text, message)
    # every output may be NULL on a call that runs
    assert lib.crm_scan_interaction_contexts_multi(hs, P, panel.handle, 0, 3, 1, _lib.ptr(null), *[None] * 8) == 0
    assert lib.crm_scan_interaction_contexts_joint_multi(hs, P, panel.handle, 0, 3, 0, _lib.ptr(null), *[None] * 10) == 0
    # the Python calls check the cohort before anything is bound
    with pytest.raises(ValueError, match="no phenotypes"):
        crm.scan_interaction_contexts_many([], base.G)
    with pytest.raises(ValueError, match="share one background"):
        crm.scan_interaction_contexts_many([crms[0], lh._device(mc.cohort(MIXED)[0])], base.G)
    with pytest.raises(ValueError, match="cis_index has"):
        crm.scan_interaction_contexts_joint_many(crms, base.G, cis_index=[(0, 1)])


def test_the_joint_entry_refuses_more_than_64_contexts():
    import cellregmap_amd as crm
    from cellregmap_amd import GenotypePanel, _lib

    lib = _lib.load()
    base, views, crms = _objects(K3)
    C = np.random.default_rng(9).normal(size=(base.n, 65))
    two = [crm.CellRegMap(v.y, v.C, W=v.W, background=crms[0]._bg, **v.device_kw()) for v in views[:2]]
    genes, hs = _handles(two, C, own=False)
    null = _nulls(hs, 2)
    panel = GenotypePanel(base.G, groups=None)
    got = {}
    launches = _timed(lambda: got.update(rc=lib.crm_scan_interaction_contexts_joint_multi(hs, 2, panel.handle, 0, 3, 1, _lib.ptr(null),
                                                                                          *[None] * 10)))
    assert got["rc"] == -3 and b"65 contexts" in lib.crm_last_error(), (got, lib.crm_last_error())
    assert launches == (0, 0.0)
    with pytest.raises(_lib.CrmError, match="65 contexts"):
        crm.scan_interaction_contexts_joint_many(two, base.G, contexts=C)
    # the per-context entry serves them
    pv, info = crm.scan_interaction_contexts_many(two, base.G, contexts=C)
    assert pv.shape == (2, base.G.shape[1], 65) and np.all(np.isfinite(pv))


def test_a_scan_from_a_progress_callback_is_refused():
    import cellregmap_amd as crm
    from cellregmap_amd import GenotypePanel, _lib

    lib = _lib.load()
    base, views, crms = _objects(K3)
    P = len(crms)
    panel = GenotypePanel(base.G, groups=None)
    genes, hs = _handles(crms, base.C)
    null = _nulls(hs, P)
    seen = []

    def nested(done, total):
        for entry, outs in ((lib.crm_scan_interaction_contexts_multi, [None] * 8),
                            (lib.crm_scan_interaction_contexts_joint_multi, [None] * 10)):
            seen.append((entry(hs, P, panel.handle, 0, 3, 1, _lib.ptr(null), *outs), lib.crm_last_error()))

    for call in (crm.scan_interaction_contexts_many, crm.scan_interaction_contexts_joint_many):
        call(crms, panel, progress=nested)
    assert len(seen) == 4
    for rc, message in seen:
        assert rc == -3 and b"another scan is running" in message, (rc, message)
    pv, _ = crm.scan_interaction_contexts_many(crms, base.G)          # ... and the context is usable afterwards
    assert np.array_equal(pv, _many(K3, True)[0])
