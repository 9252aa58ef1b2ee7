"""Does this build compute what another build of the library computes, bit for bit?  Runs the verbatim scans of a fuzz
stream under the other library (a path, or CRM_OTHER_LIB: e.g. the parent commit built in a `git worktree` of it) and
under the current one, each in its own fresh process, and compares p, rho*, Q, lml, delta and scale entry by entry and
the context's route counters after the last scan.  --forms switches kernel forms (crm_test_set_form) in both processes,
so that the routes the cost models leave to large cohorts are compared too (with CRM_KIN_ROUTE=2 in the environment the
kinship-structure route is taken wherever a background knows its donors); the counters say whether they were reached.
Behind the stream come a few cohorts whose kinship term carries the scan's own contexts, Ls = get_L_values(hK, E): the
stream's mode C hands its Ls over as dense matrices, so nothing in it can reach the pair-product forms.  Then the smallest
cohorts that reach every instantiation of the score statistic's Gram (GRAM_COHORTS): the stream stops at 144 rows and 128
contexts, so the staged kernel's grouped form is in nothing before them.
Last come the cohorts of tests/pinned_cases.py, which sit on the boundaries between the null-fit kernels that the stream
never leaves the first of: the whole trial table of crm_test_null_fit_probe(on = 2) -- lml, delta, scale, nfev and use_g
of every (variant, grid point), and the selected index -- of every null-model cohort, once from the plain scan and once
from the call that asks for model flags, and what estimate_betas_many returns on the pairs held of every effects cohort.
After them the association LRTs and the fixed-effect context tests (lrt_tables): every output array of the single-gene and
many-gene entries, with and without effect sizes, each and joint, fast and full refit, on the cohorts of
tests/pinned_cases.py (ASSOCIATION), tests/context_block_cases.py (blocks of 128 and sub-ranges of 50 variants) and
tests/context_many_cases.py (MIXED: several rho groups), on dense and donor-level panels, through a cis walk, from
first > 0 and with count = 0.
These are compared as 64-bit patterns.
Exit status 0: every array and every counter identical.
    python tools/diag/compare_builds.py <other library> [count 150] [seed 2026] [--forms name=value[,name=value...]]
    python tools/diag/compare_builds.py --child <lib or ''> <count> <seed> <out.npz> <forms or ''>"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ARRAYS = ("pv", "rho1", "Q", "lml", "delta", "scale")
COUNTERS = ("crm_test_unrelated_donor_blocks", "crm_test_donor_pair_blocks", "crm_test_gram_dma_launches",
            "crm_test_tail_launches", "crm_test_spectrum_tail_launches", "crm_test_rotation_tail_launches",
            "crm_test_rho0_position_blocks", "crm_test_tests_without_pair", "crm_test_dense_repeats")
# reported beside them, not compared: a form that one build has and the other lacks (how many blocks of the stream it served)
REPORTED = ("crm_test_wb_gram_fused_blocks", "crm_test_side_stream_blocks")
# donors, cells per donor, contexts, variants (the last one: 67 Gram rows on the unrelated-donor route, the fused Gram's range)
STRUCTURED = ((6, 120, 7, 37), (12, 90, 20, 130), (7, 60, 5, 37), (4, 70, 32, 10))
# The Gram of the score statistic (gram_ext.hip, wb_gram_fused.hip) at every template instance, on the shapes of the tests that
# hold its forms to each other: (mode, donors, cells per donor, contexts, covariates or None for the cohort's own, variants,
# cohort seed).
#   "B"  hK alone, tests/test_gpu_edges.py::test_gram_kernel_forms_agree: 1, 3 and 4 tile rows of 16 -- gram_ext_dma_kernel<2> and
#        <4> (gram_staged=1: gram_ext_kernel<2> and <4>)
#   "C"  ragged donors and Ls = get_L_values(hK, E), the first row of each tile-row count of tests/test_gpu_gram_wide.py: 2 k0 + c + 2
#        rows, 5 to 9 tile rows, on the unrelated-donor route (CRM_KIN_ROUTE=2 with kin_fold=2, kin_diag=2, donor_pairs=2), and
#        its rows of 96 and 99 rows, whose even context counts the fused Gram serves: gram_ext_dma_wide_kernel<5, 6, 7, 9> and
#        wb_gram_fused_kernel<6, 7, 8> (<5>: the last cohort of STRUCTURED); wb_gram_fused=0: the wide kernel throughout;
#        gram_strips=0: their round-robin instances; gram_staged=1: gram_ext_kernel<6>, <7>, <9>.  k0 + c + 2 rows on the other routes
#   "A"  no kinship term, tests/test_gpu_edges.py::test_interaction_scan_with_many_contexts: 162, 232 and 253 rows --
#        gram_ext_kernel<12, 2>, <15, 4> and <18, 4>
GRAM_COHORTS = (("B", 8, 30, 5, None, 40, 17), ("B", 6, 40, 37, None, 24, 17), ("B", 10, 20, 60, None, 12, 17),
                ("C", 5, 70, 31, 1, 13, 965), ("C", 5, 80, 39, 1, 11, 981), ("C", 4, 100, 47, 1, 10, 997), ("C", 4, 120, 54, 3, 9, 1013),
                ("C", 4, 150, 63, 1, 7, 1029), ("C", 4, 100, 46, 2, 9, 996), ("C", 4, 100, 48, 1, 9, 999),
                ("A", 8, 100, 100, 60, 5, 141), ("A", 8, 100, 160, 70, 5, 201), ("A", 8, 100, 250, 1, 5, 291))


def gram_cohort(mode, donors, cells, k0, c, variants, seed):
    """(y, E, W, G, keywords of CellRegMap) of one row of GRAM_COHORTS, built as its test builds it."""
    from test_gpu_gram_wide import _covariates
    from test_gpu_unrelated_donors import _ragged

    from cellregmap_amd import get_L_values
    from cellregmap_amd.synth import make_cohort

    if mode == "C":
        co, keep, G = _ragged(donors, cells, k0, variants, seed)
        y, E, hK = co.y[keep], co.E[keep], co.hK[keep]
        return y, E, _covariates(y.size, c, 2 * k0 + c + 2), G, {"Ls": get_L_values(hK, E)}
    co = make_cohort(donors, cells, k0, variants, seed=seed)
    if mode == "B":
        return co.y, co.E, co.W, co.G, {"hK": co.hK}
    W = np.concatenate([co.W, np.random.default_rng(k0 + c).normal(size=(co.y.size, c - 1))], axis=1) if c > 1 else co.W
    return co.y, co.E, W, co.G, {}


def parse_forms(text):
    return [(name, int(value)) for name, value in (item.split("=") for item in text.split(",") if item)]


def child(lib_path, count, seed, out, forms):
    from cellregmap_amd import _lib

    if lib_path:
        _lib.LIB_PATH = lib_path
        probe = ctypes.CDLL(lib_path)     # (an older build lacks the entry points added since: bind what it has)
        for name in [k for k in _lib.SIGNATURES if not hasattr(probe, k)]:
            del _lib.SIGNATURES[name]
    lib = _lib.load()
    # before any CellRegMap exists: some forms are read when the kinship structure is announced
    applied = [name for name, value in parse_forms(forms) if lib.crm_test_set_form(name.encode(), value, 0) == 0]
    from fuzz_cases import build_case, fuzz_cases

    from cellregmap_amd import CellRegMap, GenotypePanel, _engine, get_L_values
    from cellregmap_amd.synth import make_cohort

    keep = {k: [] for k in ARRAYS}

    def scan(crm, G, groups, **hooks):
        pv, info, st = crm.scan_interaction(GenotypePanel(G, groups=groups), return_stats=True, **hooks)
        keep["pv"].append(pv)
        keep["rho1"].append(info["rho1"])
        for k in ("Q", "lml", "delta", "scale"):
            keep[k].append(st[k])

    for case in fuzz_cases(count, seed=seed, wide_covariates=True):
        y, E, W, G, kw, hooks = build_case(case)
        crm = CellRegMap(y, E, W=W, **kw)
        for groups in (None, "auto"):
            scan(crm, G, groups, **hooks)
    for donors, cells, k0, variants in STRUCTURED:
        c = make_cohort(donors, cells, k0, variants, seed=300 + k0)
        G = c.G + 0.05 * np.random.default_rng(k0).normal(size=c.G.shape)     # (general genotypes: the dense path)
        scan(CellRegMap(c.y, c.E, W=c.W, Ls=get_L_values(c.hK, c.E)), G, None)
    for row in GRAM_COHORTS:
        y, E, W, G, kw = gram_cohort(*row)
        scan(CellRegMap(y, E, W=W, **kw), G, None)
    pinned = pinned_tables(lib, _engine._context(0))
    pinned.update(lrt_tables(lib, _engine._context(0)))
    ctx, counters = _engine._context(0), {}
    for name in COUNTERS + REPORTED:
        if name not in _lib.SIGNATURES:
            counters[name] = None             # (this library does not export it)
        elif _lib.SIGNATURES[name][0] is ctypes.c_long:
            counters[name] = int(getattr(lib, name)(ctx))
        else:
            value = ctypes.c_long(-1)
            _lib.check(getattr(lib, name)(ctx, ctypes.byref(value)))
            counters[name] = value.value
    np.savez(out, notes=np.array(json.dumps({"counters": counters, "forms": applied})),
             **{k: np.concatenate(v) for k, v in keep.items()}, **pinned)


def pinned_tables(lib, ctx):
    """{"pinned <cohort>, <what>": float64 array} over the cohorts of tests/pinned_cases.py."""
    import pinned_cases as pc

    import cellregmap_amd as crm
    from cellregmap_amd import _lib

    out = {}
    for name in pc.NULL_MODEL:
        cs = pc.NullModelCase(name)
        kw = {"A": {}, "B": {"hK": cs.hK}, "C": {"Ls": crm.get_L_values(cs.hK, cs.E)}}[cs.mode]
        obj = crm.CellRegMap(cs.y, cs.E, W=cs.W, **kw)
        panel = crm.GenotypePanel(cs.G, groups="auto" if cs.path == "collapsed" else None)
        for what in ("plain", "model flags"):
            buf = np.full(cs.G.shape[1] * (5 * len(cs.grid) + 1), np.nan)
            _lib.check(lib.crm_test_null_fit_probe(ctx, 2, 0.0))
            try:
                if what == "plain":
                    obj.scan_interaction(panel, progress=False)
                else:
                    obj.scan_interaction_info(panel)
                got = lib.crm_test_null_fit_probe_read(ctx, _lib.ptr(buf), buf.size)
            finally:
                _lib.check(lib.crm_test_null_fit_probe(ctx, 0, 0.0))
            assert got == buf.size, (name, what, got, buf.size)
            out["pinned %s, %s" % (name, what)] = buf
    for name, pairs in pc.EFFECTS_HELD.items():
        cs = pc.EffectsCase(name)
        bg, bgxe, info = crm.estimate_betas_many(cs.Y, cs.W, cs.E0, cs.G, maf=cs.maf, E2=cs.E2, hK=None if cs.E2 is None else cs.hK,
                                                 pairs=np.asarray(pairs), return_info=True)
        out["pinned effects %s, beta_g" % name], out["pinned effects %s, beta_gxe" % name] = np.asarray(bg, float), np.asarray(bgxe, float)
        for key in sorted(info):
            value = np.asarray(info[key])
            if value.dtype.kind in "fiu":
                out["pinned effects %s, %s" % (name, key)] = value.astype(float)
    return out


def lrt_tables(lib, ctx):
    """{"lrt <cohort>, <call>": float64 array} over the association and context scans' entries (ints go over exactly)."""
    import context_block_cases as bc
    import context_many_cases as mc
    import pinned_cases as pc

    import cellregmap_amd as crm
    from cellregmap_amd import GenotypePanel, _engine, _lib

    out = {}

    def keep(tag, pv, info, st=None):
        tables = {"pv": pv, **info, **(st or {})}
        for key in sorted(tables):
            parts = tables[key] if isinstance(tables[key], list) else [tables[key]]
            if all(np.asarray(x).dtype.kind in "fiub" for x in parts):
                out["lrt %s, %s" % (tag, key)] = np.concatenate([np.asarray(x, float).ravel() for x in parts] + [np.empty(0)])

    def donors_of(cs):     # a donor-level copy of the cohort's panel: every cell carries its donor's first cell's genotypes
        rows = np.array([np.flatnonzero(cs.donor_of_cell == d)[0] for d in range(cs.donors)])
        return cs.G[rows][cs.donor_of_cell]

    def windows(p, ng):    # phenotype 0: the whole panel; the others: stretches inside it (runs with a strict subset, first > 0)
        return [(0, p)] + [(min(p - 1, 1 + 2 * i), max(min(p - 1, 1 + 2 * i) + 1, p - i)) for i in range(1, ng)]

    def direct(tag, entry, head, spec, p):
        """The C entry itself on a stretch inside the panel and on no variants: ``head(first, count)`` its leading arguments,
        ``spec`` its outputs in order as (name, dtype, per variant?, values per row: 1, k or 6 for the null row)."""
        rows = head(0, 0)[1] if isinstance(head(0, 0)[0], ctypes.Array) else 1
        for first, count in ((1, p - 1), (p // 2, 0)):
            bufs = [np.full((rows, count * width) if each else (rows, width), -7 if dtype is np.int32 else np.nan, dtype)
                    for _, dtype, each, width in spec]
            _lib.check(entry(*head(first, count), *[_lib.ptr(b) for b in bufs]))
            for (what, _, _, _), b in zip(spec, bufs):
                out["lrt %s, from %d, %d variants, %s" % (tag, first, count, what)] = b.astype(float).ravel()

    F, I = float, np.int32
    ASSOC = [("pv", F, True, 1), ("alt_lml", F, True, 1)]
    EFFECTS = [(w, F, True, 1) for w in ("beta", "se", "delta", "scale", "logp")] + [("effect_status", I, True, 1)]

    def context_spec(joint, k, single):
        each = [("pv", F, True, k), ("alt_lml", F, True, k), ("beta", F, True, k), ("beta_se", F, True, k), ("logp", F, True, k),
                ("status", I, True, k)]
        jnt = [("pv", F, True, 1), ("logp", F, True, 1), ("alt_lml", F, True, 1), ("dof", I, True, 1), ("beta", F, True, k),
               ("beta_se", F, True, k), ("dropped", I, True, k), ("status", I, True, 1)]
        return (jnt if joint else each) + [("null_lml", F, True, 1), ("null_delta", F, True, 1)] + ([("null", F, False, 6)] if single else [])

    for name in pc.ASSOCIATION:
        cs = pc.AssociationCase(name, variants=7)
        kw = {} if cs.hK is None else {"hK": cs.hK}
        objs = [crm.CellRegMap(cs.y, cs.E, W=cs.W, E1=cs.E1, **kw)]
        objs += [crm.CellRegMap(cs.y + 0.2 * i * cs.G[:, i], cs.E, W=cs.W, E1=cs.E1, background=objs[0]._bg, **kw) for i in (1, 2)]
        for kind, G in (("dense", GenotypePanel(cs.G, groups=None)), ("donors", GenotypePanel(donors_of(cs), groups="auto"))):
            for fast in (0, 1):
                tag = "%s, %s, fast %d" % (name, kind, fast)
                scan = objs[0].scan_association_fast if fast else objs[0].scan_association
                keep(tag + ", single", *scan(G, return_stats=True, progress=False))
                keep(tag + ", single effects", *scan(G, return_stats=True, progress=False, effects=True))
                keep(tag + ", many", *crm.scan_association_many(objs, G, fast=bool(fast), return_stats=True))
                keep(tag + ", many effects", *crm.scan_association_many(objs, G, fast=bool(fast), return_stats="effects"))
                keep(tag + ", many effects cis", *crm.scan_association_many(objs, G, cis_index=windows(7, 3), fast=bool(fast),
                                                                           return_stats="effects"))
                gene = objs[0]._bind_gene()
                hs = (ctypes.c_void_p * 3)(*[o._bind_gene(like=objs[0]).value for o in objs])
                null = np.empty((3, 6))
                _lib.check(lib.crm_association_null_multi(hs, 3, _lib.ptr(null)))
                one = lambda first, count: (gene, G.handle, first, count, fast)
                many = lambda first, count: (hs, 3, G.handle, first, count, fast, _lib.ptr(null))
                direct(tag + ", single", lib.crm_scan_association, one, ASSOC + [("null", F, False, 6)], 7)
                direct(tag + ", single effects", lib.crm_scan_association_effects, one, ASSOC + [("null", F, False, 6)] + EFFECTS, 7)
                direct(tag + ", multi", lib.crm_scan_association_multi, many, ASSOC, 7)
                direct(tag + ", multi effects", lib.crm_scan_association_multi_effects, many, ASSOC + EFFECTS, 7)

    def cut(obj, cs, on):
        ldq = -(-max(obj._bg.rank(i) for i in range(len(cs.grid))) // 128) * 128
        _lib.check(lib.crm_set_block_variants(ctx, bc.BLOCK if on else 0))
        _lib.check(lib.crm_test_set_context_budget(ctx, bc.SUB * 8 * cs.k * ldq + 8 if on else 0))

    for name in bc.CASES:     # several blocks with a ragged tail, several sub-ranges per block; the joint cohorts: V in LDS and in global memory
        cs = bc.case(name)
        obj = crm.CellRegMap(cs.y, cs.C, W=cs.W, **cs.device_kw())
        panels = [("dense", GenotypePanel(cs.G, groups=None))]
        if name == bc.DOSAGES:
            panels.append(("donors", GenotypePanel.from_dosages(cs.D, cs.donor_of_cell, standardize=False)))
        cut(obj, cs, True)
        try:
            for kind, G in panels:
                for fast in (False, True):
                    for call in (("joint",) if bc.CASES[name][2] == "joint" else ("each", "joint")):
                        scan = obj.scan_interaction_contexts_joint if call == "joint" else obj.scan_interaction_contexts
                        keep("blocks %s, %s, %s, fast %d" % (name, kind, call, fast), *scan(G, fast=fast, return_stats=True))
        finally:
            cut(obj, cs, False)

    for name in mc.MIXED + ("k 48, c 128, mode B",):     # three or more phenotypes on several rho groups; the WIDE joint cohort
        base, views = mc.cohort(name)
        first = crm.CellRegMap(views[0].y, views[0].C, W=views[0].W, **views[0].device_kw())
        objs = [first] + [crm.CellRegMap(v.y, v.C, W=v.W, background=first._bg, **v.device_kw()) for v in views[1:]]
        p = base.G.shape[1]
        for kind, G in (("dense", GenotypePanel(base.G, groups=None)), ("donors", GenotypePanel(donors_of(base), groups="auto"))):
            for fast in (False, True):
                for joint in ((True,) if mc.is_joint(name) else (False, True)):
                    many = crm.scan_interaction_contexts_joint_many if joint else crm.scan_interaction_contexts_many
                    tag = "many %s, %s, joint %d, fast %d" % (name, kind, joint, fast)
                    try:
                        keep(tag, *many(objs, G, fast=fast, return_stats=True))
                        keep(tag + ", cis", *many(objs, G, cis_index=windows(p, len(objs)), fast=fast, return_stats=True))
                        genes = _engine._bind_context_genes(objs, base.C, True)
                        hs = (ctypes.c_void_p * len(genes))(*[g.value for g in genes])
                        null = np.empty((len(genes), 6))
                        _lib.check(lib.crm_association_null_multi(hs, len(genes), _lib.ptr(null)))
                        direct(tag + ", single", lib.crm_scan_interaction_contexts_joint if joint else lib.crm_scan_interaction_contexts,
                               lambda first, count: (genes[0], G.handle, first, count, int(fast)), context_spec(joint, base.k, True), p)
                        direct(tag + ", multi",
                               lib.crm_scan_interaction_contexts_joint_multi if joint else lib.crm_scan_interaction_contexts_multi,
                               lambda first, count: (hs, len(genes), G.handle, first, count, int(fast), _lib.ptr(null)),
                               context_spec(joint, base.k, False), p)
                    except _lib.CrmError as err:     # (a shape the joint test refuses: the refusal is the table)
                        out["lrt %s, refused" % tag] = np.frombuffer(str(err).encode().ljust(256)[:256], np.float64).copy()
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6])
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other", nargs="?", default=os.environ.get("CRM_OTHER_LIB"), help="the other build's libcrm_hip.so (or CRM_OTHER_LIB)")
    ap.add_argument("count", nargs="?", type=int, default=150)
    ap.add_argument("seed", nargs="?", type=int, default=2026)
    ap.add_argument("--forms", default="", help="kernel forms for both processes: name=value[,name=value...]")
    args = ap.parse_args()
    if not args.other or not os.path.exists(args.other):
        ap.error("the other library: give its path or set CRM_OTHER_LIB (got %r)" % (args.other,))
    parse_forms(args.forms)     # (a malformed list fails here, not in the children)
    other, this = os.path.abspath(args.other), os.environ.get("CRM_THIS_LIB", "")     # (this: a diagnostic build instead of the package's own library)
    outs = []
    for tag, lib in (("other", other), ("this", this)):
        out = os.path.join("/tmp", "compare_builds_%s_%d.npz" % (tag, os.getpid()))
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, str(args.count), str(args.seed), out, args.forms])
        outs.append(np.load(out))
    a, b = outs
    na, nb = json.loads(str(a["notes"])), json.loads(str(b["notes"]))
    rep = {"other_library": args.other, "this_library": this or "cellregmap_amd/libcrm_hip.so", "problems": args.count, "seed": args.seed, "structured_cohorts": len(STRUCTURED), "gram_cohorts": len(GRAM_COHORTS),
           "CRM_KIN_ROUTE": os.environ.get("CRM_KIN_ROUTE"), "forms": args.forms, "forms_applied": {"other": na["forms"], "this": nb["forms"]}, "variant_scans": int(a["pv"].size)}
    for k in ARRAYS:
        same = (a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))
        rep[k] = {"identical": int(same.sum()), "different": int((~same).sum()),
                  "worst_rel_difference": float(np.nanmax(np.abs(a[k] - b[k]) / np.maximum(np.abs(a[k]), 1e-300))) if (~same).any() else 0.0}
    names = sorted(k for k in a.files if k.startswith(("pinned ", "lrt ")))
    same = {k: k in b.files and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in names}
    rep["pinned"] = {"tables": len(names), "values": int(sum(a[k].size for k in names)), "identical_tables": int(sum(same.values())),
                     "different": [k for k in names if not same[k]], "tables_match": names == sorted(k for k in b.files if k.startswith(("pinned ", "lrt "))),
                     "lrt_tables": int(sum(k.startswith("lrt ") for k in names)), "lrt_values": int(sum(a[k].size for k in names if k.startswith("lrt ")))}
    rep["counters"] = {name[len("crm_test_"):]: {"other": na["counters"][name], "this": nb["counters"][name]} for name in COUNTERS}
    rep["reported"] = {name[len("crm_test_"):]: {"other": na["counters"].get(name), "this": nb["counters"].get(name)} for name in REPORTED}
    rep["counters_identical"] = all(v["other"] is not None and v["other"] == v["this"] for v in rep["counters"].values())
    print(json.dumps(rep, indent=1))
    dest = os.path.join(ROOT, "gpurun_out")
    os.makedirs(dest, exist_ok=True)
    tag = os.path.basename(this).replace("libcrm_hip_", "").replace(".so", "") if this else "package"
    if args.forms:
        tag += "_" + args.forms.replace("=", "-").replace(",", "_")
    with open(os.path.join(dest, "compare_builds_seed%d_%s.json" % (args.seed, tag)), "w") as fh:
        json.dump(rep, fh, indent=1)
    pinned_ok = names and not rep["pinned"]["different"] and rep["pinned"]["tables_match"]
    return 0 if rep["counters_identical"] and pinned_ok and all(rep[k]["different"] == 0 for k in ARRAYS) else 1


if __name__ == "__main__":
    sys.exit(main())
