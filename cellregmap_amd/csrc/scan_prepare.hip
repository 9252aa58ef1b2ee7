// Per-pass preparation of a scan (scan_pass.h: ScanPass): workspaces, context features, the kinship routes' operands and probes.
#include "scan_pass.h"

namespace crm {

// Records of one product per donor over the donor's own run of cells (kin_row0 / kin_len): the operands X, E and Y of p
// start at the run's first row, C at d c_step.  Returns the longest run (the launch's contraction length).
long donor_run_records(const crm_background* bg, const GemmProblem& p, long c_step, GemmProblem* out) {
    long maxlen = GEMM_BK;
    for (long d = 0; d < bg->kin_groups; d++) {
        const long r0 = bg->kin_row0[d];
        GemmProblem q = p;
        q.X = p.X + r0 * p.ldx;
        if (p.E) q.E = p.E + r0 * p.lde;
        q.Y = p.Y + r0 * p.ldy; q.C = p.C + d * c_step; q.cells = bg->kin_len[d];
        maxlen = std::max(maxlen, bg->kin_len[d]);
        out[d] = q;
    }
    return maxlen;
}

// Records of the unrelated-donor form's per-donor rotation by U_d Lambda_d^-1/2 (wb_U) over the donor's k2pad rows: X of
// donor d at p.X + d x_step, its k2 output columns at column d k2 of p.C
void woodbury_records(const crm_background* bg, const GemmProblem& p, long x_step, GemmProblem* out) {
    for (long d = 0; d < bg->kin_groups; d++) {
        GemmProblem q = p;
        q.X = p.X + d * x_step; q.Y = bg->wb_U.as<double>() + (size_t)d * bg->wb_k2pad * 128; q.ldy = 128;
        q.C = p.C + d * bg->kin_k2; q.N = bg->kin_k2; q.cells = bg->wb_k2pad;
        out[d] = q;
    }
}

// Does every pair of operands hold the same first k columns?  (the probes of the pair-product forms; one flag for all)
int same_columns(hipStream_t st, int* d_flag, int k, std::initializer_list<SameColumns> pairs, bool& same) {
    int h_flag = 0;
    CRM_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    for (const SameColumns& q : pairs) CRM_TRY(launch_same_columns(st, q.A, q.lda, q.B, q.ldb, q.rows, k, d_flag));
    CRM_HIP(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    same = h_flag == 0;
    return CRM_OK;
}

// ---- workspaces -----------------------------------------------------------------------------------------------------
int ScanPass::workspaces() {
    const int BLK = P.BLK, max_pairs = P.pair_cap;
    const long ldb = P.ldb;
    CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)nrho * BLK * P.ldT));
    // (unrelated-donor form: the rotated S stays in block order for several phenotypes -- BLK of them at most)
    // (not where the pass's Grams come straight from the pair products, wb_gram_fused.hip: the rotated S is not formed at
    // all; a block that the fused launch does not serve after all asks for the buffer itself, scan_pairs.hip)
    if (!may_fuse_gram()) CRM_TRY(ctx->ws_A.ensure(ws_A_bytes()));
    CRM_TRY(ctx->ws_Anone.ensure(sizeof(double) * (size_t)P.ldAw));
    CRM_HIP(hipMemsetAsync(ctx->ws_Anone.ptr, 0, sizeof(double) * (size_t)P.ldAw, st));
    // (the aligned copy: not where every block of the pass is read in place, scan_block.hip: copy_block)
    bool copies = false, fused = false;
    for (long done = 0; done < count; done += BLK)
        (fused_block(first + done, (int)std::min<long>(BLK, count - done)) ? fused : copies) = true;
    if (copies) CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
    if (fused && P.kin() && (ng > 1 || P.wb_block))   // (the fused pass's donor-order test direction, beside ws_Gk's Gx)
        CRM_TRY(ctx->ws_Gkt.ensure(sizeof(double) * (size_t)bg->kin_rows * ldb));
    CRM_TRY(ctx->ws_Gs.ensure(sizeof(double) * (size_t)np * P.ldp));
    CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)np * ldb));
    if (idx_G)   // (unused when the scan ends up on the collapsed path)
        CRM_TRY(ctx->ws_Gt.ensure(sizeof(double) * (size_t)np * ldb));
    z1_sz = (long)BLK * P.ldZ1, z2_sz = (long)BLK * P.ldZ2, z3_sz = (long)BLK * P.ldZ3;
    const long z1_all = z1_sz * P.ks1 * ng;
    CRM_TRY(ctx->ws_Z.ensure(sizeof(double) * (size_t)(z1_all + z2_sz * P.ks2 + z3_sz * P.ks3)));
    dZ1 = ctx->ws_Z.as<double>();
    dZ2 = dZ1 + z1_all;
    dZ3 = dZ2 + z2_sz * P.ks2;
    if (bg->fast_T) {
        CRM_TRY(ctx->ws_TH.ensure(sizeof(double) * (size_t)P.th_slab * P.ks_h));
        // The rows of the first slab that no launch of the route writes meet zero rows of the mixing matrices (the padding of
        // the contraction length; the unrelated-donor form's stage past the last donor) and must be zeros.  Every launch
        // that writes ws_TH (fold_TH, unfolded_TH, plain_TH) writes the same rows for every block of every call with the same
        // background, route and shapes, so those rows stay as the clear left them: it runs when the buffer is new and when
        // any of these changes, not on every call.
        const crm_ctx::ThKey th_key{ctx->ws_TH.serial, bg->kin_gen, (int)P.route, P.ks_h, P.ldb, P.th_slab};
        if (!(ctx->th_key == th_key)) {
            CRM_HIP(hipMemsetAsync(ctx->ws_TH.ptr, 0, sizeof(double) * (size_t)P.th_slab, st));
            ctx->th_key = th_key;
        }
    }
    CRM_TRY(ctx->ws_F.ensure(sizeof(double) * (size_t)BLK * k0 * k0));
    CRM_TRY(ctx->ws_Gext.ensure(sizeof(double) * (size_t)BLK * P.KT * P.KT));
    // the null fits' scratch with more than CRM_MAX_COV_WIDE covariate columns; the slower per-variant kernels take it
    // over once the null fits of a block are done
    if (c > CRM_MAX_COV_WIDE || P.slow_forms) {
        size_t xw = c > CRM_MAX_COV_WIDE ? nullfit_xwide_scratch_doubles(BLK, nrho, c) : 0;
        if (P.slow_forms) xw = std::max(xw, std::max(assemble_rows_scratch_doubles(BLK, k0, c), eig_scratch_doubles(BLK, k0)));
        CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * xw));
    }
    // ws_small: the block's vectors, each from a 256-byte boundary (a first pass over the list sizes it)
    const size_t stats_ws = variant_stats_workspace(BLK, std::min(c, CRM_MAX_COV));
    auto carve_small = [&](char* base) {
        size_t off = 0;
        auto carve = [&](auto*& ptr, size_t bytes) {
            ptr = base ? reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + off) : nullptr;
            off += (bytes + 255) / 256 * 256;
        };
        carve(d_gg, sizeof(double) * BLK), carve(d_gy, sizeof(double) * BLK * ng);   // (d_gy, d_fit, d_pos: [ng][BLK])
        carve(d_gW, sizeof(double) * BLK * P.ld_gW), carve(d_trial, sizeof(NullFitTrial) * BLK * nrho);
        carve(d_fit, sizeof(NullFitOut) * BLK * ng), carve(d_pos, sizeof(int) * BLK * ng), carve(d_ord, sizeof(int) * max_pairs);
        carve(d_Q, sizeof(double) * BLK), carve(d_pv, sizeof(double) * BLK), carve(d_lam, sizeof(double) * BLK * k0);
        carve(d_if, sizeof(int) * BLK), carve(d_liu, sizeof(double) * BLK), carve(d_part, stats_ws);
        carve(d_queue, sizeof(unsigned) * CRM_MAX_RHO);    // work queue of the null fits (one counter per grid point)
        carve(d_coef, sizeof(double) * (size_t)c * ldb);   // [c][ldb] projection coefficients of the block onto W
        carve(d_thr, sizeof(double) * BLK);                // the reference's rank rule as a bound on |gx|^2
        carve(d_drop, sizeof(int) * BLK);                  // 1: the variant's direction is dropped from [W, g]
        carve(d_near, sizeof(int) * BLK);   // collapsed path: 1 = repeat this variant on the dense path (also the probes' flag)
        carve(d_posw, sizeof(int) * BLK * ng);             // unrelated-donor form, several phenotypes: block position or -1
        carve(d_tp, sizeof(double) * BLK), carve(d_tlp, sizeof(double) * BLK), carve(d_tst, sizeof(int) * BLK);   // exact tail method
        return off;
    };
    CRM_TRY(ctx->ws_small.ensure(carve_small(nullptr)));
    carve_small(ctx->ws_small.as<char>());
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (P.z1_slot() + ng)));
    d_probs = ctx->ws_probs.as<GemmProblem>();
    if (!P.collapsed()) {   // the block in the fixed effects' own basis, and its product with the test direction
        CRM_TRY(ctx->ws_Gx.ensure(sizeof(double) * (size_t)np * ldb));
        CRM_TRY(ctx->ws_GG.ensure(sizeof(double) * (size_t)np * ldb));
    }
    if (P.through_H()) {   // operands of the routes through H (step 6)
        if (P.folded()) {
            // (scratch of the sliced all-cells launch for the E1 rows)
            CRM_TRY(ctx->ws_AH.ensure(sizeof(double) * (size_t)P.fold_split6 *
                                      (P.e1_pairs ? (size_t)(std::max<long>(BLK, max_pairs) + 128) * P.ldP : (size_t)bg->kin_k1 * P.ld_ah)));
        } else {
            CRM_TRY(ctx->ws_AH.ensure(sizeof(double) * (size_t)bg->ldh * P.ld_ah));
            // (zeroed by prepare_kinship, once the form of the per-donor sums is known: all of it, or its padding rows alone)
        }
        if (ng > 1) CRM_TRY(ctx->ws_XG.ensure(sizeof(double) * (size_t)P.kdim * P.ld_xg));
    }
    const long KK = P.KK;
    if (P.folded()) {
        CRM_TRY(ctx->ws_S.ensure(P.s_bytes));
        CRM_TRY(ctx->ws_Gk.ensure(sizeof(double) * (size_t)bg->kin_rows * std::max(ldb, P.ldp)));
        CRM_TRY(ctx->ws_S2.ensure(sizeof(double) * (size_t)P.fold_split3 * bg->kin_k1 * ldb));
        // rows between k1 + donors k2 and the padded contraction length stay zero
        const long used = bg->kin_k1 + bg->kin_groups * (long)bg->kin_k2;
        if (P.s_rows > used)
            CRM_HIP(hipMemsetAsync(ctx->ws_S.as<double>() + (size_t)used * P.ld_ah, 0, sizeof(double) * (size_t)(P.s_rows - used) * P.ld_ah, st));
    } else if (P.kin()) {
        CRM_TRY(ctx->ws_S.ensure(P.s_bytes));
        CRM_TRY(ctx->ws_Gk.ensure(sizeof(double) * (size_t)bg->kin_rows * std::max(ldb, P.ldp)));
        CRM_TRY(ctx->ws_S2.ensure(sizeof(double) * (size_t)bg->kin_groups_pad * KK * ldb));
        if (bg->kin_groups_pad > bg->kin_groups)
            CRM_HIP(hipMemsetAsync(ctx->ws_S2.as<double>() + (size_t)bg->kin_groups * KK * ldb, 0,
                                   sizeof(double) * (size_t)(bg->kin_groups_pad - bg->kin_groups) * KK * ldb, st));
        // rows of the padding donors (kin_groups .. kin_groups_pad) are operands of the contraction over the donors
        if (bg->kin_groups_pad > bg->kin_groups)
            CRM_HIP(hipMemsetAsync(ctx->ws_S.as<double>() + (size_t)bg->kin_groups * KK * P.ld_ah, 0,
                                   sizeof(double) * (size_t)(bg->kin_groups_pad - bg->kin_groups) * KK * P.ld_ah, st));
    }
    if (P.wb()) {
        // Unrelated-donor form: per gene Phi'[y, W] ((1 + c) rows over the positions) and E1'[y, W] (k1 x 128); per block
        // Phi'gx; the Gram of the KT + k1 rows; scratch of the per-gene constants
        const long brows = bg->kin_groups * bg->kin_k2 + GEMM_BK, kt = P.KT + bg->kin_k1;
        const size_t n_yW = (size_t)ng * (1 + c) * P.ldwb, n_E1 = (size_t)ng * bg->kin_k1 * 128, n_g = (size_t)BLK * P.ldwb,
                     n_Gw = (size_t)BLK * kt * kt, n_tmp = (size_t)(bg->kin_rows + brows) * 128;
        CRM_TRY(ctx->ws_WB.ensure(sizeof(double) * (n_yW + n_E1 + n_g + n_Gw + n_tmp)));
        wb_yW = ctx->ws_WB.as<double>();
        wb_E1yW = wb_yW + n_yW;
        wb_g = wb_E1yW + n_E1;
        wb_Gw = wb_g + n_g;
        wb_tmp = wb_Gw + n_Gw;
    }
    return CRM_OK;
}

// ---- per-pass preparation -------------------------------------------------------------------------------------------
// y o E, W o E per gene; the permuted contexts and their pair products E (x) E once -- unless the
// scan runs collapsed on donor tables the background already holds (then nothing reads them)
int ScanPass::context_features(bool shared_too) {
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        const bool both = gi == 0 && shared_too;
        if (g->tab_YE && (!both || g->tab_E)) continue;   // (kept from an earlier call: prepare_contexts has checked the key)
        CRM_TRY(g->YE.ensure(sizeof(double) * np * g->ld_ye));
        if (both) {
            CRM_TRY(g->Ep.ensure(sizeof(double) * np * g->ld_ep));
            CRM_TRY(g->EE.ensure(sizeof(double) * np * g->ld_ee));
        }
        CRM_TRY(launch_context_features(st, g->E0.as<double>(), g->lde, d_idxE, n, np, k0, g->yW.as<double>(),
                                        g->yW.as<double>() + 1, g->ld_yw, c,
                                        both ? g->Ep.as<double>() : nullptr, g->ld_ep, g->YE.as<double>(),
                                        g->ld_ye, both ? g->EE.as<double>() : nullptr, g->ld_ee));
        g->tab_YE = keep_tables();
        if (both) g->tab_E = keep_tables();
    }
    if (shared_too) {
        d_Ep = g0->Ep.as<double>();
        d_EE = g0->EE.as<double>();
    }
    return CRM_OK;
}

// context features for this permutation (E, E (x) E shared; y o E per gene) and the collapsed path's donor tables
int ScanPass::prepare_contexts() {
    CRM_TRY(g0->idx.ensure(sizeof(int) * 2 * n));
    if (idx_E) {
        d_idxE = g0->idx.as<int>();
        CRM_HIP(hipMemcpyAsync(d_idxE, idx_E, sizeof(int) * n, hipMemcpyHostToDevice, st));
    }
    if (idx_G) {
        d_idxG = g0->idx.as<int>() + n;
        CRM_HIP(hipMemcpyAsync(d_idxG, idx_G, sizeof(int) * n, hipMemcpyHostToDevice, st));
    }
    for (crm_gene* g : genes) {
        g->ld_ep = round_up(k0, 128);
        g->ld_ye = P.ldZ1;
        g->ld_ee = P.ldZ3;
        // what the gene keeps of an earlier call holds for this one when no context permutation is in use and the key matches
        const crm_gene::TableKey key{bg->kin_gen, k0, g->ld_ep, g->ld_ye, g->ld_ee};
        if (!keep_tables() || !(g->tab_key == key)) {
            g->tab_YE = g->tab_E = g->tab_kinEp = g->tab_kinUE = g->tab_kinP = g->tab_kinEE = false;
            g->tab_e1_is_E = g->tab_us_is_E = -1;
            g->tab_key = keep_tables() ? key : crm_gene::TableKey{};
        }
    }
    if (!P.collapsed()) return context_features(true);
    const double* Zt = panel->Z.as<double>();
    if (P.cross) {
        CRM_TRY(g0->dt_Zt.ensure(sizeof(double) * (size_t)np * panel->ldz + sizeof(int) * n));
        int* gperm = reinterpret_cast<int*>(g0->dt_Zt.as<double>() + (size_t)np * panel->ldz);
        CRM_TRY(launch_permute_group(st, panel->group.as<int>(), d_idxG, n, gperm));
        CRM_TRY(launch_indicator(st, gperm, n, np, (int)panel->m, g0->dt_Zt.as<double>(), panel->ldz));
        Zt = g0->dt_Zt.as<double>();
    }
    // phenotype-free tables: shared through the background when no permutation hook is in use
    // (key: contents of E0 and of the donor index), else private to this call's first gene
    const bool reusable = !idx_E && !idx_G;
    bool build_shared = false;
    if (reusable) {
        for (crm_donor_tables* t : bg->dt_cache)
            if (t->e0_key == g0->e0_key && t->group_key == panel->group_key) tab = t;
        if (!tab) {
            if ((int)bg->dt_cache.size() >= crm_background::DT_CACHE) {  // drop the least recently used
                size_t lru = 0;
                for (size_t i = 1; i < bg->dt_cache.size(); i++)
                    if (bg->dt_cache[i]->stamp < bg->dt_cache[lru]->stamp) lru = i;
                tab = bg->dt_cache[lru];
            } else {
                tab = new crm_donor_tables();
                bg->dt_cache.push_back(tab);
            }
            tab->e0_key = 0;  // invalid until built
            build_shared = true;
        }
        tab->stamp = ++bg->dt_clock;
    } else {
        tab = &g0->dt_own;
        build_shared = true;
    }
    CRM_TRY(context_features(build_shared));
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        const bool have = reusable && g->dt_group == panel->group_key && !(gi == 0 && build_shared);
        if (!have) {
            g->dt_group = 0;
            CRM_TRY(build_donor_tables(g, panel, (gi == 0 && build_shared) ? tab : nullptr, d_Ep, d_EE, Zt, P.cross));
            if (reusable) g->dt_group = panel->group_key;
        }
    }
    if (build_shared && reusable) {
        tab->e0_key = g0->e0_key;
        tab->group_key = panel->group_key;
    }
    return CRM_OK;
}

// The kinship-structure routes' operands in donor order, the probes that settle the pair-product forms (plan_scan), and
// the zero rows of AH, the operand of every route through H but the folded one
int ScanPass::prepare_kinship() {
    const long ldh = bg->ldh;
    const double* H = bg->H.as<double>();
    if (P.kin() && !g0->tab_kinEp) {   // the (permuted) contexts in donor order
        CRM_TRY(g0->kinEp.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ep));
        CRM_TRY(launch_gather_rows(st, d_Ep, g0->ld_ep, bg->kin_map.as<int>(), bg->kin_rows, (int)g0->ld_ep,
                                   g0->kinEp.as<double>(), g0->ld_ep));
        g0->tab_kinEp = keep_tables();
    }
    if (P.folded() && bg->kin_k2 == 1 && !g0->tab_kinUE) {
        // one column of us: S[(k1 + d'), (b, i)] = sum over the cells of donor d' of us(c) g_b(c) E0(c, i) is the plain product
        // G_d'' (us o E0)_d' of the donor's own cells -- its (b, i) layout is the row of S as it stands.  kinUE = us o E0 in
        // donor order.
        CRM_TRY(g0->kinUE.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ep));
        CRM_TRY(launch_scale_rows(st, g0->kinEp.as<double>(), g0->ld_ep, bg->kin_Y.as<double>(), bg->kin_ldy, bg->kin_rows,
                                  (int)g0->ld_ep, g0->kinUE.as<double>(), g0->ld_ep));
        g0->tab_kinUE = keep_tables();
    }
    // The probes: what the data says is kept on the gene (a probe ends in a wait for the host); the plan and the forms decide
    // on every call which of them are asked and what follows from them
    const SameColumns e1_is_E{H, ldh, d_Ep, g0->ld_ep, n};   // E1 = E
    const SameColumns us_is_E{bg->kin_Y.as<double>(), bg->kin_ldy, g0->kinEp.as<double>(), g0->ld_ep, bg->kin_rows};   // E2 = E
    auto asked = [&](const SameColumns& pair, int& kept, bool& same) -> int {
        if (kept < 0) {
            CRM_TRY(same_columns(st, d_near, k0, {pair}, same));
            if (keep_tables()) kept = same ? 1 : 0;
        } else
            same = kept == 1;
        return CRM_OK;
    };
    if (probed.e1_sym) CRM_TRY(asked(e1_is_E, g0->tab_e1_is_E, probed.e1_sym));
    if (P.e1_pairs && !probed.e1_sym && !g0->tab_kinP) {
        CRM_TRY(g0->kinP.ensure(sizeof(double) * (size_t)np * P.ldP));
        CRM_TRY(launch_pair_features(st, H, ldh, bg->kin_k1, d_Ep, g0->ld_ep, k0, np, g0->kinP.as<double>(), P.ldP));
        g0->tab_kinP = keep_tables();
    }
    probed.donor_pairs = probed.donor_pairs && probed.e1_sym;
    if (probed.donor_pairs) CRM_TRY(asked(us_is_E, g0->tab_us_is_E, probed.donor_pairs));
    if (probed.pairs_unfolded) CRM_TRY(asked(e1_is_E, g0->tab_e1_is_E, probed.pairs_unfolded));
    if (probed.pairs_unfolded) CRM_TRY(asked(us_is_E, g0->tab_us_is_E, probed.pairs_unfolded));
    probed.wb_rotate = probed.wb_rotate && probed.donor_pairs;
    if (probed.donor_pairs || probed.pairs_unfolded) {   // (the folded and the unfolded form respectively)
        if (!g0->tab_kinEE) {
            CRM_TRY(g0->kinEE.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ee));
            CRM_TRY(launch_gather_rows(st, d_EE, g0->ld_ee, bg->kin_map.as<int>(), bg->kin_rows, (int)g0->ld_ee,
                                       g0->kinEE.as<double>(), g0->ld_ee));
            g0->tab_kinEE = keep_tables();
        }
        CRM_TRY(ctx->ws_Pd.ensure(sizeof(double) * (size_t)(probed.donor_pairs ? bg->kin_groups : bg->kin_groups_pad) * P.pd_slab));
    }
    if (probed.donor_pairs)   // (ws_AH, the folded form's scratch, also holds the sliced pair products of the expansion pass)
        CRM_TRY(ctx->ws_AH.ensure(sizeof(double) * (size_t)std::max<long>(P.donor_pair_splits, P.fold_split6) *
                                  (size_t)std::max<long>(P.pd_slab, (std::max<long>(P.BLK, P.pair_cap) + 128) * P.ldP)));
    // (unfolded form: the slabs of the padding donors meet zero rows of hKd in the contraction over the donors: they must be
    // finite -- cleared here, not left to whatever the allocation or an earlier call put there)
    if (probed.pairs_unfolded && bg->kin_groups_pad > bg->kin_groups)
        CRM_HIP(hipMemsetAsync(ctx->ws_Pd.as<double>() + (size_t)bg->kin_groups * P.pd_slab, 0,
                               sizeof(double) * (size_t)(bg->kin_groups_pad - bg->kin_groups) * P.pd_slab, st));
    if (P.through_H() && !P.folded()) {
        // AH = H'(g o E0), the operand of the products with the mixing matrices: its rows beyond the half factor's columns meet
        // zero rows of Mix and must be finite -- zero.  The pair-feature form writes every row below them for every column it
        // is read at (columns beyond the block's only feed output rows that are never stored), so the padding rows are all
        // there is to clear: 4 rows instead of 0.67 GB per call at config 2.
        if (probed.pairs_unfolded && ldh > bg->cols)
            CRM_HIP(hipMemsetAsync(ctx->ws_AH.as<double>() + (size_t)bg->cols * P.ld_ah, 0, sizeof(double) * (size_t)(ldh - bg->cols) * P.ld_ah, st));
        else if (!probed.pairs_unfolded)
            CRM_HIP(hipMemsetAsync(ctx->ws_AH.ptr, 0, sizeof(double) * (size_t)ldh * P.ld_ah, st));
    }
    return CRM_OK;
}

// Unrelated-donor form: Phi'[y, W] and E1'[y, W] per gene -- formed on the gene's first scan against these tables
// (crm_gene::wb_yW), copied into this scan's workspace after
int ScanPass::prepare_woodbury() {
    if (!P.wb()) return CRM_OK;
    const int k2 = bg->kin_k2, k1 = bg->kin_k1;
    const long groups = bg->kin_groups, brows = groups * k2 + GEMM_BK;
    const size_t n_yW1 = (size_t)(1 + c) * P.ldwb, n_E11 = (size_t)k1 * 128;
    double* yWk = wb_tmp;                              // [y, W] in donor order
    double* Bk = yWk + (size_t)bg->kin_rows * 128;     // us_d'[y, W]_d, rows d k2 + j
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        if (g->wb_gen != bg->wb_gen) {
            CRM_TRY(g->wb_yW.ensure(sizeof(double) * (n_yW1 + n_E11)));
            CRM_HIP(hipMemsetAsync(g->wb_yW.ptr, 0, sizeof(double) * (n_yW1 + n_E11), st));
            CRM_HIP(hipMemsetAsync(Bk, 0, sizeof(double) * (size_t)brows * 128, st));
            CRM_TRY(launch_gather_rows(st, g->yW.as<double>(), g->ld_yw, bg->kin_map.as<int>(), bg->kin_rows, 1 + c, yWk, 128));
            std::vector<GemmProblem> kp((size_t)2 * groups);
            GemmProblem p{};
            p.X = bg->kin_Y.as<double>(); p.ldx = bg->kin_ldy; p.Y = yWk; p.ldy = 128; p.C = Bk; p.ldc = 128;
            p.M = k2; p.N = 1 + c;
            const long maxlen = donor_run_records(bg, p, (long)k2 * 128, kp.data());
            GemmProblem q{};   // Phi_d'[y, W]_d, stored transposed: rows y, W_1 .. W_c over the positions
            q.X = Bk; q.ldx = 128; q.C = g->wb_yW.as<double>(); q.ldc = P.ldwb; q.M = 1 + c;
            woodbury_records(bg, q, (long)k2 * 128, kp.data() + groups);
            GemmProblem e{};   // E1'[y, W] over all cells
            e.X = bg->H.as<double>(); e.ldx = bg->ldh; e.Y = g->yW.as<double>(); e.ldy = g->ld_yw;
            e.C = g->wb_yW.as<double>() + n_yW1; e.ldc = 128; e.M = k1; e.N = 1 + c;
            CRM_TRY(with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
                CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, k2, 1 + c, maxlen, false, 0, 1, 0));
                CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, (int)groups, 1 + c, k2, bg->wb_k2pad, false, 0, 1, 0));
                CRM_TRY(upload(SLOT_ONE, &e, 1));
                return launch_gemm_tn(ctx, d_probs + SLOT_ONE, 1, k1, 1 + c, np, false, 0, 1, 0);
            }));
            g->wb_gen = bg->wb_gen;
        }
        CRM_HIP(hipMemcpyAsync(wb_yW + (size_t)gi * n_yW1, g->wb_yW.as<double>(), sizeof(double) * n_yW1, hipMemcpyDeviceToDevice, st));
        CRM_HIP(hipMemcpyAsync(wb_E1yW + (size_t)gi * n_E11, g->wb_yW.as<double>() + n_yW1, sizeof(double) * n_E11,
                               hipMemcpyDeviceToDevice, st));
    }
    return CRM_OK;
}

}  // namespace crm
