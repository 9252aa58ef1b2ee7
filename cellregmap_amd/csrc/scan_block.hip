// Stages 1-5 of a block of a scan (scan_pass.h: ScanPass): copy, statistics, rotations T(rho), null fits, the fits on the host.
#include "scan_pass.h"

namespace crm {

int ctx_cus(const crm_ctx* ctx) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
    return cus;
}

// crm_scan_interaction_permuted (crm_ctx::ReplayBlock): the rows T(rho*(b)) of a block out of / back into the per-grid-point
// slabs of the rotations, T[(rho * blk + b) * ldT + j]
__global__ void replay_rows_kernel(double* __restrict__ T, long blk, long ldT, const crm::NullFitOut* __restrict__ fit, int nb,
                                   int cols, double* __restrict__ rows, int restore) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb || j >= cols) return;
    const int ri = fit[b].rho_index;
    if (ri < 0) return;
    double* slab = T + ((size_t)ri * blk + b) * ldT;
    if (restore) slab[j] = rows[(size_t)b * ldT + j];
    else rows[(size_t)b * ldT + j] = slab[j];
}

// ---- block stages ---------------------------------------------------------------------------------------------------
// 1. aligned copy of the block (and its row-permuted twin for the test direction); in
//    collapsed mode the "block" is the donor dosage slab (m_pad rows)
//
// The fused form (form("block_fused"), default): a block of a dense panel is not copied.  Its statistics read the panel
// slab in place and one pass after the projection coefficients (blockops.hip: block_pass_kernel) writes Gx, G2 = Gt o Gt,
// GG = Gt o Gx and, on the kinship routes, Gx and Gt in donor order -- what ortho_apply, the two donor-order gathers and
// square_block wrote, from the same instructions.  Gt is then the panel itself, leading dimension panel->ld, and what the
// copy left as zeros past the block's nb columns are the panel's next variants.  Who reads them:
//   - the plain products with Gt as the row operand (Z1, the E1 rows) fetch whole 128-column tiles and store rows < nb alone:
//     any finite value serves, but the tile must stay inside the panel's row -- the block starts at a multiple of 128;
//   - the Khatri-Rao products with Gt as the row operand (several phenotypes through H on the direct route; the E1 rows of the
//     folded form without pair features) fetch up to 128 columns past the block's last tile: a block without that many
//     columns of the panel's row behind it keeps the copy;
//   - a pair stage over sub-ranges (several phenotypes with more pairs than the pair-ordered buffers hold) offsets Gt by
//     b0, off the 128-column grid, and relied on the copy's slack columns: such a pass keeps the copy;
//   - everything else (the pair-order gather, the statistics) reads the block's own columns.
// The donor-order and cell-order outputs keep their zeros beyond nb: the pass writes them from g = 0 as the copy did.
bool ScanPass::fused_pass() const {
    const bool sub_ranges = ng > 1 && P.pair_cap < (long)std::min(nrho, ng) * P.BLK;
    return form("block_fused", 1) != 0 && !P.collapsed() && !panel->grouped && !idx_G && panel->n_pad == np && !sub_ranges;
}
bool ScanPass::fused_block(long col0, int nb) const {
    const bool kr_reads_Gt = (P.route == Route::direct && ng > 1) || (P.folded() && !P.e1_pairs);
    return fused_pass() && col0 % 128 == 0 && col0 + round_up(nb, 128) + (kr_reads_Gt ? 128 : 0) <= panel->ld;
}

int ScanPass::copy_block(Block& B) {
    const long ldb = P.ldb;
    const int nb = B.nb;
    B.ldt = ldb;
    if (fused_block(B.col0, nb)) {
        B.Gb = B.Gt = panel->G.as<double>() + B.col0;
        B.ldt = panel->ld;
        B.fused = true;
        ctx->fused_blocks++;
        return CRM_OK;
    }
    B.Gb = B.Gt = B.Gx = ctx->ws_Gb.as<double>();
    if (P.collapsed()) {
        CRM_TRY(launch_gather_block(st, panel->Gd.as<double>() + B.col0, panel->ld, P.mp, panel->m, nullptr, nullptr, nb, B.Gb, ldb, (int)ldb));
    } else if (panel->grouped) {
        CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + B.col0, panel->ld, panel->group.as<int>(), np, n, nullptr, nb, B.Gb, ldb, (int)ldb));
        if (idx_G) {
            B.Gt = ctx->ws_Gt.as<double>();
            CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + B.col0, panel->ld, panel->group.as<int>(), np, n, d_idxG, nb, B.Gt, ldb, (int)ldb));
        }
    } else {
        CRM_TRY(launch_gather_block(st, panel->G.as<double>() + B.col0, panel->ld, np, n, nullptr, nullptr, nb, B.Gb, ldb, (int)ldb));
        if (idx_G) {
            B.Gt = ctx->ws_Gt.as<double>();
            CRM_TRY(launch_gather_block(st, panel->G.as<double>() + B.col0, panel->ld, np, n, d_idxG, nullptr, nb, B.Gt, ldb, (int)ldb));
        }
    }
    return CRM_OK;
}

// 2. The fixed effects' role of the variants: Gx = G - W (W'W)^-1 W'G, orthogonalised against the covariates in
//    the cell axis as the reference's economic_svd([W, g]) basis is (blockops.hip); the test direction keeps G.
//    Then g'g, g'W (shared) and g'y per gene of that role.  The collapsed path works on donor-level sums and
//    cannot do this: it marks the variants that are nearly collinear with W for a second, dense pass.
int ScanPass::block_stats(Block& B) {
    const long ldb = P.ldb, ld_gW = P.ld_gW;
    const int nb = B.nb, BLK = P.BLK;
    if (!P.collapsed()) {
        B.Gx = ctx->ws_Gx.as<double>();
        CRM_TRY(launch_variant_stats(st, B.Gb, B.ldt, np, nb, g0->yW.as<double>(), g0->yW.as<double>() + 1, g0->ld_yw, c, d_part, d_gg, d_gy, d_gW, ld_gW));
        if (B.fused) {
            // (the donor-order test direction where the pair stage reads it in block order: donor_columns)
            const bool kin_t = P.kin() && (ng > 1 || P.wb_block);
            CRM_TRY(launch_block_pass(st, B.Gb, B.ldt, n, np, nb, (int)ldb, g0->yW.as<double>() + 1, g0->ld_yw, c,
                                      g0->Wproj.as<double>(), d_gW, ld_gW, d_coef, ldb, d_thr, B.Gx, ctx->ws_G2.as<double>(),
                                      ctx->ws_GG.as<double>(), ldb, P.kin() ? bg->kin_inv.as<int>() : nullptr,
                                      P.kin() ? bg->kin_inv.as<int>() + np : nullptr, P.kin() ? bg->kin_pads : 0,
                                      P.kin() ? ctx->ws_Gk.as<double>() : nullptr, kin_t ? ctx->ws_Gkt.as<double>() : nullptr));
        } else
            CRM_TRY(launch_ortho_block(st, B.Gb, ldb, np, nb, (int)ldb, g0->yW.as<double>() + 1, g0->ld_yw, c, g0->Wproj.as<double>(),
                                       d_gW, ld_gW, d_coef, ldb, d_thr, B.Gx, ldb));
    }
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        if (P.collapsed())
            CRM_TRY(launch_donor_stats(st, B.Gb, ldb, (int)panel->m, nb, g->dt_sums.as<double>(), c, d_gg, d_gy + (size_t)gi * BLK, d_gW, ld_gW));
        else
            CRM_TRY(launch_variant_stats(st, B.Gx, ldb, np, nb, g->yW.as<double>(), g->yW.as<double>() + 1, g->ld_yw, c, d_part, d_gg, d_gy + (size_t)gi * BLK, d_gW, ld_gW));
    }
    if (P.collapsed()) {
        if (near_out) CRM_TRY(launch_collinear_flag(st, d_gg, d_gW, ld_gW, g0->Wproj.as<double>(), c, nb, COLLINEAR_TAU, d_near));
    } else
        CRM_TRY(launch_ortho_rank(st, d_gg, d_thr, nb, d_drop));
    return CRM_OK;
}

// folded form: rows [0, k1) = E1'G over all cells (sliced along the cell axis), rows k1 + d' k2 + j = per-donor
// us_j'G over the donor's own cells; the contraction over the donors sits in MixK (objects.h)
int ScanPass::fold_TH(const Block& B) {
    const long ldb = P.ldb;
    const int nb = B.nb, k1 = bg->kin_k1, k2 = bg->kin_k2;
    const long groups = bg->kin_groups;
    double* Gk = ctx->ws_Gk.as<double>();
    double* TH = ctx->ws_TH.as<double>();
    if (!B.fused) CRM_TRY(launch_gather_rows(st, B.Gx, ldb, bg->kin_map.as<int>(), bg->kin_rows, (int)ldb, Gk, ldb));
    std::vector<GemmProblem> kp((size_t)groups + 1);
    GemmProblem p{};
    p.X = bg->kin_Y.as<double>(); p.ldx = bg->kin_ldy; p.Y = Gk; p.ldy = ldb; p.C = TH + (size_t)k1 * ldb; p.ldc = ldb;
    p.M = k2; p.N = nb;
    const long maxlen = donor_run_records(bg, p, (long)k2 * ldb, kp.data());
    GemmProblem& e = kp[groups];
    e.X = bg->H.as<double>(); e.ldx = bg->ldh; e.Y = B.Gx; e.ldy = ldb;
    e.C = ctx->ws_S2.as<double>(); e.ldc = ldb; e.M = k1; e.N = nb;
    const long e1_slab = (long)k1 * ldb;
    return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
        CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, k2, nb, maxlen, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, 1, k1, nb, np, false, 0, P.fold_split3, e1_slab));
        CRM_TRY(launch_reduce_splits(st, ctx->ws_S2.as<double>(), e1_slab, P.fold_split3, e1_slab));
        CRM_HIP(hipMemcpyAsync(TH, ctx->ws_S2.ptr, sizeof(double) * (size_t)e1_slab, hipMemcpyDeviceToDevice, st));
        return CRM_OK;
    });
}

// H'G donor by donor (as H'(g o E0) in step 6): per donor [us | E1]' G over its own cells, then the L rows by a
// contraction over the donors with hKd and the E1 rows as sums over the donors
int ScanPass::unfolded_TH(const Block& B) {
    const long ldb = P.ldb, KK = P.KK;
    const int nb = B.nb, k1 = bg->kin_k1, k2 = bg->kin_k2;
    const long groups = bg->kin_groups, mk = bg->kin_cols;
    double* Gk = ctx->ws_Gk.as<double>();
    double* S2 = ctx->ws_S2.as<double>();
    if (!B.fused) CRM_TRY(launch_gather_rows(st, B.Gx, ldb, bg->kin_map.as<int>(), bg->kin_rows, (int)ldb, Gk, ldb));
    std::vector<GemmProblem> kp((size_t)groups + k2);
    GemmProblem p{};
    p.X = bg->kin_Y.as<double>(); p.ldx = bg->kin_ldy; p.Y = Gk; p.ldy = ldb; p.C = S2; p.ldc = ldb;
    p.M = (int)KK; p.N = nb;
    const long maxlen = donor_run_records(bg, p, KK * ldb, kp.data());
    for (int j = 0; j < k2; j++) {
        GemmProblem& q = kp[groups + j];
        q.X = bg->kin_hKd.as<double>(); q.ldx = bg->kin_ldh; q.Y = S2 + (size_t)j * ldb; q.ldy = KK * ldb;
        q.C = ctx->ws_TH.as<double>() + (size_t)(k1 + (long)j * mk) * ldb; q.ldc = ldb; q.M = (int)mk; q.N = nb;
    }
    return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
        CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, (int)KK, nb, maxlen, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, k2, (int)mk, nb, bg->kin_groups_pad, false, 0, 1, 0));
        return launch_kin_sum_e1(st, S2, ldb, (int)KK, k2, k1, (int)groups, nb, ctx->ws_TH.as<double>(), ldb);
    });
}

int ScanPass::plain_TH(const Block& B) {
    const long ldb = P.ldb;
    GemmProblem p{};
    p.X = bg->H.as<double>(); p.ldx = bg->ldh; p.Y = B.Gx; p.ldy = ldb;
    p.C = ctx->ws_TH.as<double>(); p.ldc = ldb; p.M = (int)bg->cols; p.N = B.nb;
    CRM_TRY(upload(SLOT_ONE, &p, 1));
    CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOT_ONE, 1, (int)bg->cols, B.nb, np, false, 0, P.ks_h, P.th_slab));
    return launch_reduce_splits(st, ctx->ws_TH.as<double>(), (long)bg->cols * ldb, P.ks_h, P.th_slab);
}

// The eleven products run as one launch of equally long tiles, i.e. in rounds of as many tiles as the chip holds
// workgroups (two per CU): at config 3, 12 832 tiles are 25.06 rounds of 512 and the last 0.06 costs a whole one.
// The smallest problems that make up that remainder (there: rho = 1, r = 50, 32 tiles) are taken out and run cut
// along the contraction axis instead -- a sixteenth of a round plus a reduction.  cut_rotations works on probs[0, n_list)
// and returns the problems left in probs.  cut_choice is the choice itself, for problems of N[0 .. cnt) columns: which
// ones are cut, how many tiles they are, and the rounds the batched launch takes after it -- plan_rotations asks it
// too, to see what saves a round.
bool ScanPass::cut_choice(int nb, int cnt, const int* N, bool* is_cut, long& acc, long& rounds) const {
    const long slots = 2L * ctx_cus(ctx), mtl = (nb + GEMM_BM - 1) / GEMM_BM;
    long tiles[CRM_MAX_RHO], total = 0;
    int order[CRM_MAX_RHO];
    for (int i = 0; i < cnt; i++) { tiles[i] = mtl * ((N[i] + 127) / 128); total += tiles[i]; order[i] = i; }
    std::sort(order, order + cnt, [&](int a, int b) { return tiles[a] < tiles[b]; });
    const long need = total % slots;
    acc = 0;
    int take = 0;
    while (take < cnt - 1 && acc < need) acc += tiles[order[take++]];
    const bool cut = total > slots && need > 0 && acc >= need && acc <= slots / 4;
    rounds = ((cut ? total - acc : total) + slots - 1) / slots;
    for (int q = 0; q < take && cut; q++) is_cut[order[q]] = true;
    return cut;
}
int ScanPass::cut_rotations(const Block& B, int n_list, int& n_main) {
    const int nb = B.nb, BLK = P.BLK;
    n_main = n_list;
    const long slots = 2L * ctx_cus(ctx);
    int widths[CRM_MAX_RHO];
    bool is_cut[CRM_MAX_RHO] = {false};
    long acc = 0, rounds = 0;
    for (int i = 0; i < n_list; i++) widths[i] = probs[i].N;
    if (!cut_choice(nb, n_list, widths, is_cut, acc, rounds)) return CRM_OK;
    int n_cut = 0, cut_ks = 1;
    GemmProblem cut_probs[CRM_MAX_RHO];
    double* cut_dst[CRM_MAX_RHO];
    long cut_doubles = 0;
    while ((long)(cut_ks + 1) * acc <= slots && cut_ks < 16 && P.kdim / GEMM_BK / (cut_ks + 1) >= 8) cut_ks++;
    n_main = 0;
    for (int i = 0; i < n_list; i++) {
        if (!is_cut[i]) { probs[n_main++] = probs[i]; continue; }
        GemmProblem c = probs[i];
        cut_dst[n_cut] = c.C;
        c.ldc = round_up(c.N, 128);
        cut_doubles += (long)BLK * c.ldc;
        cut_probs[n_cut++] = c;
    }
    CRM_TRY(ctx->ws_Tcut.ensure(sizeof(double) * (size_t)cut_doubles * cut_ks));
    long at = 0;
    for (int q = 0; q < n_cut; q++) {
        cut_probs[q].C = ctx->ws_Tcut.as<double>() + at;
        at += (long)BLK * cut_probs[q].ldc;
    }
    const int slot = SLOT_RHO + n_main;
    CRM_TRY(upload(slot, cut_probs, n_cut));
    int cut_maxn = 1;
    for (int q = 0; q < n_cut; q++) cut_maxn = std::max(cut_maxn, cut_probs[q].N);
    CRM_TRY(launch_gemm_tn(ctx, d_probs + slot, n_cut, nb, cut_maxn, P.kdim, false, 0, cut_ks, cut_doubles));
    CRM_TRY(launch_reduce_splits(st, ctx->ws_Tcut.as<double>(), cut_doubles, cut_ks, cut_doubles));
    for (int q = 0; q < n_cut; q++)
        CRM_HIP(hipMemcpy2DAsync(cut_dst[q], sizeof(double) * P.ldT, cut_probs[q].C, sizeof(double) * cut_probs[q].ldc,
                                 sizeof(double) * cut_probs[q].N, nb, hipMemcpyDeviceToDevice, st));
    return CRM_OK;
}

// 3. T(rho) = G' Q0(rho) for all grid points.  With Q0(rho) = H Mix(rho) the n-length work is
//    done once, (H'G), followed by eleven small products Mix(rho)'(H'G): 2 n cols + 2 cols sum r
//    flops per variant instead of 2 n sum r.
int ScanPass::rotations(const Block& B) {
    const int nb = B.nb;
    if (P.folded()) CRM_TRY(fold_TH(B));
    else if (P.kin()) CRM_TRY(unfolded_TH(B));
    else if (P.fastT) CRM_TRY(plain_TH(B));
    // (unrelated-donor form: Phi'gx of the block, which the null fits at rho = 0 read -- H'Gx is all it needs)
    if (P.wb()) CRM_TRY(woodbury_phi(B));
    GemmProblem all[CRM_MAX_RHO];
    for (int i = 0; i < nrho; i++) {
        GemmProblem p{};
        if (P.fastT) {
            p.X = ctx->ws_TH.as<double>(); p.ldx = P.ldb;
            p.Y = P.folded() ? bg->MixK[i].as<double>() : bg->Mix[i].as<double>(); p.ldy = ldq;
        } else {
            p.X = B.Gx; p.ldx = P.ldb;
            p.Y = P.collapsed() ? tab->TZ.as<double>() + (size_t)i * P.mp * ldq : bg->Q0[i].as<double>(); p.ldy = ldq;
        }
        p.C = ctx->ws_T.as<double>() + (size_t)i * P.BLK * P.ldT; p.ldc = P.ldT;
        p.M = nb; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
        all[i] = p;
    }
    const int n_list = plan_rotations(B, all);   // (probs[0, n_list), rot_tails, rho0_pos)
    CRM_TRY(side_prepare(B));   // (the side stream's records, ahead of the launch it forks behind: scan_side.hip)
    if (n_list == 0) return side_fork(B);
    int n_main = n_list;
    if (P.fastT) CRM_TRY(cut_rotations(B, n_list, n_main));
    CRM_TRY(upload(SLOT_RHO, probs.data(), n_main));
    // (unrelated-donor form: the kernel timer brackets this launch, the rotations MixK(rho)'(H'Gx) -- the step's largest)
    const bool timing_T = P.wb() && ctx->timing && ctx->timed_used < 65536;
    if (timing_T) CRM_TRY(kernel_timer_open(ctx, st, true));
    CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOT_RHO, n_main, nb, (int)ldq, P.fastT ? P.kdim : P.xrows, false, 0, 1, 0));
    if (timing_T) {
        CRM_TRY(kernel_timer_close(ctx, st));
        for (int q = 0; q < n_main; q++) ctx->kr_flops += 2.0 * (double)P.kdim * (double)nb * (double)probs[q].N;
    }
    CRM_TRY(side_fork(B));   // (behind timer_close: the timed pair still brackets the rotations alone)
    if (!rot_tails.empty()) {   // (records behind the batched launch's and the cut ones; rot_tails lives as long as the pass)
        CRM_TRY(upload(SLOT_RHO + n_list, rot_tails.data(), rot_tails.size()));
        CRM_TRY(launch_skinny_tn(st, d_probs + SLOT_RHO + n_list, (int)rot_tails.size(), nb, P.kdim));
        ctx->rotation_tail_launches++;
    }
    return CRM_OK;
}

// What the rotations of a block leave out of the batched launch, decided together because the launch runs in rounds:
//
// rho = 0 from the positions (unrelated-donor form).  Sigma(0) = blockdiag_d kappa_d us_d us_d' has the positions
// Phi_d = us_d U_d Lambda_d^-1/2 as orthonormal eigenvectors and wb_S0 at rho = 0 as eigenvalues, and the null fit is
// a sum over the spectrum that asks for no order and no particular basis of an eigenspace: Phi'gx (woodbury_phi),
// Phi'[y, W] (prepare_woodbury) and wb_S0 serve it as they serve the assembly, and the dense product MixK(0)'(H'Gx)
// -- a tenth of the step's largest launch at config 3 -- is not formed.  Dropped positions (zero columns of Phi,
// s = 0) stay in: each adds nothing to a quadratic form and log delta to the log-determinant, as a direction of the
// complement does.  Guard: the positions seal_unrelated_donors kept must be as many as the grid point's rank
// -- else the two rank rules disagree about a direction and the dense product stays.
//
// The spectrum tails.  A spectrum a little longer than a multiple of the 128-column tile (config 3: r = 5000 = 39
// tiles + 8 columns) pays a whole column of tiles for those few columns, at every grid point; one pass over H'Gx per
// grid point forms them instead (launch_skinny_tn; eligibility as in a_records).
//
// Either changes the last bits of the null fits it touches (another summation order, another kernel), so each is
// taken only where the batched launch then runs fewer rounds (cut_choice).  Config 3, rounds of 512 tiles: all ten
// problems 10 x 32 x 40 + 32 = 12 832 tiles, 25 rounds once rho = 1 is cut out; the tails alone 12 512, still 25;
// rho = 0 alone 11 552, 23; both 9 x 32 x 39 + 32 = 11 264 = 22 rounds exactly.  A block of a few variants is a
// fraction of one round either way and keeps the dense products.  form("rho0_positions") / form("rotation_tails"): 0
// never, 1 by this rule, 2 wherever the guard / the eligibility allows (tests).
int ScanPass::plan_rotations(const Block& B, const GemmProblem* all) {
    // (both only where the rotations start from H'Gx, P.fastT: the launch cut_rotations then shapes, whose rounds
    // cut_choice models -- the unrelated-donor form is planned on the folded route alone, which has it)
    const int mode0 = P.fastT && P.wb() ? form("rho0_positions", 1) : 0;
    const int modeT = P.fastT && P.kin() && !form("kr_no_tail", 0) ? form("rotation_tails", 1) : 0;
    bool cand[CRM_MAX_RHO] = {false};
    int rem[CRM_MAX_RHO] = {0}, n_cand = 0, n_rem = 0;
    for (int i = 0; i < nrho; i++) {
        const GemmProblem& p = all[i];
        cand[i] = mode0 > 0 && bg->rho[i] == 0.0 && bg->r[i] > 0 && bg->wb_kept == bg->r[i];
        const int m = p.N % 128;
        if (modeT > 0 && p.N >= 1024 && m > 0 && m <= 16 && p.ldx % 2 == 0 && (reinterpret_cast<uintptr_t>(p.X) & 15) == 0) rem[i] = m;
        n_cand += cand[i] ? 1 : 0;
    }
    for (int i = 0; i < nrho; i++) n_rem += rem[i] > 0 ? 1 : 0;
    auto rounds = [&](bool drop, bool tails) {
        int widths[CRM_MAX_RHO], cnt = 0;
        bool is_cut[CRM_MAX_RHO] = {false};
        long acc = 0, r = 0;
        for (int i = 0; i < nrho; i++)
            if (!(drop && cand[i])) widths[cnt++] = all[i].N - (tails ? rem[i] : 0);
        if (cnt > 0) cut_choice(B.nb, cnt, widths, is_cut, acc, r);
        return r;
    };
    // try {neither, drop rho = 0, tails, both} and keep the fewest rounds; a tie keeps the earlier one, the dense
    // products first.  A forced form (value 2) is on in all four.
    const bool can0 = n_cand > 0, canT = n_rem > 0, force0 = mode0 >= 2 && can0, forceT = modeT >= 2 && canT;
    bool drop = force0, tails = forceT;
    long best = rounds(drop, tails);
    for (int pick = 1; pick < 4; pick++) {
        const bool d = force0 || (can0 && (pick & 1)), t = forceT || (canT && (pick & 2));
        const long r = rounds(d, t);
        if (r < best) { best = r; drop = d; tails = t; }
    }
    rot_tails.clear();
    int n_list = 0;
    for (int i = 0; i < nrho; i++) {
        rho0_pos[i] = drop && cand[i];
        if (rho0_pos[i]) continue;
        GemmProblem p = all[i];
        if (tails && rem[i] > 0) {
            GemmProblem t = p;
            p.N -= rem[i];
            t.Y = p.Y + p.N; t.C = p.C + p.N; t.N = rem[i];
            rot_tails.push_back(t);
        }
        probs[n_list++] = p;
    }
    return n_list;
}

// 4. null fits + rho* per gene; the probe hook (ctx->probe_on) keeps the (variant, grid point) records of this block --
//    the pass stops after it
int ScanPass::null_fits(const Block& B) {
    const int nb = B.nb, BLK = P.BLK;
    if (ctx->probe_mode == 2 && ng != 1) {   // (d_trial is written again per phenotype: the records of one only)
        set_error("null-fit records (crm_test_null_fit_probe, on = 2): one phenotype per pass, not %d", ng);
        return CRM_ERR_ARG;
    }
    trace_push("crm null fits");
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        NullFitArgs fa{};
        nullfit_gene_args(fa, g, 1);
        for (int i = 0; i < nrho; i++) {
            NullFitRho& R = fa.rho[i];
            R.T = ctx->ws_T.as<double>() + (size_t)i * BLK * P.ldT; R.ldT = P.ldT;
            if (rho0_pos[i]) {   // (the operands of the assembly: gene_results, the P.wb() branch)
                R.T = wb_g; R.ldT = P.ldwb;
                R.ty = wb_yW + (size_t)gi * (1 + c) * P.ldwb;
                R.tW = R.ty + P.ldwb; R.ldW = P.ldwb;
                R.S0 = bg->wb_S0[i].as<double>();
                R.r = (int)bg->wb_P;
            }
        }
        fa.gg = d_gg; fa.gy = d_gy + (size_t)gi * BLK; fa.gW = d_gW; fa.ld_gW = P.ld_gW;
        fa.g_drop = P.collapsed() ? nullptr : d_drop;
        if (c > CRM_MAX_COV_WIDE) fa.xwide = ctx->ws_xwide.as<double>();
        fa.trial = d_trial; fa.out = d_fit + (size_t)gi * BLK; fa.probe = ctx->probe_mode == 1 ? 1 : 0; fa.probe_x = ctx->probe_x;
        fa.track = outs[gi].flags ? 1 : 0;
        CRM_TRY(launch_nullfit(st, fa, nb, false, d_queue));
    }
    trace_pop();
    if (std::find(rho0_pos, rho0_pos + nrho, true) != rho0_pos + nrho) ctx->rho0_position_blocks++;
    if (ctx->probe_on) {
        std::vector<NullFitTrial> h_trial((size_t)nb * nrho);
        CRM_HIP(hipMemcpyAsync(h_trial.data(), d_trial, sizeof(NullFitTrial) * h_trial.size(), hipMemcpyDeviceToHost, st));
        std::vector<NullFitOut> h_out(ctx->probe_mode == 2 ? (size_t)nb : 0);
        if (!h_out.empty()) CRM_HIP(hipMemcpyAsync(h_out.data(), d_fit, sizeof(NullFitOut) * h_out.size(), hipMemcpyDeviceToHost, st));
        CRM_HIP(hipStreamSynchronize(st));
        if (ctx->probe_mode == 2) {   // (the records of the searches themselves, then the selection's choice per variant)
            ctx->probe_out.assign(5 * h_trial.size() + h_out.size(), 0.0);
            for (size_t q = 0; q < h_trial.size(); q++) {
                double* rec = &ctx->probe_out[5 * q];
                rec[0] = h_trial[q].lml; rec[1] = h_trial[q].delta; rec[2] = h_trial[q].scale;
                rec[3] = (double)h_trial[q].nfev; rec[4] = (double)h_trial[q].use_g;
            }
            for (size_t b = 0; b < h_out.size(); b++) ctx->probe_out[5 * h_trial.size() + b] = (double)h_out[b].rho_index;
            return CRM_OK;
        }
        ctx->probe_out.assign(2 * h_trial.size(), 0.0);
        for (size_t q = 0; q < h_trial.size(); q++) {
            ctx->probe_out[2 * q] = h_trial[q].lml;
            ctx->probe_out[2 * q + 1] = h_trial[q].scale;
        }
    }
    return CRM_OK;
}

// 3.-4. replayed (crm_scan_interaction_permuted): the passes after the first take the rotations at rho* and the fits of
// this block from the first one's record -- neither depends on the permutation hooks
int ScanPass::replay_block(const Block& B) {
    if (ng != 1 || ctx->replay_cursor >= ctx->replay_blocks.size()) {
        set_error("scan: the replayed pass visits a block the recorded one did not");
        return CRM_ERR_INTERNAL;
    }
    crm_ctx::ReplayBlock* rb = ctx->replay_blocks[ctx->replay_cursor++];
    if (rb->col0 != B.col0 || rb->nb != B.nb || rb->collapsed != P.collapsed() || rb->fit.size() != sizeof(NullFitOut) * (size_t)B.nb) {
        set_error("scan: the replayed pass visits its blocks in another order than the recorded one");
        return CRM_ERR_INTERNAL;
    }
    CRM_HIP(hipMemcpyAsync(d_fit, rb->fit.data(), rb->fit.size(), hipMemcpyHostToDevice, st));
    // (unrelated-donor form: the assembly reads Phi'gx and E1'gx of the block from H'Gx -- formed again, same bits)
    // (and nothing after the null fits reads the rotations on that route: no rows recorded, none to put back)
    if (P.wb()) return fold_TH(B);
    hipLaunchKernelGGL(replay_rows_kernel, dim3((unsigned)((P.ldT + 255) / 256), B.nb), dim3(256), 0, st, ctx->ws_T.as<double>(),
                       (long)P.BLK, P.ldT, d_fit, B.nb, (int)P.ldT, rb->T.as<double>(), 1);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

// Phi'gx of the block: per donor U_d Lambda_d^-1/2 applied to its rows of H'Gx (stored transposed)
int ScanPass::woodbury_phi(const Block& B) {
    const long groups = bg->kin_groups;
    phi_recs.resize((size_t)groups);
    GemmProblem p{};
    p.X = ctx->ws_TH.as<double>() + (size_t)bg->kin_k1 * P.ldb; p.ldx = P.ldb; p.C = wb_g; p.ldc = P.ldwb; p.M = B.nb;
    woodbury_records(bg, p, (long)bg->kin_k2 * P.ldb, phi_recs.data());
    // (no with_records: the host is not to wait here, ahead of the step's largest launch -- phi_recs lives as long as
    // the pass and is written again only in the next block, after gene_results has synchronised the stream)
    CRM_TRY(upload(SLOT_KIN, phi_recs.data(), phi_recs.size()));
    return launch_gemm_tn(ctx, d_probs + SLOT_KIN, (int)groups, B.nb, bg->kin_k2, bg->wb_k2pad, false, 0, 1, 0);
}

// 5. the fits of the block on the host (nb*ng*48 bytes cross PCIe): the collapsed path's near flags, the permutation
//    replay's record, the flat-optimum margins
int ScanPass::collect_fits(Block& B) {
    const int nb = B.nb, BLK = P.BLK;
    CRM_HIP(hipMemcpyAsync(h_fit.data(), d_fit, sizeof(NullFitOut) * (size_t)BLK * ng, hipMemcpyDeviceToHost, st));
    if (P.collapsed() && near_out) CRM_HIP(hipMemcpyAsync(h_near.data(), d_near, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
    if (early_pairs()) {
        // (scan_side.hip: the pair products of the block behind the copy -- the host waits for the copy alone and the
        // chip works while it reads the fits and enqueues the pair stage)
        CRM_HIP(hipEventRecord(ctx->ev_fits, st));
        CRM_TRY(launch_early_pairs(B));
        CRM_HIP(hipEventSynchronize(ctx->ev_fits));
    } else
        CRM_HIP(hipStreamSynchronize(st));
    if (P.collapsed() && near_out)
        for (int b = 0; b < nb; b++)
            if (h_near[b]) near_out->push_back(B.done + b);
    for (int gi = 0; gi < ng; gi++)
        for (int b = 0; b < nb; b++) {
            const int ri = h_fit[(size_t)gi * BLK + b].rho_index;
            if (ri < 0 || ri >= nrho) {   // (indexes host arrays below: never trust it unchecked)
                set_error("scan: the null fit of variant %ld (phenotype %d) did not run (grid index %d)", B.col0 + b, gi, ri);
                return CRM_ERR_NUMERIC;
            }
        }
    if (ctx->replay_mode == 1) {
        if (ng != 1) {
            set_error("scan: the permutation replay serves one phenotype per call");
            return CRM_ERR_INTERNAL;
        }
        crm_ctx::ReplayBlock* rb = new crm_ctx::ReplayBlock();
        ctx->replay_blocks.push_back(rb);
        rb->col0 = B.col0; rb->nb = nb; rb->collapsed = P.collapsed();
        rb->fit.resize(sizeof(NullFitOut) * (size_t)nb);
        memcpy(rb->fit.data(), h_fit.data(), rb->fit.size());
        if (!P.wb()) {   // (replay_block: the unrelated-donor form replays no rows)
            CRM_TRY(rb->T.ensure(sizeof(double) * (size_t)nb * P.ldT));
            hipLaunchKernelGGL(replay_rows_kernel, dim3((unsigned)((P.ldT + 255) / 256), nb), dim3(256), 0, st, ctx->ws_T.as<double>(),
                               (long)BLK, P.ldT, d_fit, nb, (int)P.ldT, rb->T.as<double>(), 0);
            CRM_HIP(hipGetLastError());
        }
    }
    // Flat-optimum flag, first half (info calls only; include/crm_hip.h: CRM_MODEL_FLAT_OPTIMUM): how far the search of the
    // selected fit was from taking another path -- the smallest margin of the decisions on objective values that steered
    // it (brent_search.h), in units of the first-order bound on the objective's rounding noise at the optimum
    // (nullfit.hip: cur_noise; select_rho_kernel: decision).  NaN: a fit whose kernel did not measure it.
    for (int gi = 0; gi < ng; gi++) {
        if (!outs[gi].flags) continue;
        if (B.flat_obj.empty()) B.flat_obj.assign((size_t)BLK * ng, -1.0);
        for (int b = 0; b < nb; b++) {
            const double dec = h_fit[(size_t)gi * BLK + b].decision;
            B.flat_obj[(size_t)gi * BLK + b] = dec == dec ? dec : -1.0;
        }
    }
    return CRM_OK;
}

}  // namespace crm
