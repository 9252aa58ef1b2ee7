// The plan of a scan pass (scan_pass.h: ScanPlan): block size, leading dimensions, splits and the route, from the shapes alone.
#include "scan_pass.h"

namespace crm {

// Variants per block of a scan of `count` variants.  Automatic: as many as keep the A~ buffer (block x k0 x ldq doubles)
// within 16 GB, at most 4096 -- fixed per-block costs (host round trip for the rho* groups, small launches, the last, partly
// filled round of workgroups) then weigh 2-3 % less than at 1024.
static bool scan_slow_forms(const crm_gene* g0) {
    // the slower per-variant kernels (more than 144 Gram rows or 128 contexts): their global-memory work space
    return g0->k0 + g0->c + 2 > 144 || g0->k0 > 128 || assemble_rows_scratch_doubles(1, g0->k0, g0->c) > 0;
}
int scan_block_variants(const crm_ctx* ctx, const crm_gene* g0, long count) {
    long auto_blk = (long)(16.0 * (1ull << 30) / (sizeof(double) * (double)g0->k0 * (double)g0->bg->ldq)) / 128 * 128;
    auto_blk = std::max<long>(256, std::min<long>(auto_blk, CRM_MAX_AUTO_BLOCK));
    int BLK = (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : auto_blk, round_up(count, 128));
    if (g0->c > CRM_MAX_COV_WIDE) BLK = std::min(BLK, 512);   // (63 .. 128 covariate columns: the slow null-fit kernel's scratch)
    if (scan_slow_forms(g0)) BLK = std::min(BLK, 512);
    return BLK;
}

static double largest_rank(const crm_background* bg) {   // (at least 1)
    double rbar = 1.0;
    for (int i = 0; i < bg->nrho; i++) rbar = std::max(rbar, (double)bg->r[i]);
    return rbar;
}

ScanPlan plan_scan(const std::vector<crm_gene*>& genes, const crm_panel* panel, const int* idx_G, bool allow_collapse,
                          long count) {
    const crm_gene* g0 = genes[0];
    const crm_background* bg = g0->bg;
    const crm_ctx* ctx = bg->ctx;
    const int ng = (int)genes.size(), nrho = bg->nrho, c = g0->c, k0 = g0->k0;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    ScanPlan P;
    P.ng = ng;
    P.slow_forms = scan_slow_forms(g0);
    const int BLK = P.BLK = scan_block_variants(ctx, g0, count);
    // Several phenotypes: the pair-ordered buffers (A~ and, on the routes through H, its gathered operand) grow with the
    // number of distinct (variant, rho*) pairs, up to min(nrho, ng) per variant.  They are kept within 128 GB (under half of the
    // device) by running the pair stage of a block -- steps 5 to 11 -- over sub-ranges of its variants, while the stages
    // before it (block copies, rotations and, above all, the per-phenotype null fits, which run twice as fast per variant in
    // launches of 4096 variants as in launches of 2048) keep the full block.
    P.pair_cap = BLK;
    if (ng > 1) {
        const char* cap_env = getenv("CRM_PAIR_BUFFER_GB");
        const double cap_gb = cap_env && atof(cap_env) > 0 ? atof(cap_env) : 128.0;
        const double per_pair = 2.0 * sizeof(double) * k0 * (double)ldq;
        const long most = (long)std::min(nrho, ng) * BLK, least = (long)std::min(nrho, ng) * std::min(BLK, 128);
        P.pair_cap = (int)std::max<long>(least, std::min<long>(most, (long)(cap_gb * (1ull << 30) / per_pair)));
    }
    const int max_pairs = P.pair_cap;
    P.ldb = BLK + 128;              // slack columns for the Khatri-Rao tile over-read
    P.ldp = max_pairs + 128;        // pair-ordered copy of the block
    P.ldA = P.ldT = ldq;
    P.npair = k0 * (k0 + 1) / 2;
    P.ldZ1 = round_up((long)k0 * (1 + c), 128), P.ldZ2 = round_up(k0, 128), P.ldZ3 = round_up(P.npair, 128);
    P.KT = k0 + c + 2;
    P.ld_gW = round_up(std::max(c, CRM_MAX_COV), 8);
    const int mt_blk = (BLK + GEMM_BM - 1) / GEMM_BM;
    // Z1 = Gt' [y o E, W o E] of all phenotypes in ONE batched launch per block (a problem per phenotype, each with its own
    // output region) instead of a skinny launch + reduction per phenotype -- at config 4 those 64 pairs of launches were an
    // eighth of the scan.  The slices along the cell axis shrink with the number of problems.
    P.ks1 = split_for(np, (long)mt_blk * (P.ldZ1 / GEMM_BN) * ng);
    P.ks2 = split_for(np, (long)mt_blk * (P.ldZ2 / GEMM_BN));
    P.ks3 = split_for(np, (long)mt_blk * (P.ldZ3 / GEMM_BN));
    // H'G of step 3: few output tiles (cols x block) against a long contraction (cells) -- slices along the cell axis
    // until the launch fills the chip twice with 128-wide tiles (mode B at config 3: 64 tiles, cfg3 mode C: 320)
    // (rows of the operand of the rotations' Mix products: the half factor's columns, or -- folded kinship structure,
    // objects.h: kin_fold -- k1 + donors k2)
    // (unrelated-donor form: the per-donor rotations read up to a stage past the last donor's rows -- zeros)
    P.th_slab = std::max<long>(bg->ldh, bg->kin && bg->kin_fold ? bg->kin_kdim + (bg->kin_wb ? GEMM_BK : 0) : 0) * P.ldb;
    if (bg->fast_T) {
        const long tiles_h = (long)((bg->cols + GEMM_BM - 1) / GEMM_BM) * ((BLK + 127) / 128);
        while (tiles_h * P.ks_h < 1024 && P.ks_h < 16 && np / GEMM_BK / (P.ks_h + 1) >= 16) P.ks_h++;
    }
    // donor-collapsed mode: exact when every variant is constant within the panel's groups and the
    // genotype permutation hook is not in use
    const bool grouped = panel->grouped;
    const size_t bd_bytes = grouped ? sizeof(double) * (size_t)nrho * panel->m_pad * k0 * ldq : 0;
    // (with the genotype permutation hook the test direction is constant within the permuted groups;
    // its mixed table needs the indicators as Khatri-Rao "contexts": m <= 128)
    const bool collapsed = grouped && ctx->collapse && allow_collapse && bd_bytes <= ((size_t)48 << 30) &&
                           (!idx_G || panel->m <= 128);
    P.fastT = !collapsed && bg->fast_T && ctx->fast_T;
    P.cross = collapsed && idx_G;
    P.mp = grouped ? panel->m_pad : 0;
    P.xrows = collapsed ? P.mp : np;
    P.ld_ah = round_up((long)BLK * k0, 128) + 128, P.ld_xg = round_up((long)max_pairs * k0, 128) + 128;
    // Kinship-structure route (objects.h, crm_background::kin): H'(g o E0) donor by donor, then Mix(rho*)' -- the dense
    // scan's default whenever the background knows the donor structure of its kinship factor.  S: per-donor sums.
    P.KK = bg->kin ? bg->kin_k1 + bg->kin_k2 : 0;   // rows of S per donor: [us | E1]
    // folded form (objects.h: kin_fold): S holds [E1 rows ; (donor, us_j) rows] and is the operand of the Mix product itself
    const bool fold = bg->kin && bg->kin_fold;
    P.s_rows = fold ? bg->kin_kdim + (bg->kin_wb ? GEMM_BK : 0) : 0;
    P.s_bytes = !bg->kin ? 0 : sizeof(double) * (fold ? (size_t)P.s_rows : (size_t)bg->kin_groups_pad * P.KK) * P.ld_ah;
    // The route pays when its flops per variant -- per-donor sums over runs padded to whole 16-cell stages, the E1 rows /
    // the contraction over the donors, and the product with the mixing matrix -- stay under the direct contraction's
    // 2 n r k0 (thousands of tiny donors: every run is mostly padding); a multi-gene test that forces one of the other
    // two routes (crm_test_set_shared_h 0 / 1) gets that route.
    bool kin_pays = false;
    if (bg->kin) {
        const double rbar = largest_rank(bg);
        const double kk = fold ? (double)bg->kin_kdim : (double)bg->ldh;
        const double prep = fold ? 2.0 * bg->kin_rows * bg->kin_k2 + 2.0 * (double)np * bg->kin_k1
                                 : 2.0 * bg->kin_rows * P.KK + 2.0 * (double)bg->kin_groups_pad * bg->kin_cols * bg->kin_k2;
        kin_pays = prep + 2.0 * kk * rbar < 0.9 * 2.0 * (double)n * rbar || ctx->kin_route >= 2;
    }
    const bool kin_route = bg->kin && P.fastT && ctx->kin_route > 0 && kin_pays && !(ng > 1 && ctx->tune.shared_h >= 0) &&
                           P.s_bytes <= ((size_t)48 << 30);
    const bool kfold = kin_route && fold;
    // Unrelated donors (objects.h: kin_wb): Q and F through the per-donor Woodbury inverse, no A~ = MixK(rho*)'S.  Decided
    // by the background and the shapes alone, so that every entry point and every block computes a variant alike.  Taken
    // where the Gram over the donors k2 positions with k1 more rows costs less than the MixK product it replaces.
    const int wb_k1 = bg->kin ? bg->kin_k1 : 0;
    bool wb = false;
    // (k0 + c + 2 + k1 <= 144: the single-workgroup Gram forms; wider shapes keep the MixK route.  c + 1 <= 128: this
    // route keeps [y | W] and its products in tables of 128 columns (prepare_woodbury: yWk, Bk, E1'[y, W]), so
    // c = CRM_MAX_COV_XWIDE = 128, whose [y | W] has 129, stays on the MixK route)
    constexpr int WB_MAX_ROWS = 144;
    if (kfold && bg->kin_wb && !P.slow_forms && c + 1 <= 128 && P.KT + wb_k1 <= WB_MAX_ROWS &&
        woodbury_lds_bytes(P.KT, wb_k1) <= 150 * 1024) {
        // (8x: the per-block rotations and the capacitance solves are fixed costs that small products do not repay --
        // mode B at config 3, 150 x 150 spectra: 328 000 -> 222 000 variant-tests/s at 1x)
        wb = (double)bg->kin_kdim * largest_rank(bg) * k0 > 8.0 * (P.KT + wb_k1) * (P.KT + wb_k1) * (double)bg->wb_P ||
             form("kin_diag", 1) >= 2;
    }
    P.route = collapsed ? Route::collapsed : wb ? Route::unrelated : kfold ? Route::kin_folded
            : kin_route ? Route::kin_unfolded : Route::direct;
    P.ldAw = wb ? std::max<long>(P.ldA, bg->wb_ldp) : P.ldA;   // (rows of the rotated S: donors k2 positions)
    P.ldwb = wb ? bg->wb_ldp : 0;
    P.kdim = kfold ? bg->kin_kdim : bg->ldh;
    // E1 rows of step 6: as a plain product G'P with the pair products P = E1_a o E0_i (n x k1 k0; the contraction kernel's
    // best form) followed by a re-ordering of its rows, unless P would be large (> 8 GB): then as a Khatri-Rao contraction
    // over all cells with the transposed store (64-wide tiles when k1 <= 64: 50 of 64 columns at config 3)
    P.ldP = round_up((long)(bg->kin ? bg->kin_k1 : 0) * k0, 128);
    P.e1_pairs = kfold && sizeof(double) * (double)np * (double)P.ldP <= 8.0 * (1ull << 30);
    if (kfold) {   // cell-axis slices of the folded form's all-cells launches for the E1 rows (few output tiles, long contraction)
        const long tiles6 = P.e1_pairs ? ((long)BLK + GEMM_BM - 1) / GEMM_BM * (P.ldP / 128) : ((long)BLK * k0 + GEMM_BM - 1) / GEMM_BM;
        const long slots6 = P.e1_pairs || bg->kin_k1 > 64 ? 512 : 768;
        double best = 0.0;
        for (int sps = 1; sps <= 8 && np / GEMM_BK / sps >= 64; sps++) {
            const double rounds = (double)(tiles6 * sps) / (double)slots6, eff = rounds / std::ceil(rounds);
            if (eff > best + 0.02) { best = eff; P.fold_split6 = sps; }
        }
        const long tiles3 = (long)((bg->kin_k1 + GEMM_BM - 1) / GEMM_BM) * ((BLK + 127) / 128);
        while (tiles3 * P.fold_split3 < 1024 && P.fold_split3 < 16 && np / GEMM_BK / (P.fold_split3 + 1) >= 16) P.fold_split3++;
    }
    // E1 = E, the reference's default (and no context permutation): the pair features E1_a o E0_i are the symmetric
    // E_a E_i that the scan holds anyway for E0'diag(g^2)E0 (EE: k0 (k0 + 1) / 2 columns) -- half the product
    P.e1_sym = P.e1_pairs && bg->kin_k1 == k0;
    // The kinship term's contexts are E as well (the reference's default E2 = E): the per-donor sums S_d = sum_c g_c e_c e_c'
    // are symmetric -- one batched product per donor against E (x) E in donor order, half the flops of the Khatri-Rao form and
    // a plain product, then a pass that writes the rows of S (blockops.hip: donor_pairs_expand_kernel); the E1 rows are the
    // sum of those products over the donors, so their product over all cells goes as well.  Taken where its time is the
    // smaller one (many tiny donors: the pass over S costs more than the products save).
    P.ldPd = round_up((long)P.npair, 128);
    P.pd_slab = (std::max<long>(BLK, max_pairs) + 128) * P.ldPd;
    if (P.e1_sym && bg->kin_k2 == k0 && donor_pairs_serves(k0) && form("donor_pairs", 1)) {
        const double peak = 78.6e12, hbm = 4.0e12;
        const double t_kr = 2.0 * bg->kin_rows * (double)k0 * k0 / (0.6 * peak) + 2.0 * (double)np * P.npair / (0.92 * peak);
        const double t_pairs = 2.0 * bg->kin_rows * (double)P.npair / (0.8 * peak) +
                               (double)bg->kin_groups * (2.0 * P.npair + (double)k0 * k0) * sizeof(double) / hbm;
        const bool fits = sizeof(double) * (double)bg->kin_groups * (double)P.pd_slab <= 8.0 * (1ull << 30);
        P.donor_pairs = fits && (t_pairs < t_kr || form("donor_pairs", 1) >= 2);
        // the expansion pass: four variants per workgroup, three workgroups per CU -- donor ranges fill its rounds
        const long wgs = (std::max<long>(BLK, 1) + 3) / 4;
        while ((wgs * P.donor_pair_splits) % 768 != 0 && wgs * P.donor_pair_splits < 4 * 768 && P.donor_pair_splits < 8 &&
               P.donor_pair_splits < bg->kin_groups)
            P.donor_pair_splits++;
    }
    // Unrelated-donor form with the pair products: the rotated S of every donor, (U_d Lambda_d^-1/2)' S_d, is formed from P_d
    // in one pass (blockops.hip: donor_pairs_rotate_kernel) instead of the rows of S and a per-donor product over them --
    // bit for bit the same ws_A; form("donor_pairs_rotate", 0) keeps the two launches
    P.wb_rotate = wb && P.donor_pairs && donor_pairs_rotate_serves(k0) && form("donor_pairs_rotate", 1) != 0;
    // Unrelated-donor form: nothing reads the block in rho*-sorted pair order (no MixK(rho*) product), so the pair stage runs
    // in block order for one phenotype as it does for several; form("wb_block_order", 0) keeps the sorted copy
    P.wb_block = wb && (ng > 1 || form("wb_block_order", 1) != 0);
    // The same idea on the UNFOLDED kinship-structure route (few contexts: BASELINE config 2's 20): with E1 = E2 = E the
    // per-donor blocks [us | E1]'(g o E0) are one symmetric matrix S_d = sum_c g_c e_c e_c' twice over -- one batched plain
    // product per donor against E (x) E in donor order (P_d), the contraction over the donors with the kinship factor ON THE
    // PAIR PRODUCTS (Z_c = sum_d hKd[d, c] P_d: 210 columns per variant instead of 400, and the column of ones behind hKd
    // gives the sum over the donors that the E1 rows are), then the rows of AH = H'(g o E0) written from Z in one pass --
    // instead of the Khatri-Rao launch per donor (64-wide tiles a third full), the contraction over the donors on k0 x k0
    // blocks and the E1 sums.  Config 2: 1.7 -> 0.7 ms of a 8.6 ms step.
    if (kin_route && !kfold && bg->kin_k1 == k0 && bg->kin_k2 == k0 && donor_pairs_serves(k0) && form("donor_pairs", 1) &&
        bg->kin_cols + 1 <= bg->kin_ldh) {
        const double cost_kr = 2.0 * bg->kin_rows * (double)P.KK * k0 + 2.0 * (double)bg->kin_groups_pad * bg->kin_cols * bg->kin_k2 * k0;
        const double cost_pairs = 2.0 * bg->kin_rows * (double)P.npair + 2.0 * (double)(bg->kin_cols + 1) * bg->kin_groups_pad * (double)P.ldPd;
        const bool fits = sizeof(double) * (double)bg->kin_groups_pad * (double)P.pd_slab <= 8.0 * (1ull << 30) &&
                          sizeof(double) * (double)(bg->kin_cols + 1) * (double)P.pd_slab <= (double)P.s_bytes;
        P.pairs_unfolded = fits && (cost_pairs < 0.8 * cost_kr || form("donor_pairs", 1) >= 2);
    }
    P.skip_pairs = form("pairs_without_kinship_term", 1) != 0;
    P.kin_probs = bg->kin ? bg->kin_groups * (bg->kin_wb ? 2 : 1) + bg->kin_k2 + 16 : 0;
    P.side_probs = wb ? (int)bg->kin_groups + 3 : 0;   // (scan_side.hip: the donors' pair products, Z2, Z3, Z1)
    return P;
}

}  // namespace crm
