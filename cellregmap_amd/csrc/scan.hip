// Host orchestration of the interaction scan behind the C-ABI: the scan plan and the per-block kernel pipeline
//   stats -> T(rho) = G' Q0(rho) -> null fits + rho* -> sort by rho* -> Khatri-Rao contraction
//   -> side contractions -> assemble (Q, F) -> eigenvalues + Davies.
// Reference loop being replaced: cellregmap/_cellregmap.py:340-436.  The objects it works on are built elsewhere:
// background.hip, kinship.hip, gene.hip, panel.hip, donor_tables.hip.
#include <algorithm>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace crm {

static int ctx_cus(const crm_ctx* ctx) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
    return cus;
}

// Collapsed path: a variant that keeps less than this share of its squared norm outside span(W) is repeated on the dense
// path (the donor-level sums can only form [W, g]'K^-1[W, g] in the raw basis: eps / share instead of eps / sqrt(share))
constexpr double COLLINEAR_TAU = 1e-2;

// Fit records of the flat-optimum probes (include/crm_hip.h: CRM_MODEL_FLAT_OPTIMUM): delta moved by one stopping
// tolerance of the reference's search on x = logit(delta) (brent-search: tol = 1e-6 |x| + 1e-6), unit scale -- the
// assembly derives the scale at that delta itself (assemble.hip: fit.scale < 0).
__global__ void flat_probe_fit_kernel(const crm::NullFitOut* __restrict__ fit, int count, double sign,
                                      crm::NullFitOut* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    crm::NullFitOut f = fit[b];
    const double tiny = 2.220446049250313e-16;
    const double d = fmin(fmax(f.delta, tiny), 1.0 - tiny);
    const double x = log(d) - log1p(-d);
    const double tol = 1e-6 * fabs(x) + 1e-6;
    const double dp = fmin(fmax(1.0 / (1.0 + exp(-(x + sign * tol))), tiny), 1.0 - tiny);
    f.delta = dp;
    f.v0 = 1.0 - dp;
    f.v1 = dp;
    f.scale = -1.0;
    out[b] = f;
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

// How far apart may two faithful runs of the reference's null fit stop (include/crm_hip.h: crm_scan_interaction_bounds)?
// Measured on device-vs-oracle streams of 71 000 scans (tools/diag/flat_flag_study.py, profiles/r06_flat_flag_*): the
// distance of the two stopping points in units of the search's tolerance, times the relative gain of the objective over one
// tolerance at the stopping point (NullFitTrial::curv / |lml|), never exceeded 2.2e-13 (99.9 %: 1.2e-13, 99 %: 6e-14,
// median 4e-19): the flatter the likelihood, the further rounding noise moves the last parabolic steps -- up to one whole
// tolerance, where the search's last comparison f(x +- tol) <= f(x) itself falls the other way.
constexpr double STOP_SHIFT_C = 2.5e-13;
// ... and a decision of the search counts as open to rounding outright (shift = one tolerance) when its margin is within
// this many times the first-order noise bound of the objective (nullfit.hip: objective_noise_bound); the choice of rho*
// likewise (CRM_MODEL_RHO_TIE)
constexpr double FLAT_KAPPA = 1.0;
constexpr double RHO_KAPPA = 1.0;
constexpr int FLAT_REC = 10;   // doubles per variant of the diagnostics record (crm_test_null_fit_probe_read)

struct ScanOut {  // per-gene output bases (host), each `count` long (lambda: count*k0, F: count*k0*k0)
    double *pv, *rho1, *e2, *g2, *eps2, *Q, *lml, *delta, *scale, *lambda, *F;
    int* ifault = nullptr;   // Davies' fault code per variant (0 ok; 1, 2, 4 as AS 155; < 0: no usable eigenvalues)
    double* liu = nullptr;   // the modified-Liu p-value (chiscore's info["liu_pval"])
    int* flags = nullptr;    // CRM_MODEL_* bits per variant (include/crm_hip.h)
    double* bound_Q = nullptr;   // crm_scan_interaction_bounds: how far Q / p of two faithful runs may differ (relative)
    double* bound_p = nullptr;
    bool exact = false;      // the p-value by the exact tail method (tail_pvalue.hip) instead of Davies / Liu
    double* logp = nullptr;  // exact method: log p and CRM_TAIL_* status per variant
    int* status = nullptr;
};

// Variants per block of a scan of `count` variants.  Automatic: as many as keep the A~ buffer (block x k0 x ldq doubles)
// within 16 GB, at most 4096 -- fixed per-block costs (host round trip for the rho* groups, small launches, the last, partly
// filled round of workgroups) then weigh 2-3 % less than at 1024.
static bool scan_slow_forms(const crm_gene* g0) {
    // the slower per-variant kernels (more than 144 Gram rows or 128 contexts): their global-memory work space
    return g0->k0 + g0->c + 2 > 144 || g0->k0 > 128 || assemble_rows_scratch_doubles(1, g0->k0, g0->c) > 0;
}
static int scan_block_variants(const crm_ctx* ctx, const crm_gene* g0, long count) {
    long auto_blk = (long)(16.0 * (1ull << 30) / (sizeof(double) * (double)g0->k0 * (double)g0->bg->ldq)) / 128 * 128;
    auto_blk = std::max<long>(256, std::min<long>(auto_blk, CRM_MAX_AUTO_BLOCK));
    int BLK = (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : auto_blk, round_up(count, 128));
    if (g0->c > CRM_MAX_COV_WIDE) BLK = std::min(BLK, 512);   // (63 .. 128 covariate columns: the slow null-fit kernel's scratch)
    if (scan_slow_forms(g0)) BLK = std::min(BLK, 512);
    return BLK;
}

// How the rotated test direction A~ = Q0(rho*)'(g o E0) of step 6 is formed -- and with it the rotations of step 3 and the
// operands the pass prepares
enum class Route {
    collapsed,      // donor-level tables of a grouped panel (crm_donor_tables)
    direct,         // Khatri-Rao contraction over all cells; several phenotypes decide per block whether to go through H
    kin_unfolded,   // kinship structure (objects.h: crm_background::kin): per-donor sums, then the contraction over the donors
    kin_folded,     // ... the donors folded into the mixing matrices (objects.h: kin_fold): the sums are the Mix operand
    unrelated,      // ... unrelated donors (objects.h: kin_wb): Q and F through Woodbury, the rotated S instead of A~
};

// Slots of the pass's problem records (ctx->ws_probs): [0] a single product -- in step 6 the A~ groups, then their tails;
// from 1 the rotations of step 3 (the side contractions at 1 and 2): the batched launch's problems, behind them the cut ones,
// behind those the spectrum tails -- each a part of one of the nrho products, so at most 2 nrho records; from SLOT_KIN
// the records of the kinship-structure routes (ScanPlan::kin_probs); after those, the Z1 problems
constexpr int SLOT_ONE = 0, SLOT_RHO = 1, SLOT_KIN = 2 * CRM_MAX_RHO + 4;

// What a pass does: sizes, leading dimensions, splits and the route, fixed before anything is launched (plan_scan).
// e1_sym, donor_pairs, pairs_unfolded and wb_rotate hold what the shapes allow until prepare_kinship has probed the data.
// What depends on the rho* of a block (through H or not, the splits of the A~ launch, the cut problems) is decided per block.
struct ScanPlan {
    Route route = Route::direct;
    // fastT: T(rho) through the half factor H (H'G, then small products with Mix(rho)); slow_forms: scan_slow_forms;
    // skip_pairs: ScanPass::no_kinship_term; cross: the collapsed path under the genotype permutation hook
    bool fastT = false, slow_forms = false, skip_pairs = true, cross = false;
    bool e1_pairs = false, e1_sym = false, donor_pairs = false, wb_rotate = false, pairs_unfolded = false;
    bool wb_block = false;   // unrelated-donor form: the pair stage in block order (always so with several phenotypes)
    int ng = 1, BLK = 0, pair_cap = 0;
    long ldb = 0, ldp = 0, ldA = 0, ldAw = 0, ldT = 0, ldZ1 = 0, ldZ2 = 0, ldZ3 = 0, ld_ah = 0, ld_xg = 0, ldP = 0, ldPd = 0,
         pd_slab = 0, ldwb = 0, ld_gW = 0, th_slab = 0, s_rows = 0;
    size_t s_bytes = 0;
    int ks1 = 1, ks2 = 1, ks3 = 1, ks_h = 1, fold_split6 = 1, fold_split3 = 1, donor_pair_splits = 1;
    int npair = 0, KT = 0, KK = 0, kin_probs = 0;
    // kdim: contraction length of the products with the mixing matrices; mp: groups of a grouped panel, padded; xrows:
    // contraction length of the block products -- cells, or on the collapsed path the groups
    long kdim = 0, mp = 0, xrows = 0;
    bool collapsed() const { return route == Route::collapsed; }
    bool kin() const { return route == Route::kin_unfolded || route == Route::kin_folded || route == Route::unrelated; }
    bool folded() const { return route == Route::kin_folded || route == Route::unrelated; }
    bool wb() const { return route == Route::unrelated; }
    bool through_H() const { return fastT && (ng > 1 || kin()); }   // (the operands of the routes through H exist)
    int z1_slot() const { return SLOT_KIN + kin_probs; }
};

static double largest_rank(const crm_background* bg) {   // (at least 1)
    double rbar = 1.0;
    for (int i = 0; i < bg->nrho; i++) rbar = std::max(rbar, (double)bg->r[i]);
    return rbar;
}

static ScanPlan plan_scan(const std::vector<crm_gene*>& genes, const crm_panel* panel, const int* idx_G, bool allow_collapse,
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
    return P;
}

// Records of one product per donor over the donor's own run of cells (kin_row0 / kin_len): the operands X, E and Y of p
// start at the run's first row, C at d c_step.  Returns the longest run (the launch's contraction length).
static long donor_run_records(const crm_background* bg, const GemmProblem& p, long c_step, GemmProblem* out) {
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
static void woodbury_records(const crm_background* bg, const GemmProblem& p, long x_step, GemmProblem* out) {
    for (long d = 0; d < bg->kin_groups; d++) {
        GemmProblem q = p;
        q.X = p.X + d * x_step; q.Y = bg->wb_U.as<double>() + (size_t)d * bg->wb_k2pad * 128; q.ldy = 128;
        q.C = p.C + d * bg->kin_k2; q.N = bg->kin_k2; q.cells = bg->wb_k2pad;
        out[d] = q;
    }
}

// Does every pair of operands hold the same first k columns?  (the probes of the pair-product forms; one flag for all)
struct SameColumns { const double* A; long lda; const double* B; long ldb; long rows; };
static int same_columns(hipStream_t st, int* d_flag, int k, std::initializer_list<SameColumns> pairs, bool& same) {
    int h_flag = 0;
    CRM_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    for (const SameColumns& q : pairs) CRM_TRY(launch_same_columns(st, q.A, q.lda, q.B, q.ldb, q.rows, k, d_flag));
    CRM_HIP(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    same = h_flag == 0;
    return CRM_OK;
}

struct Block {      // variants [col0, col0 + nb) of the panel, `done` into the call
    long done = 0, col0 = 0;
    int nb = 0;
    double* Gb = nullptr;   // the aligned copy (collapsed path: the group dosage slab)
    double* Gt = nullptr;   // the test direction's role (rows permuted under the genotype hook)
    double* Gx = nullptr;   // the fixed effects' role (orthogonalised against W)
    std::vector<double> flat_obj;   // (info calls) the selected fits' decision margins, [ng][BLK]
};
struct SubRange {   // the pair stage's part of a block: its positions [b0, b0 + nb), `done` into the call
    int b0 = 0, nb = 0;
    long done = 0;
};
struct Pairs {      // the sub-range's (variant, rho*) pairs in rho order: cnt[i] of them from start[i]
    int cnt[CRM_MAX_RHO] = {0}, start[CRM_MAX_RHO + 1] = {0}, npairs = 0;
};
struct AGroups {    // step 6's problems: [0, nz) in probs, their tails, the splits along the cell axis
    int nz = 0, max_m = 0, max_n = 1, kr_split = 1, tail_split = 1, tail_maxn = 0;
    double kr_flops = 0.0;
    size_t a_slab = 0;
    std::vector<GemmProblem> tails, spectrum_tails;
};

// One pass: its inputs, plan, workspaces and host scratch, and a member function per stage
struct ScanPass {
    const std::vector<crm_gene*>& genes;
    crm_panel* panel;
    const long first, count;
    const int *idx_E, *idx_G;
    const std::vector<ScanOut>& outs;
    std::vector<long>* near_out;
    const int ng;
    crm_gene* const g0;
    crm_background* const bg;
    crm_ctx* const ctx;
    const hipStream_t st;
    const long n, np, ldq, slab;
    const int nrho, c, k0;
    ScanPlan P;
    int *d_idxE = nullptr, *d_idxG = nullptr;
    const double *d_Ep = nullptr, *d_EE = nullptr;   // the permuted contexts and their pair products E (x) E, shared by the genes
    crm_donor_tables* tab = nullptr;   // phenotype-free donor tables of this call (collapsed path)
    // workspaces (workspaces())
    GemmProblem* d_probs = nullptr;
    double *dZ1 = nullptr, *dZ2 = nullptr, *dZ3 = nullptr;
    long z1_sz = 0, z2_sz = 0, z3_sz = 0;
    double *d_gg, *d_gy, *d_gW, *d_Q, *d_pv, *d_lam, *d_liu, *d_part, *d_coef, *d_thr, *d_tp, *d_tlp;   // (ws_small)
    int *d_pos, *d_ord, *d_if, *d_drop, *d_near, *d_posw, *d_tst;
    NullFitTrial* d_trial;
    NullFitOut* d_fit;
    unsigned* d_queue;
    double *wb_yW = nullptr, *wb_E1yW = nullptr, *wb_g = nullptr, *wb_Gw = nullptr, *wb_tmp = nullptr;
    // host scratch of the pass
    std::vector<NullFitOut> h_fit = std::vector<NullFitOut>((size_t)P.BLK * ng);
    std::vector<int> h_pos = std::vector<int>((size_t)P.BLK * ng), h_ord = std::vector<int>(P.pair_cap);
    std::vector<GemmProblem> probs = std::vector<GemmProblem>(CRM_MAX_RHO + 4);
    std::vector<int> pair_of = std::vector<int>((size_t)nrho * P.BLK), h_near = std::vector<int>(P.BLK);
    bool rho0_pos[CRM_MAX_RHO] = {false};   // grid points whose null fits of this block read the position basis (plan_rotations)
    std::vector<GemmProblem> rot_tails;     // the rotations' spectrum tails of the block (plan_rotations)
    std::vector<GemmProblem> phi_recs;      // the donors' records of Phi'gx of the block (woodbury_phi)

    ScanPass(const std::vector<crm_gene*>& genes_, crm_panel* panel_, long first_, long count_, const int* idx_E_,
             const int* idx_G_, const std::vector<ScanOut>& outs_, bool allow_collapse, std::vector<long>* near_out_)
        : genes(genes_), panel(panel_), first(first_), count(count_), idx_E(idx_E_), idx_G(idx_G_), outs(outs_),
          near_out(near_out_), ng((int)genes_.size()), g0(genes_[0]), bg(g0->bg), ctx(bg->ctx), st(ctx->stream), n(bg->n),
          np(bg->n_pad), ldq(bg->ldq), slab((long)(1 + g0->c) * bg->ldq), nrho(bg->nrho), c(g0->c), k0(g0->k0),
          P(plan_scan(genes_, panel_, idx_G_, allow_collapse, count_)) {}

    // ---- helpers --------------------------------------------------------------------------------------------------------
    int upload(int slot, const GemmProblem* p, size_t k) {
        CRM_HIP(hipMemcpyAsync(d_probs + slot, p, sizeof(GemmProblem) * k, hipMemcpyHostToDevice, st));
        return CRM_OK;
    }
    // records of this stack frame at a slot: `launches` reads them from d_probs + slot; the stream is synchronised after
    // them, before the host copy goes away
    template <class F>
    int with_records(int slot, const std::vector<GemmProblem>& kp, F&& launches) {
        CRM_TRY(upload(slot, kp.data(), kp.size()));
        CRM_TRY(launches(d_probs + slot));
        CRM_HIP(hipStreamSynchronize(st));
        return CRM_OK;
    }
    // the kernel timer (crm_ctx::timed): the event pair of the next timed launch, its start recorded now or by the caller
    int timer_open(bool record_start) {
        if (ctx->timed_used == ctx->timed.size()) {
            hipEvent_t a, b;
            CRM_HIP(hipEventCreate(&a));
            CRM_HIP(hipEventCreate(&b));
            ctx->timed.emplace_back(a, b);
        }
        if (record_start) CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].first, st));
        return CRM_OK;
    }
    int timer_close() {
        CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].second, st));
        ctx->timed_used++;
        return CRM_OK;
    }
    // A fit that ends with (practically) no kinship term -- delta at the upper clamp, v0 = 2.2e-16 scale: a phenotype without
    // a random effect, half of an eQTL run -- has K0 = v1 (I + (v0 / v1) Q0 S0 Q0'): where (v0 / v1) max S0 <= 1e-10 the
    // rotated test direction A~ enters Q and F with weights d_j <= 1e-10, below the tolerance of the test by four orders of
    // magnitude, while its product is most of a step.  Such tests get no (variant, rho*) pair: their Gram reads rows of zeros
    // (AssembleArgs::A_none).  rho* of such a fit is decided by rounding (the likelihood is flat in rho), so over many
    // phenotypes these are also the fits that would scatter a variant's pairs over the whole grid.
    bool no_kinship_term(const NullFitOut& f) const {
        return P.skip_pairs && f.v1 > 0.0 && f.v0 >= 0.0 && f.v0 * bg->s0_max[f.rho_index] <= 1e-10 * f.v1;
    }

    // ---- workspaces -----------------------------------------------------------------------------------------------------
    int workspaces() {
        const int BLK = P.BLK, max_pairs = P.pair_cap;
        const long ldb = P.ldb;
        CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)nrho * BLK * P.ldT));
        // (unrelated-donor form: the rotated S stays in block order for several phenotypes -- BLK of them at most)
        CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)(P.wb() ? std::max(max_pairs, BLK) : max_pairs) * k0 * P.ldAw));
        CRM_TRY(ctx->ws_Anone.ensure(sizeof(double) * (size_t)P.ldAw));
        CRM_HIP(hipMemsetAsync(ctx->ws_Anone.ptr, 0, sizeof(double) * (size_t)P.ldAw, st));
        CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
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
            CRM_HIP(hipMemsetAsync(ctx->ws_TH.ptr, 0, sizeof(double) * (size_t)P.th_slab, st));
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
    int context_features(bool shared_too) {
        for (int gi = 0; gi < ng; gi++) {
            crm_gene* g = genes[gi];
            const bool both = gi == 0 && shared_too;
            CRM_TRY(g->YE.ensure(sizeof(double) * np * g->ld_ye));
            if (both) {
                CRM_TRY(g->Ep.ensure(sizeof(double) * np * g->ld_ep));
                CRM_TRY(g->EE.ensure(sizeof(double) * np * g->ld_ee));
            }
            CRM_TRY(launch_context_features(st, g->E0.as<double>(), g->lde, d_idxE, n, np, k0, g->yW.as<double>(),
                                            g->yW.as<double>() + 1, g->ld_yw, c,
                                            both ? g->Ep.as<double>() : nullptr, g->ld_ep, g->YE.as<double>(),
                                            g->ld_ye, both ? g->EE.as<double>() : nullptr, g->ld_ee));
        }
        if (shared_too) {
            d_Ep = g0->Ep.as<double>();
            d_EE = g0->EE.as<double>();
        }
        return CRM_OK;
    }

    // context features for this permutation (E, E (x) E shared; y o E per gene) and the collapsed path's donor tables
    int prepare_contexts() {
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
    int prepare_kinship() {
        const long ldh = bg->ldh;
        const double* H = bg->H.as<double>();
        if (P.kin()) {   // the (permuted) contexts in donor order
            CRM_TRY(g0->kinEp.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ep));
            CRM_TRY(launch_gather_rows(st, d_Ep, g0->ld_ep, bg->kin_map.as<int>(), bg->kin_rows, (int)g0->ld_ep,
                                       g0->kinEp.as<double>(), g0->ld_ep));
        }
        if (P.folded() && bg->kin_k2 == 1) {
            // one column of us: S[(k1 + d'), (b, i)] = sum over the cells of donor d' of us(c) g_b(c) E0(c, i) is the plain product
            // G_d'' (us o E0)_d' of the donor's own cells -- its (b, i) layout is the row of S as it stands.  kinUE = us o E0 in
            // donor order.
            CRM_TRY(g0->kinUE.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ep));
            CRM_TRY(launch_scale_rows(st, g0->kinEp.as<double>(), g0->ld_ep, bg->kin_Y.as<double>(), bg->kin_ldy, bg->kin_rows,
                                      (int)g0->ld_ep, g0->kinUE.as<double>(), g0->ld_ep));
        }
        const SameColumns e1_is_E{H, ldh, d_Ep, g0->ld_ep, n};   // E1 = E
        const SameColumns us_is_E{bg->kin_Y.as<double>(), bg->kin_ldy, g0->kinEp.as<double>(), g0->ld_ep, bg->kin_rows};   // E2 = E
        if (P.e1_sym) CRM_TRY(same_columns(st, d_near, k0, {e1_is_E}, P.e1_sym));
        if (P.e1_pairs && !P.e1_sym) {
            CRM_TRY(g0->kinP.ensure(sizeof(double) * (size_t)np * P.ldP));
            CRM_TRY(launch_pair_features(st, H, ldh, bg->kin_k1, d_Ep, g0->ld_ep, k0, np, g0->kinP.as<double>(), P.ldP));
        }
        P.donor_pairs = P.donor_pairs && P.e1_sym;
        if (P.donor_pairs) CRM_TRY(same_columns(st, d_near, k0, {us_is_E}, P.donor_pairs));
        if (P.pairs_unfolded) CRM_TRY(same_columns(st, d_near, k0, {e1_is_E, us_is_E}, P.pairs_unfolded));
        P.wb_rotate = P.wb_rotate && P.donor_pairs;
        if (P.donor_pairs || P.pairs_unfolded) {   // (the folded and the unfolded form respectively)
            CRM_TRY(g0->kinEE.ensure(sizeof(double) * (size_t)bg->kin_rows * g0->ld_ee));
            CRM_TRY(launch_gather_rows(st, d_EE, g0->ld_ee, bg->kin_map.as<int>(), bg->kin_rows, (int)g0->ld_ee, g0->kinEE.as<double>(),
                                       g0->ld_ee));
            CRM_TRY(ctx->ws_Pd.ensure(sizeof(double) * (size_t)(P.donor_pairs ? bg->kin_groups : bg->kin_groups_pad) * P.pd_slab));
        }
        if (P.donor_pairs)   // (ws_AH, the folded form's scratch, also holds the sliced pair products of the expansion pass)
            CRM_TRY(ctx->ws_AH.ensure(sizeof(double) * (size_t)std::max<long>(P.donor_pair_splits, P.fold_split6) *
                                      (size_t)std::max<long>(P.pd_slab, (std::max<long>(P.BLK, P.pair_cap) + 128) * P.ldP)));
        // (unfolded form: the slabs of the padding donors meet zero rows of hKd in the contraction over the donors: they must be
        // finite -- cleared here, not left to whatever the allocation or an earlier call put there)
        if (P.pairs_unfolded && bg->kin_groups_pad > bg->kin_groups)
            CRM_HIP(hipMemsetAsync(ctx->ws_Pd.as<double>() + (size_t)bg->kin_groups * P.pd_slab, 0,
                                   sizeof(double) * (size_t)(bg->kin_groups_pad - bg->kin_groups) * P.pd_slab, st));
        if (P.through_H() && !P.folded()) {
            // AH = H'(g o E0), the operand of the products with the mixing matrices: its rows beyond the half factor's columns meet
            // zero rows of Mix and must be finite -- zero.  The pair-feature form writes every row below them for every column it
            // is read at (columns beyond the block's only feed output rows that are never stored), so the padding rows are all
            // there is to clear: 4 rows instead of 0.67 GB per call at config 2.
            if (P.pairs_unfolded && ldh > bg->cols)
                CRM_HIP(hipMemsetAsync(ctx->ws_AH.as<double>() + (size_t)bg->cols * P.ld_ah, 0, sizeof(double) * (size_t)(ldh - bg->cols) * P.ld_ah, st));
            else if (!P.pairs_unfolded)
                CRM_HIP(hipMemsetAsync(ctx->ws_AH.ptr, 0, sizeof(double) * (size_t)ldh * P.ld_ah, st));
        }
        return CRM_OK;
    }

    // Unrelated-donor form: Phi'[y, W] and E1'[y, W] per gene -- formed on the gene's first scan against these tables
    // (crm_gene::wb_yW), copied into this scan's workspace after
    int prepare_woodbury() {
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

    // ---- block stages ---------------------------------------------------------------------------------------------------
    // 1. aligned copy of the block (and its row-permuted twin for the test direction); in
    //    collapsed mode the "block" is the donor dosage slab (m_pad rows)
    int copy_block(Block& B) {
        const long ldb = P.ldb;
        const int nb = B.nb;
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
    int block_stats(Block& B) {
        const long ldb = P.ldb, ld_gW = P.ld_gW;
        const int nb = B.nb, BLK = P.BLK;
        if (!P.collapsed()) {
            B.Gx = ctx->ws_Gx.as<double>();
            CRM_TRY(launch_variant_stats(st, B.Gb, ldb, np, nb, g0->yW.as<double>(), g0->yW.as<double>() + 1, g0->ld_yw, c, d_part, d_gg, d_gy, d_gW, ld_gW));
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
    int fold_TH(const Block& B) {
        const long ldb = P.ldb;
        const int nb = B.nb, k1 = bg->kin_k1, k2 = bg->kin_k2;
        const long groups = bg->kin_groups;
        double* Gk = ctx->ws_Gk.as<double>();
        double* TH = ctx->ws_TH.as<double>();
        CRM_TRY(launch_gather_rows(st, B.Gx, ldb, bg->kin_map.as<int>(), bg->kin_rows, (int)ldb, Gk, ldb));
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
    int unfolded_TH(const Block& B) {
        const long ldb = P.ldb, KK = P.KK;
        const int nb = B.nb, k1 = bg->kin_k1, k2 = bg->kin_k2;
        const long groups = bg->kin_groups, mk = bg->kin_cols;
        double* Gk = ctx->ws_Gk.as<double>();
        double* S2 = ctx->ws_S2.as<double>();
        CRM_TRY(launch_gather_rows(st, B.Gx, ldb, bg->kin_map.as<int>(), bg->kin_rows, (int)ldb, Gk, ldb));
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

    int plain_TH(const Block& B) {
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
    bool cut_choice(int nb, int cnt, const int* N, bool* is_cut, long& acc, long& rounds) const {
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
    int cut_rotations(const Block& B, int n_list, int& n_main) {
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
    int rotations(const Block& B) {
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
        if (n_list == 0) return CRM_OK;
        int n_main = n_list;
        if (P.fastT) CRM_TRY(cut_rotations(B, n_list, n_main));
        CRM_TRY(upload(SLOT_RHO, probs.data(), n_main));
        // (unrelated-donor form: the kernel timer brackets this launch, the rotations MixK(rho)'(H'Gx) -- the step's largest)
        const bool timing_T = P.wb() && ctx->timing && ctx->timed_used < 65536;
        if (timing_T) CRM_TRY(timer_open(true));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOT_RHO, n_main, nb, (int)ldq, P.fastT ? P.kdim : P.xrows, false, 0, 1, 0));
        if (timing_T) {
            CRM_TRY(timer_close());
            for (int q = 0; q < n_main; q++) ctx->kr_flops += 2.0 * (double)P.kdim * (double)nb * (double)probs[q].N;
        }
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
    int plan_rotations(const Block& B, const GemmProblem* all) {
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
    int null_fits(const Block& B) {
        const int nb = B.nb, BLK = P.BLK;
        trace_push("crm null fits");
        for (int gi = 0; gi < ng; gi++) {
            crm_gene* g = genes[gi];
            NullFitArgs fa{};
            fa.nrho = nrho; fa.c = c; fa.restricted = 1; fa.n = n; fa.polish = ctx->polish ? 1 : 0; fa.exact = (ctx->nullfit_exact || form("nullfit_exact", 0)) ? 1 : 0;
            for (int i = 0; i < nrho; i++) {
                NullFitRho& R = fa.rho[i];
                R.T = ctx->ws_T.as<double>() + (size_t)i * BLK * P.ldT; R.ldT = P.ldT;
                R.ty = g->rot.as<double>() + (long)i * slab;
                R.tW = R.ty + ldq; R.ldW = ldq;
                R.S0 = bg->S0[i].as<double>();
                R.r = bg->r[i];
                if (rho0_pos[i]) {   // (the operands of the assembly: gene_results, the P.wb() branch)
                    R.T = wb_g; R.ldT = P.ldwb;
                    R.ty = wb_yW + (size_t)gi * (1 + c) * P.ldwb;
                    R.tW = R.ty + P.ldwb; R.ldW = P.ldwb;
                    R.S0 = bg->wb_S0[i].as<double>();
                    R.r = (int)bg->wb_P;
                }
            }
            fa.WW = g->WW.as<double>(); fa.Wy = g->Wy.as<double>(); fa.yy = g->yy;
            fa.gg = d_gg; fa.gy = d_gy + (size_t)gi * BLK; fa.gW = d_gW; fa.ld_gW = P.ld_gW;
            fa.g_drop = P.collapsed() ? nullptr : d_drop;
            if (c > CRM_MAX_COV_WIDE) fa.xwide = ctx->ws_xwide.as<double>();
            fa.trial = d_trial; fa.out = d_fit + (size_t)gi * BLK; fa.probe = ctx->probe_on ? 1 : 0; fa.probe_x = ctx->probe_x;
            fa.track = outs[gi].flags ? 1 : 0;
            CRM_TRY(launch_nullfit(st, fa, nb, false, d_queue));
        }
        trace_pop();
        if (std::find(rho0_pos, rho0_pos + nrho, true) != rho0_pos + nrho) ctx->rho0_position_blocks++;
        if (ctx->probe_on) {
            std::vector<NullFitTrial> h_trial((size_t)nb * nrho);
            CRM_HIP(hipMemcpyAsync(h_trial.data(), d_trial, sizeof(NullFitTrial) * h_trial.size(), hipMemcpyDeviceToHost, st));
            CRM_HIP(hipStreamSynchronize(st));
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
    int replay_block(const Block& B) {
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
    int woodbury_phi(const Block& B) {
        const long groups = bg->kin_groups;
        phi_recs.resize((size_t)groups);
        GemmProblem p{};
        p.X = ctx->ws_TH.as<double>() + (size_t)bg->kin_k1 * P.ldb; p.ldx = P.ldb; p.C = wb_g; p.ldc = P.ldwb; p.M = B.nb;
        woodbury_records(bg, p, (long)bg->kin_k2 * P.ldb, phi_recs.data());
        // (no with_records: the host is not to wait here, ahead of the step's largest launch -- phi_recs lives as long as
        // the pass and is written again only in the next block, after collect_fits has synchronised the stream)
        CRM_TRY(upload(SLOT_KIN, phi_recs.data(), phi_recs.size()));
        return launch_gemm_tn(ctx, d_probs + SLOT_KIN, (int)groups, B.nb, bg->kin_k2, bg->wb_k2pad, false, 0, 1, 0);
    }

    // 5. the fits of the block on the host (nb*ng*48 bytes cross PCIe): the collapsed path's near flags, the permutation
    //    replay's record, the flat-optimum margins
    int collect_fits(Block& B) {
        const int nb = B.nb, BLK = P.BLK;
        CRM_HIP(hipMemcpyAsync(h_fit.data(), d_fit, sizeof(NullFitOut) * (size_t)BLK * ng, hipMemcpyDeviceToHost, st));
        if (P.collapsed() && near_out) CRM_HIP(hipMemcpyAsync(h_near.data(), d_near, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
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

    // The pair stage runs over sub-ranges of the block: one unless several phenotypes ask for more (variant, rho*) pairs
    // than the pair-ordered buffers hold
    SubRange sub_range(const Block& B, int b0) const {
        SubRange R;
        R.b0 = b0;
        R.nb = B.nb - b0;
        R.done = B.done + b0;
        if (ng > 1) {
            long pairs = 0;
            int take = 0;
            for (; b0 + take < B.nb; take++) {
                unsigned seen = 0;
                for (int gi = 0; gi < ng; gi++) {
                    const NullFitOut& f = h_fit[(size_t)gi * P.BLK + b0 + take];
                    if (!no_kinship_term(f)) seen |= 1u << f.rho_index;
                }
                const int here = __builtin_popcount(seen);
                if (take > 0 && pairs + here > P.pair_cap) break;
                pairs += here;
            }
            R.nb = take;
        }
        return R;
    }

    // 5. the (rho, variant) pairs some gene selected, ordered by rho; the sub-range's columns of the block in that order (Gs)
    int select_pairs(const Block& B, const SubRange& R, Pairs& Q) {
        const int nb = R.nb, BLK = P.BLK;
        const NullFitOut* fit = h_fit.data() + R.b0;
        std::fill(pair_of.begin(), pair_of.end(), -1);
        long with_pair = 0;
        for (int gi = 0; gi < ng; gi++)
            for (int b = 0; b < nb; b++) {
                const NullFitOut& f = fit[(size_t)gi * BLK + b];
                if (no_kinship_term(f)) continue;
                pair_of[(size_t)f.rho_index * BLK + b] = 0;
                with_pair++;
            }
        ctx->tests_without_pair += (long)ng * nb - with_pair;
        // (a sub-range without any pair keeps its first test's: the launches below always have something to do)
        if (with_pair == 0) pair_of[(size_t)fit[0].rho_index * BLK] = 0;
        for (int i = 0; i < nrho; i++) {
            Q.start[i] = Q.npairs;
            for (int b = 0; b < nb; b++) {
                if (pair_of[(size_t)i * BLK + b] == 0) {
                    pair_of[(size_t)i * BLK + b] = Q.npairs;
                    h_ord[Q.npairs++] = b;
                }
            }
            Q.cnt[i] = Q.npairs - Q.start[i];
        }
        Q.start[nrho] = Q.npairs;
        for (int gi = 0; gi < ng; gi++)
            for (int b = 0; b < nb; b++) {
                const NullFitOut& f = fit[(size_t)gi * BLK + b];
                h_pos[(size_t)gi * BLK + b] = no_kinship_term(f) ? -1 : pair_of[(size_t)f.rho_index * BLK + b];
            }
        if (P.wb_block && ng == 1) {
            // (the position of a test is its variant's place in the block; the sorted copy Gs is not formed: donor_columns)
            for (int b = 0; b < nb; b++)
                if (h_pos[b] >= 0) h_pos[b] = b;
            CRM_HIP(hipMemcpyAsync(d_pos, h_pos.data(), sizeof(int) * (size_t)BLK, hipMemcpyHostToDevice, st));
            return CRM_OK;
        }
        CRM_HIP(hipMemcpyAsync(d_pos, h_pos.data(), sizeof(int) * (size_t)BLK * ng, hipMemcpyHostToDevice, st));
        if (P.wb() && ng > 1) {   // (S in block order: a variant's rows of the rotated S sit at its own position)
            std::vector<int> h_posw((size_t)BLK * ng, -1);
            for (int gi = 0; gi < ng; gi++)
                for (int b = 0; b < nb; b++)
                    if (h_pos[(size_t)gi * BLK + b] >= 0) h_posw[(size_t)gi * BLK + b] = b;
            CRM_HIP(hipMemcpyAsync(d_posw, h_posw.data(), sizeof(int) * h_posw.size(), hipMemcpyHostToDevice, st));
            CRM_HIP(hipStreamSynchronize(st));   // (h_posw lives on this scope)
        }
        CRM_HIP(hipMemcpyAsync(d_ord, h_ord.data(), sizeof(int) * Q.npairs, hipMemcpyHostToDevice, st));
        return launch_gather_block(st, B.Gt + R.b0, P.ldb, P.xrows, P.xrows, nullptr, d_ord, Q.npairs, ctx->ws_Gs.as<double>(),
                                   P.ldp, (int)P.ldp);
    }

    // Splits of the direct route's A~ launch along the cell axis (few rounds: see kr_split_for), and its spectrum tails.
    // A spectrum a little longer than a multiple of the 128-column tile (config 3: r = 5000 = 39 tiles + 8 columns)
    // would pay a whole last column of tiles -- 1 / 40 of the launch -- for those few columns: the last 128 + rem
    // columns (rem <= 32) go into a second launch of 160-column tiles instead, cut along the cell axis to fill its
    // rounds (38 x 128 + 160 = 5024 columns computed instead of 5120).
    int direct_splits(const Pairs& Q, AGroups& A, bool* tail_of) {
        A.a_slab = (size_t)P.pair_cap * k0 * P.ldA;
        long row_tiles = 0;
        int mn = 1;
        for (int i = 0; i < nrho; i++)
            if (Q.cnt[i] > 0) { row_tiles += ((long)Q.cnt[i] * k0 + GEMM_BM - 1) / GEMM_BM; mn = std::max(mn, bg->r[i]); }
        const int cap = (int)std::min<size_t>(8, ((size_t)16 << 30) / std::max<size_t>(sizeof(double) * A.a_slab, 1));
        A.kr_split = kr_split_for(ctx, row_tiles, mn, 1, np, std::max(cap, 1));
        if (A.kr_split > 1) CRM_TRY(ctx->ws_A.ensure(sizeof(double) * A.a_slab * A.kr_split));
        if (A.kr_split > 1 || !ctx->tune.glds || ctx->tune.bn == 64 || ctx->tune.bn == 160 || form("kr_no_tail", 0)) return CRM_OK;
        long tail_row_tiles = 0, main_tiles = 0;
        for (int i = 0; i < nrho; i++) {
            if (Q.cnt[i] == 0) continue;
            const int N = bg->r[i], rem = N % 128;
            const long rt = ((long)Q.cnt[i] * k0 + GEMM_BM - 1) / GEMM_BM;
            main_tiles += rt * ((N + 127) / 128);
            if (N >= 1024 && rem > 0 && rem <= 32) {
                tail_of[i] = true;
                tail_row_tiles += rt;
                A.tail_maxn = std::max(A.tail_maxn, 128 + rem);
            }
        }
        if (tail_row_tiles == 0 || main_tiles <= 1024) {
            std::fill(tail_of, tail_of + CRM_MAX_RHO, false);
        } else {
            const int saved_bn = ctx->tune.bn;
            ctx->tune.bn = 160;
            A.tail_split = kr_split_for(ctx, tail_row_tiles, A.tail_maxn, 1, np, std::max(cap, 1));
            ctx->tune.bn = saved_bn;
            // (before the problem records take addresses inside ws_A: growing the buffer does not keep its contents)
            if (A.tail_split > 1) CRM_TRY(ctx->ws_A.ensure(sizeof(double) * A.a_slab * A.tail_split));
        }
        return CRM_OK;
    }

    // the problems of step 6, one per non-empty rho group of pairs, into probs[0, nz) (none on the unrelated-donor route)
    void a_records(const Pairs& Q, bool via_H, const bool* tail_of, AGroups& A) {
        const double kin_rows = P.folded() ? bg->kin_k1 + bg->kin_groups * (long)bg->kin_k2 : bg->cols;   // (rows of the Mix products)
        for (int i = 0; i < nrho; i++) {
            if (Q.cnt[i] == 0 || P.wb()) continue;   // (unrelated-donor form: no A~ at all)
            GemmProblem p{};
            p.X = ctx->ws_Gs.as<double>() + Q.start[i]; p.ldx = P.ldp;
            p.C = ctx->ws_A.as<double>() + (size_t)Q.start[i] * k0 * P.ldA;
            if (P.collapsed()) {
                // A~(b) = sum_d gamma_d,b * Bd(rho)[d]: rows of Bd are (k0 x ldq) slabs per donor
                p.Y = tab->Bd.as<double>() + (size_t)i * P.mp * k0 * ldq; p.ldy = (long)k0 * ldq; p.ldc = (long)k0 * P.ldA;
                p.M = Q.cnt[i]; p.N = (int)((long)k0 * ldq);
            } else if (via_H) {
                if (P.kin() && ng == 1) {   // (AH / S is in pair order already, see folded_S / unfolded_AH)
                    p.X = (P.folded() ? ctx->ws_S.as<double>() : ctx->ws_AH.as<double>()) + (size_t)Q.start[i] * k0; p.ldx = P.ld_ah;
                } else {
                    p.X = ctx->ws_XG.as<double>() + (size_t)Q.start[i] * k0; p.ldx = P.ld_xg;
                }
                p.Y = P.folded() ? bg->MixK[i].as<double>() : bg->Mix[i].as<double>(); p.ldy = ldq; p.ldc = P.ldA;
                p.M = Q.cnt[i] * k0; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
                A.kr_flops += 2.0 * kin_rows * (double)bg->r[i] * (double)k0 * (double)Q.cnt[i];
            } else {
                p.E = d_Ep; p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->Q0[i].as<double>(); p.ldy = ldq; p.ldc = P.ldA;
                p.M = Q.cnt[i] * k0; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
                A.kr_flops += 2.0 * (double)n * (double)bg->r[i] * (double)k0 * (double)Q.cnt[i];
                if (tail_of[i]) {
                    GemmProblem t = p;
                    const int rem = 128 + p.N % 128;
                    p.N -= rem;
                    t.Y = p.Y + p.N; t.C = p.C + p.N; t.N = rem;
                    A.tails.push_back(t);
                }
            }
            // The mixing-matrix products of the kinship-structure route: a spectrum a little longer than a multiple of the
            // 128-column tile (config 3: r = 5000 = 39 tiles + 8 columns) would pay a whole last column of tiles -- 1 / 40 of
            // the launch -- for those few columns; they go through one pass over the operand instead (launch_skinny_tn).
            if (P.kin() && p.N >= 1024 && p.N % 128 > 0 && p.N % 128 <= 16 && p.ldx % 2 == 0 &&
                (reinterpret_cast<uintptr_t>(p.X) & 15) == 0 && !form("kr_no_tail", 0)) {
                GemmProblem t = p;
                const int rem = p.N % 128;
                A.kr_flops -= 2.0 * kin_rows * (double)rem * (double)k0 * (double)Q.cnt[i];   // (the timed launch is the tiled one alone)
                p.N -= rem;
                t.Y = p.Y + p.N; t.C = p.C + p.N; t.N = rem;
                A.spectrum_tails.push_back(t);
            }
            A.max_m = std::max(A.max_m, p.M);
            A.max_n = std::max(A.max_n, p.N);
            probs[A.nz++] = p;
        }
    }

    // The kinship routes' operand columns in donor order (Gk): one phenotype takes them in the rho*-sorted pair order (Gs)
    // straight away, so that the result is the operand of the Mix products as it stands; several phenotypes share a
    // variant between pairs: block order, then the pair gather.  The unrelated-donor form has no Mix product: block order
    struct DonorCols { bool in_pair_order; const double* G; long ldg; int ncol; };
    int donor_columns(const Block& B, const SubRange& R, const Pairs& Q, DonorCols& D) {
        D.in_pair_order = ng == 1 && !P.wb_block;
        D.G = D.in_pair_order ? ctx->ws_Gs.as<double>() : B.Gt + R.b0;
        D.ldg = D.in_pair_order ? P.ldp : P.ldb;
        D.ncol = D.in_pair_order ? Q.npairs : R.nb;
        const int blk_cols = (int)(P.ldb - R.b0);   // (columns of the block buffers from the sub-range's first one on)
        return launch_gather_rows(st, D.G, D.ldg, bg->kin_map.as<int>(), bg->kin_rows, D.in_pair_order ? (int)D.ldg : blk_cols,
                                  ctx->ws_Gk.as<double>(), D.ldg);
    }
    int gather_pairs(const double* src, long rows, const Pairs& Q) {   // (several phenotypes: the operand in pair order, XG)
        const int xg_cols = (int)std::min<long>(P.ld_xg, round_up((long)Q.npairs * k0, 128) + 128);
        return launch_gather_slabs(st, src, P.ld_ah, rows, d_ord, Q.npairs, k0, ctx->ws_XG.as<double>(), P.ld_xg, xg_cols);
    }

    // Folded form (objects.h: kin_fold): S = [E1 rows ; (donor, us_j) rows] of "H'(g o E0) before the contraction over
    // the donors", which MixK carries.  (a) the block in donor order; (b) per donor d' the Khatri-Rao contraction over
    // its own cells against us (transposed store into rows k1 + d' k2 + j); (c) the E1 rows by one Khatri-Rao
    // contraction over ALL cells against the E1 columns of the half factor, cut into slices along the cell axis so
    // that its few output tiles fill the chip, summed, and copied into rows [0, k1).
    int folded_S(const Block& B, const SubRange& R, const Pairs& Q) {
        DonorCols D;
        CRM_TRY(donor_columns(B, R, Q, D));
        double* S = ctx->ws_S.as<double>();
        double* Gk = ctx->ws_Gk.as<double>();
        const int k1 = bg->kin_k1, k2 = bg->kin_k2, ncol = D.ncol, npair = P.npair;
        const long groups = bg->kin_groups, ld_ah = P.ld_ah;
        std::vector<GemmProblem> kp((size_t)groups + P.fold_split6);
        GemmProblem p{};
        p.X = Gk; p.ldx = D.ldg;
        if (P.donor_pairs) {   // per donor G_d' (E (x) E)_d, then the rows of S and the E1 rows from it
            p.Y = g0->kinEE.as<double>(); p.ldy = g0->ld_ee; p.C = ctx->ws_Pd.as<double>(); p.ldc = P.ldPd;
            p.M = ncol; p.N = npair;
        } else if (k2 == 1) {  // plain product G_d'' (us o E0)_d': C[b, i] = row k1 + d' of S at column b k0 + i
            p.Y = g0->kinUE.as<double>(); p.ldy = g0->ld_ep; p.C = S + (size_t)k1 * ld_ah; p.ldc = k0; p.M = ncol; p.N = k0;
        } else {
            p.E = g0->kinEp.as<double>(); p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->kin_Y.as<double>(); p.ldy = bg->kin_ldy;
            p.C = S + (size_t)k1 * ld_ah; p.ldc = ld_ah; p.M = ncol * k0; p.N = k2;
        }
        const long maxlen = donor_run_records(bg, p, P.donor_pairs ? P.pd_slab : (long)k2 * ld_ah, kp.data());
        // slices of whole stages along the cell axis, the last one shorter
        const long stages_all = np / GEMM_BK, per = (stages_all + P.fold_split6 - 1) / P.fold_split6;
        const long e1_slab = (long)k1 * ld_ah;
        int slices = 0;
        long chunk_max = GEMM_BK;
        if (P.e1_pairs) {
            GemmProblem& e = kp[groups];
            e.X = D.G; e.ldx = D.ldg; e.Y = g0->kinP.as<double>(); e.ldy = P.ldP;
            e.C = ctx->ws_AH.as<double>(); e.ldc = P.ldP; e.M = ncol; e.N = k1 * k0;
            if (P.e1_sym) { e.Y = d_EE; e.ldy = g0->ld_ee; e.N = npair; }
        }
        for (int sps = 0; sps < P.fold_split6 && !P.e1_pairs; sps++) {
            const long s0 = sps * per, s1 = std::min(stages_all, s0 + per);
            if (s1 <= s0) break;
            GemmProblem& e = kp[groups + slices++];
            e.X = D.G + s0 * GEMM_BK * D.ldg; e.ldx = D.ldg;
            e.E = d_Ep + s0 * GEMM_BK * g0->ld_ep; e.lde = g0->ld_ep; e.k0 = k0;
            e.Y = bg->H.as<double>() + s0 * GEMM_BK * bg->ldh; e.ldy = bg->ldh;
            e.C = ctx->ws_AH.as<double>() + (size_t)sps * e1_slab; e.ldc = ld_ah;
            e.M = ncol * k0; e.N = k1; e.cells = (s1 - s0) * GEMM_BK;
            chunk_max = std::max(chunk_max, e.cells);
        }
        kp.resize((size_t)groups + std::max(slices, 1));
        return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
            double* AH = ctx->ws_AH.as<double>();
            if (P.donor_pairs) {
                CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, npair, maxlen, false, 0, 1, 0));
                if (P.wb_rotate)   // (the rotated S straight from the pair products: the rows of S are not formed)
                    CRM_TRY(launch_donor_pairs_rotate(st, ctx->ws_Pd.as<double>(), P.pd_slab, P.ldPd, (int)groups, ncol, k0,
                                                      bg->wb_U.as<double>(), (long)bg->wb_k2pad * 128, 128, bg->wb_k2pad,
                                                      ctx->ws_A.as<double>(), P.ldAw, AH, P.pd_slab, P.donor_pair_splits));
                else
                    CRM_TRY(launch_donor_pairs_expand(st, ctx->ws_Pd.as<double>(), P.pd_slab, P.ldPd, (int)groups, ncol, k0, k1, S, ld_ah,
                                                      AH, P.pd_slab, P.donor_pair_splits));
                CRM_TRY(launch_reduce_splits(st, AH, (long)ncol * P.ldPd, P.donor_pair_splits, P.pd_slab));
                CRM_TRY(launch_pair_rows_sym(st, AH, P.ldPd, ncol, k0, S, ld_ah));
                ctx->donor_pair_blocks++;
            } else {
                if (k2 == 1) CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, k0, maxlen, false, 0, 1, 0));
                else CRM_TRY(launch_kr_transposed(ctx, d_kp, (int)groups, ncol * k0, k2, maxlen, k0));
                if (P.e1_pairs) {
                    const long p_slab = (long)(std::max<long>(P.BLK, P.pair_cap) + 128) * P.ldP;
                    CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, 1, ncol, P.e1_sym ? npair : k1 * k0, np, false, 0, P.fold_split6, p_slab));
                    CRM_TRY(launch_reduce_splits(st, AH, (long)ncol * P.ldP, P.fold_split6, p_slab));
                    if (P.e1_sym) CRM_TRY(launch_pair_rows_sym(st, AH, P.ldP, ncol, k0, S, ld_ah));
                    else CRM_TRY(launch_pair_rows(st, AH, P.ldP, ncol, k1, k0, S, ld_ah));
                } else {
                    CRM_TRY(launch_kr_transposed(ctx, d_kp + groups, slices, ncol * k0, k1, chunk_max, k0));
                    CRM_TRY(launch_reduce_splits(st, AH, e1_slab, slices, e1_slab));
                    CRM_HIP(hipMemcpyAsync(S, AH, sizeof(double) * (size_t)e1_slab, hipMemcpyDeviceToDevice, st));
                }
            }
            // (2 kin_rows k2 k0 + 2 n k1 k0 flops per variant, outside the timed pair: the roofline figure is the MixK product's own;
            // bench.py's whole_path counts them)
            if (!D.in_pair_order && !P.wb()) CRM_TRY(gather_pairs(S, P.kdim, Q));
            return CRM_OK;
        });
    }

    // AH = H'(g o E0) without an n-length contraction against the cols columns of H:
    // (a) the block in donor order; (b) per donor d' the Khatri-Rao contraction over its own cells against
    // [us | E1] (transposed store: S[(d' KK + q), (b, i)]); (c) the L rows: for every j a contraction over the
    // donors with hKd, AH[(k1 + j m + d), .] = sum_d' hKd[d', d] S[(d' KK + j), .]; (d) the E1 rows: sums over d'
    int unfolded_AH(const Block& B, const SubRange& R, const Pairs& Q) {
        DonorCols D;
        CRM_TRY(donor_columns(B, R, Q, D));
        double* S = ctx->ws_S.as<double>();
        double* AH = ctx->ws_AH.as<double>();
        const int k1 = bg->kin_k1, k2 = bg->kin_k2, ncol = D.ncol, npair = P.npair;
        const long groups = bg->kin_groups, mk = bg->kin_cols, KK = P.KK, ld_ah = P.ld_ah;
        GemmProblem p{};
        p.X = ctx->ws_Gk.as<double>(); p.ldx = D.ldg;
        if (P.pairs_unfolded) {
            // P_d = G_d'(E (x) E)_d per donor; Z = [hKd | 1]' P over the donors (in ws_S: the per-donor blocks are not formed);
            // rows k1 + j m + c of AH from Z_c, rows [0, k1) from the sums over the donors Z_m
            double* Pd = ctx->ws_Pd.as<double>();
            double* Z = S;
            std::vector<GemmProblem> kp((size_t)groups + 1);
            p.Y = g0->kinEE.as<double>(); p.ldy = g0->ld_ee; p.C = Pd; p.ldc = P.ldPd; p.M = ncol; p.N = npair;
            const long maxlen = donor_run_records(bg, p, P.pd_slab, kp.data());
            GemmProblem& z = kp[groups];
            z.X = bg->kin_hKd.as<double>(); z.ldx = bg->kin_ldh;   // (column m of hKd: ones)
            z.Y = Pd; z.ldy = P.pd_slab; z.C = Z; z.ldc = P.pd_slab; z.M = (int)mk + 1; z.N = (int)((long)ncol * P.ldPd);
            return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
                CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, npair, maxlen, false, 0, 1, 0));
                CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, 1, (int)mk + 1, (int)((long)ncol * P.ldPd), bg->kin_groups_pad, false, 0, 1, 0));
                CRM_TRY(launch_donor_pairs_expand(st, Z, P.pd_slab, P.ldPd, (int)mk, ncol, k0, k1, AH, ld_ah, Pd, P.pd_slab, 1, 1, mk));
                CRM_TRY(launch_pair_rows_sym(st, Z + (size_t)mk * P.pd_slab, P.ldPd, ncol, k0, AH, ld_ah));
                ctx->donor_pair_blocks++;
                if (!D.in_pair_order) CRM_TRY(gather_pairs(AH, bg->ldh, Q));
                return CRM_OK;
            });
        }
        std::vector<GemmProblem> kp((size_t)groups + k2);
        p.E = g0->kinEp.as<double>(); p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->kin_Y.as<double>(); p.ldy = bg->kin_ldy;
        p.C = S; p.ldc = ld_ah; p.M = ncol * k0; p.N = (int)KK;
        const long maxlen = donor_run_records(bg, p, KK * ld_ah, kp.data());
        for (int j = 0; j < k2; j++) {
            GemmProblem& q = kp[groups + j];
            q.X = bg->kin_hKd.as<double>(); q.ldx = bg->kin_ldh; q.Y = S + (size_t)j * ld_ah; q.ldy = KK * ld_ah;
            q.C = AH + (size_t)(k1 + (long)j * mk) * ld_ah; q.ldc = ld_ah; q.M = (int)mk; q.N = ncol * k0;
        }
        return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
            CRM_TRY(launch_kr_transposed(ctx, d_kp, (int)groups, ncol * k0, (int)KK, maxlen, k0));
            CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, k2, (int)mk, ncol * k0, bg->kin_groups_pad, false, 0, 1, 0));
            CRM_TRY(launch_kin_sum_e1(st, S, ld_ah, (int)KK, k2, k1, (int)groups, (long)ncol * k0, AH, ld_ah));
            // (2 kin_rows KK k0 + 2 groups_pad m k2 k0 flops per variant, outside the timed pair: the roofline figure is the Mix
            // product's own; bench.py's whole_path counts them)
            if (!D.in_pair_order) CRM_TRY(gather_pairs(AH, bg->ldh, Q));
            return CRM_OK;
        });
    }

    // several phenotypes on the direct route through H: AH = H'(g o E0) over all cells, then the pair gather
    int direct_AH(const Block& B, const SubRange& R, const Pairs& Q, AGroups& A) {
        GemmProblem p{};
        p.X = B.Gt + R.b0; p.ldx = P.ldb; p.E = d_Ep; p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->H.as<double>(); p.ldy = bg->ldh;
        p.C = ctx->ws_AH.as<double>(); p.ldc = P.ld_ah; p.M = R.nb * k0; p.N = (int)bg->cols;
        CRM_TRY(upload(SLOT_ONE, &p, 1));
        CRM_TRY(launch_kr_transposed(ctx, d_probs + SLOT_ONE, 1, p.M, p.N, np, k0));
        A.kr_flops += 2.0 * (double)n * (double)bg->cols * (double)k0 * (double)R.nb;
        return gather_pairs(ctx->ws_AH.as<double>(), bg->ldh, Q);
    }

    // Unrelated-donor form: the rotated S, rows (col k0 + i) over the donors k2 positions -- per donor
    // (U_d Lambda_d^-1/2)' S_d, stored transposed into ws_A; col = the pair (one phenotype) or the block position
    int woodbury_S(const SubRange& R, const Pairs& Q) {
        const long groups = bg->kin_groups;
        const int ncol = P.wb_block ? R.nb : Q.npairs;
        std::vector<GemmProblem> kp((size_t)groups);
        GemmProblem p{};
        p.X = ctx->ws_S.as<double>() + (size_t)bg->kin_k1 * P.ld_ah; p.ldx = P.ld_ah;
        p.C = ctx->ws_A.as<double>(); p.ldc = P.ldAw; p.M = ncol * k0;
        woodbury_records(bg, p, (long)bg->kin_k2 * P.ld_ah, kp.data());
        return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) {
            return launch_gemm_tn(ctx, d_kp, (int)groups, ncol * k0, bg->kin_k2, bg->wb_k2pad, false, 0, 1, 0);
        });
    }

    // 6. A~ = KR(Gs, Ep)' Q0(rho), one problem per non-empty rho group of pairs.
    //    Several genes can select several rho* for one variant; with Q0(rho) = H Mix(rho) the
    //    n-length Khatri-Rao contraction is then done once per variant against H (stored transposed)
    //    and every (variant, rho) pair costs a cols-length product with Mix(rho) instead.
    int form_A(const Block& B, const SubRange& R, const Pairs& Q) {
        bool via_H = P.kin();
        if (P.fastT && ng > 1 && !P.kin()) {
            double direct = 0.0, via = (double)R.nb * (double)bg->cols * (double)n;
            for (int i = 0; i < nrho; i++) {
                direct += (double)Q.cnt[i] * bg->r[i] * (double)n;
                via += (double)Q.cnt[i] * bg->r[i] * (double)bg->ldh;
            }
            via_H = ctx->tune.shared_h < 0 ? via < 0.9 * direct : ctx->tune.shared_h > 0;
        }
        const bool direct = !P.collapsed() && !via_H;
        if (direct)
            for (int i = 0; i < nrho; i++)
                if (Q.cnt[i] > 0) CRM_TRY(crm_background_require_q0(bg, i));
        AGroups A;
        bool tail_of[CRM_MAX_RHO] = {false};
        if (direct) CRM_TRY(direct_splits(Q, A, tail_of));
        a_records(Q, via_H, tail_of, A);
        const bool timing = !P.wb() && ctx->timing && ctx->timed_used < 65536;  // bounded: a forgotten timer cannot grow for ever
        // (kinship-structure route: the pair brackets the dominant launch alone, the Mix(rho*)' product further down)
        if (timing) CRM_TRY(timer_open(!P.kin()));
        if (P.folded()) CRM_TRY(folded_S(B, R, Q));
        else if (P.kin()) CRM_TRY(unfolded_AH(B, R, Q));
        else if (via_H) CRM_TRY(direct_AH(B, R, Q, A));
        CRM_TRY(upload(SLOT_ONE, probs.data(), A.nz));
        GemmProblem* d_A = d_probs + SLOT_ONE;
        if (P.collapsed()) {
            CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, (int)((long)k0 * ldq), P.mp, false, 0, 1, 0));
        } else if (P.wb()) {
            if (!P.wb_rotate) CRM_TRY(woodbury_S(R, Q));   // (else the rotated S is in ws_A already: launch_donor_pairs_rotate)
        } else if (P.kin()) {
            if (timing) CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].first, st));
            struct Restore { crm_ctx* c; ~Restore() { c->tune.tag = 0; } } restore{ctx};
            ctx->tune.tag = 1;
            CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, P.kdim, false, 0, 1, 0));
        } else if (via_H) {
            CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, P.kdim, false, 0, 1, 0));
        } else {
            CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, np, true, k0, A.kr_split, (long)A.a_slab));
            CRM_TRY(launch_reduce_splits(st, ctx->ws_A.as<double>(), (long)Q.npairs * k0 * P.ldA, A.kr_split, (long)A.a_slab));
            if (!A.tails.empty()) {
                const int saved_bn = ctx->tune.bn;
                ctx->tune.bn = 160;
                struct Restore { crm_ctx* c; int bn; ~Restore() { c->tune.bn = bn; } } restore{ctx, saved_bn};
                CRM_TRY(upload(A.nz, A.tails.data(), A.tails.size()));
                CRM_TRY(launch_gemm_tn(ctx, d_probs + A.nz, (int)A.tails.size(), A.max_m, A.tail_maxn, np, true, k0, A.tail_split, (long)A.a_slab));
                ctx->tail_launches++;
                for (const GemmProblem& t : A.tails)
                    CRM_TRY(launch_reduce_splits_band(st, t.C, (long)t.M, t.ldc, 0, t.N, A.tail_split, (long)A.a_slab));
            }
        }
        if (timing) {
            CRM_TRY(timer_close());
            ctx->kr_flops += A.kr_flops;
        }
        if (!A.spectrum_tails.empty()) {
            CRM_TRY(upload(A.nz, A.spectrum_tails.data(), A.spectrum_tails.size()));
            CRM_TRY(launch_skinny_tn(st, d_probs + A.nz, (int)A.spectrum_tails.size(), A.max_m, P.kdim));
            ctx->spectrum_tail_launches++;
            CRM_HIP(hipStreamSynchronize(st));   // (the records live on this stack frame)
        }
        return CRM_OK;
    }

    // 7. elementwise products for the side contractions
    // 8. y-free side contractions: Z2 = (Gt o G)' E, Z3 = (Gt o Gt)' (E (x) E)
    int side_contractions(const Block& B, const SubRange& R) {
        const long ldb = P.ldb;
        const int nb = R.nb;
        double* const Gt = B.Gt + R.b0;
        double* G2 = ctx->ws_G2.as<double>();
        double* GG = !P.collapsed() ? ctx->ws_GG.as<double>() : nullptr;   // (test direction) o (fixed-effect role)
        CRM_TRY(launch_square_block(st, Gt, B.Gx + R.b0, ldb, ldb, P.xrows, (int)(ldb - R.b0), G2, GG, ldb));
        if (!GG) GG = G2;
        const int s2 = P.collapsed() ? 1 : P.ks2, s3 = P.collapsed() ? 1 : P.ks3;
        GemmProblem p{};
        p.ldx = ldb; p.M = nb;
        p.X = GG; p.Y = P.collapsed() ? tab->Z2.as<double>() : d_Ep; p.ldy = g0->ld_ep; p.C = dZ2; p.ldc = P.ldZ2; p.N = k0;
        probs[1] = p;
        p.X = G2; p.Y = P.collapsed() ? tab->Z3.as<double>() : d_EE; p.ldy = g0->ld_ee; p.C = dZ3; p.ldc = P.ldZ3; p.N = P.npair;
        probs[2] = p;
        CRM_TRY(upload(SLOT_RHO, probs.data() + 1, 2));
        if (P.cross) {
            CRM_TRY(launch_donor_cross(st, nb, B.Gb + R.b0, ldb, (int)panel->m, tab->Z2.as<double>(), P.ldZ2, k0, dZ2, P.ldZ2));
        } else {
            CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOT_RHO, 1, nb, k0, P.xrows, false, 0, s2, z2_sz));
            CRM_TRY(launch_reduce_splits(st, dZ2, z2_sz, s2, z2_sz));
        }
        CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOT_RHO + 1, 1, nb, P.npair, P.xrows, false, 0, s3, z3_sz));
        return launch_reduce_splits(st, dZ3, z3_sz, s3, z3_sz);
    }

    // 9. Z1 = Gt' [y o E, W o E] of every phenotype, one launch (ScanPlan::ks1)
    int z1_products(const Block& B, const SubRange& R) {
        const int s1 = P.collapsed() ? 1 : P.ks1;
        std::vector<GemmProblem> zp((size_t)ng);
        for (int gi = 0; gi < ng; gi++) {
            crm_gene* g = genes[gi];
            GemmProblem& p = zp[(size_t)gi];
            p.X = B.Gt + R.b0; p.ldx = P.ldb; p.Y = P.collapsed() ? g->dt_Z1.as<double>() : g->YE.as<double>(); p.ldy = g->ld_ye;
            p.C = dZ1 + (size_t)gi * z1_sz * P.ks1; p.ldc = P.ldZ1; p.M = R.nb; p.N = k0 * (1 + c);
        }
        CRM_TRY(upload(P.z1_slot(), zp.data(), zp.size()));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + P.z1_slot(), ng, R.nb, k0 * (1 + c), P.xrows, false, 0, s1, z1_sz));
        for (int gi = 0; gi < ng; gi++)
            CRM_TRY(launch_reduce_splits(st, dZ1 + (size_t)gi * z1_sz * P.ks1, z1_sz, s1, z1_sz));
        return CRM_OK;
    }

    // flat-optimum probes (info calls only): the score test again with delta one stopping tolerance of the
    // reference's search to either side; how far Q and p move says whether the search's last comparison matters.
    // flat[b]: 1 = FLAT_OPTIMUM, 2 = STATISTIC_AT_TOLERANCE
    int flat_probes(const Block& B, const SubRange& R, int gi, const AssembleArgs& aa, double* slow_ws, std::vector<char>& flat,
                    std::vector<double>& probe_rec) {
        const ScanOut& o = outs[gi];
        const int nb = R.nb;
        const NullFitOut* fit = h_fit.data() + (size_t)gi * P.BLK + R.b0;
        const double flat_kappa = FLAT_KAPPA * 1e-3 * form("flat_kappa_milli", 1000);
        probe_rec.assign((size_t)nb * FLAT_REC, 0.0);
        std::vector<double> q0(nb), p0(nb), q1(nb), p1(nb), lam0((size_t)nb * k0);
        CRM_HIP(hipMemcpyAsync(lam0.data(), d_lam, sizeof(double) * (size_t)nb * k0, hipMemcpyDeviceToHost, st));
        CRM_HIP(hipMemcpyAsync(q0.data(), d_Q, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        CRM_HIP(hipMemcpyAsync(p0.data(), d_pv, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        DevBuf probe;
        CRM_TRY(probe.ensure(sizeof(NullFitOut) * (size_t)nb + 64));
        flat.assign(nb, 0);
        for (int side = 0; side < 2; side++) {
            hipLaunchKernelGGL(flat_probe_fit_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, aa.fit, nb,
                               side == 0 ? 1.0 : -1.0, probe.as<NullFitOut>());
            CRM_HIP(hipGetLastError());
            AssembleArgs ap = aa;
            ap.fit = probe.as<NullFitOut>();
            CRM_TRY(launch_assemble(st, ap, nb, ctx->ws_Gext.as<double>(), slow_ws, &ctx->gram_dma_launches));
            CRM_TRY(launch_eig_davies(st, ctx->ws_F.as<double>(), d_Q, nb, k0, d_lam, d_pv, d_if, d_liu, true, slow_ws));
            CRM_HIP(hipMemcpyAsync(q1.data(), d_Q, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
            CRM_HIP(hipMemcpyAsync(p1.data(), d_pv, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
            CRM_HIP(hipStreamSynchronize(st));
            for (int b = 0; b < nb; b++) {
                // (Q against max(Q, its expectation under the null = tr F): a score vector that nearly vanishes,
                // p ~ 1, leaves Q itself ill-conditioned)
                double trace = 0.0;
                for (int j = 0; j < k0; j++) trace += lam0[(size_t)b * k0 + j];
                // (equal values -- a p-value that underflows to zero on both sides included -- have not moved)
                const double mq = q1[b] == q0[b] ? 0.0 : std::fabs(q1[b] - q0[b]) / std::max(std::fabs(q0[b]), trace);
                const double mp = p1[b] == p0[b] ? 0.0 : std::fabs(p1[b] - p0[b]) / std::fabs(p0[b]);
                const NullFitOut& fo = fit[b];
                double* rec = &probe_rec[(size_t)b * FLAT_REC];
                // (NaN -- a probe that could not be evaluated -- must survive the maximum)
                rec[1] = (mq == mq && rec[1] == rec[1]) ? std::max(rec[1], mq) : NAN;
                rec[2] = (mp == mp && rec[2] == rec[2]) ? std::max(rec[2], mp) : NAN;
                rec[0] = B.flat_obj.empty() ? -1.0 : B.flat_obj[(size_t)gi * P.BLK + R.b0 + b];
                rec[3] = fo.margin; rec[4] = fo.noise; rec[5] = fo.rho_decision; rec[6] = fo.gap; rec[7] = fo.lml;
                rec[8] = fo.curv; rec[9] = fo.delta;
            }
        }
        // the bounds: (movement of Q / p over one tolerance) x (the largest distance, in tolerances, at which two
        // faithful searches stop: STOP_SHIFT_C / relative gain of the objective over one tolerance, at most one --
        // and one outright where a decision of the search itself was within the objective's noise bound)
        for (int b = 0; b < nb; b++) {
            const NullFitOut& fo = fit[b];
            const double* rec = &probe_rec[(size_t)b * FLAT_REC];
            const double gain = fo.curv / std::fabs(fo.lml);
            double shift = (gain > 0.0 && gain == gain) ? std::min(1.0, STOP_SHIFT_C / gain) : 1.0;
            if (!(rec[0] > flat_kappa)) shift = 1.0;
            const double bq = rec[1] * shift, bp = rec[2] * shift;
            if (o.bound_Q) o.bound_Q[R.done + b] = bq;
            if (o.bound_p) o.bound_p[R.done + b] = bp;
            if (!(bp <= 1e-5)) flat[b] |= 1;
            if (!(bq <= 1e-6)) flat[b] |= 2;
        }
        return CRM_OK;
    }

    // 10.-11. per gene: Q and F, eigenvalues + Davies (or the exact tail), results
    int gene_results(const Block& B, const SubRange& R, int gi) {
        crm_gene* g = genes[gi];
        const ScanOut& o = outs[gi];
        const int nb = R.nb, BLK = P.BLK, b0 = R.b0;
        const long done = R.done;
        AssembleArgs aa{};
        for (int i = 0; i < nrho; i++) {
            AssembleRho& Rr = aa.rho[i];
            Rr.ty = g->rot.as<double>() + (long)i * slab;
            Rr.tW = Rr.ty + ldq; Rr.ldW = ldq;
            Rr.S0 = bg->S0[i].as<double>();
            Rr.T = ctx->ws_T.as<double>() + ((size_t)i * BLK + b0) * P.ldT; Rr.ldT = P.ldT;
            Rr.r = bg->r[i];
        }
        aa.fit = d_fit + (size_t)gi * BLK + b0; aa.sorted_pos = d_pos + (size_t)gi * BLK;
        aa.A = ctx->ws_A.as<double>(); aa.ldA = P.ldA; aa.k0 = k0; aa.c = c; aa.n = n; aa.A_none = ctx->ws_Anone.as<double>();
        aa.Z1 = dZ1 + (size_t)gi * z1_sz * P.ks1; aa.ldZ1 = P.ldZ1; aa.Z2 = dZ2; aa.ldZ2 = P.ldZ2; aa.Z3 = dZ3; aa.ldZ3 = P.ldZ3;
        aa.WW = g->WW.as<double>(); aa.Wy = g->Wy.as<double>(); aa.yy = g->yy;
        aa.gg = d_gg + b0; aa.gy = d_gy + b0 + (size_t)gi * BLK; aa.gW = d_gW + (size_t)b0 * P.ld_gW; aa.ld_gW = P.ld_gW;
        aa.coef = P.collapsed() ? nullptr : d_coef + b0; aa.ld_coef = P.ldb; aa.Q = d_Q; aa.F = ctx->ws_F.as<double>();
        for (int i = 0; i < nrho; i++) aa.rho[i].rho = bg->rho[i];
        if (P.wb()) {   // (assemble.hip: woodbury_kernel)
            for (int i = 0; i < nrho; i++) {
                AssembleRho& Rr = aa.rho[i];
                Rr.ty = wb_yW + (size_t)gi * (1 + c) * P.ldwb;
                Rr.tW = Rr.ty + P.ldwb; Rr.ldW = P.ldwb;
                Rr.S0 = bg->wb_S0[i].as<double>();
                Rr.T = wb_g + (size_t)b0 * P.ldwb; Rr.ldT = P.ldwb;
                Rr.r = (int)bg->wb_P;
            }
            aa.sorted_pos = (ng == 1 ? d_pos : d_posw) + (size_t)gi * BLK; aa.A = ctx->ws_A.as<double>(); aa.ldA = P.ldAw;
            aa.wb_k1 = bg->kin_k1; aa.wb_R = bg->wb_R.as<double>(); aa.wb_ldR = P.ldwb;
            aa.wb_E1X = ctx->ws_S.as<double>(); aa.wb_ldE1X = P.ld_ah;
            aa.wb_E1yW = wb_E1yW + (size_t)gi * bg->kin_k1 * 128; aa.wb_ldE1yW = 128;
            aa.wb_E1g = ctx->ws_TH.as<double>() + b0; aa.wb_ldE1g = P.ldb; aa.wb_EE = bg->wb_EE.as<double>(); aa.wb_Gw = wb_Gw;
        }
        double* slow_ws = P.slow_forms ? ctx->ws_xwide.as<double>() : nullptr;   // (the null fits of the block are done: their scratch is free)
        CRM_TRY(launch_assemble(st, aa, nb, ctx->ws_Gext.as<double>(), slow_ws, &ctx->gram_dma_launches));
        CRM_TRY(launch_eig_davies(st, ctx->ws_F.as<double>(), d_Q, nb, k0, d_lam, d_pv, d_if, d_liu, true, slow_ws));
        if (o.exact) {
            CRM_TRY(launch_tail_pvalue(st, d_Q, d_lam, nb, k0, d_tp, d_tlp, d_tst));
            if (o.logp) CRM_HIP(hipMemcpyAsync(o.logp + done, d_tlp, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
            if (o.status) CRM_HIP(hipMemcpyAsync(o.status + done, d_tst, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        }
        if (o.pv) CRM_HIP(hipMemcpyAsync(o.pv + done, o.exact ? d_tp : d_pv, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        if (o.Q) CRM_HIP(hipMemcpyAsync(o.Q + done, d_Q, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        if (o.lambda) CRM_HIP(hipMemcpyAsync(o.lambda + done * k0, d_lam, sizeof(double) * nb * k0, hipMemcpyDeviceToHost, st));
        if (o.F) CRM_HIP(hipMemcpyAsync(o.F + done * k0 * k0, ctx->ws_F.ptr, sizeof(double) * nb * k0 * k0, hipMemcpyDeviceToHost, st));
        if (o.ifault) CRM_HIP(hipMemcpyAsync(o.ifault + done, d_if, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        if (o.liu) CRM_HIP(hipMemcpyAsync(o.liu + done, d_liu, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        std::vector<char> flat;
        std::vector<double> probe_rec;
        if (o.flags) CRM_TRY(flat_probes(B, R, gi, aa, slow_ws, flat, probe_rec));
        if (o.flags && ng == 1) {   // (diagnostics: what the probes measured, crm_test_null_fit_probe_read)
            if (done == 0) ctx->probe_out.clear();
            ctx->probe_out.insert(ctx->probe_out.end(), probe_rec.begin(), probe_rec.end());
        }
        const double rho_kappa = RHO_KAPPA * 1e-3 * form("flat_kappa_milli", 1000);
        int rmax = 0;
        for (int i = 0; i < nrho; i++) rmax = std::max(rmax, bg->r[i]);
        const bool saturated = (long)rmax + c + 1 >= n;
        const NullFitOut* fit = h_fit.data() + (size_t)gi * BLK + b0;
        for (int b = 0; b < nb; b++) {
            const NullFitOut& f = fit[b];
            const double rho = bg->rho[f.rho_index];
            if (o.flags) {
                int fl = saturated ? CRM_MODEL_SATURATED : 0;
                if (!(f.delta > 1e-8)) fl |= CRM_MODEL_DELTA_AT_ZERO;
                if (!f.use_g) fl |= CRM_MODEL_G_IN_SPAN_W;
                if (!flat.empty() && (flat[b] & 1)) fl |= CRM_MODEL_FLAT_OPTIMUM;
                if (!flat.empty() && (flat[b] & 2)) fl |= CRM_MODEL_STATISTIC_AT_TOLERANCE;
                if (f.rho_decision == f.rho_decision && !(f.rho_decision > rho_kappa)) fl |= CRM_MODEL_RHO_TIE;
                o.flags[done + b] = fl;
            }
            if (o.rho1) o.rho1[done + b] = rho;
            if (o.e2) o.e2[done + b] = f.v0 * rho;
            if (o.g2) o.g2[done + b] = f.v0 * (1 - rho);
            if (o.eps2) o.eps2[done + b] = f.v1;
            if (o.lml) o.lml[done + b] = f.lml;
            if (o.delta) o.delta[done + b] = f.delta;
            if (o.scale) o.scale[done + b] = f.scale;
        }
        // the per-gene device buffers (Q, F, pv) are reused by the next gene
        CRM_HIP(hipStreamSynchronize(st));
        return CRM_OK;
    }
};

// One pass over variants [first, first + count) for one or several genes that share the background,
// the covariates W and the contexts E0 (several phenotypes against one panel).  What does not depend
// on the phenotype is done once per block: the block copies, T(rho) = G'Q0(rho), the Khatri-Rao
// contraction per (variant, rho) pair that at least one gene selected, and the y-free side
// contractions.  Per gene: g'y, the null fits, E'(g o y), assembly, eigenvalues and Davies.
//
// allow_collapse = false keeps a grouped panel on the dense path; near_out (collapsed passes only) receives the positions
// (relative to `first`) of the variants that are nearly collinear with the covariates -- scan_core repeats those on the
// dense path, where the block is orthogonalised against W in the cell axis (blockops.hip: launch_ortho_block).
static int scan_pass(const std::vector<crm_gene*>& genes, crm_panel* panel, long first, long count,
                     const int* idx_E, const int* idx_G, const std::vector<ScanOut>& outs, bool allow_collapse,
                     std::vector<long>* near_out) {
    crm_gene* g0 = genes[0];
    crm_background* bg = g0->bg;
    crm_ctx* ctx = bg->ctx;
    if (panel->ctx != ctx) {
        set_error("scan: gene and panel live on different contexts");
        return CRM_ERR_ARG;
    }
    if (panel->n != bg->n) {
        set_error("scan: panel has %ld cells, background has %ld", panel->n, bg->n);
        return CRM_ERR_ARG;
    }
    if (panel->grouped && panel->m + 1 > BLOCK_SLACK_MAX) {
        set_error("scan: grouped panel with %ld groups (supported up to %d)", panel->m, BLOCK_SLACK_MAX - 1);
        return CRM_ERR_UNSUPPORTED;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("scan: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    for (crm_gene* g : genes) {
        // the shared pass computes g'W, the context features and the donor tables once, from the first
        // gene's W and E0: the others must hold the same values, not just the same shapes
        if (g->bg != bg || g->c != g0->c || g->k0 != g0->k0 || g->w_key != g0->w_key || g->e0_key != g0->e0_key) {
            set_error("scan: genes of one call must share the background, W and E0 (contents, not only shapes)");
            return CRM_ERR_ARG;
        }
    }
    if (count == 0) return CRM_OK;
    if (ctx->in_scan) {
        set_error("scan: another scan is running on this context (started from a progress callback?); its work buffers are in use");
        return CRM_ERR_UNSUPPORTED;
    }
    struct InScan { crm_ctx* c; explicit InScan(crm_ctx* c_) : c(c_) { c->in_scan = true; } ~InScan() { c->in_scan = false; } } in_scan(ctx);
    // (the Gram kernel stages all k0 + c + 2 rows of a variant in LDS: refused here, before anything is launched, with
    // the limit named; past 144 rows / 128 contexts the scan runs through the slower forms of its per-variant kernels)
    if (g0->k0 + g0->c + 2 > CRM_MAX_GRAM_ROWS) {
        set_error("interaction scan: %d contexts with %d covariate columns (supported: contexts + covariates + 2 <= %d; "
                  "the association scans take up to %d covariate columns)", g0->k0, g0->c, CRM_MAX_GRAM_ROWS,
                  CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    if (ctx->polish && g0->c > CRM_MAX_COV) {
        set_error("interaction scan: the null-fit polish is only built for up to %d covariate columns", CRM_MAX_COV);
        return CRM_ERR_UNSUPPORTED;
    }
    CRM_HIP(hipSetDevice(ctx->device));
    const long n = bg->n;
    for (long i = 0; i < n; i++) {
        if ((idx_E && (idx_E[i] < 0 || idx_E[i] >= n)) || (idx_G && (idx_G[i] < 0 || idx_G[i] >= n))) {
            set_error("scan: permutation index out of range at position %ld", i);
            return CRM_ERR_ARG;
        }
    }
    if ((int)bg->s0_max.size() != bg->nrho) {   // (filled when the background was sealed / created)
        set_error("scan: the background was not sealed");
        return CRM_ERR_INTERNAL;
    }
    ScanPass S(genes, panel, first, count, idx_E, idx_G, outs, allow_collapse, near_out);
    const ScanPlan& P = S.P;
    CRM_TRY(S.workspaces());
    CRM_TRY(S.prepare_contexts());
    CRM_TRY(S.prepare_kinship());
    CRM_TRY(S.prepare_woodbury());
    for (long done = 0; done < count; done += P.BLK) {
        Block B;
        B.done = done;
        B.col0 = first + done;
        B.nb = (int)std::min<long>(P.BLK, count - done);
        TraceRange range_block("crm scan block");
        CRM_TRY(S.copy_block(B));
        CRM_TRY(S.block_stats(B));
        if (!P.fastT && !P.collapsed()) CRM_TRY(crm_background_require_q0(bg, -1));
        if (ctx->replay_mode == 2) {
            CRM_TRY(S.replay_block(B));
            if (P.wb()) CRM_TRY(S.woodbury_phi(B));
        } else {
            CRM_TRY(S.rotations(B));   // (unrelated-donor form: with Phi'gx, woodbury_phi)
            CRM_TRY(S.null_fits(B));
            if (ctx->probe_on) return CRM_OK;   // (test hook: the pass ends with this block's records)
        }
        if (P.wb()) ctx->unrelated_donor_blocks++;
        CRM_TRY(S.collect_fits(B));
        for (int b0 = 0; b0 < B.nb;) {
            const SubRange R = S.sub_range(B, b0);
            Pairs Q;
            CRM_TRY(S.select_pairs(B, R, Q));
            CRM_TRY(S.form_A(B, R, Q));
            CRM_TRY(S.side_contractions(B, R));
            CRM_TRY(S.z1_products(B, R));
            for (int gi = 0; gi < S.ng; gi++) CRM_TRY(S.gene_results(B, R, gi));
            b0 += R.nb;
        }
        ctx->report(done + B.nb, count);   // (the reference's tqdm, :340)
    }
    return CRM_OK;
}

// The scan of [first, first + count): one pass, plus -- after a collapsed pass -- a dense pass over every run of variants
// the collapsed one marked as nearly collinear with the covariates (their results are overwritten).
static int scan_core(const std::vector<crm_gene*>& genes, crm_panel* panel, long first, long count,
                     const int* idx_E, const int* idx_G, const std::vector<ScanOut>& outs) {
    std::vector<long> near;
    CRM_TRY(scan_pass(genes, panel, first, count, idx_E, idx_G, outs, true, &near));
    crm_ctx* ctx = genes[0]->ctx;
    if (near.empty() || ctx->probe_on) return CRM_OK;
    const int k0 = genes[0]->k0;
    struct Quiet {   // (the repeated variants were reported as done by the first pass)
        crm_ctx* c;
        explicit Quiet(crm_ctx* c_) : c(c_) { c->progress_muted = true; }
        ~Quiet() { c->progress_muted = false; }
    } quiet(ctx);
    ctx->dense_repeats += (long)near.size();
    // runs of marked variants, neighbours closer than 32 variants merged (a dense pass has a fixed cost of a few
    // milliseconds whatever its length); a panel that is marked on more than a quarter of its variants is simply scanned
    // again as a whole
    if ((long)near.size() * 4 > count) {
        near.resize((size_t)count);
        for (long v = 0; v < count; v++) near[(size_t)v] = v;
    }
    for (size_t i = 0; i < near.size();) {
        size_t j = i + 1;
        while (j < near.size() && near[j] <= near[j - 1] + 32) j++;
        const long off = near[i], len = near[j - 1] - near[i] + 1;
        std::vector<ScanOut> shifted(outs);
        for (ScanOut& o : shifted) {
            auto at = [&](double* p, long stride) { return p ? p + off * stride : nullptr; };
            o.pv = at(o.pv, 1); o.rho1 = at(o.rho1, 1); o.e2 = at(o.e2, 1); o.g2 = at(o.g2, 1); o.eps2 = at(o.eps2, 1);
            o.Q = at(o.Q, 1); o.lml = at(o.lml, 1); o.delta = at(o.delta, 1); o.scale = at(o.scale, 1);
            o.lambda = at(o.lambda, k0); o.F = at(o.F, (long)k0 * k0); o.liu = at(o.liu, 1); o.logp = at(o.logp, 1);
            if (o.ifault) o.ifault += off;
            if (o.status) o.status += off;
            if (o.flags) o.flags += off;
        }
        CRM_TRY(scan_pass(genes, panel, first + off, len, idx_E, idx_G, shifted, false, nullptr));
        i = j;
    }
    return CRM_OK;
}

}  // namespace crm

extern "C" {

int crm_scan_interaction(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                         const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2,
                         double* out_g2, double* out_eps2, double* out_Q, double* out_lml,
                         double* out_delta, double* out_scale, double* out_lambda, double* out_F) {
    return crm::guarded_on("crm_scan_interaction", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    std::vector<ScanOut> outs{{out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q, out_lml, out_delta,
                               out_scale, out_lambda, out_F}};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

int crm_scan_interaction_tail(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                              const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2,
                              double* out_g2, double* out_eps2, double* out_Q, double* out_lml,
                              double* out_delta, double* out_scale, double* out_lambda, double* out_F,
                              double* out_logp, int* out_status) {
    return crm::guarded_on("crm_scan_interaction_tail", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q, out_lml, out_delta, out_scale, out_lambda, out_F};
    o.exact = true;
    o.logp = out_logp;
    o.status = out_status;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

int crm_scan_interaction_info(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                              const int* idx_G, double* out_pvalue, int* out_ifault, double* out_liu_pvalue,
                              int* out_model_flags) {
    return crm::guarded_on("crm_scan_interaction_info", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    o.ifault = out_ifault;
    o.liu = out_liu_pvalue;
    o.flags = out_model_flags;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

// B permutations of one scan (include/crm_hip.h): the first permutation's pass records, per block, the fits and the rows
// T(rho*); the others replay them.  The panel is walked in chunks that keep the record within REPLAY_CAP_BYTES.
static int scan_permuted(crm_gene* gene, crm_panel* panel, long first, long count, int nperm, const int* idx_E,
                         const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                         double* out_eps2, double* out_Q, bool exact, double* out_logp, int* out_status) {
    if (!gene || !panel || nperm < 1 || !out_pvalue) return CRM_ERR_ARG;
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("scan: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    crm_ctx* ctx = gene->ctx;
    if (ctx->replay_mode != 0 || ctx->in_scan) {
        set_error("scan: another scan is running on this context");
        return CRM_ERR_UNSUPPORTED;
    }
    const long n = gene->bg->n;
    constexpr double REPLAY_CAP_BYTES = 8.0 * (1ull << 30);
    // (whole blocks of the scan as one call over all `count` variants would cut them: the same launches, the same bits)
    const long blk = scan_block_variants(ctx, gene, count);
    const long chunk_cap = std::max<long>(blk, (long)(REPLAY_CAP_BYTES / (sizeof(double) * (double)gene->bg->ldq)) / blk * blk);
    struct Clear { crm_ctx* c; ~Clear() { c->replay_clear(); } } clear{ctx};
    std::vector<crm_gene*> genes{gene};
    for (long at = 0; at < count; at += chunk_cap) {
        const long len = std::min(chunk_cap, count - at);
        ctx->replay_clear();
        for (int q = 0; q < nperm; q++) {
            ctx->replay_mode = q == 0 ? 1 : 2;
            ctx->replay_cursor = 0;
            // (rho*, the variance components and the fit do not depend on the permutation: written by the first pass)
            ScanOut o{out_pvalue + (size_t)q * count + at, nullptr, nullptr, nullptr, nullptr,
                      out_Q ? out_Q + (size_t)q * count + at : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (q == 0) {
                o.rho1 = out_rho1 ? out_rho1 + at : nullptr; o.e2 = out_e2 ? out_e2 + at : nullptr;
                o.g2 = out_g2 ? out_g2 + at : nullptr; o.eps2 = out_eps2 ? out_eps2 + at : nullptr;
            }
            o.exact = exact;
            o.logp = out_logp ? out_logp + (size_t)q * count + at : nullptr;
            o.status = out_status ? out_status + (size_t)q * count + at : nullptr;
            std::vector<ScanOut> outs{o};
            const int rc = scan_core(genes, panel, first + at, len, idx_E ? idx_E + (size_t)q * n : nullptr,
                                     idx_G ? idx_G + (size_t)q * n : nullptr, outs);
            if (rc != CRM_OK) return rc;
        }
    }
    return CRM_OK;
}

int crm_scan_interaction_permuted(crm_gene* gene, crm_panel* panel, long first, long count, int nperm, const int* idx_E,
                                  const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                                  double* out_eps2, double* out_Q) {
    return crm::guarded_on("crm_scan_interaction_permuted", gene ? gene->ctx : nullptr, [&]() -> int {
    return scan_permuted(gene, panel, first, count, nperm, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2,
                         out_Q, false, nullptr, nullptr);
    });
}

int crm_scan_interaction_permuted_tail(crm_gene* gene, crm_panel* panel, long first, long count, int nperm,
                                       const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                                       double* out_e2, double* out_g2, double* out_eps2, double* out_Q,
                                       double* out_logp, int* out_status) {
    return crm::guarded_on("crm_scan_interaction_permuted_tail", gene ? gene->ctx : nullptr, [&]() -> int {
    return scan_permuted(gene, panel, first, count, nperm, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2,
                         out_Q, true, out_logp, out_status);
    });
}

int crm_scan_interaction_bounds(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E, const int* idx_G,
                                double* out_pvalue, int* out_ifault, double* out_liu_pvalue, int* out_model_flags,
                                double* out_bound_Q, double* out_bound_p) {
    return crm::guarded_on("crm_scan_interaction_bounds", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel || !out_model_flags) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    o.ifault = out_ifault;
    o.liu = out_liu_pvalue;
    o.flags = out_model_flags;
    o.bound_Q = out_bound_Q;
    o.bound_p = out_bound_p;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

long crm_test_tail_launches(const crm_ctx* ctx) { return ctx ? ctx->tail_launches : -1; }

long crm_test_spectrum_tail_launches(const crm_ctx* ctx) { return ctx ? ctx->spectrum_tail_launches : -1; }

long crm_test_dense_repeats(const crm_ctx* ctx) { return ctx ? ctx->dense_repeats : -1; }

long crm_test_donor_pair_blocks(const crm_ctx* ctx) { return ctx ? ctx->donor_pair_blocks : -1; }

int crm_test_gram_dma_launches(const crm_ctx* ctx, long* launches) {
    return crm::guarded("crm_test_gram_dma_launches", [&]() -> int {
    if (!ctx || !launches) return CRM_ERR_ARG;
    *launches = ctx->gram_dma_launches;
    return CRM_OK;
    });
}
int crm_test_unrelated_donor_blocks(const crm_ctx* ctx, long* blocks) {
    return crm::guarded("crm_test_unrelated_donor_blocks", [&]() -> int {
    if (!ctx || !blocks) return CRM_ERR_ARG;
    *blocks = ctx->unrelated_donor_blocks;
    return CRM_OK;
    });
}

int crm_test_rho0_position_blocks(const crm_ctx* ctx, long* blocks) {
    return crm::guarded("crm_test_rho0_position_blocks", [&]() -> int {
    if (!ctx || !blocks) return CRM_ERR_ARG;
    *blocks = ctx->rho0_position_blocks;
    return CRM_OK;
    });
}
int crm_test_rotation_tail_launches(const crm_ctx* ctx, long* launches) {
    return crm::guarded("crm_test_rotation_tail_launches", [&]() -> int {
    if (!ctx || !launches) return CRM_ERR_ARG;
    *launches = ctx->rotation_tail_launches;
    return CRM_OK;
    });
}

long crm_test_tests_without_pair(const crm_ctx* ctx) { return ctx ? ctx->tests_without_pair : -1; }

int crm_test_set_shared_h(crm_ctx* ctx, int mode) {
    return crm::guarded_on("crm_test_set_shared_h", ctx, [&]() -> int {
    if (!ctx) return CRM_ERR_ARG;
    ctx->tune.shared_h = mode < 0 ? -1 : (mode > 0 ? 1 : 0);
    return CRM_OK;
    });
}

static int scan_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, const int* idx_E,
                      const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                      double* out_eps2, double* out_Q, bool exact, double* out_logp, int* out_status) {
    if (!genes || ngenes < 1 || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> gs(genes, genes + ngenes);
    for (crm_gene* g : gs)
        if (!g) return CRM_ERR_ARG;
    std::vector<ScanOut> outs(ngenes);
    for (int i = 0; i < ngenes; i++) {
        auto at = [&](double* base) { return base ? base + (size_t)i * count : nullptr; };
        outs[i] = ScanOut{at(out_pvalue), at(out_rho1), at(out_e2), at(out_g2), at(out_eps2), at(out_Q),
                          nullptr, nullptr, nullptr, nullptr, nullptr};
        outs[i].exact = exact;
        outs[i].logp = at(out_logp);
        outs[i].status = out_status ? out_status + (size_t)i * count : nullptr;
    }
    return scan_core(gs, panel, first, count, idx_E, idx_G, outs);
}

int crm_scan_interaction_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                               const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                               double* out_e2, double* out_g2, double* out_eps2, double* out_Q) {
    return crm::guarded_on("crm_scan_interaction_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    return scan_multi(genes, ngenes, panel, first, count, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q,
                      false, nullptr, nullptr);
    });
}

int crm_scan_interaction_multi_tail(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                                    const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                                    double* out_e2, double* out_g2, double* out_eps2, double* out_Q, double* out_logp,
                                    int* out_status) {
    return crm::guarded_on("crm_scan_interaction_multi_tail", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr,
                           [&]() -> int {
    return scan_multi(genes, ngenes, panel, first, count, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q,
                      true, out_logp, out_status);
    });
}

}  // extern "C"

