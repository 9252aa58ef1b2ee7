// The scan pass behind the interaction scan's entry points (scan.hip): its plan, the records its stages hand on, and ScanPass
// itself -- one member function per stage, defined in scan_prepare.hip, scan_block.hip, scan_pairs.hip and scan_results.hip.
#pragma once
#include <algorithm>
#include <vector>

#include "assemble.h"
#include "nullfit.h"
#include "objects.h"

namespace crm {

int ctx_cus(const crm_ctx* ctx);   // (scan_block.hip)

// Collapsed path: a variant that keeps less than this share of its squared norm outside span(W) is repeated on the dense
// path (the donor-level sums can only form [W, g]'K^-1[W, g] in the raw basis: eps / share instead of eps / sqrt(share))
constexpr double COLLINEAR_TAU = 1e-2;

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

    // The same outputs from variant `off` on: what scan_core hands to the dense repeat of a run of variants.  EVERY
    // per-variant array of the list above is shifted here and nowhere else -- a field added to the list gets its line in
    // `advanced` with it, or the repeat writes it at the start of the call's range (as bound_Q / bound_p once were).
    ScanOut advanced(long off, int k0) const {
        ScanOut o = *this;
        auto at = [off](auto* p, long stride) { return p ? p + off * stride : nullptr; };
        o.pv = at(pv, 1); o.rho1 = at(rho1, 1); o.e2 = at(e2, 1); o.g2 = at(g2, 1); o.eps2 = at(eps2, 1);
        o.Q = at(Q, 1); o.lml = at(lml, 1); o.delta = at(delta, 1); o.scale = at(scale, 1);
        o.lambda = at(lambda, k0); o.F = at(F, (long)k0 * k0);
        o.ifault = at(ifault, 1); o.liu = at(liu, 1); o.flags = at(flags, 1);
        o.bound_Q = at(bound_Q, 1); o.bound_p = at(bound_p, 1);
        o.logp = at(logp, 1); o.status = at(status, 1);
        return o;
    }
};

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
// the records of the kinship-structure routes (ScanPlan::kin_probs); after those, the records of the side stream's launches
// (ScanPlan::side_probs: the donors' pair products, Z2, Z3, Z1 -- read while the main stream writes the slots before them);
// last, the Z1 problems
constexpr int SLOT_ONE = 0, SLOT_RHO = 1, SLOT_KIN = 2 * CRM_MAX_RHO + 4;

// What a pass does: sizes, leading dimensions, splits and the route, fixed before anything is launched (plan_scan).
// e1_sym, donor_pairs, pairs_unfolded and wb_rotate are what the shapes allow: the data has the last word (ScanPass::probed).
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
    int npair = 0, KT = 0, KK = 0, kin_probs = 0, side_probs = 0;
    // kdim: contraction length of the products with the mixing matrices; mp: groups of a grouped panel, padded; xrows:
    // contraction length of the block products -- cells, or on the collapsed path the groups
    long kdim = 0, mp = 0, xrows = 0;
    bool collapsed() const { return route == Route::collapsed; }
    bool kin() const { return route == Route::kin_unfolded || route == Route::kin_folded || route == Route::unrelated; }
    bool folded() const { return route == Route::kin_folded || route == Route::unrelated; }
    bool wb() const { return route == Route::unrelated; }
    bool through_H() const { return fastT && (ng > 1 || kin()); }   // (the operands of the routes through H exist)
    int side_slot() const { return SLOT_KIN + kin_probs; }
    int z1_slot() const { return side_slot() + side_probs; }
};

// (scan_plan.hip)
int scan_block_variants(const crm_ctx* ctx, const crm_gene* g0, long count);
ScanPlan plan_scan(const std::vector<crm_gene*>& genes, const crm_panel* panel, const int* idx_G, bool allow_collapse,
                   long count);

// (scan_prepare.hip)
long donor_run_records(const crm_background* bg, const GemmProblem& p, long c_step, GemmProblem* out);
void woodbury_records(const crm_background* bg, const GemmProblem& p, long x_step, GemmProblem* out);
struct SameColumns { const double* A; long lda; const double* B; long ldb; long rows; };
int same_columns(hipStream_t st, int* d_flag, int k, std::initializer_list<SameColumns> pairs, bool& same);

struct Block {      // variants [col0, col0 + nb) of the panel, `done` into the call
    long done = 0, col0 = 0;
    int nb = 0;
    double* Gb = nullptr;   // the aligned copy (collapsed path: the group dosage slab)
    double* Gt = nullptr;   // the test direction's role (rows permuted under the genotype hook)
    double* Gx = nullptr;   // the fixed effects' role (orthogonalised against W)
    long ldt = 0;           // leading dimension of Gb and Gt: the block buffers', or the panel's where the block is read in place
    bool fused = false;     // read in place; block_stats' fused pass has written G2, GG and the donor-order copies as well
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
struct DonorCols {  // (ScanPass::donor_columns) the operand columns in cell order (G) and in donor order (Gk)
    bool in_pair_order;
    const double* G; long ldg;
    const double* Gk; long ldk;
    int ncol;
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
    const ScanPlan P;
    // what prepare_kinship found in the data about the forms the plan allows; written there alone, read by the pair stage
    struct Probed { bool e1_sym, donor_pairs, pairs_unfolded, wb_rotate; } probed{P.e1_sym, P.donor_pairs, P.pairs_unfolded, P.wb_rotate};
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
    bool gram_fused = false;                // the sub-range's wb_Gw came from the pair products (folded_S: launch_wb_gram_fused)
    // The side stream (scan_side.hip).  side_form: form("side_stream") where the pass is served, else 0; side_recs: the host
    // copy of the block's side records, alive as long as the pass (side_maxlen: the longest donor run of its pair products);
    // side_enqueued: the block's side launches are in the side stream's queue
    int side_form = 0;
    bool side_enqueued = false;
    long side_maxlen = 0;
    std::vector<GemmProblem> side_recs;

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
    // A fit that ends with (practically) no kinship term -- delta at the upper clamp, v0 = 2.2e-16 scale: a phenotype without
    // a random effect, half of an eQTL run -- has K0 = v1 (I + (v0 / v1) Q0 S0 Q0'): where (v0 / v1) max S0 <= 1e-10 the
    // rotated test direction A~ enters Q and F with weights d_j <= 1e-10, below the tolerance of the test by four orders of
    // magnitude, while its product is most of a step.  Such tests get no (variant, rho*) pair: their Gram reads rows of zeros
    // (AssembleArgs::A_none).  rho* of such a fit is decided by rounding (the likelihood is flat in rho), so over many
    // phenotypes these are also the fits that would scatter a variant's pairs over the whole grid.
    bool no_kinship_term(const NullFitOut& f) const {
        return P.skip_pairs && f.v1 > 0.0 && f.v0 >= 0.0 && f.v0 * bg->s0_max[f.rho_index] <= 1e-10 * f.v1;
    }

    // ---- scan_prepare.hip -------------------------------------------------------------------------------------------
    int workspaces();
    bool keep_tables() const { return !idx_E; }
    int context_features(bool shared_too);
    int prepare_contexts();
    int prepare_kinship();
    int prepare_woodbury();
    // ---- scan_block.hip ---------------------------------------------------------------------------------------------
    bool fused_pass() const;
    bool fused_block(long col0, int nb) const;
    int copy_block(Block& B);
    int block_stats(Block& B);
    int fold_TH(const Block& B);
    int unfolded_TH(const Block& B);
    int plain_TH(const Block& B);
    bool cut_choice(int nb, int cnt, const int* N, bool* is_cut, long& acc, long& rounds) const;
    int cut_rotations(const Block& B, int n_list, int& n_main);
    int rotations(const Block& B);
    int plan_rotations(const Block& B, const GemmProblem* all);
    int null_fits(const Block& B);
    int replay_block(const Block& B);
    int woodbury_phi(const Block& B);
    int collect_fits(Block& B);
    // ---- scan_pairs.hip ---------------------------------------------------------------------------------------------
    SubRange sub_range(const Block& B, int b0) const;
    int select_pairs(const Block& B, const SubRange& R, Pairs& Q);
    int direct_splits(const Pairs& Q, AGroups& A, bool* tail_of);
    void a_records(const Pairs& Q, bool via_H, const bool* tail_of, AGroups& A);
    int donor_columns(const Block& B, const SubRange& R, const Pairs& Q, DonorCols& D, hipStream_t on);   // (null: no gather)
    int gather_pairs(const double* src, long rows, const Pairs& Q);
    int folded_S(const Block& B, const SubRange& R, const Pairs& Q);
    int pair_stage(const Block& B, const SubRange& R, const Pairs& Q, const DonorCols& D, GemmProblem* d_kp, long maxlen, long chunk_max,
                   int slices);
    int unfolded_AH(const Block& B, const SubRange& R, const Pairs& Q);
    int direct_AH(const Block& B, const SubRange& R, const Pairs& Q, AGroups& A);
    int woodbury_S(const SubRange& R, const Pairs& Q);
    int form_A(const Block& B, const SubRange& R, const Pairs& Q);
    void side_records(const SubRange& R, GemmProblem* out) const;
    int side_launches(const Block& B, const SubRange& R, hipStream_t on, const GemmProblem* d_recs);
    int side_contractions(const Block& B, const SubRange& R);
    void z1_records(const Block& B, const SubRange& R, GemmProblem* out) const;
    int z1_launches(const SubRange& R, hipStream_t on, const GemmProblem* d_recs);
    int z1_products(const Block& B, const SubRange& R);
    // ---- scan_side.hip ----------------------------------------------------------------------------------------------
    bool side_serves() const;
    bool early_pairs() const { return side_form != 0 && probed.donor_pairs; }   // (the pair products leave the pair stage too)
    int side_prepare(const Block& B);
    int side_fork(const Block& B);
    int side_enqueue(const Block& B);
    int side_join(const Block& B);
    int launch_early_pairs(const Block& B);
    // ---- scan_results.hip -------------------------------------------------------------------------------------------
    int flat_probes(const Block& B, const SubRange& R, int gi, const AssembleArgs& aa, double* slow_ws, std::vector<char>& flat,
                    std::vector<double>& probe_rec);
    AssembleArgs assemble_args(const SubRange& R, int gi) const;
    // the rotated test direction's buffer (unrelated-donor form: the rotated S in block order for several phenotypes -- BLK
    // of them at most), and whether this pass can do without it: every condition of the fused Gram that is known before
    // the first block (the operands' alignment has the last word: wb_gram_fused_serves)
    size_t ws_A_bytes() const {
        return sizeof(double) * (size_t)(P.wb() ? std::max(P.pair_cap, P.BLK) : P.pair_cap) * k0 * P.ldAw;
    }
    bool may_fuse_gram() const {
        const int ts = (2 * k0 + c + 2 + 15) / 16;
        return P.wb_rotate && ng == 1 && P.wb_block && !outs[0].flags && ctx->replay_mode == 0 && k0 % 2 == 0 && ts >= 5 && ts <= 8 &&
               form("wb_gram_fused", 1) != 0 && form("gram_staged", 0) == 0;
    }
    int gene_results(const Block& B, const SubRange& R, int gi);
};

}  // namespace crm
