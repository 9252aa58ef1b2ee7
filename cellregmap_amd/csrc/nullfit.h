// Argument records shared by the per-variant kernels and the host orchestration.
#pragma once
#include "crm_internal.h"

namespace crm {

// ---- null fits (nullfit.hip) -------------------------------------------------------------
struct NullFitRho {
    const double* T;   // [variants x ldT]   rows = Q0(rho)' g
    const double* ty;  // [r]                Q0(rho)' y
    const double* tW;  // [c x ldW]          rows = Q0(rho)' W_i
    const double* S0;  // [r]
    long ldT, ldW;
    int r;
    int pad_;
};

struct NullFitTrial {  // one (variant, rho) fit
    double lml, delta, scale;
    int use_g, nfev;
    double margin;  // brent_search.h: the smallest margin of the decisions that steered the search (units of the objective)
    double noise;   // first-order bound on the rounding noise of the objective at the optimum, in roundings (x 2^-53)
    double curv;    // (f(x + tol) + f(x - tol)) / 2 - f(x) at the stopping point x, tol = 1e-6 |x| + 1e-6: what the objective gains
                    // over one stopping tolerance (units of the objective)
};

struct NullFitOut {
    int rho_index;
    int use_g;  // 0 when g lies in span(W): X = [W, g] is rank deficient
    double lml, delta, scale, v0, v1;
    // How far the fit is from another outcome, in units of its own noise bound (select_rho_kernel):
    // decision = margin / (2^-53 noise) of the search at rho* (include/crm_hip.h: CRM_MODEL_FLAT_OPTIMUM);
    // rho_decision = min over the other grid points i of (lml(rho*) - lml(i)) / (2^-53 (noise(rho*) + noise(i))): how far
    // the choice of rho* itself is from another one (CRM_MODEL_RHO_TIE).  NaN where a kernel does not measure it.
    double decision, rho_decision;
    double margin, noise, gap, curv;   // (the raw figures of the winner: decision = margin / noise; curv: NullFitTrial)
};

struct NullFitArgs {
    NullFitRho rho[CRM_MAX_RHO];
    int nrho, c, restricted;
    int polish;        // secant refinement of the optimum on the analytic derivative
    int exact;         // spectrum pass with IEEE division and one log per entry (the reference's own operations)
    int track;         // 1: the searches leave their trace behind (brent_search.h: margins of their decisions, movement of the
                       // stopping point; the objective's noise bound) -- calls that ask for model flags
    int probe;         // 1: evaluate the objective at probe_x instead of searching (register kernels; test hook)
    double probe_x;
    long n;            // cells (unpadded)
    const double* WW;  // [c x c]
    const double* Wy;  // [c]
    double yy;
    const double* gg;  // [variants]
    const double* gy;  // [variants]
    const double* gW;  // [variants x ld_gW]
    long ld_gW;
    const int* g_drop; // [variants] 1: the variant's direction falls under the reference's rank rule (launch_ortho_rank);
                       // null: decided here from the last pivot of the Cholesky factor of X'X (relative 1e-12)
    double* xwide;        // scratch of the 63..128-column kernel: nullfit_xwide_scratch_doubles(variants, nrho, c) doubles
    NullFitTrial* trial;  // [variants x nrho]
    NullFitOut* out;      // [variants]
};
// nrho, c, n, polish, exact, the grid's rotations of [y, W] and spectra, W'W, W'y, y'y of `gene` on its background
void nullfit_gene_args(NullFitArgs& a, const crm_gene* gene, int restricted);

// c <= CRM_MAX_COV: register kernel (nullfit.hip); larger c (or force_wide): LDS kernel
// (nullfit_wide.hip).  Both end with the rho* selection into a.out.
// queue: CRM_MAX_RHO unsigned counters in device memory (optional; enables the LDS-shared form for c == 1)
int launch_nullfit(hipStream_t st, const NullFitArgs& a, int variants, bool force_wide = false, unsigned* queue = nullptr);
int launch_nullfit_wide(hipStream_t st, const NullFitArgs& a, int variants);
// 63 .. 128 covariate columns (nullfit_xwide.hip): needs NullFitArgs::xwide
int launch_nullfit_xwide(hipStream_t st, const NullFitArgs& a, int variants);
size_t nullfit_xwide_scratch_doubles(int variants, int nrho, int c);

// ---- association paths (assoc.hip) ---------------------------------------------------------------
struct AssocArgs {
    const double* T;   // [variants x ldT] rows Q0(rho*)' g
    const double* ty;  // [r]
    const double* tW;  // [c x ldW]
    const double* S0;  // [r]
    long ldT, ldW;
    int r, c;
    long n;
    double delta0;     // the null model's delta
    const double* WW; const double* Wy; double yy;
    const double* gg; const double* gy; const double* gW; long ld_gW;
};
size_t fastscan_prep_doubles();
int launch_fastscan_prep(hipStream_t st, const AssocArgs& a, double* prep, double* wts);
// one workgroup per gene: args_dev[g] (device memory) -> record prep + g prep_stride, weights wts + g wts_stride
int launch_fastscan_prep_batch(hipStream_t st, const AssocArgs* args_dev, int genes, int c, double* prep, long prep_stride,
                               double* wts, long wts_stride);
int launch_fastscan(hipStream_t st, const AssocArgs& a, const double* prep, const double* wts,
                    int variants, double* alt_lml);
int launch_lrt(hipStream_t st, const double* alt_lml, double null_lml, int count, double* pv);
int launch_gather_trial_lml(hipStream_t st, const NullFitTrial* trial, int count, double* out);

// ---- effect sizes of the association scans (assoc_effects.hip) ------------------------------------
// One phenotype of an effects launch (device copy).  Test (gene a, variant b) reads the variant's row of T(rho*) at
// T[b t_sb + k t_sk] (k over the spectrum), its plain products g'W_u at gW[b gW_sb + u gW_su], gg[b] and gy[b], and
// writes entry b of the outputs (each may be null).
struct AssocEffectsGene {
    const double* T; long t_sb, t_sk;
    const double* ty;  // [r]
    const double* tW;  // [c x ldW]
    const double* S0;  // [r]
    long ldW;
    int r, c;
    long n;
    const double* WW; const double* Wy; double yy;
    const double* gg; const double* gy; const double* gW; long gW_sb, gW_su;
    const double* prep; const double* wts; double delta0;   // fast: the gene's fastscan_prep record, weights and delta
    const NullFitTrial* trial;                               // full refit: [variants] the alt fits (delta, use_g, lml)
    const double* alt_lml;                                   // [variants] what the scan returns
    double null_lml;
    double* out_beta; double* out_se; double* out_delta; double* out_scale; double* out_logp;
    int* out_status;
};
// the host arrays an effects call fills (each may be null)
struct AssocEffectsOut {
    double* beta; double* se; double* delta; double* scale; double* logp;
    int* status;
};
// tests in the order b ngenes + a; c: the covariate columns of every gene of the launch
int launch_assoc_effects(hipStream_t st, const AssocEffectsGene* genes_dev, int ngenes, int variants, int c, bool fast);
// logp[i] = log erfc(sqrt(lrs[i] / 2)), lrs below 0 taken as 0 (the effects kernels' statement; test hook)
int launch_lrt_logp(hipStream_t st, const double* lrs, int count, double* logp);

// ---- per-context fixed-effect tests (context_lrt.hip) ----------------------------------------------
// One launch over a sub-range of variants.  Variant b tests its k candidates x_j = g_b o C_j, one at a time, beside
// X = [X0, g_b] at the variance ratio delta[b]; every n-length product arrives rotated (over the spectrum of Sigma(rho*))
// or as a plain cell-space table.
struct ContextLrtArgs {
    const double* Tx; long tx_slab, ldT;   // candidate j of variant b: Tx + b tx_slab + j ldT, r entries: Q0(rho*)'(g_b o C_j)
    const double* Tg; long ldTg;           // row b: Q0(rho*)'g_b
    const double* tX; long ldW;            // [c x ldW] rows Q0(rho*)'X0_u
    const double* ty;                      // [r]
    const double* S0;                      // [r]
    int r, c, k;
    long n;
    const double* WW; const double* Wy; double yy;                        // X0'X0 [c x c], X0'y [c], y'y
    const double* gg; const double* gy; const double* gW; long ld_gW;     // per variant: g'g, g'y, g'X0
    const double* xXy; long ld_xXy;        // row b k + j: column 0 x_j'y, columns 1 .. c x_j'X0_u
    const double* xx; long ld_xx;          // row b, column j: x_j'x_j
    const double* xg; long ld_xg;          // row b, column j: x_j'g_b
    const double* delta;                   // [variants]
    const int* drop;                       // [variants] 1: the scan's rank rule dropped g_b from [X0, g_b]; null: decided here
    double* phi; long ld_phi;              // scratch, row b: r weights
    // outputs: per candidate (index b k + j), per variant
    double* pvalue; double* alt_lml; double* beta; double* beta_se; double* logp; int* status;
    double* null_lml;
    // several phenotypes in one launch only (xXy then holds x_j'X0_u in columns 0 .. c - 1, shared by the genes)
    const double* xy; long ld_xy;          // row b k + j: x_j'y of this gene
};
size_t context_lrt_lds_bytes(int c);
int launch_context_lrt(hipStream_t st, const ContextLrtArgs& a, int variants);
// The same test over the grid (variant, gene): workgroup (b, q) runs variant b on genes_dev[q] -- one record per gene of a
// rho group, in device memory, whose per-gene tables (ty, X0'y, y'y, g'y, x_j'y, delta, drop), scratch row (phi) and outputs
// are that gene's own and whose Tx, Tg, S0 and plain tables are the group's.  c, k: of every record.
int launch_context_lrt_multi(hipStream_t st, const ContextLrtArgs* genes_dev, int ngenes, int c, int k, int variants);
// Cq[i, j] = E[i, j], C2[i, j] = E[i, j]^2 for j < k, zeros up to ld_out: the contexts as the Khatri-Rao operand and as the
// right-hand operands of the plain products x_j'g = (g o g)'C_j, x_j'x_j = (g o g)'C_j^2
int launch_context_operands(hipStream_t st, const double* E, long lde, long cells_pad, int k, double* Cq, double* C2, long ld_out);
// delta[b] and drop[b] of a sub-block: the gene's delta0 (trial == null), or the alt fits' own
int launch_context_deltas(hipStream_t st, const NullFitTrial* trial, const int* g_drop, double delta0, int variants, double* delta,
                          int* drop);

// ---- joint fixed-effect test of all contexts (context_joint.hip) --------------------------------------
// One launch over a sub-range of variants: variant b tests its k candidates together beside X = [X0, g_b].  `base` as the
// per-context launch takes it, with pvalue, alt_lml, logp and status per VARIANT (index b), beta and beta_se per candidate
// (index b k + j); base.xx is not read.
struct ContextJointArgs {
    ContextLrtArgs base;
    const double* xxp; long ld_xxp;        // row b, column i (i + 1) / 2 + j (j <= i): x_i'x_j
    double* V; long v_slab;                // scratch, row b: (c + 1) x k -- read where context_joint_v_in_lds(c, k) is false
    int v_in_lds;
    int* dof;                              // [variants] candidates kept
    int* dropped;                          // index b k + j: 1 where the candidate left the test
};
bool context_joint_v_in_lds(int c, int k);
size_t context_joint_lds_bytes(int c, int k);
int context_joint_check(int c, int k);     // CRM_ERR_UNSUPPORTED (with the message) past k <= CRM_JOINT_MAX_K, c <= CRM_MAX_COV_XWIDE
int launch_context_joint(hipStream_t st, const ContextJointArgs& a, int variants);
// grid (variant, gene) as launch_context_lrt_multi; every record's V row (where V lives in global memory) is its gene's own
int launch_context_joint_multi(hipStream_t st, const ContextJointArgs* genes_dev, int ngenes, int c, int k, bool v_global,
                               int variants);
// CC[i, a (a + 1) / 2 + b] = E[i, a] E[i, b], b <= a < k, zeros up to ld_out: the right-hand operand of x_a'x_b = (g o g)'(C_a o C_b)
int launch_context_pairs(hipStream_t st, const double* E, long lde, long cells_pad, int k, double* CC, long ld_out);

// ---- small per-block kernels (blockops.hip) ----------------------------------------------------
// gg, gy, gW for a block of variants: column reductions of G (cells x ldg), deterministic.
int launch_variant_stats(hipStream_t st, const double* G, long ldg, long cells, int variants,
                         const double* y, const double* W, long ldw, int c, double* partial,
                         double* gg, double* gy, double* gW, long ld_gW);
size_t variant_stats_workspace(int variants, int c);
// The block in the fixed effects' own basis (blockops.hip): Gx = G - W coef with coef = (W'W)^-1 W'g (gW = W'g of the
// block as launch_variant_stats leaves it; proj = crm_gene::Wproj), thr = the bound on |gx|^2 below which
// numpy_sugar.economic_svd drops the variant's direction from [W, g].  coef: [c x ld_coef], ld_coef >= cols.
int launch_ortho_block(hipStream_t st, const double* G, long ldg, long cells_pad, int variants, int cols,
                       const double* W, long ldw, int c, const double* proj, const double* gW, long ld_gW,
                       double* coef, long ld_coef, double* thr, double* Gx, long ldx);
// The same for a block read in place in the panel, in one pass with the products of launch_square_block and the donor-order
// copies of the kinship routes (blockops.hip: block_pass_kernel); Gx, G2, GG: [cells_pad x ld_out], Gkx, Gkt: donor order
int launch_block_pass(hipStream_t st, const double* G, long ldg, long cells, long cells_pad, int variants, int cols,
                      const double* W, long ldw, int c, const double* proj, const double* gW, long ld_gW, double* coef,
                      long ld_coef, double* thr, double* Gx, double* G2, double* GG, long ld_out, const int* inv,
                      const int* pad_rows, long pads, double* Gkx, double* Gkt);
int launch_ortho_rank(hipStream_t st, const double* gg, const double* thr, int variants, int* drop);
// near[b] = 1 when gg - gW'(W'W)^-1 gW <= tau gg (donor-level sums: the collapsed path's guard)
int launch_collinear_flag(hipStream_t st, const double* gg, const double* gW, long ld_gW, const double* proj, int c,
                          int variants, double tau, int* near);
// out[i, b] = src[row(i), col(b)]: optional row permutation (idx_G) and column order (sorted by rho*).
int launch_gather_block(hipStream_t st, const double* src, long ld_src, long cells_pad, long cells,
                        const int* row_index, const int* col_index, int variants, double* dst,
                        long ld_dst, int dst_cols);
// dst[h, p*k0 + j] = src[h, ord[p]*k0 + j] for p < npairs, zero in the remaining dst_cols
int launch_gather_slabs(hipStream_t st, const double* src, long ld_src, long rows, const int* ord, int npairs,
                        int k0, double* dst, long ld_dst, int dst_cols);
// rows in the donor order of a background's kinship structure: dst[k, :cols] = src[map[k], :cols], zeros where map[k] < 0
int launch_gather_rows(hipStream_t st, const double* src, long ld_src, const int* map, long rows, int cols, double* dst,
                       long ld_dst);
// the per-donor right-hand operand [us | E1] in donor order (crm_background::kin_Y)
int launch_kin_operand(hipStream_t st, const double* U, int k2, const double* H, long ldh, int k1, const int* map, long rows,
                       double* Y, long ldy);
// E1 rows of H'(g o E0): sums of the per-donor blocks S over the donors
int launch_kin_verify(hipStream_t st, const double* H, long ldh, int k1, const double* U, int k2, const int* group,
                      const double* hKd, long ldk, long m, long n, unsigned long long* out);
int launch_kin_sum_e1(hipStream_t st, const double* S, long ld_s, int KT, int k2, int k1, int groups, long cols, double* AH,
                      long ld_ah);
// pair products P[c, a k0 + i] = H[c, a] Ep[c, i] (a < k1), and the rows S[a, b k0 + i] = C[b, a k0 + i] of a product G'P
int launch_pair_features(hipStream_t st, const double* H, long ldh, int k1, const double* Ep, long ld_ep, int k0,
                         long cells_pad, double* P, long ldp);
int launch_pair_rows(hipStream_t st, const double* C, long ldc, int variants, int k1, int k0, double* S, long lds);
// are H[:, :k] and Ep[:, :k] the same numbers (flag[0] |= 1 if not)?  and S[a, b k0 + i] = C[b, pair(a, i)] for E1 = E
int launch_same_columns(hipStream_t st, const double* H, long ldh, const double* Ep, long ld_ep, long cells, int k, int* flag);
int launch_pair_rows_sym(hipStream_t st, const double* C, long ldc, int variants, int k0, double* S, long lds);
bool donor_pairs_serves(int k0);
// (row_d, row_j: row of (donor d, context j) = k1 + d row_d + j row_j; default (k0, 1): the folded form's layout)
int launch_donor_pairs_expand(hipStream_t st, const double* P, long p_slab, long ldp, int donors, int variants, int k0, int k1,
                              double* S, long lds, double* Psum, long psum_slab, int splits, long row_d = 0, long row_j = 0);
bool donor_pairs_rotate_serves(int k0);
// unrelated-donor form: A[(b k0 + i), d k0 + j] = sum_k S_d[k, i] U_d[k, j] with S_d expanded from the pair products, the
// donor sums as launch_donor_pairs_expand forms them (k2 = k0; U: donors slabs of k2pad x ldu)
int launch_donor_pairs_rotate(hipStream_t st, const double* P, long p_slab, long ldp, int donors, int variants, int k0,
                              const double* U, long u_slab, long ldu, int k2pad, double* A, long lda, double* Psum, long psum_slab,
                              int splits);
// dst[k, :cols] = src[k, :cols] * scale[k * ld_scale]
int launch_scale_rows(hipStream_t st, const double* src, long ld_src, const double* scale, long ld_scale, long rows, int cols,
                      double* dst, long ld_dst);
// dense block from a grouped panel: dst[i, b] = Gd[group[row(i)], b]
int launch_expand_block(hipStream_t st, const double* Gd, long ld_gd, const int* group, long cells_pad,
                        long cells, const int* row_index, int variants, double* dst, long ld_dst,
                        int dst_cols);
// Z[i, d] = (group[i] == d)
int launch_indicator(hipStream_t st, const int* group, long cells, long cells_pad, int m, double* Z, long ldz);
// collapsed statistics: gg = sum_d gamma^2 n_d, gy = sum_d gamma ysum_d, gW likewise (sums: [m_pad x 16])
int launch_donor_stats(hipStream_t st, const double* Gam, long ld_gam, int m, int variants,
                       const double* sums, int c, double* gg, double* gy, double* gW, long ld_gW);
// G2 = Gt o Gt, GG = Gt o G
int launch_square_block(hipStream_t st, const double* Gt, const double* G, long ldg, long ldg_t,
                        long cells_pad, int cols, double* G2, double* GG, long ld_out);
// rows of E permuted; YE = [y o E, W_1 o E, ...]; EE = pairwise products E_j E_j' (j <= j')
int launch_context_features(hipStream_t st, const double* E, long lde, const int* row_index,
                            long cells, long cells_pad, int k0, const double* y, const double* W,
                            long ldw, int c, double* Ep, long ld_ep, double* YE, long ld_ye,
                            double* EE, long ld_ee);

// ---- eigenvalues + Davies / Liu (davies.hip) -----------------------------------------------------
// lambda: ascending eigenvalues of the lower triangle of F (count x k x k); pvalue per SKAT rule.
// scratch: eig_scratch_doubles(count, k) doubles (0: F fits LDS, k <= 128)
// trace (test hook only; null in every scan): count x 3 ints -- evaluation counter, abscissas summed, integrations of AS 155
int launch_eig_davies(hipStream_t st, const double* F, const double* Q, int count, int k,
                      double* lambda, double* pvalue, int* ifault, double* liu, bool do_eig, double* scratch = nullptr,
                      int* trace = nullptr);
size_t eig_scratch_doubles(int count, int k);

// ---- exact tail p-values (tail_pvalue.hip) ------------------------------------------------------
// Q [count], lambda [count x k] (as launch_eig_davies writes them) -> pvalue, logp (natural log), status (CRM_TAIL_*).
int launch_tail_pvalue(hipStream_t st, const double* Q, const double* lambda, int count, int k, double* pvalue,
                       double* logp, int* status);

}  // namespace crm
