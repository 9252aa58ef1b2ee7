/* Unit-test hooks of libcrm_hip.so: single kernels exercised through the same C-ABI, and the knobs
 * that force a kernel variant.  Not part of the drop-in boundary (include/crm_hip.h); every knob lives in
 * the context it is given, so distinct contexts stay independent. */
#ifndef CRM_HIP_TEST_H
#define CRM_HIP_TEST_H

#include <stddef.h>

#include "crm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel forms kept beside the default one (process-wide; reset != 0 returns the form to its default):
 *   "gram_staged" 1       score-statistic Gram through the register-staged kernel instead of the direct-to-LDS ones (which
 *                         serve up to 144 rows when every operand row starts on a 16-byte boundary)
 *   "kr_no_tail" 1        the product over the spectrum (Khatri-Rao contraction, or the mixing-matrix product of the
 *                         kinship-structure route) of a block in one launch of 128-column tiles whatever the spectrum
 *   "nullfit_per_wave" 1  null fits with one independent wavefront per (variant, grid point), not the LDS-shared queue
 *   "kin_fold" 0 / 2      never fold the donor-level kinship factor into the mixing matrices / fold with few columns too
 *   "eigh_one_stage" 1    the constructor tridiagonalises every grid point on its own (eigh_trd.hip) instead of the
 *                         two-stage family solver (eigh2_band.hip, eigh2_chase.hip)
 *   "nullfit_exact" 1     null-fit likelihood with IEEE division and one log per spectrum entry
 *   "donor_pairs" 0 / 2   per-donor sums of the kinship-structure route never / always from the symmetric pair features
 *                         (default 1: where the kinship term's contexts are the scan's own and a cost model says so)
 *   "pairs_without_kinship_term" 0   form the rotated test direction for every test, also where the fit has no kinship
 *                         term to speak of (default: not formed where (v0 / v1) max S0 <= 1e-10)
 *   "nullfit_one_per_wave" 1   the LDS-shared null-fit kernel with one fit per wavefront (default: four, one per row of sixteen
 *                         lanes, nullfit.hip) -- the two forms give the same bits
 *   "chase_abort" 1       the bulge chase of the two-stage eigen-solver gives up at its first inter-workgroup wait (what a
 *                         device shared with another process does to it after 2 s): the constructor must come out through
 *                         the one-stage solver with the same spectra
 *   "rho0_positions" 0 / 2   unrelated-donor form: the null fits at rho = 0 never / wherever the background allows it from the
 *                         position basis instead of the rotation MixK(0)'(H'Gx) (default 1: where the batched launch of the
 *                         rotations then runs fewer rounds)
 *   "rotation_tails" 0 / 2   the last r mod 128 <= 16 spectrum columns of the rotations never / wherever eligible through the
 *                         skinny one-pass kernel (default 1: where that saves a round; "kr_no_tail" 1 switches them off too)
 *   "block_fused" 0       a block of a dense panel goes through the copy and the elementwise launches after it, not read in
 *                         place and prepared by the fused pass (default 1; crm_test_fused_blocks)
 *   "wb_gram_fused" 0     unrelated-donor form: the rotated S goes through memory between the rotation launch and the Gram launch,
 *                         not from the pair products straight into the Gram (default 1; crm_test_wb_gram_fused_blocks)
 *   "wb_gram_spread" 0    that fused launch issues a donor's LDS-DMA instructions in a bunch behind each barrier, not one by one
 *                         among the MFMAs of the phase that follows (default 1; the same bits either way)
 *   "side_stream" 0 / 2 / 3   unrelated-donor form, one phenotype: the products of a block that do not depend on its fits 0: in
 *                         the pair stage behind the fits, as before; 1 (default): Z2, Z3 and Z1 on a second, lowest-priority
 *                         stream beside the spectrum tails and the null fits, the per-donor pair products on the main stream
 *                         while the host reads the fits; 2: the main stream waits for the side stream right behind the fork;
 *                         3: the side stream starts only when the main stream has reached the join -- the two extremes of
 *                         the interleaving (crm_test_side_stream_blocks)
 *   "flat_kappa_milli" v  factor (in thousandths) on the noise bound of CRM_MODEL_FLAT_OPTIMUM / CRM_MODEL_RHO_TIE (study tool)
 * These replace the environment switches of earlier versions; the GPU suite flips every one of them. */
int crm_test_set_form(const char* name, int value, int reset);
/* Contraction kernel variant for subsequent launches on this context: tile_width 0 = chosen per
 * launch, 64 or 128 forced; lds_dma = 1 lets 128-wide launches use the direct-to-LDS kernel. */
int crm_test_set_contraction(crm_ctx* ctx, int tile_width, int lds_dma);
/* every > 0 (default 1): Khatri-Rao launches of more than 1024 tiles run as 8 x 64 persistent workgroups that walk
 * contiguous tile runs per XCD and re-align (bounded wait) every `every` generations -- 7.5x less L2-fabric
 * traffic, 0.65 % slower; 0: one workgroup per tile. */
int crm_test_set_contraction_sync(crm_ctx* ctx, int every);
/* Times this context gave the persistent form up because its bounded waits ran out (the 512 workgroups were not
 * co-resident: a shared GPU); from then on its launches use one workgroup per tile. */
long crm_test_sync_fallbacks(const crm_ctx* ctx);
/* CRM_POISON=1 only (else always 0): number of device buffers of this process whose red zone -- 4 KiB of 0xFF behind every
 * allocation -- was found overwritten when the buffer was released, i.e. kernels that wrote past the end of a buffer. */
long crm_test_overruns(void);
/* Bytes held by the live device buffers of the process (red zones not counted): equal before and after a round that
 * creates and destroys its objects, or something leaked. */
long crm_test_live_device_bytes(void);
/* ... and the same inspection, now, of the context's own work buffers (which live as long as the context). */
int crm_test_check_context(crm_ctx* ctx);
/* Self-test of that detector: writes eight bytes past the end of a scratch buffer on purpose (CRM_POISON=1 only) and
 * returns by how much the overrun count grew (1 with the poison fill, 0 without). */
int crm_test_overrun_selftest(crm_ctx* ctx);
/* What a genotype panel holds in device memory, read back as it lies (padding included) so that the builders can be held
 * to a reference.  Layout: out[8] = n, n_pad, p, ld, grouped (0 / 1), m, m_pad, ldz (the last three 0 for a dense panel). */
int crm_test_panel_layout(const crm_panel* panel, long out[8]);
/* One whole buffer of the panel to the host -- what = 0: G double[n_pad x ld] (dense panels), 1: Gd double[m_pad x ld],
 * 2: group int[n], 3: Z double[n_pad x ldz] (grouped panels) -- after waiting for the context's stream and its upload
 * stream, under the context's lock.  A buffer the panel does not hold, or `bytes` other than the buffer's size, is
 * CRM_ERR_ARG with a message; the panel is left as it was. */
int crm_test_panel_read(crm_panel* panel, int what, void* dst, size_t bytes);
/* C (M x N, ld N) = X' Y with X: cells x M, Y: cells x N (row-major, tight). */
int crm_test_contract(crm_ctx* ctx, long cells, int M, int N, const double* X, const double* Y,
                      double* C, int ksplit);
/* C ((B*k0) x N) = KR(G, E)' Y with G: cells x B, E: cells x k0, Y: cells x N. */
int crm_test_contract_kr(crm_ctx* ctx, long cells, int B, int k0, int N, const double* G,
                         const double* E, const double* Y, double* C);
/* Route of the multi-gene scan's contraction: -1 (default) cost model, 0 always per (variant, rho)
 * pair against Q0(rho), 1 once per variant against H followed by Mix(rho) per pair (when the
 * background keeps H). */
int crm_test_set_shared_h(crm_ctx* ctx, int mode);
/* on = 0: scans on this context contract against Q0(rho*) over all cells even when the background knows the donor
 * structure of its kinship factor (crm_background_set_kinship_groups); 1 (default): the kinship-structure route where its
 * flop count is below the direct contraction's; 2: always (environment: CRM_KIN_ROUTE=0 / 1 / 2). */
int crm_test_set_kinship_route(crm_ctx* ctx, int on);
/* Number of Khatri-Rao blocks of this context's scans whose last columns went through the 160-column-tile launch
 * (scan_pairs.hip: spectra with r mod 128 <= 32); tests use it to know which form they exercised. */
long crm_test_tail_launches(const crm_ctx* ctx);
/* ... and whose last few columns of the spectrum (r mod 128 <= 16 on the kinship-structure route) went through the skinny
 * one-pass kernel instead of another 128-column tile of the product with the mixing matrix. */
long crm_test_spectrum_tail_launches(const crm_ctx* ctx);
/* Variants that scans on the donor-collapsed path repeated on the dense path because they were nearly collinear with the
 * covariates (scan_pass.h: COLLINEAR_TAU; the dense path orthogonalises the block against W in the cell axis). */
long crm_test_dense_repeats(const crm_ctx* ctx);
/* Blocks of this context's scans whose per-donor sums H'(g o E0) came from one batched product against the symmetric pair
 * features E (x) E (scan_plan.hip: donor pairs -- the kinship term's contexts are the scan's own; form "donor_pairs": 0 never,
 * 1 where its estimated time is the smaller one, 2 always). */
long crm_test_donor_pair_blocks(const crm_ctx* ctx);
/* Blocks of this context's scans served by the unrelated-donor form: a folded kinship structure whose donor-level kinship
 * hKd hKd' is diagonal takes Q and F through a per-donor Woodbury inverse instead of the product A~ = MixK(rho*)'S
 * (scan_plan.hip: kin_wb; form "kin_diag": 0 never, 1 where the background allows it and the cost model says it pays, 2 wherever
 * the background and the shapes allow it -- k0 + c + 2 + k1 <= 144).  *blocks: the count so far. */
int crm_test_unrelated_donor_blocks(const crm_ctx* ctx, long* blocks);
/* Blocks of this context's interaction scans that were read in place in the panel and prepared by the fused pass (scan_block.hip:
 * copy_block; blockops.hip: block_pass_kernel) instead of the copy and the elementwise launches after it.  Form "block_fused":
 * 0 keeps those launches, 1 (default) fuses every block of a dense panel that starts at a multiple of 128 variants; a block
 * that kept the copy does not count.  *blocks: the count so far. */
int crm_test_fused_blocks(const crm_ctx* ctx, long* blocks);
/* Blocks of this context's scans on the unrelated-donor form whose weighted Gram was formed straight from the per-donor pair
 * products, the rotated S staying in LDS (wb_gram_fused.hip), instead of by the rotation launch and the Gram launch with the
 * rotated S between them.  Form "wb_gram_fused": 0 keeps the two launches, 1 (default) fuses where one phenotype is scanned
 * without model flags or permutation replay, the context count is even and the Gram has 65 to 128 rows.  *blocks: the count
 * so far. */
int crm_test_wb_gram_fused_blocks(const crm_ctx* ctx, long* blocks);
/* Blocks of this context's scans whose side contractions Z2 and Z3 and whose Z1 were enqueued on the context's side stream
 * (scan_side.hip: one phenotype on the unrelated-donor form in block order, no permutation replay, no launch of the
 * persistent contraction form in the pass; form "side_stream": 0 never).  *blocks: the count so far. */
int crm_test_side_stream_blocks(const crm_ctx* ctx, long* blocks);
/* Blocks of this context's scans on the unrelated-donor form whose null fits at rho = 0 read the position basis -- Phi'gx,
 * Phi'[y, W] and s_p(0), the assembly's own operands -- so that the rotation MixK(0)'(H'Gx) was not formed (scan_block.hip:
 * plan_rotations; taken where the kept positions are as many as the grid point's rank; form "rho0_positions" = 0: never).
 * *blocks: the count so far. */
int crm_test_rho0_position_blocks(const crm_ctx* ctx, long* blocks);
/* Blocks whose rotations MixK(rho)'(H'Gx) sent the last few columns of their spectra (r mod 128 <= 16, kinship-structure
 * routes) through the skinny one-pass kernel (scan_block.hip: plan_rotations; form "rotation_tails": 0 never, 1 where the
 * batched launch then takes fewer rounds, 2 wherever a problem is eligible).  *launches: the count so far. */
int crm_test_rotation_tail_launches(const crm_ctx* ctx, long* launches);
/* Score-statistic Grams of this context's scans that went through a direct-to-LDS kernel (gram_ext.hip: up to 144 rows
 * with 16-byte-aligned operands, form "gram_staged" = 0) and not through the register-staged one.  *launches: the count so far. */
int crm_test_gram_dma_launches(const crm_ctx* ctx, long* launches);
/* (phenotype, variant) tests of this context's scans whose selected fit has no kinship term to speak of --
 * (v0 / v1) max S0(rho*) <= 1e-10: delta at its upper clamp -- and for which no rotated test direction A~ was formed
 * (scan_pass.h: no_kinship_term; form "pairs_without_kinship_term" = 0 forms it for every test). */
long crm_test_tests_without_pair(const crm_ctx* ctx);
/* The same product stored transposed: CT (N x (B*k0)). */
int crm_test_contract_kr_t(crm_ctx* ctx, long cells, int B, int k0, int N, const double* G,
                           const double* E, const double* Y, double* CT);
/* Null-fit objective at a given point instead of the search (c <= 8 covariate columns): while on, crm_scan_interaction
 * stops after the null-fit kernels of its first block (outputs untouched) and keeps, per (variant, grid point), the
 * log-likelihood and the scale at x = logit(delta); crm_test_null_fit_probe_read copies them out as
 * [variants][grid points][2] doubles and returns their number (> capacity: CRM_ERR_ARG).  Lets a test compare the
 * likelihood itself with the oracle's at the same point, apart from where the two searches stop.
 * on = 2: the searches run as in any scan (every kernel, every launch form, any covariate count; x is not read) and the
 * pass ends at the same place; crm_test_null_fit_probe_read then copies out [variants][grid points][5] doubles -- lml,
 * delta, scale, the number of objective evaluations and use_g of each search, as the kernels left them in the trial table
 * that the selection of rho* reads -- followed by [variants] doubles: the grid index that selection wrote per variant
 * (variants x (5 grid points + 1) numbers in all, which is the count returned).  One phenotype per pass: the trial table is
 * written again per phenotype, so a pass over several returns CRM_ERR_ARG.  on = 0 switches the hook off; any other value
 * is CRM_ERR_ARG. */
int crm_test_null_fit_probe(crm_ctx* ctx, int on, double x);
int crm_test_null_fit_probe_read(crm_ctx* ctx, double* out, long capacity);
/* Eigenvalues (ascending) of `count` symmetric k x k matrices (lower triangle read). */
int crm_test_eigvalsh(crm_ctx* ctx, int count, int k, const double* F, double* lambda);
/* Davies/Liu p-values for `count` (Q, lambda[k]) pairs after the eigenvalue filter. */
int crm_test_davies(crm_ctx* ctx, int count, int k, const double* Q, const double* lambda,
                    double* pvalue, int* ifault, double* liu);
/* The same launch, which also reports the path AS 155 took per pair: trace [count][3] = (evaluation counter, abscissas summed
 * over all integrations, number of integrations), written by lane 0 of each wavefront.  Every other launch of the kernel passes
 * a null trace and runs the instantiation that keeps no such counters; pvalue, ifault and liu have the bits crm_test_davies
 * gives. */
int crm_test_davies_trace(crm_ctx* ctx, int count, int k, const double* Q, const double* lambda,
                          double* pvalue, int* ifault, double* liu, int* trace);
/* Exact tail p-values (crm_scan_interaction_tail's method) for `count` (Q, lambda[k]) pairs, lambda as the scan's
 * eigenvalues (the filter is applied here): p, log p (natural) and CRM_TAIL_* status per pair. */
int crm_test_tail_pvalue(crm_ctx* ctx, int count, int k, const double* Q, const double* lambda, double* pvalue,
                         double* logp, int* status);

/* The log p-value of the association effects calls (out_logp) for `count` likelihood-ratio statistics. */
int crm_test_lrt_logp(crm_ctx* ctx, int count, const double* lrs, double* logp);

/* Bytes the rotated candidates Q0(rho*)'(g o C_j) of one sub-range of crm_scan_interaction_contexts may take (a block of
 * variants is cut into sub-ranges of at least one variant that stay within it); 0 restores the default of 8 GB.  The
 * results do not depend on it, bit for bit. */
int crm_test_set_context_budget(crm_ctx* ctx, long bytes);

/* The background constructor's symmetric eigen-solver on `batch` host matrices A (dim x dim each, row-major,
 * tight): lam (batch x dim, ascending), Z (batch x dim x dim, column j = eigenvector j; may be NULL).
 * stage 0: the whole solver; 1: tridiagonalisation only (d_out / e_out: batch x dim diagonals and
 * sub-diagonals, e[dim - 1] unused); 2: tridiagonal eigenproblem without the back-transformation (Z then
 * holds the eigenvectors of the tridiagonal matrix). */
int crm_test_eigh(crm_ctx* ctx, int batch, int dim, const double* A, double* lam, double* Z, int stage,
                  double* d_out, double* e_out);

/* The constructor's two-stage solver for a family of grid points A_q = D_q C D_q, D_q = diag(wa[q] on the first 64
 * coordinates, wb[q] on the rest) (cellregmap_amd/csrc/eigh2_band.hip, eigh2_chase.hip): C dim x dim host matrix
 * (row-major, symmetric).  stage 0: everything -- lam (nq x dim, ascending), Z (nq x dim x dim, column j = eigenvector j;
 * may be NULL); stage 1: the dense -> band reduction only (band_out: dim x dim, its lower triangle holds Q1' C Q1);
 * stage 2: ... and the chase of every scaled band (d_out / e_out: nq x dim diagonals and sub-diagonals). */
int crm_test_eigh2(crm_ctx* ctx, int nq, int dim, const double* C, const double* wa, const double* wb, double* lam, double* Z,
                   int stage, double* d_out, double* e_out, double* band_out);

/* Host-only (no GPU needed): the deflation plan of one divide-and-conquer merge of the eigen-solver -- eigenvalues
 * lam[n] of the two halves (n1 + n2), z[n] = last / first components of their eigenvectors, coupling beta.  Returns
 * k surviving poles, the rho of the normalised secular problem, rows[n] (local source rows: k survivors in pole order,
 * then the deflated ones), dl / w (poles and normalised update vector for the first k; deflated eigenvalues behind),
 * and the Givens rotations (a, b, c, s) x nrot that were applied. */
int crm_test_dc_plan(const double* lam, const double* z, int n1, int n, double beta, int* k, double* rho, int* rows,
                     double* dl, double* w, int* nrot, double* rots);

/* Host-only: the task table of the back-transformation through the chase's reflectors (cellregmap_amd/csrc/eigh2_back.hip)
 * for `batch` matrices of order `dim` on a device of `cus` compute units: count triples (matrix, first tile of sixteen
 * eigenvectors, tiles <= 8) in launch order.  CRM_ERR_ARG when capacity (ints) is too small; *count is set either way. */
int crm_test_back_tasks(int batch, long dim, int cus, int* tasks, int capacity, int* count);

#ifdef __cplusplus
}
#endif
#endif /* CRM_HIP_TEST_H */
