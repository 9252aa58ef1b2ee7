// The fixed-effect GxC tests of several phenotypes against one panel in one pass (C-ABI crm_scan_interaction_contexts_multi,
// crm_scan_interaction_contexts_joint_multi).  The single-gene entries and their body
// (context_host.hip: scan_contexts) stay as they are; this is the same sequence with what does not depend on the phenotype
// taken once:
//   per call             the context operand tables C, C^2 and (joint) C_i o C_j; the phenotype matrix [X0 | y_1 .. y_P]
//   per block            the gathered / expanded block, (g o g), the plain products against C^2, C and the pair table,
//                        g'g and g'X0 -- the launches of scan_contexts, with the same arguments
//   per distinct rho*    T_g = Q0(rho*)'g and, per sub-range, ONE Khatri-Rao contraction T_x = Q0(rho*)'(g o C_j), read by every
//                        gene whose null sits on that grid point (the large launch of section 12)
//   per gene             g'y_i and x_j'y_i as products against the phenotype matrix (one launch each for all genes: g'y_i one
//                        thread per (gene, variant) over the cells in order, x_j'y_i the Khatri-Rao contraction),
//                        delta_i (full refit: the gene's own alt fits on the shared T_g), and its column of the test
//                        launch, whose grid is (variant, gene of the rho group)
// The nulls are not fitted here: they arrive as the rows of crm_association_null_multi, as crm_scan_association_multi takes
// them -- a context gene's null is crm_scan_association's null of that gene.
// Every cell-axis sum runs unsplit, one accumulator per output element over the cells in order, so a gene's numbers do not
// depend on the other genes of the call, on their order, or on where a variant sits in a block, sub-range or panel.
#include "lrt_scan.h"

using namespace crm;

namespace {

constexpr size_t SCRATCH_BUDGET = (size_t)1 << 30;   // phi rows (and V rows) of the genes of one test launch

struct ContextMultiOut {
    double* pvalue; double* alt_lml; double* beta; double* beta_se; double* logp;
    int* status;
    double* null_lml; double* null_delta;
    bool joint; int* dof; int* dropped;
};

// gy[q, b] = sum_i G[i, b] Y[i, q]: g'y of every (gene, variant), one thread each, the cells in order in one accumulator --
// the statement of variant_stats_general_kernel (blockops.hip), which serves the single-gene entries from nine covariate
// columns on, so that a gene's g'y, and with it the delta_i of its refits, is that entry's bit for bit at any number of genes
__global__ __launch_bounds__(64) void phenotype_products_kernel(const double* __restrict__ G, long ldg, long cells, int variants,
                                                                const double* __restrict__ Y, long ldy, double* __restrict__ gy,
                                                                long ld_gy) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int q = blockIdx.y;
    if (b >= variants) return;
    const double* col = Y + q;
    double acc = 0.0;
    for (long i = 0; i < cells; i++) acc += G[i * ldg + b] * col[i * ldy];
    gy[(long)q * ld_gy + b] = acc;
}

// One call of crm_scan_interaction_contexts(_joint)_multi: what is fixed once the checks have passed, one function per stage.
struct ContextMultiScan {
    LrtBlock B;
    ContextTables X;
    crm_gene* const* genes; const int ngenes; const double* null;
    const NullRows& R;
    const ContextMultiOut& out;
    crm_background* bg; crm_ctx* ctx; hipStream_t st;
    const int BLK, c, k, SUB, ngrp;
    const bool fast, joint;
    const long n, np, ldq, ldb, ldT, ldcy;
    const size_t tests, tslab, rec_bytes;
    PhenotypeMatrix Y;
    long ld_p;
    size_t per_gene;   // bytes of a gene's phi rows (and V rows) in a test launch
    int GCH;           // genes per test launch: their scratch stays within the budget
    double *d_gy = nullptr, *d_gW1 = nullptr;   // g'y_i: [ngenes x ldcy]; d_gW1: written beside it where variant_stats_kernel serves, not read
    NullFitTrial* d_trial = nullptr; NullFitOut* d_fit = nullptr; char* d_rec = nullptr;
    double *d_xXy = nullptr, *d_delta = nullptr, *d_nlml = nullptr, *d_res = nullptr;   // d_res: output q of gene i at (q ngenes + i) tests
    int *d_cdrop = nullptr, *d_status = nullptr, *d_dof = nullptr, *d_dropped = nullptr;
    double *d_phi = nullptr, *d_V = nullptr;   // gene slot s of a launch: rows s SUB .. of ldq / of v_slab
    GemmProblem* d_probs = nullptr; double* Tb = nullptr;
    std::vector<NullFitArgs> fa;
    std::vector<ContextLrtArgs> rec_l;     // (host sources of asynchronous copies: alive until the sync
    std::vector<ContextJointArgs> rec_j;   //  that ends a sub-range)
    std::vector<GemmProblem> pr, pt;

    ContextMultiScan(crm_gene* const* genes_, int ngenes_, crm_panel* panel, long first, long count, int fast_, const double* null_,
                     const NullRows& R_, const ContextMultiOut& out_)
        : B(genes_[0], panel, first, count, fast_), X(B, genes_[0]->k0, out_.joint), genes(genes_), ngenes(ngenes_), null(null_), R(R_),
          out(out_), bg(B.bg), ctx(B.ctx), st(B.st), BLK(B.BLK), c(B.c), k(X.k), SUB(X.SUB), ngrp(R_.ngrp()), fast(B.fast),
          joint(X.joint), n(B.n), np(B.np), ldq(B.ldq), ldb(B.ldb), ldT(B.ldq), ldcy(B.ldb), tests(X.tests),
          tslab((size_t)B.BLK * B.ldq), rec_bytes(out_.joint ? sizeof(ContextJointArgs) : sizeof(ContextLrtArgs)), fa(ngenes_),
          rec_l(out_.joint ? 0 : ngenes_), rec_j(out_.joint ? ngenes_ : 0), pr(CONTEXT_SLOTS), pt(ngrp) {
        Y.plan(genes, ngenes);
        ld_p = round_up(Y.ncol, 8);
        per_gene = sizeof(double) * (size_t)SUB * (size_t)(ldq + (X.v_global ? X.v_slab : 0));
        GCH = (int)std::min<size_t>((size_t)ngenes, std::max<size_t>(SCRATCH_BUDGET / per_gene, 1));
    }

    int workspaces() {
        CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)ngrp * tslab));
        CRM_TRY(B.ensure());
        CRM_TRY(X.ensure(B));
        CRM_TRY(Y.ensure(ctx, np));
        CRM_TRY(ctx->ws_F.ensure((size_t)GCH * per_gene));
        CRM_TRY(carve_workspace(ctx->ws_small, [&](auto& take) {
            B.carve(take, !fast);   // (d_gy: the first gene's y rides along in the block's preparation; its g'y is not read)
            take(d_gW1, sizeof(double) * BLK * B.ld_gW), take(d_gy, sizeof(double) * (size_t)ngenes * ldcy);
            take(d_trial, !fast ? sizeof(NullFitTrial) * BLK : 0), take(d_fit, !fast ? sizeof(NullFitOut) * BLK : 0);
            take(Y.d_srcs, Y.srcs_bytes()), take(d_rec, rec_bytes * ngenes);
        }));
        // shared plain tables, then per gene: delta, drop and the null lml of the block, the results of a sub-range
        CRM_TRY(carve_workspace(ctx->ws_ctxP, [&](auto& take) {
            take(d_xXy, sizeof(double) * tests * ld_p), take(X.d_xx, sizeof(double) * BLK * X.ld_k);
            take(X.d_xg, sizeof(double) * BLK * X.ld_k), take(X.d_xxp, sizeof(double) * (size_t)BLK * X.ld_pp);
            take(d_delta, sizeof(double) * (size_t)ngenes * BLK), take(d_cdrop, sizeof(int) * (size_t)ngenes * BLK);
            take(d_nlml, sizeof(double) * (size_t)ngenes * BLK), take(d_res, sizeof(double) * 5 * tests * ngenes);
            take(d_status, sizeof(int) * tests * ngenes), take(d_dof, joint ? sizeof(int) * (size_t)SUB * ngenes : 0);
            take(d_dropped, joint ? sizeof(int) * tests * ngenes : 0);
        }));
        d_phi = ctx->ws_F.as<double>();
        d_V = d_phi + (size_t)GCH * SUB * ldq;
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + CONTEXT_SLOTS)));
        d_probs = ctx->ws_probs.as<GemmProblem>();
        Tb = ctx->ws_T.as<double>();
        return CRM_OK;
    }

    // the phenotype matrix, the context tables, and per gene what its records and its alt fits take from the gene and its null row
    int operands() {
        CRM_TRY(Y.clear(st, np));
        CRM_TRY(Y.fill(st, np));
        CRM_TRY(X.operands(B));
        for (int i = 0; i < ngenes; i++) nullfit_gene_args(fa[i], genes[i], 0);
        if (!fast && c > CRM_MAX_COV_WIDE) CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(BLK, B.nrho, c)));
        if (fast)   // delta_i = the gene's delta0 on every variant
            for (int i = 0; i < ngenes; i++)
                CRM_TRY(launch_context_deltas(st, nullptr, nullptr, null[6 * (size_t)i + 5], BLK, d_delta + (size_t)i * BLK,
                                              d_cdrop + (size_t)i * BLK));
        return CRM_OK;
    }

    // the block's products against the context tables; g'y_i of every gene; T_g per distinct rho*
    int block_products(int nb) {
        CRM_TRY(X.block_products(B, nb, pr.data()));
        CRM_HIP(hipMemcpyAsync(d_probs + 1, pr.data() + 1, sizeof(GemmProblem) * 5, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 1, 2, nb, k, np, false, 0, 1, 0));
        if (joint) CRM_TRY(launch_gemm_tn(ctx, d_probs + 5, 1, nb, X.npair, np, false, 0, 1, 0));
        // g'y_i in the order of the sums of the single-gene entry's own launch_variant_stats (the delta_i of a refit follows
        // g'y to the search's tolerance, not to rounding): from nine covariate columns on that is one thread per (variant,
        // column) over the cells in order -- here one launch against the phenotype matrix [y_1 .. y_P]; up to eight columns
        // it is the split sum of variant_stats_kernel, whose y column does not depend on the column count -- here that kernel
        // per gene, with one covariate column riding along (its g'g and g'X0_1 land in scratch)
        if (c > CRM_MAX_COV) {
            hipLaunchKernelGGL(phenotype_products_kernel, dim3((unsigned)((nb + 63) / 64), (unsigned)ngenes), dim3(64), 0, st, B.Gx,
                               ldb, np, nb, Y.XY + Y.yoff, Y.ldxy, d_gy, ldcy);
            CRM_HIP(hipGetLastError());
        } else {
            for (int i = 0; i < ngenes; i++)
                CRM_TRY(launch_variant_stats(st, B.Gx, ldb, np, nb, genes[i]->yW.as<double>(), B.g0->yW.as<double>() + 1,
                                             genes[i]->ld_yw, 1, B.d_part, B.d_gy, d_gy + (size_t)i * ldcy, d_gW1, B.ld_gW));
        }
        for (int q = 0; q < ngrp; q++) pt[q] = B.rotation(R.grp_rho[q], nb, Tb + (size_t)q * tslab, ldT);
        CRM_HIP(hipMemcpyAsync(d_probs + CONTEXT_SLOTS, pt.data(), sizeof(GemmProblem) * ngrp, hipMemcpyHostToDevice, st));
        for (int q = 0; q < ngrp; q++) CRM_TRY(launch_gemm_tn(ctx, d_probs + CONTEXT_SLOTS + q, 1, nb, (int)ldq, np, false, 0, 1, 0));
        return CRM_OK;
    }

    // delta_i of every gene on the block's variants (fast: set once per call, in operands)
    int block_deltas(long done, int nb) {
        if (!fast) CRM_TRY(refit_deltas(nb));
        return copy_rows(out.null_delta, done, 1, nb, d_delta, BLK);
    }
    // full refit: LMM(y_i, [X0, g]) per variant at the gene's rho*, on the group's T_g
    int refit_deltas(int nb) {
        for (int i = 0; i < ngenes; i++) {
            NullFitArgs alt = fa[i];
            alt.nrho = 1;
            alt.rho[0] = fa[i].rho[R.ri[i]];
            alt.rho[0].T = Tb + (size_t)R.grp_of_rho[R.ri[i]] * tslab;
            alt.rho[0].ldT = ldT;
            alt.gg = B.d_gg; alt.gy = d_gy + (size_t)i * ldcy; alt.gW = B.d_gW; alt.ld_gW = B.ld_gW;
            alt.trial = d_trial; alt.out = d_fit; alt.g_drop = B.d_drop;
            alt.xwide = c > CRM_MAX_COV_WIDE ? ctx->ws_xwide.as<double>() : nullptr;
            CRM_TRY(launch_nullfit(st, alt, nb));
            CRM_TRY(launch_context_deltas(st, d_trial, B.d_drop, null[6 * (size_t)i + 5], nb, d_delta + (size_t)i * BLK,
                                          d_cdrop + (size_t)i * BLK));
        }
        return CRM_OK;
    }

    // the record of gene i in slot s of a test launch of rho group q, variants [b0, ..) of the block
    ContextLrtArgs record(int q, int i, int s, int b0) const {
        const int gi = R.grp_rho[q];
        ContextLrtArgs a{};
        a.Tx = ctx->ws_A.as<double>(); a.tx_slab = (long)k * ldq; a.ldT = ldq;
        a.Tg = Tb + (size_t)q * tslab + (size_t)b0 * ldT; a.ldTg = ldT;
        a.tX = fa[i].rho[gi].tW; a.ldW = ldq; a.ty = fa[i].rho[gi].ty; a.S0 = fa[i].rho[gi].S0;
        a.r = bg->r[gi]; a.c = c; a.k = k; a.n = n;
        a.WW = fa[i].WW; a.Wy = fa[i].Wy; a.yy = fa[i].yy;
        a.gg = B.d_gg + b0; a.gy = d_gy + (size_t)i * ldcy + b0; a.gW = B.d_gW + (size_t)b0 * B.ld_gW; a.ld_gW = B.ld_gW;
        a.xXy = d_xXy; a.ld_xXy = ld_p; a.xy = d_xXy + Y.yoff + i; a.ld_xy = ld_p;
        a.xx = X.d_xx + (size_t)b0 * X.ld_k; a.ld_xx = X.ld_k; a.xg = X.d_xg + (size_t)b0 * X.ld_k; a.ld_xg = X.ld_k;
        a.delta = d_delta + (size_t)i * BLK + b0; a.drop = d_cdrop + (size_t)i * BLK + b0;
        a.phi = d_phi + (size_t)s * SUB * ldq; a.ld_phi = ldq;
        a.pvalue = d_res + (size_t)(0 * ngenes + i) * tests; a.alt_lml = d_res + (size_t)(1 * ngenes + i) * tests;
        a.beta = d_res + (size_t)(2 * ngenes + i) * tests; a.beta_se = d_res + (size_t)(3 * ngenes + i) * tests;
        a.logp = d_res + (size_t)(4 * ngenes + i) * tests; a.status = d_status + (size_t)i * tests;
        a.null_lml = d_nlml + (size_t)i * BLK + b0;
        return a;
    }

    // variants [b0, b0 + ns) of the block: x_j'[X0 | y_1 .. y_P] for all genes in one Khatri-Rao contraction against the
    // phenotype matrix; per rho group T_x = Q0(rho*)'(g o C_j), shared by its genes, and their tests, GCH genes to a launch
    // of grid (variant, gene)
    int sub_range_tests(int b0, int ns) {
        const GemmProblem& pb = pr[4] = X.khatri_rao(B, b0, ns, Y.XY, Y.ldxy, (int)Y.ncol, d_xXy, ld_p);
        CRM_HIP(hipMemcpyAsync(d_probs + 4, &pb, sizeof(GemmProblem), hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 4, 1, pb.M, pb.N, np, true, k, 1, 0));
        for (int q = 0; q < ngrp; q++) {
            const int gi = R.grp_rho[q], r = bg->r[gi];
            const GemmProblem& pa = pr[3] = X.khatri_rao(B, b0, ns, bg->Q0[gi].as<double>(), ldq, r > 0 ? r : 1, ctx->ws_A.as<double>(), ldq);
            CRM_HIP(hipMemcpyAsync(d_probs + 3, &pa, sizeof(GemmProblem), hipMemcpyHostToDevice, st));
            CRM_TRY(X.launch_rotated(B, d_probs + 3, pa, r, ns));
            const std::vector<int>& mem = R.members[q];
            for (size_t m0 = 0; m0 < mem.size(); m0 += GCH) {
                const int ng = (int)std::min<size_t>(GCH, mem.size() - m0);
                for (int s = 0; s < ng; s++) {
                    const int i = mem[m0 + s];
                    const ContextLrtArgs a = record(q, i, s, b0);
                    if (!joint) { rec_l[m0 + s] = a; continue; }
                    ContextJointArgs& j = rec_j[m0 + s];
                    j = ContextJointArgs{};
                    j.base = a;
                    j.xxp = X.d_xxp + (size_t)b0 * X.ld_pp; j.ld_xxp = X.ld_pp;
                    j.V = X.v_global ? d_V + (size_t)s * SUB * X.v_slab : nullptr; j.v_slab = X.v_slab;
                    j.v_in_lds = X.v_global ? 0 : 1;
                    j.dof = d_dof + (size_t)i * SUB; j.dropped = d_dropped + (size_t)i * tests;
                }
                // (the records of the launches of this sub-range sit side by side: slot m0 of the group's stretch)
                char* d_r = d_rec + rec_bytes * m0;
                if (joint) {
                    CRM_HIP(hipMemcpyAsync(d_r, rec_j.data() + m0, rec_bytes * ng, hipMemcpyHostToDevice, st));
                    CRM_TRY(launch_context_joint_multi(st, (const ContextJointArgs*)d_r, ng, c, k, X.v_global, ns));
                } else {
                    CRM_HIP(hipMemcpyAsync(d_r, rec_l.data() + m0, rec_bytes * ng, hipMemcpyHostToDevice, st));
                    CRM_TRY(launch_context_lrt_multi(st, (const ContextLrtArgs*)d_r, ng, c, k, ns));
                }
            }
            CRM_HIP(hipStreamSynchronize(st));   // (the next group writes T_x and the records anew)
        }
        return CRM_OK;
    }

    // rows of `width` values per variant, gene-major on the host: `cnt` variants from variant `at` of row i of
    // [ngenes x count x width], from device rows `d_pitch` values apart
    template <class T>
    int copy_rows(T* dst, long at, int width, int cnt, const T* d_rows, size_t d_pitch) {
        if (dst)
            CRM_HIP(hipMemcpy2DAsync(dst + (size_t)at * width, sizeof(T) * (size_t)B.count * width, d_rows, sizeof(T) * d_pitch,
                                     sizeof(T) * (size_t)cnt * width, ngenes, hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }

    int copy_sub_range(long at, int ns) {
        double* const outs[5] = {out.pvalue, out.alt_lml, out.beta, out.beta_se, out.logp};
        for (int q = 0; q < 5; q++)   // joint: only beta and beta_se are per variant and context
            CRM_TRY(copy_rows(outs[q], at, !joint || q == 2 || q == 3 ? k : 1, ns, d_res + (size_t)q * ngenes * tests, tests));
        CRM_TRY(copy_rows(out.status, at, joint ? 1 : k, ns, d_status, tests));
        if (joint) CRM_TRY(copy_rows(out.dof, at, 1, ns, d_dof, (size_t)SUB));
        if (joint) CRM_TRY(copy_rows(out.dropped, at, k, ns, d_dropped, tests));
        return CRM_OK;
    }
};

int scan_contexts_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, int fast,
                        const double* null, const ContextMultiOut& out) {
    const char* what = out.joint ? "joint context tests (multi)" : "context tests (multi)";
    CRM_TRY(check_shared_genes(what, genes, ngenes, true));
    if (!panel || !null) {
        set_error("%s: %s is NULL", what, panel ? "null" : "panel");
        return CRM_ERR_ARG;
    }
    crm_background* bg = genes[0]->bg;
    CRM_TRY(check_panel_range(what, bg, panel, first, count));
    NullRows R;
    CRM_TRY(R.read(what, bg, null, ngenes, fast != 0));
    CRM_TRY(ContextTables::check(what, genes[0]->c, genes[0]->k0, false));
    if (ngenes > 65535) {
        set_error("%s: %d genes in one call (supported up to 65535)", what, ngenes);
        return CRM_ERR_UNSUPPORTED;
    }
    if (out.joint) CRM_TRY(context_joint_check(genes[0]->c, genes[0]->k0));
    InScan in_scan;
    CRM_TRY(in_scan.enter(bg->ctx, what));
    if (count == 0) return CRM_OK;
    CRM_HIP(hipSetDevice(bg->ctx->device));
    CRM_TRY(R.group(bg));
    ContextMultiScan S(genes, ngenes, panel, first, count, fast, null, R, out);
    CRM_TRY(S.workspaces());
    CRM_TRY(S.operands());
    for (long done = 0; done < count; done += S.BLK) {
        const int nb = S.B.nb_at(done);
        CRM_TRY(S.B.prepare(done, nb, S.c));
        CRM_TRY(S.block_products(nb));
        CRM_TRY(S.block_deltas(done, nb));
        for (int b0 = 0; b0 < nb; b0 += S.SUB) {
            const int ns = std::min(S.SUB, nb - b0);
            CRM_TRY(S.sub_range_tests(b0, ns));
            CRM_TRY(S.copy_sub_range(done + b0, ns));
            CRM_HIP(hipStreamSynchronize(S.st));   // (the next sub-range writes the same buffers)
        }
        CRM_TRY(S.copy_rows(out.null_lml, done, 1, nb, S.d_nlml, (size_t)S.BLK));
        CRM_HIP(hipStreamSynchronize(S.st));
        S.ctx->report(done + nb, count);
    }
    return CRM_OK;
}

}  // namespace

extern "C" int crm_scan_interaction_contexts_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                                                   int fast, const double* null, double* out_pvalue, double* out_alt_lml,
                                                   double* out_beta, double* out_beta_se, double* out_logp, int* out_status,
                                                   double* out_null_lml, double* out_null_delta) {
    return crm::guarded_on("crm_scan_interaction_contexts_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr,
                           [&]() -> int {
    const ContextMultiOut out{out_pvalue, out_alt_lml, out_beta, out_beta_se, out_logp, out_status, out_null_lml, out_null_delta,
                              false, nullptr, nullptr};
    return scan_contexts_multi(genes, ngenes, panel, first, count, fast, null, out);
    });
}

extern "C" int crm_scan_interaction_contexts_joint_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first,
                                                         long count, int fast, const double* null, double* out_pvalue,
                                                         double* out_logp, double* out_alt_lml, int* out_dof, double* out_beta,
                                                         double* out_beta_se, int* out_dropped, int* out_status,
                                                         double* out_null_lml, double* out_null_delta) {
    return crm::guarded_on("crm_scan_interaction_contexts_joint_multi",
                           (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    const ContextMultiOut out{out_pvalue, out_alt_lml, out_beta, out_beta_se, out_logp, out_status, out_null_lml, out_null_delta,
                              true, out_dof, out_dropped};
    return scan_contexts_multi(genes, ngenes, panel, first, count, fast, null, out);
    });
}
