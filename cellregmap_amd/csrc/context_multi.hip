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
#include <algorithm>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace {

constexpr size_t CONTEXT_BUDGET = (size_t)8 << 30;   // T_x of one rho group and sub-range (scan_contexts' own)
constexpr size_t SCRATCH_BUDGET = (size_t)1 << 30;   // phi rows (and V rows) of the genes of one test launch

struct ContextMultiOut {
    double* pvalue; double* alt_lml; double* beta; double* beta_se; double* logp;
    int* status;
    double* null_lml; double* null_delta;
    bool joint; int* dof; int* dropped;
};

// XY[i, dst] = src[i * ld] for the columns of [X0 | y_1 .. y_P] (cells_pad rows: the sources are zero padded)
struct ColumnSource {
    const double* src;
    long ld;
    long dst;
};
__global__ __launch_bounds__(256) void context_columns_kernel(const ColumnSource* __restrict__ cols, long rows, double* __restrict__ XY,
                                                              long ldxy) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const ColumnSource s = cols[blockIdx.y];
    XY[i * ldxy + s.dst] = s.src[i * s.ld];
}

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

int check_context_genes(crm_gene* const* genes, int ngenes, const char* what) {
    if (!genes || ngenes <= 0) {
        set_error("%s: no genes", what);
        return CRM_ERR_ARG;
    }
    for (int i = 0; i < ngenes; i++)
        if (!genes[i] || !genes[i]->bg) {
            set_error("%s: gene %d is NULL", what, i);
            return CRM_ERR_ARG;
        }
    const crm_gene* g0 = genes[0];
    for (int i = 1; i < ngenes; i++) {
        const crm_gene* g = genes[i];
        // the shared pass takes g'X0, the orthogonalisation and the context tables from the first gene
        if (g->bg != g0->bg || g->ctx != g0->ctx) {
            set_error("%s: genes of one call must share the background (gene %d differs from gene 0)", what, i);
            return CRM_ERR_ARG;
        }
        if (g->k0 != g0->k0 || g->e0_key != g0->e0_key) {
            set_error("%s: genes of one call must hold the same contexts C (gene %d differs from gene 0)", what, i);
            return CRM_ERR_ARG;
        }
        if (g->c != g0->c || g->w_key != g0->w_key) {
            set_error("%s: genes of one call must hold the same covariates X0 (gene %d differs from gene 0)", what, i);
            return CRM_ERR_ARG;
        }
    }
    return CRM_OK;
}

int scan_contexts_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, int fast,
                        const double* null, const ContextMultiOut& out) {
    const char* what = out.joint ? "joint context tests (multi)" : "context tests (multi)";
    CRM_TRY(check_context_genes(genes, ngenes, what));
    if (!panel || !null) {
        set_error("%s: %s is NULL", what, panel ? "null" : "panel");
        return CRM_ERR_ARG;
    }
    crm_gene* g0 = genes[0];
    crm_background* bg = g0->bg;
    crm_ctx* ctx = bg->ctx;
    if (panel->ctx != ctx || panel->n != bg->n) {
        set_error("%s: genes and panel do not match (context / cell count)", what);
        return CRM_ERR_ARG;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("%s: variants [%ld, %ld) outside the panel (p = %ld)", what, first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    const int nrho = bg->nrho;
    std::vector<int> ri(ngenes);
    for (int i = 0; i < ngenes; i++) {
        const double* row = null + 6 * (size_t)i;
        ri[i] = -1;
        for (int q = 0; q < nrho; q++)
            if (bg->rho[q] == row[0]) { ri[i] = q; break; }
        if (ri[i] < 0) {
            set_error("%s: null row %d has rho1 = %.17g, not a point of the background's grid", what, i, row[0]);
            return CRM_ERR_ARG;
        }
        if (!std::isfinite(row[4])) {
            set_error("%s: null row %d has a non-finite lml (the null model could not be fitted)", what, i);
            return CRM_ERR_ARG;
        }
        if (fast && !(row[5] > 0.0 && row[5] <= 1.0)) {
            set_error("%s: null row %d has delta = %g outside (0, 1]", what, i, row[5]);
            return CRM_ERR_ARG;
        }
    }
    const int c = g0->c, k = g0->k0;
    if (k < 1 || k > CRM_MAX_K0) {
        set_error("%s: %d contexts (supported 1..%d)", what, k, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    if (c < 1 || c > CRM_MAX_COV_XWIDE) {
        set_error("%s: the covariates and contexts span %d columns (supported 1..%d)", what, c, CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    if (ngenes > 65535) {
        set_error("%s: %d genes in one call (supported up to 65535)", what, ngenes);
        return CRM_ERR_UNSUPPORTED;
    }
    if (out.joint) CRM_TRY(context_joint_check(c, k));
    if (ctx->in_scan) {
        set_error("%s: another scan is running on this context (started from a progress callback?)", what);
        return CRM_ERR_UNSUPPORTED;
    }
    if (count == 0) return CRM_OK;
    struct InScan { crm_ctx* c; explicit InScan(crm_ctx* c_) : c(c_) { c->in_scan = true; } ~InScan() { c->in_scan = false; } } in_scan(ctx);
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    const int BLK = (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : CRM_DEFAULT_BLOCK,
                                        round_up(std::max<long>(count, 1), 128));
    const long ldb = BLK + 128, ldT = ldq;
    const long ld_gW = round_up(c, 8), ld_k = round_up(k, 8), ld_cq = round_up(k, 128);
    const bool joint = out.joint;
    const int npair = k * (k + 1) / 2;
    const long ld_pp = joint ? round_up(npair, 128) : 0;
    const bool v_global = joint && !context_joint_v_in_lds(c, k);
    const long v_slab = (long)(c + 1) * k;
    // variants per sub-range: the rotated candidates of ONE rho group stay within the budget (scan_contexts' rule)
    const size_t budget = ctx->context_budget > 0 ? ctx->context_budget : CONTEXT_BUDGET;
    const int SUB = (int)std::min<size_t>((size_t)BLK, std::max<size_t>(budget / (sizeof(double) * (size_t)k * ldq), 1));
    // genes per test launch: their phi rows (and V rows) stay within the scratch budget
    const size_t per_gene = sizeof(double) * (size_t)SUB * (size_t)(ldq + (v_global ? v_slab : 0));
    const int GCH = (int)std::min<size_t>((size_t)ngenes, std::max<size_t>(SCRATCH_BUDGET / per_gene, 1));

    // rho groups: the distinct grid indices of the genes' nulls in grid order, and their genes in the order given
    std::vector<int> grp_of_rho(nrho, -1), grp_rho;
    for (int i = 0; i < ngenes; i++) grp_of_rho[ri[i]] = 0;
    for (int q = 0; q < nrho; q++)
        if (grp_of_rho[q] == 0) { grp_of_rho[q] = (int)grp_rho.size(); grp_rho.push_back(q); }
    const int ngrp = (int)grp_rho.size();
    std::vector<std::vector<int>> members(ngrp);
    for (int i = 0; i < ngenes; i++) members[grp_of_rho[ri[i]]].push_back(i);
    for (int q : grp_rho) CRM_TRY(crm_background_require_q0(bg, q));

    // [X0 | y_1 .. y_P] (cells x ldxy): X0 at columns 0 .. c - 1, the phenotypes from column yoff
    const long yoff = round_up(c, 16);
    const long ncol = yoff + ngenes;
    const long ldxy = round_up(ncol, 128) + 128;   // (column tiles read from column 0 or from yoff stay inside a row)
    const long ld_p = round_up(ncol, 8);
    const long ldcy = ldb;

    const size_t tslab = (size_t)BLK * ldT;
    CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)ngrp * tslab));
    CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
    CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)np * ldb));
    if (!fast) {
        CRM_TRY(ctx->ws_Gx.ensure(sizeof(double) * (size_t)np * ldb));
        CRM_TRY(ctx->ws_GG.ensure(sizeof(double) * (size_t)np * ldb));
    }
    CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)SUB * k * ldq));
    CRM_TRY(ctx->ws_ctxE.ensure(sizeof(double) * (size_t)np * (2 * ld_cq + ld_pp)));
    CRM_TRY(ctx->ws_XG.ensure(sizeof(double) * (size_t)np * ldxy));
    CRM_TRY(ctx->ws_F.ensure((size_t)GCH * per_gene));
    std::vector<ColumnSource> srcs;
    for (int u = 0; u < c; u++) srcs.push_back({g0->yW.as<double>() + 1 + u, g0->ld_yw, u});
    for (int i = 0; i < ngenes; i++) srcs.push_back({genes[i]->yW.as<double>(), genes[i]->ld_yw, yoff + i});
    const size_t tests = (size_t)SUB * k;
    const size_t rec_bytes = joint ? sizeof(ContextJointArgs) : sizeof(ContextLrtArgs);

    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_gg = carve(sizeof(double) * BLK), o_gy0 = carve(sizeof(double) * BLK),
                 o_gW = carve(sizeof(double) * BLK * ld_gW), o_gW1 = carve(sizeof(double) * BLK * ld_gW), o_gy = carve(sizeof(double) * (size_t)ngenes * ldcy),
                 o_trial = carve(!fast ? sizeof(NullFitTrial) * BLK : 0), o_fit = carve(!fast ? sizeof(NullFitOut) * BLK : 0),
                 o_part = carve(variant_stats_workspace(BLK, std::min(c, CRM_MAX_COV))),
                 o_coef = carve(!fast ? sizeof(double) * (size_t)c * ldb : 0), o_thr = carve(!fast ? sizeof(double) * BLK : 0),
                 o_drop = carve(!fast ? sizeof(int) * BLK : 0), o_src = carve(sizeof(ColumnSource) * srcs.size()),
                 o_rec = carve(rec_bytes * ngenes);
    CRM_TRY(ctx->ws_small.ensure(off));
    char* sm = ctx->ws_small.as<char>();
    double* d_gg = (double*)(sm + o_gg);
    double* d_gy0 = (double*)(sm + o_gy0);
    double* d_gW = (double*)(sm + o_gW);
    double* d_gy = (double*)(sm + o_gy);
    double* d_gW1 = (double*)(sm + o_gW1);   // (written beside a gene's g'y where variant_stats_kernel serves; not read)
    NullFitTrial* d_trial = (NullFitTrial*)(sm + o_trial);
    NullFitOut* d_fit = (NullFitOut*)(sm + o_fit);
    double* d_part = (double*)(sm + o_part);
    double* d_coef = (double*)(sm + o_coef);
    double* d_thr = (double*)(sm + o_thr);
    int* d_drop = (int*)(sm + o_drop);
    off = 0;
    // shared plain tables, then per gene: delta, drop and the null lml of the block, the results of a sub-range
    const size_t o_xXy = carve(sizeof(double) * tests * ld_p), o_xx = carve(sizeof(double) * BLK * ld_k),
                 o_xg = carve(sizeof(double) * BLK * ld_k), o_xxp = carve(sizeof(double) * (size_t)BLK * ld_pp),
                 o_delta = carve(sizeof(double) * (size_t)ngenes * BLK), o_cdrop = carve(sizeof(int) * (size_t)ngenes * BLK),
                 o_nlml = carve(sizeof(double) * (size_t)ngenes * BLK), o_res = carve(sizeof(double) * 5 * tests * ngenes),
                 o_status = carve(sizeof(int) * tests * ngenes), o_dof = carve(joint ? sizeof(int) * (size_t)SUB * ngenes : 0),
                 o_dropped = carve(joint ? sizeof(int) * tests * ngenes : 0);
    CRM_TRY(ctx->ws_ctxP.ensure(off));
    char* cp = ctx->ws_ctxP.as<char>();
    double* d_xXy = (double*)(cp + o_xXy);
    double* d_xx = (double*)(cp + o_xx);
    double* d_xg = (double*)(cp + o_xg);
    double* d_xxp = (double*)(cp + o_xxp);
    double* d_delta = (double*)(cp + o_delta);
    int* d_cdrop = (int*)(cp + o_cdrop);
    double* d_nlml = (double*)(cp + o_nlml);
    double* d_res = (double*)(cp + o_res);      // output q of gene i: d_res + (q ngenes + i) tests
    int* d_status = (int*)(cp + o_status);
    int* d_dof = (int*)(cp + o_dof);
    int* d_dropped = (int*)(cp + o_dropped);
    double* d_phi = ctx->ws_F.as<double>();     // gene slot s of a launch: rows s SUB .. of ldq
    double* d_V = d_phi + (size_t)GCH * SUB * ldq;
    constexpr int SLOTS = 8;   // 0 T_g, 1 / 2 the squared block's products, 3 / 4 the two Khatri-Rao contractions, 5 x_i'x_j
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + SLOTS)));
    GemmProblem* d_probs = ctx->ws_probs.as<GemmProblem>();
    const double* d_W = g0->yW.as<double>() + 1;

    // the phenotype matrix
    double* XY = ctx->ws_XG.as<double>();
    CRM_HIP(hipMemsetAsync(XY, 0, sizeof(double) * (size_t)np * ldxy, st));
    CRM_HIP(hipMemcpyAsync(sm + o_src, srcs.data(), sizeof(ColumnSource) * srcs.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(context_columns_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)srcs.size()), dim3(256), 0, st,
                       (const ColumnSource*)(sm + o_src), np, XY, ldxy);
    CRM_HIP(hipGetLastError());

    // the contexts as the Khatri-Rao operand (rows padded to whole 128-column tiles) and squared; joint: the pair products
    double* Cq = ctx->ws_ctxE.as<double>();
    double* C2 = Cq + (size_t)np * ld_cq;
    CRM_TRY(launch_context_operands(st, g0->E0.as<double>(), g0->lde, np, k, Cq, C2, ld_cq));
    double* CC = C2 + (size_t)np * ld_cq;
    if (joint) CRM_TRY(launch_context_pairs(st, g0->E0.as<double>(), g0->lde, np, k, CC, ld_pp));

    // per gene: what its records and its alt fits take from the gene and its null row
    std::vector<NullFitArgs> fa(ngenes);
    for (int i = 0; i < ngenes; i++) nullfit_gene_args(fa[i], genes[i], 0);
    if (!fast && c > CRM_MAX_COV_WIDE) CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(BLK, nrho, c)));
    if (fast)   // delta_i = the gene's delta0 on every variant
        for (int i = 0; i < ngenes; i++)
            CRM_TRY(launch_context_deltas(st, nullptr, nullptr, null[6 * (size_t)i + 5], BLK, d_delta + (size_t)i * BLK,
                                          d_cdrop + (size_t)i * BLK));

    std::vector<ContextLrtArgs> rec_l(joint ? 0 : ngenes);     // (host sources of asynchronous copies: alive until the sync
    std::vector<ContextJointArgs> rec_j(joint ? ngenes : 0);   //  that ends a sub-range)
    std::vector<GemmProblem> pr(SLOTS);
    double* Tb = ctx->ws_T.as<double>();
    for (long done = 0; done < count; done += BLK) {
        const int nb = (int)std::min<long>(BLK, count - done);
        double* Gb = ctx->ws_Gb.as<double>();   // the block as given: the candidates are g o C_j of these columns
        if (panel->grouped)
            CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + first + done, panel->ld, panel->group.as<int>(),
                                        np, n, nullptr, nb, Gb, ldb, (int)ldb));
        else
            CRM_TRY(launch_gather_block(st, panel->G.as<double>() + first + done, panel->ld, np, n, nullptr, nullptr,
                                        nb, Gb, ldb, (int)ldb));
        // g'g and g'X0 as scan_contexts takes them (the first gene's y rides along; its g'y is not read)
        CRM_TRY(launch_variant_stats(st, Gb, ldb, np, nb, g0->yW.as<double>(), d_W, g0->ld_yw, c, d_part, d_gg, d_gy0, d_gW, ld_gW));
        double* Gx = Gb;                        // the column that stands for g beside X0
        if (!fast) {
            Gx = ctx->ws_Gx.as<double>();
            CRM_TRY(launch_ortho_block(st, Gb, ldb, np, nb, (int)ldb, d_W, g0->ld_yw, c, g0->Wproj.as<double>(), d_gW, ld_gW,
                                       d_coef, ldb, d_thr, Gx, ldb));
            CRM_TRY(launch_variant_stats(st, Gx, ldb, np, nb, g0->yW.as<double>(), d_W, g0->ld_yw, c, d_part, d_gg, d_gy0, d_gW,
                                         ld_gW));
            CRM_TRY(launch_ortho_rank(st, d_gg, d_thr, nb, d_drop));
        }
        double* G2 = ctx->ws_G2.as<double>();
        double* GG = fast ? nullptr : ctx->ws_GG.as<double>();
        CRM_TRY(launch_square_block(st, Gb, Gx, ldb, ldb, np, (int)ldb, G2, GG, ldb));
        // x_j'x_j = (g o g)'C_j^2 and x_j'g = (g o gx)'C_j; joint: x_i'x_j = (g o g)'(C_i o C_j), i >= j
        GemmProblem& p2 = pr[1];
        p2 = GemmProblem{};
        p2.X = G2; p2.ldx = ldb; p2.Y = C2; p2.ldy = ld_cq; p2.C = d_xx; p2.ldc = ld_k; p2.M = nb; p2.N = k;
        GemmProblem& p3 = pr[2];
        p3 = p2;
        p3.X = GG ? GG : G2; p3.Y = Cq; p3.C = d_xg;
        GemmProblem& p5 = pr[5];
        p5 = p2;
        p5.Y = CC; p5.ldy = ld_pp; p5.C = d_xxp; p5.ldc = ld_pp; p5.N = npair;
        CRM_HIP(hipMemcpyAsync(d_probs + 1, pr.data() + 1, sizeof(GemmProblem) * 5, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 1, 2, nb, k, np, false, 0, 1, 0));
        if (joint) CRM_TRY(launch_gemm_tn(ctx, d_probs + 5, 1, nb, npair, np, false, 0, 1, 0));
        // g'y_i of every gene, in the order of the sums of the single-gene entry's own launch_variant_stats (the delta_i of a
        // refit follows g'y to the search's tolerance, not to rounding): from nine covariate columns on that is one thread per
        // (variant, column) over the cells in order -- here one launch against the phenotype matrix [y_1 .. y_P]; up to eight
        // columns it is the split sum of variant_stats_kernel, whose y column does not depend on the column count -- here that
        // kernel per gene, with one covariate column riding along (its g'g and g'X0_1 land in scratch)
        if (c > CRM_MAX_COV) {
            hipLaunchKernelGGL(phenotype_products_kernel, dim3((unsigned)((nb + 63) / 64), (unsigned)ngenes), dim3(64), 0, st, Gx,
                               ldb, np, nb, XY + yoff, ldxy, d_gy, ldcy);
            CRM_HIP(hipGetLastError());
        } else {
            for (int i = 0; i < ngenes; i++)
                CRM_TRY(launch_variant_stats(st, Gx, ldb, np, nb, genes[i]->yW.as<double>(), d_W, genes[i]->ld_yw, 1, d_part, d_gy0,
                                             d_gy + (size_t)i * ldcy, d_gW1, ld_gW));
        }
        // T_g = Q0(rho*)'gx per distinct rho*: scan_contexts' launch, once per group
        std::vector<GemmProblem> pt(ngrp);
        for (int q = 0; q < ngrp; q++) {
            const int r = bg->r[grp_rho[q]];
            pt[q] = GemmProblem{};
            pt[q].X = Gx; pt[q].ldx = ldb; pt[q].Y = bg->Q0[grp_rho[q]].as<double>(); pt[q].ldy = ldq;
            pt[q].C = Tb + (size_t)q * tslab; pt[q].ldc = ldT; pt[q].M = nb; pt[q].N = r > 0 ? r : 1;
        }
        CRM_HIP(hipMemcpyAsync(d_probs + SLOTS, pt.data(), sizeof(GemmProblem) * ngrp, hipMemcpyHostToDevice, st));
        for (int q = 0; q < ngrp; q++) CRM_TRY(launch_gemm_tn(ctx, d_probs + SLOTS + q, 1, nb, (int)ldq, np, false, 0, 1, 0));
        if (!fast) {
            // delta_i of every gene: LMM(y_i, [X0, g]) per variant at the gene's rho*, on the group's T_g
            for (int i = 0; i < ngenes; i++) {
                NullFitArgs alt = fa[i];
                alt.nrho = 1;
                alt.rho[0] = fa[i].rho[ri[i]];
                alt.rho[0].T = Tb + (size_t)grp_of_rho[ri[i]] * tslab;
                alt.rho[0].ldT = ldT;
                alt.gg = d_gg; alt.gy = d_gy + (size_t)i * ldcy; alt.gW = d_gW; alt.ld_gW = ld_gW;
                alt.trial = d_trial; alt.out = d_fit;
                alt.g_drop = d_drop;
                alt.xwide = c > CRM_MAX_COV_WIDE ? ctx->ws_xwide.as<double>() : nullptr;
                CRM_TRY(launch_nullfit(st, alt, nb));
                CRM_TRY(launch_context_deltas(st, d_trial, d_drop, null[6 * (size_t)i + 5], nb, d_delta + (size_t)i * BLK,
                                              d_cdrop + (size_t)i * BLK));
            }
        }
        if (out.null_delta)
            CRM_HIP(hipMemcpy2DAsync(out.null_delta + done, sizeof(double) * count, d_delta, sizeof(double) * BLK,
                                     sizeof(double) * nb, ngenes, hipMemcpyDeviceToHost, st));

        for (int b0 = 0; b0 < nb; b0 += SUB) {
            const int ns = std::min(SUB, nb - b0);
            // x_j'[X0 | y_1 .. y_P]: one Khatri-Rao contraction against the phenotype matrix for all genes
            GemmProblem& pb = pr[4];
            pb = GemmProblem{};
            pb.X = Gb + b0; pb.ldx = ldb; pb.E = Cq; pb.lde = ld_cq; pb.k0 = k;
            pb.Y = XY; pb.ldy = ldxy; pb.C = d_xXy; pb.ldc = ld_p; pb.M = ns * k; pb.N = (int)ncol;
            CRM_HIP(hipMemcpyAsync(d_probs + 4, &pb, sizeof(GemmProblem), hipMemcpyHostToDevice, st));
            CRM_TRY(launch_gemm_tn(ctx, d_probs + 4, 1, pb.M, pb.N, np, true, k, 1, 0));
            for (int q = 0; q < ngrp; q++) {
                const int gi = grp_rho[q], r = bg->r[gi];
                // T_x = Q0(rho*)'(g o C_j) of the sub-range, shared by the genes of the group
                GemmProblem& pa = pr[3];
                pa = pb;
                pa.Y = bg->Q0[gi].as<double>(); pa.ldy = ldq; pa.C = ctx->ws_A.as<double>(); pa.ldc = ldq; pa.N = r > 0 ? r : 1;
                CRM_HIP(hipMemcpyAsync(d_probs + 3, &pa, sizeof(GemmProblem), hipMemcpyHostToDevice, st));
                const bool timing = ctx->timing && ctx->timed_used < 65536;
                if (timing) {
                    if (ctx->timed_used == ctx->timed.size()) {
                        hipEvent_t e0, e1;
                        CRM_HIP(hipEventCreate(&e0));
                        CRM_HIP(hipEventCreate(&e1));
                        ctx->timed.emplace_back(e0, e1);
                    }
                    CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].first, st));
                }
                CRM_TRY(launch_gemm_tn(ctx, d_probs + 3, 1, pa.M, pa.N, np, true, k, 1, 0));
                if (timing) {
                    CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].second, st));
                    ctx->timed_used++;
                    ctx->kr_flops += 2.0 * (double)n * (double)r * (double)k * (double)ns;
                }
                // the genes of the group, GCH to a launch: grid (variant, gene)
                const std::vector<int>& mem = members[q];
                for (size_t m0 = 0; m0 < mem.size(); m0 += GCH) {
                    const int ng = (int)std::min<size_t>(GCH, mem.size() - m0);
                    for (int s = 0; s < ng; s++) {
                        const int i = mem[m0 + s];
                        ContextLrtArgs a{};
                        a.Tx = ctx->ws_A.as<double>(); a.tx_slab = (long)k * ldq; a.ldT = ldq;
                        a.Tg = Tb + (size_t)q * tslab + (size_t)b0 * ldT; a.ldTg = ldT;
                        a.tX = fa[i].rho[gi].tW; a.ldW = ldq; a.ty = fa[i].rho[gi].ty; a.S0 = fa[i].rho[gi].S0;
                        a.r = r; a.c = c; a.k = k; a.n = n;
                        a.WW = fa[i].WW; a.Wy = fa[i].Wy; a.yy = fa[i].yy;
                        a.gg = d_gg + b0; a.gy = d_gy + (size_t)i * ldcy + b0; a.gW = d_gW + (size_t)b0 * ld_gW; a.ld_gW = ld_gW;
                        a.xXy = d_xXy; a.ld_xXy = ld_p; a.xy = d_xXy + yoff + i; a.ld_xy = ld_p;
                        a.xx = d_xx + (size_t)b0 * ld_k; a.ld_xx = ld_k; a.xg = d_xg + (size_t)b0 * ld_k; a.ld_xg = ld_k;
                        a.delta = d_delta + (size_t)i * BLK + b0; a.drop = d_cdrop + (size_t)i * BLK + b0;
                        a.phi = d_phi + (size_t)s * SUB * ldq; a.ld_phi = ldq;
                        a.pvalue = d_res + (size_t)(0 * ngenes + i) * tests; a.alt_lml = d_res + (size_t)(1 * ngenes + i) * tests;
                        a.beta = d_res + (size_t)(2 * ngenes + i) * tests; a.beta_se = d_res + (size_t)(3 * ngenes + i) * tests;
                        a.logp = d_res + (size_t)(4 * ngenes + i) * tests; a.status = d_status + (size_t)i * tests;
                        a.null_lml = d_nlml + (size_t)i * BLK + b0;
                        if (joint) {
                            ContextJointArgs& j = rec_j[m0 + s];
                            j = ContextJointArgs{};
                            j.base = a;
                            j.xxp = d_xxp + (size_t)b0 * ld_pp; j.ld_xxp = ld_pp;
                            j.V = v_global ? d_V + (size_t)s * SUB * v_slab : nullptr; j.v_slab = v_slab;
                            j.v_in_lds = v_global ? 0 : 1;
                            j.dof = d_dof + (size_t)i * SUB; j.dropped = d_dropped + (size_t)i * tests;
                        } else {
                            rec_l[m0 + s] = a;
                        }
                    }
                    // (the records of the launches of this sub-range sit side by side: slot m0 of the group's stretch)
                    char* d_rec = sm + o_rec + rec_bytes * m0;
                    if (joint) {
                        CRM_HIP(hipMemcpyAsync(d_rec, rec_j.data() + m0, rec_bytes * ng, hipMemcpyHostToDevice, st));
                        CRM_TRY(launch_context_joint_multi(st, (const ContextJointArgs*)d_rec, ng, c, k, v_global, ns));
                    } else {
                        CRM_HIP(hipMemcpyAsync(d_rec, rec_l.data() + m0, rec_bytes * ng, hipMemcpyHostToDevice, st));
                        CRM_TRY(launch_context_lrt_multi(st, (const ContextLrtArgs*)d_rec, ng, c, k, ns));
                    }
                }
                CRM_HIP(hipStreamSynchronize(st));   // (the next group writes T_x and the records anew)
            }
            // the sub-range's results, gene-major on the host: row i of [ngenes x count (x k)]
            const size_t at = (size_t)(done + b0) * k, cnt = (size_t)ns * k;
            double* const outs[5] = {out.pvalue, out.alt_lml, out.beta, out.beta_se, out.logp};
            for (int q = 0; q < 5; q++) {
                if (!outs[q]) continue;
                const bool each = !joint || q == 2 || q == 3;   // joint: only beta and beta_se are per variant and context
                CRM_HIP(hipMemcpy2DAsync(outs[q] + (each ? at : (size_t)(done + b0)), sizeof(double) * (size_t)count * (each ? k : 1),
                                         d_res + (size_t)q * ngenes * tests, sizeof(double) * tests,
                                         sizeof(double) * (each ? cnt : (size_t)ns), ngenes, hipMemcpyDeviceToHost, st));
            }
            if (out.status)
                CRM_HIP(hipMemcpy2DAsync(out.status + (joint ? (size_t)(done + b0) : at), sizeof(int) * (size_t)count * (joint ? 1 : k),
                                         d_status, sizeof(int) * tests, sizeof(int) * (joint ? (size_t)ns : cnt), ngenes,
                                         hipMemcpyDeviceToHost, st));
            if (joint && out.dof)
                CRM_HIP(hipMemcpy2DAsync(out.dof + done + b0, sizeof(int) * (size_t)count, d_dof, sizeof(int) * SUB, sizeof(int) * ns,
                                         ngenes, hipMemcpyDeviceToHost, st));
            if (joint && out.dropped)
                CRM_HIP(hipMemcpy2DAsync(out.dropped + at, sizeof(int) * (size_t)count * k, d_dropped, sizeof(int) * tests,
                                         sizeof(int) * cnt, ngenes, hipMemcpyDeviceToHost, st));
            CRM_HIP(hipStreamSynchronize(st));   // (the next sub-range writes the same buffers)
        }
        if (out.null_lml)
            CRM_HIP(hipMemcpy2DAsync(out.null_lml + done, sizeof(double) * count, d_nlml, sizeof(double) * BLK, sizeof(double) * nb,
                                     ngenes, hipMemcpyDeviceToHost, st));
        CRM_HIP(hipStreamSynchronize(st));
        ctx->report(done + nb, count);
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
