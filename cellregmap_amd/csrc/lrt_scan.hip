// The host steps shared by the association LRTs and the fixed-effect GxC context tests (lrt_scan.h).
#include "lrt_scan.h"

namespace crm {

namespace {

__global__ __launch_bounds__(256) void columns_kernel(const ColumnSource* __restrict__ cols, long rows, double* __restrict__ XY,
                                                      long ldxy) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const ColumnSource s = cols[blockIdx.y];
    XY[i * ldxy + s.dst] = s.src[i * s.ld];
}

}  // namespace

int check_panel_range(const char* what, const crm_background* bg, const crm_panel* panel, long first, long count) {
    if (panel->ctx != bg->ctx || panel->n != bg->n) {
        set_error("%s: genes and panel do not match (context / cell count: %ld against %ld)", what, panel->n, bg->n);
        return CRM_ERR_ARG;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("%s: variants [%ld, %ld) outside the panel (p = %ld)", what, first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    return CRM_OK;
}

int check_shared_genes(const char* what, crm_gene* const* genes, int ngenes, bool contexts_too) {
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
        const bool other_bg = g->bg != g0->bg || g->ctx != g0->ctx, other_W = g->c != g0->c || g->w_key != g0->w_key;
        const char* differs = nullptr;
        if (!contexts_too) differs = other_bg || other_W ? "share the background and W" : nullptr;
        else if (other_bg) differs = "share the background";
        else if (g->k0 != g0->k0 || g->e0_key != g0->e0_key) differs = "hold the same contexts C";
        else if (other_W) differs = "hold the same covariates X0";
        if (differs) {
            set_error("%s: genes of one call must %s (gene %d differs from gene 0)", what, differs, i);
            return CRM_ERR_ARG;
        }
    }
    return CRM_OK;
}

int launch_gene_null(hipStream_t st, crm_gene* gene, const ZeroVariant& z, NullFitOut* d_fit, double* xwide, NullFitArgs& fa) {
    fa = NullFitArgs{};
    nullfit_gene_args(fa, gene, 0);
    for (int i = 0; i < fa.nrho; i++) { fa.rho[i].T = z.zero; fa.rho[i].ldT = 0; }
    fa.gg = z.gg; fa.gy = z.gy; fa.gW = z.gW; fa.ld_gW = z.ld_gW;
    fa.trial = z.trial; fa.out = d_fit; fa.xwide = xwide;
    return launch_nullfit(st, fa, 1);
}

int gene_null_row(const char* what, const crm_background* bg, int gene, const NullFitOut& fit, double* row) {
    const int ri = fit.rho_index;
    if (ri < 0 || ri >= bg->nrho) {
        char which[32] = "";
        if (gene >= 0) snprintf(which, sizeof which, " of gene %d", gene);
        set_error("%s: the null model's fit%s did not run (grid index %d)", what, which, ri);
        return CRM_ERR_NUMERIC;
    }
    if (row) {
        const double rho = bg->rho[ri];
        row[0] = rho, row[1] = fit.v0 * rho, row[2] = fit.v0 * (1 - rho);
        row[3] = fit.v1, row[4] = fit.lml, row[5] = fit.delta;
    }
    return CRM_OK;
}

int fit_gene_null(const char* what, crm_gene* gene, const ZeroVariant& z, NullFitOut* d_fit, int variants, DevBuf& xwide,
                  NullFitArgs& fa, NullFitOut& null, double* out_row) {
    const crm_background* bg = gene->bg;
    hipStream_t st = gene->ctx->stream;
    CRM_HIP(hipMemsetAsync(z.zero, 0, sizeof(double) * bg->ldq, st));
    CRM_HIP(hipMemsetAsync(z.gg, 0, sizeof(double), st));
    CRM_HIP(hipMemsetAsync(z.gy, 0, sizeof(double), st));
    CRM_HIP(hipMemsetAsync(z.gW, 0, sizeof(double) * z.ld_gW, st));
    if (gene->c > CRM_MAX_COV_WIDE)   // 63 .. 128 columns: nullfit_xwide.hip
        CRM_TRY(xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(std::max(variants, 1), bg->nrho, gene->c)));
    CRM_TRY(launch_gene_null(st, gene, z, d_fit, xwide.as<double>(), fa));
    CRM_HIP(hipMemcpyAsync(&null, d_fit, sizeof null, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    return gene_null_row(what, bg, -1, null, out_row);
}

int NullRows::read(const char* what, const crm_background* bg, const double* null, int ngenes, bool fast) {
    ri.assign(ngenes, -1);
    for (int i = 0; i < ngenes; i++) {
        const double* row = null + 6 * (size_t)i;
        for (int k = 0; k < bg->nrho; k++)
            if (bg->rho[k] == row[0]) { ri[i] = k; break; }
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
    return CRM_OK;
}

int NullRows::group(crm_background* bg) {
    grp_of_rho.assign(bg->nrho, -1);
    grp_rho.clear();
    for (int k : ri) grp_of_rho[k] = 0;
    for (int k = 0; k < bg->nrho; k++)
        if (grp_of_rho[k] == 0) { grp_of_rho[k] = (int)grp_rho.size(); grp_rho.push_back(k); }
    members.assign(grp_rho.size(), {});
    for (size_t i = 0; i < ri.size(); i++) members[grp_of_rho[ri[i]]].push_back((int)i);
    for (int k : grp_rho) CRM_TRY(crm_background_require_q0(bg, k));
    return CRM_OK;
}

void PhenotypeMatrix::plan(crm_gene* const* genes, int ngenes) {
    const crm_gene* g0 = genes[0];
    yoff = round_up(g0->c, 16);
    ncol = yoff + ngenes;
    ldxy = round_up(ncol, 128) + 128;   // (column tiles read from column 0 or from yoff stay inside a row)
    srcs.clear();
    for (int u = 0; u < g0->c; u++) srcs.push_back({g0->yW.as<double>() + 1 + u, g0->ld_yw, u});
    for (int i = 0; i < ngenes; i++) srcs.push_back({genes[i]->yW.as<double>(), genes[i]->ld_yw, yoff + i});
}

int PhenotypeMatrix::ensure(crm_ctx* ctx, long cells_pad) {
    CRM_TRY(ctx->ws_XG.ensure(sizeof(double) * (size_t)cells_pad * ldxy));
    XY = ctx->ws_XG.as<double>();
    return CRM_OK;
}

int PhenotypeMatrix::clear(hipStream_t st, long cells_pad) {
    CRM_HIP(hipMemsetAsync(XY, 0, sizeof(double) * (size_t)cells_pad * ldxy, st));
    return CRM_OK;
}

int PhenotypeMatrix::fill(hipStream_t st, long cells_pad) {
    CRM_HIP(hipMemcpyAsync(d_srcs, srcs.data(), srcs_bytes(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(columns_kernel, dim3((unsigned)((cells_pad + 255) / 256), (unsigned)srcs.size()), dim3(256), 0, st,
                       (const ColumnSource*)d_srcs, cells_pad, XY, ldxy);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int LrtBlock::ensure() {
    CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
    if (!fast) CRM_TRY(ctx->ws_Gx.ensure(sizeof(double) * (size_t)np * ldb));
    return CRM_OK;
}

int LrtBlock::prepare(long done, int nb, int plain_cols) {
    const double *d_y = g0->yW.as<double>(), *d_W = d_y + 1;
    Gb = Gx = ctx->ws_Gb.as<double>();
    if (panel->grouped)
        CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + first + done, panel->ld, panel->group.as<int>(), np, n, nullptr,
                                    nb, Gb, ldb, (int)ldb));
    else
        CRM_TRY(launch_gather_block(st, panel->G.as<double>() + first + done, panel->ld, np, n, nullptr, nullptr, nb, Gb, ldb,
                                    (int)ldb));
    CRM_TRY(launch_variant_stats(st, Gb, ldb, np, nb, d_y, d_W, g0->ld_yw, plain_cols, d_part, d_gg, d_gy, d_gW, ld_gW));
    if (fast) return CRM_OK;
    Gx = ctx->ws_Gx.as<double>();
    CRM_TRY(launch_ortho_block(st, Gb, ldb, np, nb, (int)ldb, d_W, g0->ld_yw, c, g0->Wproj.as<double>(), d_gW, ld_gW, d_coef, ldb,
                               d_thr, Gx, ldb));
    CRM_TRY(launch_variant_stats(st, Gx, ldb, np, nb, d_y, d_W, g0->ld_yw, c, d_part, d_gg, d_gy, d_gW, ld_gW));
    CRM_TRY(launch_ortho_rank(st, d_gg, d_thr, nb, d_drop));
    return CRM_OK;
}

GemmProblem LrtBlock::rotation(int k, int nb, double* C, long ldc) const {
    GemmProblem p{};
    p.X = Gx; p.ldx = ldb; p.Y = bg->Q0[k].as<double>(); p.ldy = ldq;
    p.C = C; p.ldc = ldc; p.M = nb; p.N = bg->r[k] > 0 ? bg->r[k] : 1;
    return p;
}

int ContextTables::check(const char* what, int c, int k, bool joint) {
    if (k < 1 || k > CRM_MAX_K0) {
        set_error("%s: %d contexts (supported 1..%d)", what, k, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    if (c < 1 || c > CRM_MAX_COV_XWIDE) {
        set_error("%s: the covariates and contexts span %d columns (supported 1..%d)", what, c, CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    return joint ? context_joint_check(c, k) : CRM_OK;
}

ContextTables::ContextTables(const LrtBlock& B, int k_, bool joint_)
    : k(k_), npair(k_ * (k_ + 1) / 2), joint(joint_), v_global(joint_ && !context_joint_v_in_lds(B.c, k_)), ld_k(round_up(k_, 8)),
      ld_cq(round_up(k_, 128)), ld_pp(joint_ ? round_up(npair, 128) : 0), v_slab((long)(B.c + 1) * k_) {
    // variants per sub-range: their rotated candidates (of one rho group) stay within the budget
    const size_t budget = B.ctx->context_budget > 0 ? B.ctx->context_budget : CONTEXT_BUDGET;
    SUB = (int)std::min<size_t>((size_t)B.BLK, std::max<size_t>(budget / (sizeof(double) * (size_t)k * B.ldq), 1));
    tests = (size_t)SUB * k;
}

int ContextTables::ensure(const LrtBlock& B) {
    crm_ctx* ctx = B.ctx;
    CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)B.np * B.ldb));
    if (!B.fast) CRM_TRY(ctx->ws_GG.ensure(sizeof(double) * (size_t)B.np * B.ldb));
    CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)SUB * k * B.ldq));
    CRM_TRY(ctx->ws_ctxE.ensure(sizeof(double) * (size_t)B.np * (2 * ld_cq + ld_pp)));
    return CRM_OK;
}

int ContextTables::operands(const LrtBlock& B) {
    Cq = B.ctx->ws_ctxE.as<double>();
    C2 = Cq + (size_t)B.np * ld_cq;
    CC = C2 + (size_t)B.np * ld_cq;
    CRM_TRY(launch_context_operands(B.st, B.g0->E0.as<double>(), B.g0->lde, B.np, k, Cq, C2, ld_cq));
    if (joint) CRM_TRY(launch_context_pairs(B.st, B.g0->E0.as<double>(), B.g0->lde, B.np, k, CC, ld_pp));
    return CRM_OK;
}

int ContextTables::block_products(const LrtBlock& B, int nb, GemmProblem* pr) const {
    double* G2 = B.ctx->ws_G2.as<double>();
    double* GG = B.fast ? nullptr : B.ctx->ws_GG.as<double>();
    CRM_TRY(launch_square_block(B.st, B.Gb, B.Gx, B.ldb, B.ldb, B.np, (int)B.ldb, G2, GG, B.ldb));
    GemmProblem& p2 = pr[1];
    p2 = GemmProblem{};
    p2.X = G2; p2.ldx = B.ldb; p2.Y = C2; p2.ldy = ld_cq; p2.C = d_xx; p2.ldc = ld_k; p2.M = nb; p2.N = k;
    GemmProblem& p3 = pr[2];
    p3 = p2;
    p3.X = GG ? GG : G2; p3.Y = Cq; p3.C = d_xg;
    GemmProblem& p5 = pr[5];
    p5 = p2;
    p5.Y = CC; p5.ldy = ld_pp; p5.C = d_xxp; p5.ldc = ld_pp; p5.N = npair;
    return CRM_OK;
}

GemmProblem ContextTables::khatri_rao(const LrtBlock& B, int b0, int ns, const double* Y, long ldy, int N, double* C, long ldc) const {
    GemmProblem p{};
    p.X = B.Gb + b0; p.ldx = B.ldb; p.E = Cq; p.lde = ld_cq; p.k0 = k;
    p.Y = Y; p.ldy = ldy; p.C = C; p.ldc = ldc; p.M = ns * k; p.N = N;
    return p;
}

int ContextTables::launch_rotated(const LrtBlock& B, const GemmProblem* d_p, const GemmProblem& p, int r, int ns) const {
    crm_ctx* ctx = B.ctx;
    const bool timing = ctx->timing && ctx->timed_used < 65536;   // bounded: a forgotten timer cannot grow for ever
    if (timing) CRM_TRY(kernel_timer_open(ctx, B.st, true));
    CRM_TRY(launch_gemm_tn(ctx, d_p, 1, p.M, p.N, B.np, true, k, 1, 0));
    if (timing) {
        CRM_TRY(kernel_timer_close(ctx, B.st));
        ctx->kr_flops += 2.0 * (double)B.n * (double)r * (double)k * (double)ns;
    }
    return CRM_OK;
}

}  // namespace crm
