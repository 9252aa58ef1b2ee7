// Host orchestration of the per-context fixed-effect GxC tests (C-ABI crm_scan_interaction_contexts).
// Reference: cellregmap/test/test_fixed_gxe.py:79-102 with cellregmap/_cellregmap.py:246-314 and :443-469.
//
// Per block of variants: the block, its plain products and its rotation T_g = Q0(rho*)'g as crm_scan_association forms
// them (full refit: in the basis orthogonal to X0, with the alt fits for delta_i); the cell-space tables of the
// candidates x_j = g o C_j -- x_j'x_j and x_j'g as plain products of the squared block against C^2 and C -- and then,
// per sub-range of the block, the Khatri-Rao contraction of the interaction scan twice: against Q0(rho*) for the rotated
// candidates T_x, against [y, X0] for x_j'[y, X0]; one launch of context_lrt.hip ends the sub-range.  T_x is the large
// buffer (variants x k x ldq doubles: 8 GB for 4096 variants at 50 contexts and a spectrum of 5 000), so a block is cut
// into sub-ranges that keep it within a byte budget, as the pair stage of the interaction scan sizes its own.
//
// The joint test of all k candidates (crm_scan_interaction_contexts_joint) runs the same body: one
// more table per call (the context pair products C_i o C_j), one more plain product per block (x_i'x_j against it), and
// context_joint.hip's launch in place of context_lrt.hip's.
#include <algorithm>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace {

constexpr size_t CONTEXT_BUDGET = (size_t)8 << 30;

struct ContextOut {
    double* pvalue; double* alt_lml; double* beta; double* beta_se; double* logp;
    int* status;
    double* null_lml; double* null_delta; double* null;
    // joint test: pvalue, alt_lml, logp and status per variant, beta and beta_se per variant and context, and
    bool joint; int* dof; int* dropped;
};

int scan_contexts(crm_gene* gene, crm_panel* panel, long first, long count, int fast, const ContextOut& out) {
    if (!gene || !panel) return CRM_ERR_ARG;
    crm_background* bg = gene->bg;
    crm_ctx* ctx = bg->ctx;
    if (panel->ctx != ctx || panel->n != bg->n) {
        set_error("context tests: gene and panel do not match (context / cell count)");
        return CRM_ERR_ARG;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("context tests: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    const int c = gene->c, k = gene->k0;
    if (k < 1 || k > CRM_MAX_K0) {
        set_error("context tests: %d contexts (supported 1..%d)", k, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    if (c < 1 || c > CRM_MAX_COV_XWIDE) {
        set_error("context tests: the covariates and contexts span %d columns (supported 1..%d)", c, CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    if (out.joint) CRM_TRY(context_joint_check(c, k));
    if (ctx->in_scan) {
        set_error("context tests: another scan is running on this context (started from a progress callback?)");
        return CRM_ERR_UNSUPPORTED;
    }
    struct InScan { crm_ctx* c; explicit InScan(crm_ctx* c_) : c(c_) { c->in_scan = true; } ~InScan() { c->in_scan = false; } } in_scan(ctx);
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    const int nrho = bg->nrho;
    const int BLK = (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : CRM_DEFAULT_BLOCK,
                                        round_up(std::max<long>(count, 1), 128));
    const long ldb = BLK + 128, ldT = ldq;
    const long ld_gW = round_up(c, 8), ld_p = round_up(1 + c, 8), ld_k = round_up(k, 8), ld_cq = round_up(k, 128);
    const bool joint = out.joint;
    const int npair = k * (k + 1) / 2;
    const long ld_pp = joint ? round_up(npair, 128) : 0;
    const bool v_global = joint && !context_joint_v_in_lds(c, k);
    const long v_slab = (long)(c + 1) * k;
    // variants per sub-range: their rotated candidates stay within the budget
    const size_t budget = ctx->context_budget > 0 ? ctx->context_budget : CONTEXT_BUDGET;
    const int SUB = (int)std::min<size_t>((size_t)BLK, std::max<size_t>(budget / (sizeof(double) * (size_t)k * ldq), 1));

    CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)BLK * ldT));
    CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
    CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)np * ldb));
    if (!fast) {
        CRM_TRY(ctx->ws_Gx.ensure(sizeof(double) * (size_t)np * ldb));
        CRM_TRY(ctx->ws_GG.ensure(sizeof(double) * (size_t)np * ldb));
    }
    CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)SUB * k * ldq));
    CRM_TRY(ctx->ws_ctxE.ensure(sizeof(double) * (size_t)np * (2 * ld_cq + ld_pp)));
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_gg = carve(sizeof(double) * BLK), o_gy = carve(sizeof(double) * BLK),
                 o_gW = carve(sizeof(double) * BLK * ld_gW),
                 o_trial = carve(sizeof(NullFitTrial) * std::max(BLK, nrho) * nrho),
                 o_fit = carve(sizeof(NullFitOut) * BLK), o_zero = carve(sizeof(double) * ldq),
                 o_part = carve(variant_stats_workspace(BLK, std::min(c, CRM_MAX_COV))),
                 o_coef = carve(sizeof(double) * (size_t)c * ldb), o_thr = carve(sizeof(double) * BLK),
                 o_drop = carve(sizeof(int) * BLK);
    CRM_TRY(ctx->ws_small.ensure(off));
    char* sm = ctx->ws_small.as<char>();
    double* d_gg = (double*)(sm + o_gg);
    double* d_gy = (double*)(sm + o_gy);
    double* d_gW = (double*)(sm + o_gW);
    NullFitTrial* d_trial = (NullFitTrial*)(sm + o_trial);
    NullFitOut* d_fit = (NullFitOut*)(sm + o_fit);
    double* d_zero = (double*)(sm + o_zero);
    double* d_part = (double*)(sm + o_part);
    double* d_coef = (double*)(sm + o_coef);
    double* d_thr = (double*)(sm + o_thr);
    int* d_drop = (int*)(sm + o_drop);
    off = 0;
    const size_t tests = (size_t)SUB * k;
    const size_t o_xXy = carve(sizeof(double) * tests * ld_p), o_xx = carve(sizeof(double) * BLK * ld_k),
                 o_xg = carve(sizeof(double) * BLK * ld_k), o_phi = carve(sizeof(double) * (size_t)SUB * ldq),
                 o_delta = carve(sizeof(double) * BLK), o_cdrop = carve(sizeof(int) * BLK),
                 o_res = carve(sizeof(double) * 5 * tests), o_status = carve(sizeof(int) * tests),
                 o_nlml = carve(sizeof(double) * BLK);
    const size_t o_xxp = carve(sizeof(double) * (size_t)BLK * ld_pp), o_V = carve(v_global ? sizeof(double) * (size_t)SUB * v_slab : 0),
                 o_dof = carve(joint ? sizeof(int) * BLK : 0), o_dropped = carve(joint ? sizeof(int) * tests : 0);
    CRM_TRY(ctx->ws_ctxP.ensure(off));
    char* cp = ctx->ws_ctxP.as<char>();
    double* d_xXy = (double*)(cp + o_xXy);
    double* d_xx = (double*)(cp + o_xx);
    double* d_xg = (double*)(cp + o_xg);
    double* d_delta = (double*)(cp + o_delta);
    int* d_cdrop = (int*)(cp + o_cdrop);
    double* d_res = (double*)(cp + o_res);
    int* d_status = (int*)(cp + o_status);
    double* d_nlml = (double*)(cp + o_nlml);
    double* d_xxp = (double*)(cp + o_xxp);
    int* d_dof = (int*)(cp + o_dof);
    int* d_dropped = (int*)(cp + o_dropped);
    constexpr int SLOTS = 8;   // 0 T_g, 1 / 2 the squared block's products, 3 / 4 the two Khatri-Rao contractions, 5 x_i'x_j (joint)
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + SLOTS)));
    GemmProblem* d_probs = ctx->ws_probs.as<GemmProblem>();
    const double* d_y = gene->yW.as<double>();
    const double* d_W = gene->yW.as<double>() + 1;

    // ---- gene-level null: ML fit with X = X0 over the rho grid, as crm_scan_association fits its own -------------------
    CRM_HIP(hipMemsetAsync(d_zero, 0, sizeof(double) * ldq, st));
    CRM_HIP(hipMemsetAsync(d_gg, 0, sizeof(double), st));
    CRM_HIP(hipMemsetAsync(d_gy, 0, sizeof(double), st));
    CRM_HIP(hipMemsetAsync(d_gW, 0, sizeof(double) * ld_gW, st));
    NullFitArgs fa{};
    nullfit_gene_args(fa, gene, 0);
    for (int i = 0; i < nrho; i++) { fa.rho[i].T = d_zero; fa.rho[i].ldT = 0; }
    fa.gg = d_gg; fa.gy = d_gy; fa.gW = d_gW; fa.ld_gW = ld_gW;
    fa.trial = d_trial; fa.out = d_fit;
    DevBuf xwide;
    if (c > CRM_MAX_COV_WIDE) {
        CRM_TRY(xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(std::max(BLK, 1), nrho, c)));
        fa.xwide = xwide.as<double>();
    }
    CRM_TRY(launch_nullfit(st, fa, 1));
    NullFitOut null{};
    CRM_HIP(hipMemcpyAsync(&null, d_fit, sizeof null, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    const int ri = null.rho_index;
    if (ri < 0 || ri >= nrho) {
        set_error("context tests: the null model's fit did not run (grid index %d)", ri);
        return CRM_ERR_NUMERIC;
    }
    const double rho = bg->rho[ri];
    if (out.null) {
        out.null[0] = rho;
        out.null[1] = null.v0 * rho;
        out.null[2] = null.v0 * (1 - rho);
        out.null[3] = null.v1;
        out.null[4] = null.lml;
        out.null[5] = null.delta;
    }
    if (count == 0) return CRM_OK;
    if (!std::isfinite(null.lml)) {
        set_error("context tests: the null model could not be fitted");
        return CRM_ERR_NUMERIC;
    }

    NullFitArgs alt = fa;   // full refit: LMM(y, [X0, g]) per variant at the null's rho
    alt.nrho = 1;
    alt.rho[0] = fa.rho[ri];
    alt.rho[0].T = ctx->ws_T.as<double>();
    alt.rho[0].ldT = ldT;
    alt.g_drop = d_drop;

    // the contexts as the Khatri-Rao operand (rows padded to whole 128-column tiles) and squared
    double* Cq = ctx->ws_ctxE.as<double>();
    double* C2 = Cq + (size_t)np * ld_cq;
    CRM_TRY(launch_context_operands(st, gene->E0.as<double>(), gene->lde, np, k, Cq, C2, ld_cq));
    double* CC = C2 + (size_t)np * ld_cq;   // joint: the pair products C_i o C_j, i >= j
    if (joint) CRM_TRY(launch_context_pairs(st, gene->E0.as<double>(), gene->lde, np, k, CC, ld_pp));
    CRM_TRY(crm_background_require_q0(bg, ri));
    const int r = bg->r[ri];

    ContextLrtArgs ca{};
    ca.Tx = ctx->ws_A.as<double>(); ca.tx_slab = (long)k * ldq; ca.ldT = ldq;
    ca.ldTg = ldT;
    ca.tX = fa.rho[ri].tW; ca.ldW = ldq; ca.ty = fa.rho[ri].ty; ca.S0 = fa.rho[ri].S0;
    ca.r = r; ca.c = c; ca.k = k; ca.n = n;
    ca.WW = fa.WW; ca.Wy = fa.Wy; ca.yy = fa.yy;
    ca.ld_gW = ld_gW; ca.xXy = d_xXy; ca.ld_xXy = ld_p; ca.ld_xx = ld_k; ca.ld_xg = ld_k;
    ca.phi = (double*)(cp + o_phi); ca.ld_phi = ldq;
    ca.pvalue = d_res; ca.alt_lml = d_res + tests; ca.beta = d_res + 2 * tests; ca.beta_se = d_res + 3 * tests;
    ca.logp = d_res + 4 * tests; ca.status = d_status;
    ContextJointArgs ja{};
    ja.ld_xxp = ld_pp; ja.V = v_global ? (double*)(cp + o_V) : nullptr; ja.v_slab = v_slab; ja.v_in_lds = v_global ? 0 : 1;
    ja.dof = d_dof; ja.dropped = d_dropped;

    for (long done = 0; done < count; done += BLK) {
        const int nb = (int)std::min<long>(BLK, count - done);
        double* Gb = ctx->ws_Gb.as<double>();   // the block as given: the candidates are g o C_j of these columns
        if (panel->grouped)
            CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + first + done, panel->ld, panel->group.as<int>(),
                                        np, n, nullptr, nb, Gb, ldb, (int)ldb));
        else
            CRM_TRY(launch_gather_block(st, panel->G.as<double>() + first + done, panel->ld, np, n, nullptr, nullptr,
                                        nb, Gb, ldb, (int)ldb));
        CRM_TRY(launch_variant_stats(st, Gb, ldb, np, nb, d_y, d_W, gene->ld_yw, c, d_part, d_gg, d_gy, d_gW, ld_gW));
        double* Gx = Gb;                        // the column that stands for g beside X0
        if (!fast) {
            // as crm_scan_association's refit: the basis of economic_svd([X0, g]), same span as [X0, g]
            Gx = ctx->ws_Gx.as<double>();
            CRM_TRY(launch_ortho_block(st, Gb, ldb, np, nb, (int)ldb, d_W, gene->ld_yw, c, gene->Wproj.as<double>(), d_gW, ld_gW,
                                       d_coef, ldb, d_thr, Gx, ldb));
            CRM_TRY(launch_variant_stats(st, Gx, ldb, np, nb, d_y, d_W, gene->ld_yw, c, d_part, d_gg, d_gy, d_gW, ld_gW));
            CRM_TRY(launch_ortho_rank(st, d_gg, d_thr, nb, d_drop));
        }
        std::vector<GemmProblem> pr(SLOTS);
        GemmProblem& pt = pr[0];
        pt.X = Gx; pt.ldx = ldb; pt.Y = bg->Q0[ri].as<double>(); pt.ldy = ldq;
        pt.C = ctx->ws_T.as<double>(); pt.ldc = ldT; pt.M = nb; pt.N = r > 0 ? r : 1;
        // x_j'x_j = (g o g)'C_j^2 and x_j'g = (g o gx)'C_j (gx: the column that stands for g)
        double* G2 = ctx->ws_G2.as<double>();
        double* GG = fast ? nullptr : ctx->ws_GG.as<double>();
        CRM_TRY(launch_square_block(st, Gb, Gx, ldb, ldb, np, (int)ldb, G2, GG, ldb));
        GemmProblem& p2 = pr[1];
        p2.X = G2; p2.ldx = ldb; p2.Y = C2; p2.ldy = ld_cq; p2.C = d_xx; p2.ldc = ld_k; p2.M = nb; p2.N = k;
        GemmProblem& p3 = pr[2];
        p3 = p2;
        p3.X = GG ? GG : G2; p3.Y = Cq; p3.C = d_xg;
        CRM_HIP(hipMemcpyAsync(d_probs, pr.data(), sizeof(GemmProblem) * 3, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, 1, nb, (int)ldq, np, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 1, 2, nb, k, np, false, 0, 1, 0));
        if (joint) {
            // x_i'x_j = (g o g)'(C_i o C_j), i >= j
            GemmProblem& p5 = pr[5];
            p5 = p2;
            p5.Y = CC; p5.ldy = ld_pp; p5.C = d_xxp; p5.ldc = ld_pp; p5.N = npair;
            CRM_HIP(hipMemcpyAsync(d_probs + 5, &p5, sizeof(GemmProblem), hipMemcpyHostToDevice, st));
            CRM_TRY(launch_gemm_tn(ctx, d_probs + 5, 1, nb, npair, np, false, 0, 1, 0));
        }
        if (!fast) CRM_TRY(launch_nullfit(st, alt, nb));
        CRM_TRY(launch_context_deltas(st, fast ? nullptr : d_trial, fast ? nullptr : d_drop, null.delta, nb, d_delta, d_cdrop));
        if (out.null_delta) CRM_HIP(hipMemcpyAsync(out.null_delta + done, d_delta, sizeof(double) * nb, hipMemcpyDeviceToHost, st));

        for (int b0 = 0; b0 < nb; b0 += SUB) {
            const int ns = std::min(SUB, nb - b0);
            GemmProblem& pa = pr[3];
            pa = GemmProblem{};
            pa.X = Gb + b0; pa.ldx = ldb; pa.E = Cq; pa.lde = ld_cq; pa.k0 = k;
            pa.Y = bg->Q0[ri].as<double>(); pa.ldy = ldq; pa.C = ctx->ws_A.as<double>(); pa.ldc = ldq;
            pa.M = ns * k; pa.N = r > 0 ? r : 1;
            GemmProblem& pb = pr[4];
            pb = pa;
            pb.Y = gene->yW.as<double>(); pb.ldy = gene->ld_yw; pb.C = d_xXy; pb.ldc = ld_p; pb.N = 1 + c;
            CRM_HIP(hipMemcpyAsync(d_probs + 3, pr.data() + 3, sizeof(GemmProblem) * 2, hipMemcpyHostToDevice, st));
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
            CRM_TRY(launch_gemm_tn(ctx, d_probs + 4, 1, pb.M, pb.N, np, true, k, 1, 0));
            ContextLrtArgs sa = ca;
            sa.Tg = ctx->ws_T.as<double>() + (size_t)b0 * ldT;
            sa.gg = d_gg + b0; sa.gy = d_gy + b0; sa.gW = d_gW + (size_t)b0 * ld_gW;
            sa.xx = d_xx + (size_t)b0 * ld_k; sa.xg = d_xg + (size_t)b0 * ld_k;
            sa.delta = d_delta + b0; sa.drop = d_cdrop + b0; sa.null_lml = d_nlml + b0;
            const size_t at = (size_t)(done + b0) * k, cnt = (size_t)ns * k;
            double* const outs[5] = {out.pvalue, out.alt_lml, out.beta, out.beta_se, out.logp};
            if (joint) {
                ContextJointArgs sj = ja;
                sj.base = sa;
                sj.xxp = d_xxp + (size_t)b0 * ld_pp;
                CRM_TRY(launch_context_joint(st, sj, ns));
                for (int q = 0; q < 5; q++) {
                    const bool each = q == 2 || q == 3;   // beta, beta_se: per variant and context
                    if (outs[q])
                        CRM_HIP(hipMemcpyAsync(outs[q] + (each ? at : (size_t)(done + b0)), d_res + (size_t)q * tests,
                                               sizeof(double) * (each ? cnt : (size_t)ns), hipMemcpyDeviceToHost, st));
                }
                if (out.status) CRM_HIP(hipMemcpyAsync(out.status + done + b0, d_status, sizeof(int) * ns, hipMemcpyDeviceToHost, st));
                if (out.dof) CRM_HIP(hipMemcpyAsync(out.dof + done + b0, d_dof, sizeof(int) * ns, hipMemcpyDeviceToHost, st));
                if (out.dropped) CRM_HIP(hipMemcpyAsync(out.dropped + at, d_dropped, sizeof(int) * cnt, hipMemcpyDeviceToHost, st));
            } else {
                CRM_TRY(launch_context_lrt(st, sa, ns));
                for (int q = 0; q < 5; q++)
                    if (outs[q])
                        CRM_HIP(hipMemcpyAsync(outs[q] + at, d_res + (size_t)q * tests, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
                if (out.status) CRM_HIP(hipMemcpyAsync(out.status + at, d_status, sizeof(int) * cnt, hipMemcpyDeviceToHost, st));
            }
            CRM_HIP(hipStreamSynchronize(st));   // (the next sub-range writes the same buffers)
        }
        if (out.null_lml) CRM_HIP(hipMemcpyAsync(out.null_lml + done, d_nlml, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        CRM_HIP(hipStreamSynchronize(st));
        ctx->report(done + nb, count);
    }
    return CRM_OK;
}

}  // namespace

extern "C" int crm_scan_interaction_contexts(crm_gene* gene, crm_panel* panel, long first, long count, int fast,
                                             double* out_pvalue, double* out_alt_lml, double* out_beta, double* out_beta_se,
                                             double* out_logp, int* out_status, double* out_null_lml, double* out_null_delta,
                                             double* out_null) {
    return crm::guarded_on("crm_scan_interaction_contexts", gene ? gene->ctx : nullptr, [&]() -> int {
    const ContextOut out{out_pvalue, out_alt_lml, out_beta, out_beta_se, out_logp, out_status, out_null_lml, out_null_delta,
                         out_null, false, nullptr, nullptr};
    return scan_contexts(gene, panel, first, count, fast, out);
    });
}

extern "C" int crm_scan_interaction_contexts_joint(crm_gene* gene, crm_panel* panel, long first, long count, int fast,
                                                   double* out_pvalue, double* out_logp, double* out_alt_lml, int* out_dof,
                                                   double* out_beta, double* out_beta_se, int* out_dropped, int* out_status,
                                                   double* out_null_lml, double* out_null_delta, double* out_null) {
    return crm::guarded_on("crm_scan_interaction_contexts_joint", gene ? gene->ctx : nullptr, [&]() -> int {
    const ContextOut out{out_pvalue, out_alt_lml, out_beta, out_beta_se, out_logp, out_status, out_null_lml, out_null_delta,
                         out_null, true, out_dof, out_dropped};
    return scan_contexts(gene, panel, first, count, fast, out);
    });
}

extern "C" int crm_test_set_context_budget(crm_ctx* ctx, long bytes) {
    return crm::guarded_on("crm_test_set_context_budget", ctx, [&]() -> int {
    if (!ctx || bytes < 0) return CRM_ERR_ARG;
    ctx->context_budget = (size_t)bytes;
    return CRM_OK;
    });
}
