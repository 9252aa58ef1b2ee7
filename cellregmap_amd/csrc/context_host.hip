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
#include "lrt_scan.h"

using namespace crm;

namespace {

struct ContextOut {
    double* pvalue; double* alt_lml; double* beta; double* beta_se; double* logp;
    int* status;
    double* null_lml; double* null_delta; double* null;
    // joint test: pvalue, alt_lml, logp and status per variant, beta and beta_se per variant and context, and
    bool joint; int* dof; int* dropped;
};

// One call of crm_scan_interaction_contexts(_joint): what is fixed once the checks have passed, one function per stage.
struct ContextScan {
    LrtBlock B;
    ContextTables X;
    const ContextOut& out;
    crm_gene* gene; crm_background* bg; crm_ctx* ctx;
    hipStream_t st;
    const int BLK, c, k, SUB;
    const bool fast, joint;
    const long ldq, ldT, ld_p;
    const size_t tests;
    ZeroVariant zero;
    NullFitOut* d_fit = nullptr;
    double *d_xXy = nullptr, *d_phi = nullptr, *d_delta = nullptr, *d_res = nullptr, *d_nlml = nullptr, *d_V = nullptr;
    int *d_cdrop = nullptr, *d_status = nullptr, *d_dof = nullptr, *d_dropped = nullptr;
    GemmProblem* d_probs = nullptr;
    DevBuf xwide;        // (per call: the context's ws_xwide serves the many-gene scans)
    NullFitArgs fa{}, alt{};
    NullFitOut null{};
    int ri = -1, r = 0;  // grid index of the null's rho, its spectrum's length
    ContextLrtArgs ca{}; ContextJointArgs ja{};
    std::vector<GemmProblem> pr;

    ContextScan(crm_gene* gene_, crm_panel* panel, long first, long count, int fast_, const ContextOut& out_)
        : B(gene_, panel, first, count, fast_), X(B, gene_->k0, out_.joint), out(out_), gene(gene_), bg(B.bg), ctx(B.ctx), st(B.st),
          BLK(B.BLK), c(B.c), k(X.k), SUB(X.SUB), fast(B.fast), joint(X.joint), ldq(B.ldq), ldT(B.ldq), ld_p(round_up(1 + B.c, 8)),
          tests(X.tests), pr(CONTEXT_SLOTS) {}

    int workspaces() {
        CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)BLK * ldT));
        CRM_TRY(B.ensure());
        CRM_TRY(X.ensure(B));
        zero.ld_gW = B.ld_gW;
        CRM_TRY(carve_workspace(ctx->ws_small, [&](auto& take) {
            B.carve(take, true);
            take(zero.trial, sizeof(NullFitTrial) * std::max(BLK, B.nrho) * B.nrho), take(d_fit, sizeof(NullFitOut) * BLK);
            take(zero.zero, sizeof(double) * ldq);
        }));
        zero.gg = B.d_gg; zero.gy = B.d_gy; zero.gW = B.d_gW;   // (the null is fitted before the first block fills them)
        CRM_TRY(carve_workspace(ctx->ws_ctxP, [&](auto& take) {
            take(d_xXy, sizeof(double) * tests * ld_p), take(X.d_xx, sizeof(double) * BLK * X.ld_k);
            take(X.d_xg, sizeof(double) * BLK * X.ld_k), take(d_phi, sizeof(double) * (size_t)SUB * ldq);
            take(d_delta, sizeof(double) * BLK), take(d_cdrop, sizeof(int) * BLK);
            take(d_res, sizeof(double) * 5 * tests), take(d_status, sizeof(int) * tests), take(d_nlml, sizeof(double) * BLK);
            take(X.d_xxp, sizeof(double) * (size_t)BLK * X.ld_pp);
            take(d_V, X.v_global ? sizeof(double) * (size_t)SUB * X.v_slab : 0);
            take(d_dof, joint ? sizeof(int) * BLK : 0), take(d_dropped, joint ? sizeof(int) * tests : 0);
        }));
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + CONTEXT_SLOTS)));
        d_probs = ctx->ws_probs.as<GemmProblem>();
        return CRM_OK;
    }

    // the gene-level null: ML fit with X = X0 over the rho grid, as crm_scan_association fits its own
    int null_model() {
        CRM_TRY(fit_gene_null("context tests", gene, zero, d_fit, BLK, xwide, fa, null, out.null));
        ri = null.rho_index;
        return CRM_OK;
    }

    int operands() {
        alt = fa;   // full refit: LMM(y, [X0, g]) per variant at the null's rho
        alt.nrho = 1;
        alt.rho[0] = fa.rho[ri];
        alt.rho[0].T = ctx->ws_T.as<double>();
        alt.rho[0].ldT = ldT;
        alt.g_drop = B.d_drop;
        CRM_TRY(X.operands(B));
        CRM_TRY(crm_background_require_q0(bg, ri));
        r = bg->r[ri];
        ca.Tx = ctx->ws_A.as<double>(); ca.tx_slab = (long)k * ldq; ca.ldT = ldq;
        ca.ldTg = ldT;
        ca.tX = fa.rho[ri].tW; ca.ldW = ldq; ca.ty = fa.rho[ri].ty; ca.S0 = fa.rho[ri].S0;
        ca.r = r; ca.c = c; ca.k = k; ca.n = B.n;
        ca.WW = fa.WW; ca.Wy = fa.Wy; ca.yy = fa.yy;
        ca.ld_gW = B.ld_gW; ca.xXy = d_xXy; ca.ld_xXy = ld_p; ca.ld_xx = X.ld_k; ca.ld_xg = X.ld_k;
        ca.phi = d_phi; ca.ld_phi = ldq;
        ca.pvalue = d_res; ca.alt_lml = d_res + tests; ca.beta = d_res + 2 * tests; ca.beta_se = d_res + 3 * tests;
        ca.logp = d_res + 4 * tests; ca.status = d_status;
        ja.ld_xxp = X.ld_pp; ja.V = X.v_global ? d_V : nullptr; ja.v_slab = X.v_slab; ja.v_in_lds = X.v_global ? 0 : 1;
        ja.dof = d_dof; ja.dropped = d_dropped;
        return CRM_OK;
    }

    // T_g and the block's products against the context tables
    int block_products(int nb) {
        pr[0] = B.rotation(ri, nb, ctx->ws_T.as<double>(), ldT);
        CRM_TRY(X.block_products(B, nb, pr.data()));
        CRM_HIP(hipMemcpyAsync(d_probs, pr.data(), sizeof(GemmProblem) * 3, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, 1, nb, (int)ldq, B.np, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 1, 2, nb, k, B.np, false, 0, 1, 0));
        if (joint) {
            CRM_HIP(hipMemcpyAsync(d_probs + 5, &pr[5], sizeof(GemmProblem), hipMemcpyHostToDevice, st));
            CRM_TRY(launch_gemm_tn(ctx, d_probs + 5, 1, nb, X.npair, B.np, false, 0, 1, 0));
        }
        return CRM_OK;
    }

    // delta_i: the null's, or the alt fit's of every variant
    int block_deltas(long done, int nb) {
        if (!fast) CRM_TRY(launch_nullfit(st, alt, nb));
        CRM_TRY(launch_context_deltas(st, fast ? nullptr : zero.trial, fast ? nullptr : B.d_drop, null.delta, nb, d_delta, d_cdrop));
        if (out.null_delta) CRM_HIP(hipMemcpyAsync(out.null_delta + done, d_delta, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }

    // variants [b0, b0 + ns) of the block: T_x, x_j'[y, X0] and the test launch
    int sub_range_tests(int b0, int ns) {
        const GemmProblem& pa = pr[3] = X.khatri_rao(B, b0, ns, bg->Q0[ri].as<double>(), ldq, r > 0 ? r : 1, ctx->ws_A.as<double>(), ldq);
        const GemmProblem& pb = pr[4] = X.khatri_rao(B, b0, ns, gene->yW.as<double>(), gene->ld_yw, 1 + c, d_xXy, ld_p);
        CRM_HIP(hipMemcpyAsync(d_probs + 3, pr.data() + 3, sizeof(GemmProblem) * 2, hipMemcpyHostToDevice, st));
        CRM_TRY(X.launch_rotated(B, d_probs + 3, pa, r, ns));
        CRM_TRY(launch_gemm_tn(ctx, d_probs + 4, 1, pb.M, pb.N, B.np, true, k, 1, 0));
        ContextLrtArgs sa = ca;
        sa.Tg = ctx->ws_T.as<double>() + (size_t)b0 * ldT;
        sa.gg = B.d_gg + b0; sa.gy = B.d_gy + b0; sa.gW = B.d_gW + (size_t)b0 * B.ld_gW;
        sa.xx = X.d_xx + (size_t)b0 * X.ld_k; sa.xg = X.d_xg + (size_t)b0 * X.ld_k;
        sa.delta = d_delta + b0; sa.drop = d_cdrop + b0; sa.null_lml = d_nlml + b0;
        if (!joint) return launch_context_lrt(st, sa, ns);
        ContextJointArgs sj = ja;
        sj.base = sa;
        sj.xxp = X.d_xxp + (size_t)b0 * X.ld_pp;
        return launch_context_joint(st, sj, ns);
    }

    int copy_sub_range(long at0, int ns) {
        const size_t at = (size_t)at0 * k, cnt = (size_t)ns * k;
        double* const outs[5] = {out.pvalue, out.alt_lml, out.beta, out.beta_se, out.logp};
        for (int q = 0; q < 5; q++) {
            const bool each = !joint || q == 2 || q == 3;   // joint: only beta and beta_se are per variant and context
            if (outs[q])
                CRM_HIP(hipMemcpyAsync(outs[q] + (each ? at : (size_t)at0), d_res + (size_t)q * tests,
                                       sizeof(double) * (each ? cnt : (size_t)ns), hipMemcpyDeviceToHost, st));
        }
        if (out.status)
            CRM_HIP(hipMemcpyAsync(out.status + (joint ? (size_t)at0 : at), d_status, sizeof(int) * (joint ? (size_t)ns : cnt),
                                   hipMemcpyDeviceToHost, st));
        if (joint && out.dof) CRM_HIP(hipMemcpyAsync(out.dof + at0, d_dof, sizeof(int) * ns, hipMemcpyDeviceToHost, st));
        if (joint && out.dropped) CRM_HIP(hipMemcpyAsync(out.dropped + at, d_dropped, sizeof(int) * cnt, hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }
};

int scan_contexts(crm_gene* gene, crm_panel* panel, long first, long count, int fast, const ContextOut& out) {
    if (!gene || !panel) return CRM_ERR_ARG;
    CRM_TRY(check_panel_range("context tests", gene->bg, panel, first, count));
    CRM_TRY(ContextTables::check("context tests", gene->c, gene->k0, out.joint));
    InScan in_scan;
    CRM_TRY(in_scan.enter(gene->bg->ctx, "context tests"));
    CRM_HIP(hipSetDevice(gene->bg->ctx->device));
    ContextScan S(gene, panel, first, count, fast, out);
    CRM_TRY(S.workspaces());
    CRM_TRY(S.null_model());
    if (count == 0) return CRM_OK;
    if (!std::isfinite(S.null.lml)) {
        set_error("context tests: the null model could not be fitted");
        return CRM_ERR_NUMERIC;
    }
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
        if (out.null_lml) CRM_HIP(hipMemcpyAsync(out.null_lml + done, S.d_nlml, sizeof(double) * nb, hipMemcpyDeviceToHost, S.st));
        CRM_HIP(hipStreamSynchronize(S.st));
        S.ctx->report(done + nb, count);
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
