// Host orchestration of the association scans (C-ABI crm_scan_association, crm_scan_association_effects).
// Reference: cellregmap/_cellregmap.py:246-314 and :443-469.
#include <algorithm>

#include "lrt_scan.h"

using namespace crm;

namespace {

// One call of crm_scan_association (eff null: its launches and nothing else) or crm_scan_association_effects (one more
// launch per block, after the alt fits: assoc_effects.hip): what is fixed once the checks have passed, one function per stage.
struct AssocScan {
    LrtBlock B;
    crm_gene* gene; crm_background* bg; crm_ctx* ctx;
    hipStream_t st;
    const AssocEffectsOut* eff;
    const int BLK, c;
    const bool fast;
    const long ldq, ldT;
    ZeroVariant zero;
    NullFitOut* d_fit = nullptr;
    double *d_lml = nullptr, *d_pv = nullptr, *d_prep = nullptr, *d_wts = nullptr, *d_eff = nullptr;
    AssocEffectsGene* d_effg = nullptr;
    DevBuf xwide;        // (per call: the context's ws_xwide serves the many-gene scans)
    NullFitArgs fa{}, alt{};
    NullFitOut null{};
    int ri = -1;         // grid index of the null's rho
    AssocArgs aa{};
    AssocEffectsGene eg{};   // (host source of an asynchronous copy: alive until the first block's sync)

    AssocScan(crm_gene* gene_, crm_panel* panel, long first, long count, int fast_, const AssocEffectsOut* eff_)
        : B(gene_, panel, first, count, fast_), gene(gene_), bg(B.bg), ctx(B.ctx), st(B.st), eff(eff_), BLK(B.BLK), c(B.c),
          fast(B.fast), ldq(B.ldq), ldT(B.ldq) {}

    int workspaces() {
        CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)BLK * ldT));
        CRM_TRY(B.ensure());
        zero.ld_gW = B.ld_gW;
        CRM_TRY(carve_workspace(ctx->ws_small, [&](auto& take) {
            B.carve(take, true);
            take(zero.trial, sizeof(NullFitTrial) * std::max(BLK, B.nrho) * B.nrho), take(d_fit, sizeof(NullFitOut) * BLK);
            take(d_lml, sizeof(double) * BLK), take(d_pv, sizeof(double) * BLK);
            take(d_prep, sizeof(double) * fastscan_prep_doubles()), take(d_wts, sizeof(double) * ldq);
            take(zero.zero, sizeof(double) * ldq);
            take(d_eff, eff ? sizeof(double) * 5 * BLK + sizeof(int) * BLK : 0), take(d_effg, eff ? sizeof(AssocEffectsGene) : 0);
        }));
        zero.gg = B.d_gg; zero.gy = B.d_gy; zero.gW = B.d_gW;   // (the null is fitted before the first block fills them)
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + 4)));
        return CRM_OK;
    }

    // the null model into out_null
    int null_model(double* out_null) {
        CRM_TRY(fit_gene_null("association", gene, zero, d_fit, BLK, xwide, fa, null, out_null));
        ri = null.rho_index;
        return CRM_OK;
    }

    // per-SNP arguments at the null's rho
    int operands() {
        alt = fa;
        alt.nrho = 1;
        alt.rho[0] = fa.rho[ri];
        alt.rho[0].T = ctx->ws_T.as<double>();
        alt.rho[0].ldT = ldT;
        alt.g_drop = B.d_drop;   // (full refit: LMM(y, [W, g]) reduces [W, g] by economic_svd, see launch_ortho_block)
        aa.T = ctx->ws_T.as<double>(); aa.ldT = ldT;
        aa.ty = fa.rho[ri].ty; aa.tW = fa.rho[ri].tW; aa.ldW = ldq; aa.S0 = fa.rho[ri].S0;
        aa.r = bg->r[ri]; aa.c = c; aa.n = B.n; aa.delta0 = null.delta;
        aa.WW = fa.WW; aa.Wy = fa.Wy; aa.yy = fa.yy;
        aa.gg = B.d_gg; aa.gy = B.d_gy; aa.gW = B.d_gW; aa.ld_gW = B.ld_gW;
        if (fast) CRM_TRY(launch_fastscan_prep(st, aa, d_prep, d_wts));
        if (eff) {
            eg.T = aa.T; eg.t_sb = ldT; eg.t_sk = 1;
            eg.ty = aa.ty; eg.tW = aa.tW; eg.S0 = aa.S0; eg.ldW = aa.ldW; eg.r = aa.r; eg.c = c; eg.n = B.n;
            eg.WW = aa.WW; eg.Wy = aa.Wy; eg.yy = aa.yy;
            eg.gg = B.d_gg; eg.gy = B.d_gy; eg.gW = B.d_gW; eg.gW_sb = B.ld_gW; eg.gW_su = 1;
            eg.prep = d_prep; eg.wts = d_wts; eg.delta0 = null.delta;
            eg.trial = zero.trial; eg.alt_lml = d_lml; eg.null_lml = null.lml;
            eg.out_beta = d_eff; eg.out_se = d_eff + BLK; eg.out_delta = d_eff + 2 * BLK; eg.out_scale = d_eff + 3 * BLK;
            eg.out_logp = d_eff + 4 * BLK; eg.out_status = (int*)(d_eff + 5 * BLK);
            CRM_HIP(hipMemcpyAsync(d_effg, &eg, sizeof eg, hipMemcpyHostToDevice, st));
        }
        return CRM_OK;
    }

    // T_g = Q0(rho*)'gx of the block
    int rotate(int nb) {
        CRM_TRY(crm_background_require_q0(bg, ri));
        const GemmProblem p = B.rotation(ri, nb, ctx->ws_T.as<double>(), ldT);
        CRM_HIP(hipMemcpyAsync(ctx->ws_probs.ptr, &p, sizeof p, hipMemcpyHostToDevice, st));
        return launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>(), 1, nb, (int)ldq, B.np, false, 0, 1, 0);
    }

    // the alt fits, the LRT and (eff) the effect sizes: T(rho*), the block's plain products and the alt fits are in place
    int tests(int nb) {
        if (fast) {
            CRM_TRY(launch_fastscan(st, aa, d_prep, d_wts, nb, d_lml));
        } else {
            CRM_TRY(launch_nullfit(st, alt, nb));
            CRM_TRY(launch_gather_trial_lml(st, zero.trial, nb, d_lml));
        }
        return launch_lrt(st, d_lml, null.lml, nb, d_pv);
    }

    int copy_out(long done, int nb, double* out_pvalue, double* out_alt_lml) {
        if (out_pvalue) CRM_HIP(hipMemcpyAsync(out_pvalue + done, d_pv, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        if (out_alt_lml) CRM_HIP(hipMemcpyAsync(out_alt_lml + done, d_lml, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }

    int effects(long done, int nb) {
        CRM_TRY(launch_assoc_effects(st, d_effg, 1, nb, c, fast));
        double* const outs[5] = {eff->beta, eff->se, eff->delta, eff->scale, eff->logp};
        for (int q = 0; q < 5; q++)
            if (outs[q])
                CRM_HIP(hipMemcpyAsync(outs[q] + done, d_eff + (size_t)q * BLK, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
        if (eff->status)
            CRM_HIP(hipMemcpyAsync(eff->status + done, d_eff + (size_t)5 * BLK, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }
};

int scan_association(crm_gene* gene, crm_panel* panel, long first, long count, int fast, double* out_pvalue,
                     double* out_alt_lml, double* out_null, const AssocEffectsOut* eff) {
    if (!gene || !panel) return CRM_ERR_ARG;
    CRM_TRY(check_panel_range("association", gene->bg, panel, first, count));
    InScan in_scan;
    CRM_TRY(in_scan.enter(gene->bg->ctx, "association"));
    CRM_HIP(hipSetDevice(gene->bg->ctx->device));
    AssocScan S(gene, panel, first, count, fast, eff);
    CRM_TRY(S.workspaces());
    CRM_TRY(S.null_model(out_null));
    if (count == 0) return CRM_OK;
    if (!std::isfinite(S.null.lml)) {
        set_error("association: the null model could not be fitted");
        return CRM_ERR_NUMERIC;
    }
    CRM_TRY(S.operands());
    for (long done = 0; done < count; done += S.BLK) {
        const int nb = S.B.nb_at(done);
        CRM_TRY(S.B.prepare(done, nb, S.c));
        CRM_TRY(S.rotate(nb));
        CRM_TRY(S.tests(nb));
        CRM_TRY(S.copy_out(done, nb, out_pvalue, out_alt_lml));
        if (eff) CRM_TRY(S.effects(done, nb));
        CRM_HIP(hipStreamSynchronize(S.st));
        S.ctx->report(done + nb, count);   // (the reference's tqdm, :270)
    }
    return CRM_OK;
}

}  // namespace

extern "C" int crm_scan_association(crm_gene* gene, crm_panel* panel, long first, long count, int fast,
                                    double* out_pvalue, double* out_alt_lml, double* out_null) {
    return crm::guarded_on("crm_scan_association", gene ? gene->ctx : nullptr, [&]() -> int {
    return scan_association(gene, panel, first, count, fast, out_pvalue, out_alt_lml, out_null, nullptr);
    });
}

extern "C" int crm_scan_association_effects(crm_gene* gene, crm_panel* panel, long first, long count, int fast,
                                            double* out_pvalue, double* out_alt_lml, double* out_null, double* out_beta,
                                            double* out_se, double* out_delta, double* out_scale, double* out_logp,
                                            int* out_status) {
    return crm::guarded_on("crm_scan_association_effects", gene ? gene->ctx : nullptr, [&]() -> int {
    const AssocEffectsOut eff{out_beta, out_se, out_delta, out_scale, out_logp, out_status};
    return scan_association(gene, panel, first, count, fast, out_pvalue, out_alt_lml, out_null, &eff);
    });
}
