// Steps 10-11 of a scan per phenotype (scan_pass.h: ScanPass): Q and F, eigenvalues and p-values, the flat-optimum probes.
#include "scan_pass.h"

namespace crm {

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

// flat-optimum probes (info calls only): the score test again with delta one stopping tolerance of the
// reference's search to either side; how far Q and p move says whether the search's last comparison matters.
// flat[b]: 1 = FLAT_OPTIMUM, 2 = STATISTIC_AT_TOLERANCE
int ScanPass::flat_probes(const Block& B, const SubRange& R, int gi, const AssembleArgs& aa, double* slow_ws, std::vector<char>& flat,
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

// the assembly's operands of gene gi over a sub-range (also what the fused Gram of the pair stage reads: folded_S)
AssembleArgs ScanPass::assemble_args(const SubRange& R, int gi) const {
    crm_gene* g = genes[gi];
    const int BLK = P.BLK, b0 = R.b0;
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
    return aa;
}

// 10.-11. per gene: Q and F, eigenvalues + Davies (or the exact tail), results
int ScanPass::gene_results(const Block& B, const SubRange& R, int gi) {
    const ScanOut& o = outs[gi];
    const int nb = R.nb, BLK = P.BLK, b0 = R.b0;
    const long done = R.done;
    AssembleArgs aa = assemble_args(R, gi);
    aa.wb_gram_done = gram_fused ? 1 : 0;   // (folded_S: wb_Gw of this sub-range is formed)
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

}  // namespace crm
