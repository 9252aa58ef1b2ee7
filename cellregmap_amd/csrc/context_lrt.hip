// Per-context fixed-effect GxC tests (C-ABI crm_scan_interaction_contexts): after an interaction hit,
// in WHICH context does the variant's effect change?  The reference poses it in cellregmap/test/test_fixed_gxe.py:79-102:
// per variant the ML null LMM(y, [M, g, E]) and a FastScanner pass over the columns of E * g, one degree of freedom each
// (the closed form of oracle/lmm.py:247-267; lrt_pvalues, _cellregmap.py:443-469).
//
// One workgroup per variant b, X = [X0, g_b] (c + 1 columns), candidates x_j = g_b o C_j, delta = delta[b]:
//   a'K^-1b = a'b / delta - sum_s phi_s ta_s tb_s,   phi_s = (1 - delta) S0_s / (delta ((1 - delta) S0_s + delta))
// which is sum_s w_s ta_s tb_s + (a'b - sum_s ta_s tb_s) / delta with w_s = 1 / ((1 - delta) S0_s + delta) -- the weighted
// sum and its unweighted twin share their products, so they are taken in one pass with the weight w_s - 1 / delta = -phi_s;
// t. are the rotations by Q0(rho*), a'b the plain cell-space products.
//   1. phi over the spectrum (scratch row of the variant) and log|K|
//   2. the Gram of [tX; tg; ty] in that metric, packed lower triangle in LDS
//   3. its Cholesky factor over [X0, g] with the y row carried along: L, z = L^-1 X'K^-1y, rss0 = y'K^-1y - z'z
//   4. per group of 32 candidates: the (c + 2) x 32 products of [tX; tg; ty] with the rotated candidates and the 32 weighted
//      diagonals, forward solves v_j = L^-1 X'K^-1x_j (eight lanes per candidate), then
//        d_j = x_j'K^-1x_j - v_j'v_j,  m_j = x_j'K^-1y - v_j'z,  rss1_j = rss0 - m_j^2 / d_j,  beta_j = m_j / d_j
// The products of 2 and 4 run on v_mfma_f64_16x16x4_f64: A = 16 rows of [tX; tg; ty] times phi (the weight is applied as
// the rows are staged, w o T_x is never formed), B = 16 candidates, both staged through LDS in chunks of 32 spectrum
// entries (rows contiguous along the spectrum: 256-byte runs per row).  Candidates beyond k and rows beyond c + 2 are
// staged as zeros, so any k >= 1 and any r are served by the one form.
// Steps 1 to 3, the product scheme and the forward solves are stated once, in context_common.h: the joint test of all k
// candidates (context_joint.hip) runs them too.
#include "context_common.h"

namespace crm {

using namespace context_detail;

namespace {

// Variant b of the launch described by `a`.  MULTI: `a` is one gene's record of a launch over several phenotypes.
template <bool MULTI>
__device__ __forceinline__ void context_lrt_body(const ContextLrtArgs& a, const int b) {
    extern __shared__ __align__(16) double cl_smem[];
    const int tid = threadIdx.x;
    const int c = a.c, k = a.k;
    const int R = c + 2, Rp = (R + 15) / 16 * 16, iy = c + 1;
    double* const Hp = cl_smem;                          // packed lower triangle of the (c + 2)^2 Gram, then L with the y row
    double* const zone = Hp + R * (R + 1) / 2;           // [Rp + NG][LS]
    double* const red = zone + (Rp + NG) * LS;           // [NG * CH]
    double* const diag = red + NG * CH;                  // [NG]
    double* const scal = diag + NG;                      // [8]
    const double n = (double)a.n;
    const double* __restrict__ tg = a.Tg + (long)b * a.ldTg;
    double* __restrict__ phi = a.phi + (long)b * a.ld_phi;

    // 1 to 3: the weights and log|K|, the Gram of [tX; tg; ty], its Cholesky factor with the y row (context_common.h)
    const ContextNull nm = context_null_model(a, b, tg, phi, Hp, zone, red, scal);
    const double inv_d = 1.0 / nm.delta, logdetK = nm.logdetK, rss0 = nm.rss0, lml0 = nm.lml0;
    const int P = nm.P;
    const bool ok = nm.ok;
    if (tid == 0) a.null_lml[b] = lml0;

    // 4. the candidates
    const double* __restrict__ tx = a.Tx + (long)b * a.tx_slab;
    for (int j0 = 0; j0 < k; j0 += NG) {
        double dacc[4] = {0.0, 0.0, 0.0, 0.0};
        context_candidate_products(a, tg, phi, tx, j0, zone, dacc);
#pragma unroll
        for (int i = 0; i < 4; i++) red[((tid >> 5) + 8 * i) * CH + (tid & 31)] = dacc[i];
        __syncthreads();
        if (tid < NG) {
            double s = 0.0;
            for (int qq = 0; qq < CH; qq++) s += red[tid * CH + qq];
            diag[tid] = s;
        }
        context_candidate_metric<MULTI>(a, b, j0, inv_d, zone);   // X'K^-1x_j and y'K^-1x_j in place
        __syncthreads();
        const int col = tid >> 3, part = tid & 7;
        const SolveSums sums = context_forward_solves(Hp, P, iy, zone);
        const double vv = sums.vv, vz = sums.vz;
        const int j = j0 + col;
        if (part == 0 && j < k) {
            const double xKx = a.xx[(long)b * a.ld_xx + j] * inv_d - diag[col];
            const double d = xKx - vv;
            const double m = zone[iy * NG + col] - vz;
            double pv, alt, beta, se, lp;
            int status = CRM_CONTEXT_OK;
            if (!ok || !(lml0 == lml0)) {
                status = CRM_CONTEXT_NO_FIT;
                pv = alt = beta = se = lp = NAN;
            } else if (P == c || !(d > 1e-12 * xKx)) {
                // x_j in the span of [X0, g] (lstsq drops it), or g itself in the span of X0: nothing is tested
                status = CRM_CONTEXT_COLLINEAR;
                pv = 1.0 - EPS_TINY;
                alt = lml0;
                beta = se = NAN;
                lp = 0.0;
            } else {
                const double rss1 = rss0 - m * m / d;
                const double s1 = fmax(rss1 / n, EPS_SMALL);
                beta = m / d;
                se = sqrt(s1 / d);
                alt = -0.5 * (n * LOG2PI + n + n * log(s1) + logdetK);
                double lrs = -2.0 * lml0 + 2.0 * alt;     // (launch_lrt's statement and clips)
                lp = log_sf(lrs > 0.0 ? lrs : 0.0);
                if (lrs < DBL_TINY) lrs = DBL_TINY;
                pv = erfc(sqrt(0.5 * lrs));
                if (pv < DBL_TINY) pv = DBL_TINY;
                if (pv > 1.0 - EPS_TINY) pv = 1.0 - EPS_TINY;
                if (!(isfinite(beta) && isfinite(se) && isfinite(alt) && isfinite(lp))) status = CRM_CONTEXT_NON_FINITE;
            }
            const long o = (long)b * k + j;
            a.pvalue[o] = pv;
            a.alt_lml[o] = alt;
            a.beta[o] = beta;
            a.beta_se[o] = se;
            a.logp[o] = lp;
            a.status[o] = status;
        }
        __syncthreads();
    }
}

// (two workgroups per CU where the LDS allows it -- up to about 90 covariate columns: 233 VGPRs, nothing spilled)
__global__ __launch_bounds__(256, 2) void context_lrt_kernel(ContextLrtArgs a) { context_lrt_body<false>(a, blockIdx.x); }

// Several phenotypes: workgroup (b, q) reads the record of gene q of the rho group (uniform: scalar loads) and runs variant b
// on it.  The records share Tx, Tg, S0 and the plain tables of the block; a second gene finds T_x in L2 or HBM.
__global__ __launch_bounds__(256, 2) void context_lrt_multi_kernel(const ContextLrtArgs* __restrict__ genes) {
    const ContextLrtArgs a = genes[blockIdx.y];
    context_lrt_body<true>(a, blockIdx.x);
}

__global__ void context_operands_kernel(const double* __restrict__ E, long lde, long cells_pad, int k, double* __restrict__ Cq,
                                        double* __restrict__ C2, long ld_out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cells_pad * ld_out) return;
    const long i = e / ld_out;
    const int j = (int)(e - i * ld_out);
    const double v = j < k ? E[i * lde + j] : 0.0;
    Cq[e] = v;
    C2[e] = v * v;
}

__global__ void context_deltas_kernel(const NullFitTrial* __restrict__ trial, const int* __restrict__ g_drop, double delta0,
                                      int variants, double* __restrict__ delta, int* __restrict__ drop) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= variants) return;
    delta[i] = trial ? trial[i].delta : delta0;
    drop[i] = trial ? ((g_drop && g_drop[i]) || !trial[i].use_g ? 1 : 0) : 0;
}

}  // namespace

size_t context_lrt_lds_bytes(int c) {
    const int R = c + 2, Rp = (R + 15) / 16 * 16;
    return sizeof(double) * ((size_t)R * (R + 1) / 2 + (size_t)(Rp + NG) * LS + NG * CH + NG + 8);
}

int launch_context_lrt(hipStream_t st, const ContextLrtArgs& a, int variants) {
    if (variants <= 0) return CRM_OK;
    if (a.c < 1 || a.c > CRM_MAX_COV_XWIDE || a.k < 1 || a.k > CRM_MAX_K0 || a.r < 0) {
        set_error("context tests: %d covariate columns, %d contexts (supported 1..%d, 1..%d)", a.c, a.k, CRM_MAX_COV_XWIDE,
                  CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    const size_t lds = context_lrt_lds_bytes(a.c);
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&context_lrt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(context_lrt_kernel, dim3((unsigned)variants), dim3(256), lds, st, a);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_context_lrt_multi(hipStream_t st, const ContextLrtArgs* genes_dev, int ngenes, int c, int k, int variants) {
    if (variants <= 0 || ngenes <= 0) return CRM_OK;
    if (!genes_dev || c < 1 || c > CRM_MAX_COV_XWIDE || k < 1 || k > CRM_MAX_K0 || ngenes > 65535) {
        set_error("context tests: %d genes, %d covariate columns, %d contexts (supported 1..65535, 1..%d, 1..%d)", ngenes, c, k,
                  CRM_MAX_COV_XWIDE, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    const size_t lds = context_lrt_lds_bytes(c);
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&context_lrt_multi_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(context_lrt_multi_kernel, dim3((unsigned)variants, (unsigned)ngenes), dim3(256), lds, st, genes_dev);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_context_operands(hipStream_t st, const double* E, long lde, long cells_pad, int k, double* Cq, double* C2,
                            long ld_out) {
    const long total = cells_pad * ld_out;
    if (total <= 0) return CRM_OK;
    hipLaunchKernelGGL(context_operands_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, E, lde, cells_pad, k, Cq,
                       C2, ld_out);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_context_deltas(hipStream_t st, const NullFitTrial* trial, const int* g_drop, double delta0, int variants,
                          double* delta, int* drop) {
    if (variants <= 0) return CRM_OK;
    hipLaunchKernelGGL(context_deltas_kernel, dim3((unsigned)((variants + 255) / 256)), dim3(256), 0, st, trial, g_drop, delta0,
                       variants, delta, drop);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace crm
