// Joint fixed-effect GxC test (C-ABI crm_scan_interaction_contexts_joint): is there ANY fixed-effect
// GxC at this variant?  One likelihood-ratio test of all k columns g o C at once, k degrees of freedom -- the
// multi-environment LRT the interaction score test is compared against.  The reference poses the model family in
// cellregmap/test/test_fixed_gxe.py:79-102 and lrt_pvalues(null, alt, dof) (_cellregmap.py:443-469): the ML null
// LMM(y, [M, g, E]), the alternative LMM(y, [M, g, E, E * g]) at the null's delta.
//
// One workgroup per variant b.  Steps 1 to 3 are the per-context kernel's (context_common.h): phi, log|K|, the packed
// Cholesky factor L of A = X'K^-1X, X = [X0, g_b], with z = L^-1 X'K^-1y below it, rss0.  Then, with X_c = [x_1 .. x_k]:
//   4. per group of 32 candidates the (c + 2) x 32 products with [tX; tg; ty] and the forward solves, as the per-context
//      kernel runs them: V = L^-1 X'K^-1X_c (kept: LDS where it fits beside the rest, else the variant's global scratch
//      row), m = X_c'K^-1y - V'z
//   5. the k x k weighted Gram sum_s phi_s T_x[i][s] T_x[j][s] on the same MFMA tiles: per group of 32 columns the rows
//      from that group on (the lower triangle of group pairs; a diagonal pair in full), then
//      S = X_c'K^-1X_c - V'V as a packed triangle in LDS with m as its last row
//   6. the Cholesky factor of S in column order.  A candidate whose pivot is <= 1e-12 x_j'K^-1x_j is dropped: its row and
//      column leave the factor (zeros, a unit diagonal), so it takes no part in later columns; the m row becomes u
//   7. rss1 = rss0 - u'u, dof = kept columns, the chi^2_dof tail in closed form, and per kept candidate column j of
//      L_s^-1: beta_j = (L_s^-T u)_j, beta_se_j = sqrt(scale1 ||column j||^2)
#include "context_common.h"

namespace crm {

using namespace context_detail;

namespace {

// log Q(dof / 2, lrs / 2), the upper tail of chi^2_dof, by the finite sums (all terms positive: exact in the far tail)
//   dof even:  Q = e^-x sum_{i < dof / 2} x^i / i!
//   dof odd:   Q = erfc(sqrt x) + e^-x sum_{1 <= i <= (dof - 1) / 2} x^(i - 1/2) / Gamma(i + 1/2)
// x = lrs / 2; dof = 1 is log_sf with its three branches.
__device__ inline double log_chi2_sf(int dof, double lrs) {
    if (dof == 1) return log_sf(lrs);
    const double x = 0.5 * lrs;
    if ((dof & 1) == 0) {
        double t = 1.0, sum = 1.0;
        for (int i = 1; i < dof / 2; i++) {
            t *= x / (double)i;
            sum += t;
        }
        return log(sum) - x;
    }
    const double sx = sqrt(x);
    double t = sx * 1.1283791670955126;   // x^(1/2) / Gamma(3/2)
    double sum = t;
    for (int i = 1; i < (dof - 1) / 2; i++) {
        t *= x / ((double)i + 0.5);
        sum += t;
    }
    return log(erfcx(sx) + sum) - x;
}

__device__ inline int round16(int v) { return (v + 15) / 16 * 16; }

// Variant b of the launch described by `ja`.  MULTI: `ja` is one gene's record of a launch over several phenotypes.
template <bool MULTI>
__device__ __forceinline__ void context_joint_body(const ContextJointArgs& ja, const int b) {
    extern __shared__ __align__(16) double cj_smem[];
    const ContextLrtArgs& a = ja.base;
    const int tid = threadIdx.x;
    const int c = a.c, k = a.k;
    const int R = c + 2, Rp = round16(R), iy = c + 1, Kp = round16(k);
    const int zrows = (Rp > Kp ? Rp : Kp) + NG;
    double* const Hp = cj_smem;                          // packed L of [X0, g] with the y row
    double* const Sp = Hp + R * (R + 1) / 2;             // packed S (k rows), then L_s; row k: m, then u
    double* const zone = Sp + (k + 1) * (k + 2) / 2;     // [zrows][LS]; at the end the packed L_s^-1
    double* const red = zone + zrows * LS;               // [256]
    double* const xkx = red + 256;                       // [JOINT_MAX_K] x_j'K^-1x_j
    int* const kept = (int*)(xkx + CRM_JOINT_MAX_K);     // [JOINT_MAX_K]
    double* const scal = xkx + CRM_JOINT_MAX_K + CRM_JOINT_MAX_K / 2;   // [8]
    double* const Vs = ja.v_in_lds ? scal + 8 : ja.V + (long)b * ja.v_slab;   // [(c + 1) x k]
    const double n = (double)a.n;
    const double* __restrict__ tg = a.Tg + (long)b * a.ldTg;
    double* __restrict__ phi = a.phi + (long)b * a.ld_phi;
    const long ob = (long)b * k;

    const ContextNull nm = context_null_model(a, b, tg, phi, Hp, zone, red, scal);
    const double inv_d = 1.0 / nm.delta, lml0 = nm.lml0;
    const int P = nm.P;
    if (tid == 0) a.null_lml[b] = lml0;
    if (!nm.ok || !(lml0 == lml0) || P == c) {
        // no fit, or g itself in the span of X0: nothing is tested
        const bool nofit = !nm.ok || !(lml0 == lml0);
        for (int j = tid; j < k; j += 256) {
            a.beta[ob + j] = NAN;
            a.beta_se[ob + j] = NAN;
            ja.dropped[ob + j] = nofit ? 0 : 1;
        }
        if (tid == 0) {
            a.pvalue[b] = nofit ? NAN : 1.0 - EPS_TINY;
            a.logp[b] = nofit ? NAN : 0.0;
            a.alt_lml[b] = nofit ? NAN : lml0;
            a.status[b] = nofit ? CRM_CONTEXT_NO_FIT : CRM_CONTEXT_COLLINEAR;
            ja.dof[b] = 0;
        }
        return;
    }

    // 4. V and m, 32 candidates at a time
    const double* __restrict__ tx = a.Tx + (long)b * a.tx_slab;
    for (int j0 = 0; j0 < k; j0 += NG) {
        context_candidate_products(a, tg, phi, tx, j0, zone, nullptr);
        context_candidate_metric<MULTI>(a, b, j0, inv_d, zone);
        __syncthreads();
        const SolveSums sums = context_forward_solves(Hp, P, iy, zone);
        const int col = tid >> 3, j = j0 + col;
        if ((tid & 7) == 0 && j < k) Sp[tri(k, j)] = zone[iy * NG + col] - sums.vz;
        for (int e = tid; e < P * NG; e += 256) {
            const int u = e / NG, jj = e - u * NG;
            if (j0 + jj < k) Vs[u * k + j0 + jj] = zone[e];
        }
        __syncthreads();
    }

    // 5. X_c'K^-1X_c: per group of columns the rows from that group on
    const double* __restrict__ xxp = ja.xxp + (long)b * ja.ld_xxp;
    for (int j0 = 0; j0 < k; j0 += NG) {
        const int Rk = round16(k - j0);
        weighted_products(a.r, phi, Rk, zone,
                          [=](int u) -> const double* { return j0 + u < k ? tx + (long)(j0 + u) * a.ldT : nullptr; },
                          [=](int jj) -> const double* { return j0 + jj < k ? tx + (long)(j0 + jj) * a.ldT : nullptr; }, nullptr);
        for (int e = tid; e < Rk * NG; e += 256) {
            const int u = e / NG, jj = e - u * NG, i = j0 + u, j = j0 + jj;
            if (i >= k || j > i) continue;
            Sp[tri(i, j)] = xxp[tri(i, j)] * inv_d - zone[e];
        }
        __syncthreads();
    }
    //    S = X_c'K^-1X_c - V'V
    for (int e = tid; e < k * (k + 1) / 2; e += 256) {
        const int i = tri_row(e), j = e - tri(i, 0);
        double s = 0.0;
        for (int u = 0; u < P; u++) s += Vs[u * k + i] * Vs[u * k + j];
        const double full = Sp[e];
        if (i == j) xkx[i] = full;
        Sp[e] = full - s;
    }

    // 6. the factor of S in column order with the m row carried along
    int dof = 0;
    for (int j = 0; j < k; j++) {
        __syncthreads();
        if (tid == 0) {
            double d = Sp[tri(j, j)];
            for (int kk = 0; kk < j; kk++) d -= Sp[tri(j, kk)] * Sp[tri(j, kk)];
            scal[0] = d;
        }
        __syncthreads();
        const double d = scal[0];
        if (!(d > 1e-12 * xkx[j])) {
            // x_j in the span of [X0, g] and the candidates kept so far: out of the factor
            for (int i = j + 1 + tid; i <= k; i += 256) Sp[tri(i, j)] = 0.0;
            for (int kk = tid; kk < j; kk += 256) Sp[tri(j, kk)] = 0.0;
            if (tid == 0) {
                Sp[tri(j, j)] = 1.0;
                kept[j] = 0;
            }
            continue;
        }
        dof++;
        const double l = sqrt(d);
        for (int i = j + 1 + tid; i <= k; i += 256) {
            double s = Sp[tri(i, j)];
            for (int kk = 0; kk < j; kk++) s -= Sp[tri(i, kk)] * Sp[tri(j, kk)];
            Sp[tri(i, j)] = s / l;
        }
        if (tid == 0) {
            Sp[tri(j, j)] = l;
            kept[j] = 1;
        }
    }
    __syncthreads();

    // 7. the statistic, its tail, the coefficients
    if (dof == 0) {
        for (int j = tid; j < k; j += 256) {
            a.beta[ob + j] = NAN;
            a.beta_se[ob + j] = NAN;
            ja.dropped[ob + j] = 1;
        }
        if (tid == 0) {
            a.pvalue[b] = 1.0 - EPS_TINY;
            a.logp[b] = 0.0;
            a.alt_lml[b] = lml0;
            a.status[b] = CRM_CONTEXT_COLLINEAR;
            ja.dof[b] = 0;
        }
        return;
    }
    double uu = 0.0;
    for (int j = 0; j < k; j++) uu += Sp[tri(k, j)] * Sp[tri(k, j)];
    const double rss1 = nm.rss0 - uu;
    const double s1 = fmax(rss1 / n, EPS_SMALL);
    const double alt = -0.5 * (n * LOG2PI + n + n * log(s1) + nm.logdetK);
    double* const Li = zone;   // packed: column j of L_s^-1 at tri(i, j), i >= j
    bool finite = true;
    if (tid < k) {
        const int j = tid;
        double beta = NAN, se = NAN;
        if (kept[j]) {
            const double w0 = 1.0 / Sp[tri(j, j)];
            Li[tri(j, j)] = w0;
            beta = w0 * Sp[tri(k, j)];
            double nrm = w0 * w0;
            for (int i = j + 1; i < k; i++) {
                double s = 0.0;
                for (int kk = j; kk < i; kk++) s += Sp[tri(i, kk)] * Li[tri(kk, j)];
                const double w = -s / Sp[tri(i, i)];
                Li[tri(i, j)] = w;
                beta += w * Sp[tri(k, i)];
                nrm += w * w;
            }
            se = sqrt(s1 * nrm);
            finite = isfinite(beta) && isfinite(se);
        }
        a.beta[ob + j] = beta;
        a.beta_se[ob + j] = se;
        ja.dropped[ob + j] = kept[j] ? 0 : 1;
    }
    const int bad = __syncthreads_or(finite ? 0 : 1);
    if (tid == 0) {
        double lrs = -2.0 * lml0 + 2.0 * alt;     // (lrt_pvalues' statement and clips, with dof degrees of freedom)
        const double lp = log_chi2_sf(dof, lrs > 0.0 ? lrs : 0.0);
        if (lrs < DBL_TINY) lrs = DBL_TINY;
        double pv = dof == 1 ? erfc(sqrt(0.5 * lrs)) : exp(log_chi2_sf(dof, lrs));
        if (pv < DBL_TINY) pv = DBL_TINY;
        if (pv > 1.0 - EPS_TINY) pv = 1.0 - EPS_TINY;
        a.pvalue[b] = pv;
        a.logp[b] = lp;
        a.alt_lml[b] = alt;
        a.status[b] = (bad || !(isfinite(alt) && isfinite(lp))) ? CRM_CONTEXT_NON_FINITE : CRM_CONTEXT_OK;
        ja.dof[b] = dof;
    }
}

// (two workgroups per CU up to 80 KB of LDS: config 3's k = 50, c = 51 takes 69 KB with V in LDS; 115 VGPRs, nothing spilled)
__global__ __launch_bounds__(256, 2) void context_joint_kernel(ContextJointArgs ja) { context_joint_body<false>(ja, blockIdx.x); }

// Several phenotypes: workgroup (b, q) reads the record of gene q of the rho group and runs variant b on it
// (context_lrt_multi_kernel's scheme; a record's V row in global memory is indexed by its gene and the variant).
__global__ __launch_bounds__(256, 2) void context_joint_multi_kernel(const ContextJointArgs* __restrict__ genes) {
    const ContextJointArgs ja = genes[blockIdx.y];
    context_joint_body<true>(ja, blockIdx.x);
}

// CC[i, tri(a, b)] = E[i, a] E[i, b] for b <= a < k, zeros up to ld_out
__global__ void context_pairs_kernel(const double* __restrict__ E, long lde, long cells_pad, int k, double* __restrict__ CC,
                                     long ld_out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cells_pad * ld_out) return;
    const long i = e / ld_out;
    const int q = (int)(e - i * ld_out);
    double v = 0.0;
    if (q < k * (k + 1) / 2) {
        const int u = tri_row(q), w = q - tri(u, 0);
        v = E[i * lde + u] * E[i * lde + w];
    }
    CC[e] = v;
}

constexpr size_t LDS_PER_CU = 160 * 1024;

size_t joint_base_doubles(int c, int k) {
    const int R = c + 2, Rp = (R + 15) / 16 * 16, Kp = (k + 15) / 16 * 16;
    return (size_t)R * (R + 1) / 2 + (size_t)(k + 1) * (k + 2) / 2 + (size_t)(std::max(Rp, Kp) + NG) * LS + 256 +
           CRM_JOINT_MAX_K + CRM_JOINT_MAX_K / 2 + 8;
}

}  // namespace

bool context_joint_v_in_lds(int c, int k) {
    // beside the rest where that keeps two workgroups per CU, or where one workgroup per CU is all the rest allows anyway
    const size_t base = sizeof(double) * joint_base_doubles(c, k), with = base + sizeof(double) * (size_t)(c + 1) * k;
    return with <= LDS_PER_CU / 2 || (base > LDS_PER_CU / 2 && with <= LDS_PER_CU);
}

size_t context_joint_lds_bytes(int c, int k) {
    return sizeof(double) * (joint_base_doubles(c, k) + (context_joint_v_in_lds(c, k) ? (size_t)(c + 1) * k : 0));
}

int context_joint_check(int c, int k) {
    if (k < 1 || k > CRM_JOINT_MAX_K) {
        set_error("joint context test: %d contexts (supported 1..%d)", k, CRM_JOINT_MAX_K);
        return CRM_ERR_UNSUPPORTED;
    }
    if (c < 1 || c > CRM_MAX_COV_XWIDE) {
        set_error("joint context test: the covariates and contexts span %d columns (supported 1..%d)", c, CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    return CRM_OK;
}

int launch_context_joint(hipStream_t st, const ContextJointArgs& ja, int variants) {
    if (variants <= 0) return CRM_OK;
    const ContextLrtArgs& a = ja.base;
    CRM_TRY(context_joint_check(a.c, a.k));
    const bool in_lds = context_joint_v_in_lds(a.c, a.k);
    if (a.r < 0 || (ja.v_in_lds != 0) != in_lds || (!in_lds && (!ja.V || ja.v_slab < (long)(a.c + 1) * a.k))) {
        set_error("joint context test: the launch does not match the kernel's layout (r = %d)", a.r);
        return CRM_ERR_ARG;
    }
    const size_t lds = context_joint_lds_bytes(a.c, a.k);
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&context_joint_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(context_joint_kernel, dim3((unsigned)variants), dim3(256), lds, st, ja);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_context_joint_multi(hipStream_t st, const ContextJointArgs* genes_dev, int ngenes, int c, int k, bool v_global,
                               int variants) {
    if (variants <= 0 || ngenes <= 0) return CRM_OK;
    CRM_TRY(context_joint_check(c, k));
    if (!genes_dev || ngenes > 65535 || v_global == context_joint_v_in_lds(c, k)) {
        set_error("joint context test: the launch over %d genes does not match the kernel's layout", ngenes);
        return CRM_ERR_ARG;
    }
    const size_t lds = context_joint_lds_bytes(c, k);
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&context_joint_multi_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(context_joint_multi_kernel, dim3((unsigned)variants, (unsigned)ngenes), dim3(256), lds, st, genes_dev);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_context_pairs(hipStream_t st, const double* E, long lde, long cells_pad, int k, double* CC, long ld_out) {
    const long total = cells_pad * ld_out;
    if (total <= 0) return CRM_OK;
    hipLaunchKernelGGL(context_pairs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, E, lde, cells_pad, k, CC,
                       ld_out);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace crm
