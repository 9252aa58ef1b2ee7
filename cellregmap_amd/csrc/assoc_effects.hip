// Effect sizes of the association scans (C-ABI crm_scan_association_effects, crm_scan_association_multi_effects):
// per (phenotype, variant) one more evaluation of the ML profile of y ~ [W, g] at the variance ratio the scan settled on,
//   beta      = the g coefficient of (X'K^-1X)^-1 X'K^-1y,  X = [W, g],  K = (1 - delta) Sigma(rho*) + delta I
//   beta_se   = sqrt(scale / schur),  schur = g'K^-1g - g'K^-1W (W'K^-1W)^-1 W'K^-1g
//   alt_scale = (y'K^-1y - b'beta_hat) / n  (the ML scale, without the scan's floor)
//   alt_delta = delta: the null model's (fast), the optimum of the variant's own search (full refit)
//   log_pvalue = log erfc(sqrt(lrs / 2)),  lrs = max(2 (alt_lml - null_lml), 0), without a clip
// The reference keeps none of these (cellregmap/_cellregmap.py:276, :308-309 read the lml only); DESIGN.md section 11.
// The sums run over the rotated block T(rho*) the scan's own launches have just read, in the form of delta_search.h:
//   u'K^-1v = sum_k t_u[k] t_v[k] / ((1 - delta) S0[k] + delta) + (u'v - sum_k t_u[k] t_v[k]) / delta.
// Two kernels, one workgroup per test:
//   fast   delta is the gene's: its fastscan_prep record (L = chol(W'K^-1W), zy, the weights) is reused and only the
//          g column is new -- the statements of fastscan_kernel (assoc.hip) with the quotients kept
//   full   delta differs per variant: the Gram of [W, g, y] over the spectrum (tile_gram.h), packed Cholesky of the
//          [W, g] block, forward substitution of the y row; every width up to CRM_MAX_COV_XWIDE
#include "delta_search.h"
#include "objects.h"
#include "tile_gram.h"
#include "wave_ops.h"

namespace crm {

namespace {

constexpr int CMAX = CRM_MAX_COV_XWIDE;   // layout constant of the fastscan_prep record (assoc.hip)
constexpr int CHX = 32;                   // spectrum entries per staging step of the Gram

// log of the chi2_1 survival function at lrs >= 0: log erfc(x), x = sqrt(lrs / 2).  Near 1 through erf (erfc(x) rounds to
// 1 - O(eps) there and its log would lose every digit), below 1e-300 through the scaled complement, as tail_pvalue.hip
// does for one weight; both terms there are negative, nothing cancels.
__device__ inline double chi2_1_log_sf(double lrs) {
    const double h = 0.5 * lrs;
    const double x = sqrt(h);
    if (x < 0.5) return log1p(-erf(x));
    const double p = erfc(x);
    return p > 1e-300 ? log(p) : log(erfcx(x)) - h;
}

// the four block totals of a pair of partial sums: wave totals (wave_ops.h), then the four waves in ascending order
__device__ inline void block_sum2(double& a, double& b, double* red) {
    const int tid = threadIdx.x;
    a = wave_total(a);
    b = wave_total(b);
    __syncthreads();
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = a; red[2 * (tid >> 6) + 1] = b; }
    __syncthreads();
    a = (red[0] + red[2]) + (red[4] + red[6]);
    b = (red[1] + red[3]) + (red[5] + red[7]);
}

// thread 0: the record of test (gene, b).  in_span: the scan's rank rule dropped g; no_fit: the scan's alt lml is NaN.
__device__ inline void write_effect(const AssocEffectsGene& g, int b, double beta, double se, double delta, double scale,
                                    bool in_span, bool no_fit) {
    const double alt = g.alt_lml[b];
    double logp = NAN;
    if (alt == alt && g.null_lml == g.null_lml) {
        const double lrs = 2.0 * (alt - g.null_lml);
        logp = chi2_1_log_sf(lrs > 0.0 ? lrs : 0.0);
    }
    int status = CRM_EFFECT_OK;
    if (no_fit || !(alt == alt)) {
        status = CRM_EFFECT_NO_FIT;
        beta = se = NAN;
    } else if (in_span) {
        status = CRM_EFFECT_G_IN_SPAN_W;
        beta = se = NAN;
    } else if (!(isfinite(beta) && isfinite(se) && isfinite(delta) && isfinite(scale) && isfinite(logp))) {
        status = CRM_EFFECT_NON_FINITE;
    }
    if (g.out_beta) g.out_beta[b] = beta;
    if (g.out_se) g.out_se[b] = se;
    if (g.out_delta) g.out_delta[b] = delta;
    if (g.out_scale) g.out_scale[b] = scale;
    if (g.out_logp) g.out_logp[b] = logp;
    if (g.out_status) g.out_status[b] = status;
}

// Fast mode.  Test blockIdx.x = b ngenes + a: the genes of a variant are neighbours, so the T row they share (the genes of
// one rho group) is read from the cache by all but the first.
__global__ __launch_bounds__(256) void assoc_effects_fast_kernel(const AssocEffectsGene* __restrict__ genes, int ngenes) {
    __shared__ double red[8];
    __shared__ double hgW[CMAX];
    __shared__ double hsc[2];
    const int a = blockIdx.x % ngenes, b = blockIdx.x / ngenes;
    const AssocEffectsGene& g = genes[a];
    const int tid = threadIdx.x;
    const int c = g.c, r = g.r;
    const double inv_d = 1.0 / g.delta0;
    const double* __restrict__ tg = g.T + (long)b * g.t_sb;
    const long sk = g.t_sk;
    const double* __restrict__ wts = g.wts;
    for (int u = 0; u < c + 2; u++) {
        // u < c: W_u ; u == c: g ; u == c + 1: y
        const double* tu = u < c ? g.tW + (long)u * g.ldW : g.ty;
        double sw = 0.0, s1 = 0.0;
        for (int j = tid; j < r; j += 256) {
            const double t = tg[j * sk];
            const double p = t * (u == c ? t : tu[j]);
            sw += p * wts[j];
            s1 += p;
        }
        block_sum2(sw, s1, red);
        if (tid == 0) {
            double plain;
            if (u < c) plain = g.gW[(long)b * g.gW_sb + (long)u * g.gW_su];
            else if (u == c) plain = g.gg[b];
            else plain = g.gy[b];
            const double k = sw + (plain - s1) * inv_d;
            if (u < c) hgW[u] = k;
            else hsc[u - c] = k;
        }
    }
    if (tid == 0) {
        const double* prep = g.prep;
        const double* zy = prep + 8;
        const double* L = prep + 8 + CMAX;
        double zz = 0.0, zzy = 0.0;
        for (int i = 0; i < c; i++) {
            double s = hgW[i];
            for (int k = 0; k < i; k++) s -= L[i * CMAX + k] * hgW[k];   // (hgW[k], k < i: already z[k])
            s /= L[i * CMAX + i];
            hgW[i] = s;
            zz += s * s;
            zzy += s * zy[i];
        }
        const double schur = hsc[0] - zz;
        const double num = hsc[1] - zzy;
        const bool in_span = !(schur > 1e-12 * hsc[0]);   // fastscan_kernel's rule
        double rss = prep[0];
        if (!in_span) rss -= num * num / schur;
        const double scale = rss / (double)g.n;
        write_effect(g, b, num / schur, sqrt(scale / schur), g.delta0, scale, in_span, prep[3] == 0.0);
    }
}

// Full refit.  Rows of the Gram: W (0 .. c - 1), g (c), y (c + 1).
// LDS: S [16 TS][CHX + 1], sd [CHX], Hp [KT (KT + 1) / 2], scal [8], z [KT]
template <int TS>
__global__ __launch_bounds__(256) void assoc_effects_full_kernel(const AssocEffectsGene* __restrict__ genes, int ngenes) {
    extern __shared__ __align__(16) double esm[];
    const int a = blockIdx.x % ngenes, b = blockIdx.x / ngenes;
    const AssocEffectsGene& g = genes[a];
    const int tid = threadIdx.x;
    const int c = g.c, r = g.r, KT = c + 2;
    double* const S = esm;
    double* const sd = S + 16 * TS * (CHX + 1);
    double* const Hp = sd + CHX;
    double* const scal = Hp + KT * (KT + 1) / 2;
    double* const z = scal + 8;
    const NullFitTrial t = g.trial[b];
    const double delta = t.delta;
    if (!(t.lml == t.lml) || !(delta > 0.0) || !(delta <= 1.0)) {   // (the same for every thread)
        if (tid == 0) write_effect(g, b, NAN, NAN, delta, NAN, false, !(t.lml == t.lml));
        return;
    }
    const double inv_d = 1.0 / delta, omd = 1.0 - delta;
    const double* __restrict__ tg = g.T + (long)b * g.t_sb;
    const long sk = g.t_sk;
    auto value = [&](int row, int j) -> double {
        if (row < c) return g.tW[(long)row * g.ldW + j];
        if (row == c) return tg[j * sk];
        return g.ty[j];
    };
    auto plain = [&](int row, int col) -> double {   // col <= row
        if (row < c) return g.WW[col * c + row];
        if (row == c) return col < c ? g.gW[(long)b * g.gW_sb + (long)col * g.gW_su] : g.gg[b];
        return col < c ? g.Wy[col] : (col == c ? g.gy[b] : g.yy);
    };
    // complements (u'v - t_u't_v) / delta, then the weighted sums on top (every entry has one owner in both passes)
    gram_tiles<TS, CHX>(S, sd, nullptr, nullptr, KT, r, true, [&](int, int, double&) -> double { return 1.0; }, value,
                        [&](int row, int col, double v) {
                            if (col <= row) Hp[tri(row, col)] = (plain(row, col) - v) * inv_d;
                        });
    gram_tiles<TS, CHX>(S, sd, nullptr, nullptr, KT, r, true,
                        [&](int c0, int q, double&) -> double { return sqrt(1.0 / (omd * g.S0[c0 + q] + delta)); }, value,
                        [&](int row, int col, double v) {
                            if (col <= row) Hp[tri(row, col)] += v;
                        });
    __syncthreads();
    const bool use_g = t.use_g != 0;
    const int P = use_g ? c + 1 : c;
    double logdet;
    const bool ok = packed_cholesky(Hp, P, scal, logdet);
    __syncthreads();
    if (tid == 0) {
        if (!ok) {
            write_effect(g, b, INFINITY, INFINITY, delta, NAN, !use_g, false);   // (not positive definite: NON_FINITE)
        } else {
            // L z = X'K^-1y;  rss = y'K^-1y - z'z;  the last pivot is sqrt(schur), z_g = num / sqrt(schur)
            const int y = c + 1;
            double rss = Hp[tri(y, y)];
            for (int i = 0; i < P; i++) {
                double s = Hp[tri(y, i)];
                for (int k = 0; k < i; k++) s -= Hp[tri(i, k)] * z[k];
                s /= Hp[tri(i, i)];
                z[i] = s;
                rss -= s * s;
            }
            const double scale = rss / (double)g.n;
            double beta = NAN, se = NAN;
            if (use_g) {
                const double lg = Hp[tri(c, c)];
                beta = z[c] / lg;
                se = sqrt(scale) / lg;
            }
            write_effect(g, b, beta, se, delta, scale, !use_g, false);
        }
    }
}

__global__ void lrt_logp_kernel(const double* __restrict__ lrs, int count, double* __restrict__ logp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double x = lrs[i];
    logp[i] = x == x ? chi2_1_log_sf(x > 0.0 ? x : 0.0) : NAN;
}

size_t full_lds(int c, int ts) {
    const size_t KT = (size_t)c + 2;
    return sizeof(double) * ((size_t)16 * ts * (CHX + 1) + CHX + KT * (KT + 1) / 2 + 8 + KT);
}

template <int TS>
int launch_full(hipStream_t st, const AssocEffectsGene* genes_dev, int ngenes, int variants, int c) {
    const size_t lds = full_lds(c, TS);
    // (only past the 64 KB a launch may take as it is -- 95 columns and more; the attribute is kept per device, so it is
    // asked for with the launch that needs it, not remembered in a flag that a second device would find set)
    if (lds > 64 * 1024)
        CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&assoc_effects_full_kernel<TS>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(assoc_effects_full_kernel<TS>, dim3((unsigned)variants * ngenes), dim3(256), lds, st, genes_dev, ngenes);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace

int launch_assoc_effects(hipStream_t st, const AssocEffectsGene* genes_dev, int ngenes, int variants, int c, bool fast) {
    if (ngenes <= 0 || variants <= 0) return CRM_OK;
    if (c > CMAX) {
        set_error("association effects: %d covariate columns (supported up to %d)", c, CMAX);
        return CRM_ERR_UNSUPPORTED;
    }
    if (fast) {
        hipLaunchKernelGGL(assoc_effects_fast_kernel, dim3((unsigned)variants * ngenes), dim3(256), 0, st, genes_dev, ngenes);
        CRM_HIP(hipGetLastError());
        return CRM_OK;
    }
    const int ts = (c + 2 + 15) / 16;
    if (ts <= 2) return launch_full<2>(st, genes_dev, ngenes, variants, c);
    if (ts <= 4) return launch_full<4>(st, genes_dev, ngenes, variants, c);
    if (ts <= 6) return launch_full<6>(st, genes_dev, ngenes, variants, c);
    return launch_full<9>(st, genes_dev, ngenes, variants, c);
}

int launch_lrt_logp(hipStream_t st, const double* lrs, int count, double* logp) {
    if (count <= 0) return CRM_OK;
    hipLaunchKernelGGL(lrt_logp_kernel, dim3((count + 255) / 256), dim3(256), 0, st, lrs, count, logp);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace crm
