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
#include "delta_search.h"
#include "objects.h"
#include "tile_gram.h"

namespace crm {

namespace {

constexpr double DBL_TINY = 2.2250738585072014e-308;   // numpy_sugar.epsilon.super_tiny
constexpr int NG = 32;        // candidates per group (two 16-column MFMA tiles)
constexpr int CH = 32;        // spectrum entries per staging step
constexpr int LS = CH + 1;    // LDS row stride of the staged chunks
constexpr int RTW = 3;        // 16-row tiles per wavefront: 4 x 3 x 16 = 192 >= CRM_MAX_COV_XWIDE + 2

typedef double cl_v4d __attribute__((ext_vector_type(4)));

// as assoc_effects.hip states it: log erfc(sqrt(lrs / 2)) without a clip
__device__ inline double log_sf(double lrs) {
    const double h = 0.5 * lrs;
    const double x = sqrt(h);
    if (x < 0.5) return log1p(-erf(x));
    const double p = erfc(x);
    return p > 1e-300 ? log(p) : log(erfcx(x)) - h;
}

__device__ inline double block_total(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

// Pt[u][jj] = sum_s phi_s U_u[s] V_jj[s] for the R rows U = [tX; tg; ty] and the NG columns col(jj) (null: a column of
// zeros); dacc (may be null): this thread's four partial sums of phi_s V_jj[s]^2, jj = tid / 32 + 8 i, over s = tid % 32 + 32 t.
// zone: [Rp + NG][LS] while the chunks are staged, then Pt [Rp][NG] over the same memory.  Ends with a barrier.
template <class Col>
__device__ __forceinline__ void weighted_products(const ContextLrtArgs& a, const double* __restrict__ tg,
                                                  const double* __restrict__ phi, int R, int Rp, double* zone, Col&& col,
                                                  double* dacc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int r = a.r, c = a.c, RT = Rp / 16;
    double* const Us = zone;
    double* const Vs = zone + Rp * LS;
    cl_v4d acc[RTW][2];
#pragma unroll
    for (int t = 0; t < RTW; t++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++) acc[t][ct] = (cl_v4d){0.0, 0.0, 0.0, 0.0};
    const double* vcol[4];
#pragma unroll
    for (int i = 0; i < 4; i++) vcol[i] = col((tid >> 5) + 8 * i);
    const int q = tid & 31;
    for (int s0 = 0; s0 < r; s0 += CH) {
        const int s = s0 + q;
        const bool in = s < r;
        const double ph = in ? phi[s] : 0.0;
        for (int row = tid >> 5; row < Rp; row += 8) {
            double v = 0.0;
            if (in && row < R) {
                const double* src = row < c ? a.tX + (long)row * a.ldW : (row == c ? tg : a.ty);
                v = src[s] * ph;
            }
            Us[row * LS + q] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double v = (in && vcol[i]) ? vcol[i][s] : 0.0;
            Vs[((tid >> 5) + 8 * i) * LS + q] = v;
            if (dacc) dacc[i] += ph * v * v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CH / 4; kk++) {
            const double b0 = Vs[l15 * LS + kk * 4 + lq];
            const double b1 = Vs[(16 + l15) * LS + kk * 4 + lq];
#pragma unroll
            for (int t = 0; t < RTW; t++) {
                const int rt = wave + 4 * t;
                if (rt < RT) {
                    const double av = Us[(rt * 16 + l15) * LS + kk * 4 + lq];
                    acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc[t][0], 0, 0, 0);
                    acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc[t][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // accumulator register `reg` of lane (l15, lq): row lq + 4 reg of the A tile, column l15 of the B tile
    double* const Pt = zone;
#pragma unroll
    for (int t = 0; t < RTW; t++) {
        const int rt = wave + 4 * t;
        if (rt < RT) {
#pragma unroll
            for (int ct = 0; ct < 2; ct++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) Pt[(rt * 16 + lq + 4 * reg) * NG + ct * 16 + l15] = acc[t][ct][reg];
        }
    }
    __syncthreads();
}

// (two workgroups per CU where the LDS allows it -- up to about 90 covariate columns: 233 VGPRs, nothing spilled)
__global__ __launch_bounds__(256, 2) void context_lrt_kernel(ContextLrtArgs a) {
    extern __shared__ __align__(16) double cl_smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int c = a.c, k = a.k, r = a.r;
    const int R = c + 2, Rp = (R + 15) / 16 * 16, iy = c + 1;
    double* const Hp = cl_smem;                          // packed lower triangle of the (c + 2)^2 Gram, then L with the y row
    double* const zone = Hp + R * (R + 1) / 2;           // [Rp + NG][LS]
    double* const red = zone + (Rp + NG) * LS;           // [NG * CH]
    double* const diag = red + NG * CH;                  // [NG]
    double* const scal = diag + NG;                      // [8]
    const double delta = a.delta[b], inv_d = 1.0 / delta, omd = 1.0 - delta;
    const double n = (double)a.n;
    const double* __restrict__ tg = a.Tg + (long)b * a.ldTg;
    double* __restrict__ phi = a.phi + (long)b * a.ld_phi;

    // 1. the weights and log|K|
    double lpart = 0.0;
    for (int s = tid; s < r; s += 256) {
        const double S = a.S0[s], D = omd * S + delta;
        phi[s] = omd * S / (delta * D);
        lpart += log(D);
    }
    const double logdetK = block_total(lpart, red) + (n - (double)r) * log(delta);   // (its barriers publish phi)

    // 2. the Gram of [tX; tg; ty], 32 columns at a time
    for (int v0 = 0; v0 < R; v0 += NG) {
        weighted_products(a, tg, phi, R, Rp, zone,
                          [&](int jj) -> const double* {
                              const int v = v0 + jj;
                              return v < c ? a.tX + (long)v * a.ldW : (v == c ? tg : (v == iy ? a.ty : nullptr));
                          },
                          nullptr);
        for (int e = tid; e < R * NG; e += 256) {
            const int u = e / NG, jj = e - u * NG, v = v0 + jj;
            if (v > u || v >= R) continue;
            double plain;
            if (u < c) plain = a.WW[u * c + v];
            else if (u == c) plain = v < c ? a.gW[(long)b * a.ld_gW + v] : a.gg[b];
            else plain = v < c ? a.Wy[v] : (v == c ? a.gy[b] : a.yy);
            Hp[tri(u, v)] = plain * inv_d - zone[u * NG + jj];
        }
        __syncthreads();
    }

    // 3. Cholesky over [X0, g] with the y row carried along (its entries become z)
    const double gKg = Hp[tri(c, c)];
    const bool dropped_before = a.drop && a.drop[b] != 0;
    bool ok = true;
    int P = c + 1;
    for (int j = 0; j <= c; j++) {
        __syncthreads();
        if (tid == 0) {
            double d = Hp[tri(j, j)];
            for (int kk = 0; kk < j; kk++) d -= Hp[tri(j, kk)] * Hp[tri(j, kk)];
            scal[0] = d;
        }
        __syncthreads();
        const double d = scal[0];
        if (j == c) {
            // g in the span of X0: the rank rule of fastscan_kernel (assoc.hip), or the scan's own (full refit)
            if (dropped_before || !(d > 1e-12 * gKg)) { P = c; break; }
        } else if (!(d > 0.0)) {
            ok = false;
            break;
        }
        const double l = sqrt(d);
        for (int i = j + 1 + tid; i < R; i += 256) {
            double s = Hp[tri(i, j)];
            for (int kk = 0; kk < j; kk++) s -= Hp[tri(i, kk)] * Hp[tri(j, kk)];
            Hp[tri(i, j)] = s / l;
        }
        if (tid == 0) Hp[tri(j, j)] = l;
    }
    __syncthreads();
    double rss0 = Hp[tri(iy, iy)];
    for (int kk = 0; kk < P; kk++) rss0 -= Hp[tri(iy, kk)] * Hp[tri(iy, kk)];
    const double s_null = fmax(rss0 / n, EPS_SMALL);
    const double lml0 = ok ? -0.5 * (n * LOG2PI + n + n * log(s_null) + logdetK) : NAN;
    if (tid == 0) a.null_lml[b] = lml0;

    // 4. the candidates
    const double* __restrict__ tx = a.Tx + (long)b * a.tx_slab;
    for (int j0 = 0; j0 < k; j0 += NG) {
        double dacc[4] = {0.0, 0.0, 0.0, 0.0};
        weighted_products(a, tg, phi, R, Rp, zone,
                          [&](int jj) -> const double* { return j0 + jj < k ? tx + (long)(j0 + jj) * a.ldT : nullptr; }, dacc);
#pragma unroll
        for (int i = 0; i < 4; i++) red[((tid >> 5) + 8 * i) * CH + (tid & 31)] = dacc[i];
        __syncthreads();
        if (tid < NG) {
            double s = 0.0;
            for (int qq = 0; qq < CH; qq++) s += red[tid * CH + qq];
            diag[tid] = s;
        }
        // X'K^-1x_j and y'K^-1x_j in place
        for (int e = tid; e < R * NG; e += 256) {
            const int u = e / NG, jj = e - u * NG, j = j0 + jj;
            if (j >= k) continue;
            const double* row = a.xXy + ((long)b * k + j) * a.ld_xXy;
            const double plain = u < c ? row[1 + u] : (u == c ? a.xg[(long)b * a.ld_xg + j] : row[0]);
            zone[u * NG + jj] = plain * inv_d - zone[u * NG + jj];
        }
        __syncthreads();
        // forward solves: eight lanes per candidate share the dot product of a row
        const int col = tid >> 3, part = tid & 7;
        double vv = 0.0, vz = 0.0;
        for (int i = 0; i < P; i++) {
            double s = 0.0;
            for (int kk = part; kk < i; kk += 8) s += Hp[tri(i, kk)] * zone[kk * NG + col];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            const double v = (zone[i * NG + col] - s) / Hp[tri(i, i)];
            if (part == 0) zone[i * NG + col] = v;   // (read again by the same eight lanes only: one wavefront, in order)
            __syncthreads();
            vv += v * v;
            vz += v * Hp[tri(iy, i)];
        }
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
