// What the two kernels of the fixed-effect GxC tests share (context_lrt.hip: k tests of one degree of freedom, DESIGN.md
// section 12; context_joint.hip: one test of k degrees of freedom, section 13; both over one phenotype per launch or over
// the genes of a rho group, section 14): the staging and MFMA scheme of the products
// in the phi metric, and the null model of a variant -- phi, log|K|, the Gram of [tX; tg; ty] and its Cholesky factor with
// the y row carried along.  One statement of each, so that the two calls report the same null bit for bit.
#pragma once
#include "delta_search.h"
#include "objects.h"
#include "tile_gram.h"

namespace crm {
namespace context_detail {

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

// Pt[u][jj] = sum_s phi_s U_u[s] V_jj[s] over the spectrum of r entries, for the rows U_u = row(u), u < Rp (null: a row of
// zeros) and the NG columns col(jj) (null: a column of zeros); dacc (may be null): this thread's four partial sums of
// phi_s V_jj[s]^2, jj = tid / 32 + 8 i, over s = tid % 32 + 32 t.
// zone: [Rp + NG][LS] while the chunks are staged, then Pt [Rp][NG] over the same memory.  Ends with a barrier.
template <class Row, class Col>
__device__ __forceinline__ void weighted_products(int r, const double* __restrict__ phi, int Rp, double* zone, const Row row,
                                                  const Col col, double* dacc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int RT = Rp / 16;
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
        for (int u = tid >> 5; u < Rp; u += 8) {
            double v = 0.0;
            if (in) {
                const double* src = row(u);
                if (src) v = src[s] * ph;
            }
            Us[u * LS + q] = v;
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

// row u of [tX; tg; ty] (u < c + 2), null beyond
struct BaseRows {
    const double* tX; long ldW; const double* tg; const double* ty; int c;
    __device__ __forceinline__ const double* operator()(int u) const {
        return u < c ? tX + (long)u * ldW : (u == c ? tg : (u == c + 1 ? ty : nullptr));
    }
};

// The null model of variant b at delta[b]: X = [X0, g_b] of P columns (P = c: g_b in the span of X0).
struct ContextNull {
    double delta, logdetK, rss0, lml0;
    int P;
    bool ok;      // false: X0'K^-1X0 is not positive definite
};

// Steps 1 to 3 of both kernels.  phi: the variant's scratch row (written); Hp: the packed lower triangle of the
// (c + 2)^2 Gram, left holding L with the y row (z) below it; zone: [Rp + NG][LS]; red: [256]; scal: [1].
__device__ __forceinline__ ContextNull context_null_model(const ContextLrtArgs& a, int b, const double* __restrict__ tg,
                                                          double* __restrict__ phi, double* Hp, double* zone, double* red,
                                                          double* scal) {
    const int tid = threadIdx.x;
    const int c = a.c, r = a.r;
    const int R = c + 2, Rp = (R + 15) / 16 * 16, iy = c + 1;
    const double delta = a.delta[b], inv_d = 1.0 / delta, omd = 1.0 - delta;
    const double n = (double)a.n, yy = a.yy;
    const BaseRows rows{a.tX, a.ldW, tg, a.ty, c};

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
        weighted_products(r, phi, Rp, zone, rows, [=](int jj) -> const double* { return rows(v0 + jj); }, nullptr);
        for (int e = tid; e < R * NG; e += 256) {
            const int u = e / NG, jj = e - u * NG, v = v0 + jj;
            if (v > u || v >= R) continue;
            double plain;
            if (u < c) plain = a.WW[u * c + v];
            else if (u == c) plain = v < c ? a.gW[(long)b * a.ld_gW + v] : a.gg[b];
            else if (v < c) plain = a.Wy[v];
            else plain = v == c ? a.gy[b] : yy;
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
    return ContextNull{delta, logdetK, rss0, lml0, P, ok};
}

// The (c + 2) x NG weighted products of [tX; tg; ty] with the rotated candidates j0 .. j0 + NG - 1 (tx: the variant's slab
// of T_x), left in zone[u NG + jj]; dacc as weighted_products takes it.
__device__ __forceinline__ void context_candidate_products(const ContextLrtArgs& a, const double* __restrict__ tg,
                                                           const double* __restrict__ phi, const double* __restrict__ tx,
                                                           int j0, double* zone, double* dacc) {
    const int c = a.c, k = a.k, R = c + 2, Rp = (R + 15) / 16 * 16;
    weighted_products(a.r, phi, Rp, zone, BaseRows{a.tX, a.ldW, tg, a.ty, c},
                      [=](int jj) -> const double* { return j0 + jj < k ? tx + (long)(j0 + jj) * a.ldT : nullptr; }, dacc);
}

// X'K^-1x_j and y'K^-1x_j from the weighted products in zone and the plain tables, in place.  No barrier.
// MULTI (a launch over several phenotypes): x_j'X0 from the shared table, x_j'y from the gene's own.
template <bool MULTI>
__device__ __forceinline__ void context_candidate_metric(const ContextLrtArgs& a, int b, int j0, double inv_d, double* zone) {
    const int c = a.c, k = a.k, R = c + 2;
    for (int e = threadIdx.x; e < R * NG; e += 256) {
        const int u = e / NG, jj = e - u * NG, j = j0 + jj;
        if (j >= k) continue;
        const double* row = a.xXy + ((long)b * k + j) * a.ld_xXy;
        double plain;
        if (MULTI) plain = u < c ? row[u] : (u == c ? a.xg[(long)b * a.ld_xg + j] : a.xy[((long)b * k + j) * a.ld_xy]);
        else plain = u < c ? row[1 + u] : (u == c ? a.xg[(long)b * a.ld_xg + j] : row[0]);
        zone[u * NG + jj] = plain * inv_d - zone[u * NG + jj];
    }
}

// Forward solves of the NG staged candidates against L (P columns): zone[i NG + col] becomes v = L^-1 X'K^-1x for i < P.
// Eight lanes per candidate share the dot product of a row; vv = v'v and vz = v'z of this thread's candidate tid / 8.
struct SolveSums { double vv, vz; };
__device__ __forceinline__ SolveSums context_forward_solves(const double* Hp, int P, int iy, double* zone) {
    const int tid = threadIdx.x;
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
    return SolveSums{vv, vz};
}

}  // namespace context_detail
}  // namespace crm
