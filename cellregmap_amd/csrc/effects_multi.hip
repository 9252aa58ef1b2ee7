// Batched effect sizes (estimate_betas, cellregmap/_cellregmap.py:137-205) for many (phenotype, variant) pairs through the
// rank-k0 (Woodbury) form of the per-SNP covariance:
//
//   Sigma_p(rho) = rho U U' + (1 - rho) L L',   U = g o E0 (n x k0),   L L' = Q_L S_L Q_L' (one decomposition per call)
//   D(delta)     = (1 - delta) Sigma_p + delta I = N + (1 - delta) rho U U',   N = delta I + a Q_L S_L Q_L',
//   a = (1 - delta)(1 - rho),  w_j = 1 / (delta + a S_L[j]),  t_u = Q_L'u,  c(u, v) = u'v - t_u't_v:
//     u'N^-1 v = sum_j w_j t_u[j] t_v[j] + c(u, v) / delta
//     C        = I / ((1 - delta) rho) + U'N^-1 U                    (k0 x k0)
//     u'D^-1 v = u'N^-1 v - (U'N^-1 u)' C^-1 (U'N^-1 v)
//     log|D|   = sum_j log(delta + a S_L[j]) + (n - r_L) log delta + log|C| + k0 log((1 - delta) rho)
//
// No per-SNP eigen-solve and no per-SNP rotation against an 11-point grid: the n-length work is Q_L'[W, E0] per call,
// Q_L'y per phenotype, Q_L'g and Q_L'(g o E0) per variant (the scan's contraction kernels, gemm_tn.hip), and the complement
// numerators of Z = [W, g, E0, y, U] per pair.  Then one 256-thread workgroup per (pair, grid point) runs the reference's
// search (brent_search.h on delta_search.h's memoised objective, the noise bound never asked for) on the REML objective of
// oracle/lmm.py evaluated through the form above: Grams by tile_gram.h's gram_tiles, 32 positions per staging step, the
// complement numerators in global memory and the packed systems (tile_gram.h: packed_cholesky) in LDS.  A last kernel takes
// the strict `>` over the grid and forms beta and the BLUP coefficients u = U'K^-1 (y - M beta) at the chosen point.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "delta_search.h"
#include "objects.h"
#include "tile_gram.h"

using namespace crm;

namespace {

constexpr int CHX = 32;          // spectrum entries (or cells) per staging step
constexpr int EKT_MAX = 130;     // columns of Z = [W, g, E0, y, U]: c_W + 2 k0 + 2 <= 130
constexpr int VARIANT_BLOCK = 64;    // distinct variants per rotation block (bounds the Q_L'(g o E0) workspace)
constexpr int PAIR_CHUNK = 2048;     // pairs per launch (bounds the complement numerators: KT^2 doubles each)

struct EffTrial {
    double lml, delta, scale;
    int nfev, pad;
};

struct EffArgs {
    // rotations: rows over the spectrum of L L' (leading dimension ldq); r = 0 (mode A): none are read
    const double* TXE;   // [(cW + k0) x ldq]: Q_L'W_i, then Q_L'E0_j
    const double* TY;    // [ny x ldq]: Q_L'y_p
    const double* TG;    // [vb x ldq]: Q_L'g_b, variants of the block
    const double* TU;    // [(vb k0) x ldq]: row b k0 + j = Q_L'(g_b o E0_j)
    const double* S;     // [r]: S_L
    long ldq;
    int r;
    // the same columns in the cell axis (row-major, rows past n are zero)
    const double* XE; long ldxe;   // [n_pad x ldxe]: W | E0
    const double* Yd; long ldy;    // [n_pad x ldy]
    const double* Gd; long ldg;    // [n_pad x ldg]: variants of the block
    long n;
    int cW, k0;
    const int* pv;   // [pairs]: variant of the pair (column of the block)
    const int* pp;   // [pairs]: phenotype of the pair (column of Yd)
    int nrho;
    double rho[CRM_MAX_RHO];
    double* Cp;      // [pairs][KT x KT]: complement numerators c(u, v)
    double* PX;      // [pairs][P x P]: plain X'X, X = [W, g, E0]
    EffTrial* trial; // [pairs x nrho]
    double* fit;     // [pairs x 6]: rho, v0, v1, lml, delta, grid index
    double* beta;    // [pairs x P]
    double* u;       // [pairs x k0]
};

// Column z of Z = [W (cW), g, E0 (k0), y, U (k0)] for the pair (v, p): its spectrum row and its entry at cell i.
struct ZCols {
    const EffArgs& a;
    int v, p, P;
    __device__ inline const double* trow(int z) const {
        if (z < a.cW) return a.TXE + (long)z * a.ldq;
        if (z == a.cW) return a.TG + (long)v * a.ldq;
        if (z < P) return a.TXE + (long)(z - 1) * a.ldq;
        if (z == P) return a.TY + (long)p * a.ldq;
        return a.TU + ((long)v * a.k0 + (z - P - 1)) * a.ldq;
    }
    __device__ inline double cell(int z, long i) const {
        if (z < a.cW) return a.XE[i * a.ldxe + z];
        if (z == a.cW) return a.Gd[i * a.ldg + v];
        if (z < P) return a.XE[i * a.ldxe + (z - 1)];
        if (z == P) return a.Yd[i * a.ldy + p];
        return a.Gd[i * a.ldg + v] * a.XE[i * a.ldxe + a.cW + (z - P - 1)];
    }
};

// Complement numerators c(u, v) = u'v - t_u't_v of Z and the plain X'X, once per pair (they depend on neither delta nor rho).
template <int TS>
__global__ __launch_bounds__(256) void effects_numerators_kernel(EffArgs a) {
    extern __shared__ __align__(16) double esm[];
    const int b = blockIdx.x;
    const int P = a.cW + 1 + a.k0, KT = P + 1 + a.k0;
    const ZCols z{a, a.pv[b], a.pp[b], P};
    double* const S = esm;
    double* const sd = S + 16 * TS * (CHX + 1);
    double* const Cp = a.Cp + (size_t)b * KT * KT;
    double* const PX = a.PX + (size_t)b * P * P;
    auto one = [&](long, int, double&) -> double { return 1.0; };
    gram_tiles<TS, CHX>(S, sd, nullptr, nullptr, KT, a.n, false, one, [&](int row, long i) { return z.cell(row, i); },
                   [&](int row, int col, double v) {
                       Cp[(size_t)row * KT + col] = v;
                       if (row < P && col < P) PX[(size_t)row * P + col] = v;
                   });
    __threadfence();
    __syncthreads();
    // (entries written above by this thread only: each (row, col) has one owner in both passes)
    gram_tiles<TS, CHX>(S, sd, nullptr, nullptr, KT, (long)a.r, true, one, [&](int row, long j) { return z.trow(row)[j]; },
                   [&](int row, int col, double v) { Cp[(size_t)row * KT + col] -= v; });
}

// BLUP = false: one workgroup per (pair, grid point) runs the search and writes its trial record.
// BLUP = true: one workgroup per pair takes the best grid point (strict >, first wins) and forms beta and u there.
template <int TS, bool BLUP>
__global__ __launch_bounds__(256) void effects_fit_kernel(EffArgs a) {
    extern __shared__ __align__(16) double esm[];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int cW = a.cW, k0 = a.k0;
    const int P = cW + 1 + k0, KT = P + 1 + k0, P1 = P + 1;
    const ZCols z{a, a.pv[b], a.pp[b], P};
    const double n = (double)a.n;
    const int r = a.r;
    // LDS: S [16 TS][CHX + 1], sd [CHX], Hp [P1 (P1 + 1) / 2], Cc [k0 (k0 + 1) / 2], Bm [k0 x P1], red [256], scal [8],
    //      vec [P + k0]
    double* const S = esm;
    double* const sd = S + 16 * TS * (CHX + 1);
    double* const Hp = sd + CHX;
    double* const Cc = Hp + (size_t)P1 * (P1 + 1) / 2;
    double* const Bm = Cc + (size_t)k0 * (k0 + 1) / 2;
    double* const red = Bm + (size_t)k0 * P1;
    double* const scal = red + 256;
    double* const vec = scal + 8;
    const double* const Cp = a.Cp + (size_t)b * KT * KT;

    int w;
    if constexpr (BLUP) {
        w = -1;
        double best = -INFINITY;
        for (int i = 0; i < a.nrho; i++) {
            const double l = a.trial[(size_t)b * a.nrho + i].lml;
            if (l > best) { best = l; w = i; }
        }
        if (w < 0) {
            if (tid == 0) {
                double* f = a.fit + (size_t)b * 6;
                f[0] = f[1] = f[2] = f[3] = f[4] = NAN;
                f[5] = -1.0;
                for (int i = 0; i < P; i++) a.beta[(size_t)b * P + i] = NAN;
                for (int i = 0; i < k0; i++) a.u[(size_t)b * k0 + i] = NAN;
            }
            return;
        }
    } else {
        w = blockIdx.y;
    }
    const double rho = a.rho[w];
    const bool woodbury = rho > 0.0;

    // log|X'X| (plain Gram; the reference's slogdet of its SVD basis differs by a basis-independent amount that cancels
    // against the same change of log|X'K^-1X|)
    const double* PX = a.PX + (size_t)b * P * P;
    for (int e = tid; e < P * (P + 1) / 2; e += 256) {
        const int i = tri_row(e);
        Hp[e] = PX[(size_t)i * P + (e - tri(i, 0))];
    }
    double logdetXX;
    if (!packed_cholesky(Hp, P, scal, logdetXX)) logdetXX = NAN;
    __syncthreads();
    const double df = n - (double)P;

    // evaluation at delta: lml and scale; with want_blup also beta (vec[0..P)) and U'D^-1 r (vec[P..P + k0))
    auto evaluate = [&](double delta, bool want_blup) -> DeltaValue {
        DeltaValue out{false, NAN, NAN, NAN};
        const double omd = 1.0 - delta;
        const double aa = omd * (1.0 - rho);
        const double inv_d = 1.0 / delta;
        const double cdiag = woodbury ? 1.0 / (omd * rho) : 0.0;
        const double lsum = gram_tiles<TS, CHX>(
            S, sd, red, scal, KT, (long)r, true,
            [&](long c0, int q, double& lpart) {
                const double D = delta + aa * a.S[c0 + q];
                lpart += log(D);
                return sqrt(1.0 / D);
            },
            [&](int row, long j) { return z.trow(row)[j]; },
            [&](int row, int col, double v) {
                const double k = v + Cp[(size_t)row * KT + col] * inv_d;   // u'N^-1 v
                if (row < P1) {
                    if (col <= row) Hp[tri(row, col)] = k;
                } else if (col < P1) {
                    if (woodbury || want_blup) Bm[(row - P1) * P1 + col] = k;
                } else if (woodbury && col <= row) {
                    Cc[tri(row - P1, col - P1)] = k + (row == col ? cdiag : 0.0);
                }
            });
        double logdetD = lsum + (n - (double)r) * log(delta);
        if (woodbury) {
            double logdetC;
            if (!packed_cholesky(Cc, k0, scal, logdetC)) return out;
            logdetD += logdetC + (double)k0 * log(omd * rho);
            // Z = Lc^-1 U'N^-1 [X, y], column by column
            for (int col = tid; col < P1; col += 256) {
                for (int i = 0; i < k0; i++) {
                    double s = Bm[i * P1 + col];
                    for (int q = 0; q < i; q++) s -= Cc[tri(i, q)] * Bm[q * P1 + col];
                    Bm[i * P1 + col] = s / Cc[tri(i, i)];
                }
            }
            __syncthreads();
            // [X, y]'D^-1[X, y] = [X, y]'N^-1[X, y] - Z'Z
            for (int e = tid; e < P1 * (P1 + 1) / 2; e += 256) {
                const int i = tri_row(e);
                const int k = e - tri(i, 0);
                double s = 0.0;
                for (int q = 0; q < k0; q++) s += Bm[q * P1 + i] * Bm[q * P1 + k];
                Hp[e] -= s;
            }
            __syncthreads();
        }
        double logdetH;
        if (!packed_cholesky(Hp, P, scal, logdetH)) return out;
        if (tid == 0) {
            // rss = y'D^-1y - z'z with L z = X'D^-1y (forward substitution)
            double rss = Hp[tri(P, P)];
            for (int i = 0; i < P; i++) {
                double s = Hp[tri(P, i)];
                for (int k = 0; k < i; k++) s -= Hp[tri(i, k)] * red[k];
                s /= Hp[tri(i, i)];
                red[i] = s;
                rss -= s * s;
            }
            scal[2] = rss;
            if (want_blup) {
                for (int i = P - 1; i >= 0; i--) {
                    double t = red[i];
                    for (int k = i + 1; k < P; k++) t -= Hp[tri(k, i)] * vec[k];
                    vec[i] = t / Hp[tri(i, i)];
                }
                // U'D^-1 r, r = y - X beta: rho > 0: C^-1 (U'N^-1 r) / ((1 - delta) rho) = Lc^-T (Z_y - Z_X beta) / (...);
                // rho = 0: U'N^-1 r itself
                double* const t = vec + P;
                for (int i = 0; i < k0; i++) {
                    double s = Bm[i * P1 + P];
                    for (int k = 0; k < P; k++) s -= Bm[i * P1 + k] * vec[k];
                    t[i] = s;
                }
                if (woodbury) {
                    for (int i = k0 - 1; i >= 0; i--) {
                        double s = t[i];
                        for (int q = i + 1; q < k0; q++) s -= Cc[tri(q, i)] * t[q];
                        t[i] = s / Cc[tri(i, i)];
                    }
                    for (int i = 0; i < k0; i++) t[i] *= cdiag;
                }
            }
        }
        __syncthreads();
        const double rss = scal[2];
        const double s = fmax(rss / df, EPS_SMALL);
        double val = -0.5 * (df * LOG2PI + df + n * log(s) + logdetD);
        val += 0.5 * (logdetXX - (logdetH - (double)P * log(s)));
        out.ok = true;
        out.scale = s;
        out.lml = val;
        __syncthreads();
        return out;
    };

    if constexpr (BLUP) {
        const EffTrial t = a.trial[(size_t)b * a.nrho + w];
        (void)evaluate(t.delta, true);
        if (tid == 0) {
            double* f = a.fit + (size_t)b * 6;
            f[0] = rho;
            f[1] = t.scale * (1.0 - t.delta);
            f[2] = t.scale * t.delta;
            f[3] = t.lml;
            f[4] = t.delta;
            f[5] = (double)w;
            for (int i = 0; i < P; i++) a.beta[(size_t)b * P + i] = vec[i];
            for (int i = 0; i < k0; i++) a.u[(size_t)b * k0 + i] = vec[P + i] / t.scale;
        }
    } else {
        auto eval = [&](double delta, bool) -> DeltaValue { return evaluate(delta, false); };
        OutOfLineObjective<decltype(eval)> f(eval, false);
        BrentTrace trace;
        double bf0;
        const double bx0 = brent_search<false>(f, trace, bf0);
        f(bx0);   // (the record at the stopping point, as the null fits leave it)
        if (tid == 0) {
            EffTrial t;
            t.lml = f.lml;
            t.delta = f.delta;
            t.scale = f.scale;
            t.nfev = f.nfev;
            t.pad = 0;
            a.trial[(size_t)b * a.nrho + w] = t;
        }
    }
}

int tile_size(int KT) {
    const int ts = (KT + 15) / 16;
    return ts <= 2 ? 2 : ts <= 4 ? 4 : ts <= 6 ? 6 : 9;
}

size_t fit_lds(int cW, int k0, int ts) {
    const size_t P1 = (size_t)cW + k0 + 2;
    return sizeof(double) * ((size_t)16 * ts * (CHX + 1) + CHX + P1 * (P1 + 1) / 2 + (size_t)k0 * (k0 + 1) / 2 +
                             (size_t)k0 * P1 + 256 + 8 + (P1 - 1) + k0);
}

template <int TS>
int launch_effects(hipStream_t st, const EffArgs& a, int pairs) {
    const int KT = a.cW + 2 * a.k0 + 2;
    const size_t lds_num = sizeof(double) * ((size_t)16 * TS * (CHX + 1) + CHX);
    const size_t lds_fit = fit_lds(a.cW, a.k0, TS);
    (void)KT;
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&effects_fit_kernel<TS, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fit));
    CRM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&effects_fit_kernel<TS, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fit));
    hipLaunchKernelGGL(effects_numerators_kernel<TS>, dim3(pairs), dim3(256), lds_num, st, a);
    CRM_HIP(hipGetLastError());
    hipLaunchKernelGGL((effects_fit_kernel<TS, false>), dim3(pairs, a.nrho), dim3(256), lds_fit, st, a);
    CRM_HIP(hipGetLastError());
    hipLaunchKernelGGL((effects_fit_kernel<TS, true>), dim3(pairs), dim3(256), lds_fit, st, a);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace

extern "C" int crm_effects_multi(crm_ctx* ctx, crm_background* bg, long n, const double* W, int cW, const double* E0,
                                 int k0, const double* Y, int ny, const double* G, int nv, const int* pairs, int np,
                                 int nrho, const double* rho, double* out_fit, double* out_beta, double* out_u) {
    return crm::guarded_on("crm_effects_multi", ctx, [&]() -> int {
    if (!ctx || n <= 0 || !W || cW < 1 || !E0 || k0 < 1 || !Y || ny < 1 || !G || nv < 1 || !pairs || np < 0 ||
        nrho < 1 || nrho > CRM_MAX_RHO || !rho || (np > 0 && (!out_fit || !out_beta || !out_u))) {
        set_error("effects_multi: bad arguments (n=%ld, cW=%d, k0=%d, ny=%d, nv=%d, pairs=%d, nrho=%d)", n, cW, k0, ny, nv,
                  np, nrho);
        return CRM_ERR_ARG;
    }
    if (cW + 2 * k0 + 2 > EKT_MAX) {
        set_error("effects_multi: c_W + 2 k0 + 2 = %d columns (supported up to %d)", cW + 2 * k0 + 2, EKT_MAX);
        return CRM_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < nrho; i++) {
        if (!(rho[i] >= 0.0 && rho[i] <= 1.0)) {
            set_error("effects_multi: rho[%d] = %g outside [0, 1]", i, rho[i]);
            return CRM_ERR_ARG;
        }
    }
    for (int i = 0; i < np; i++) {
        if (pairs[2 * i] < 0 || pairs[2 * i] >= ny || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= nv) {
            set_error("effects_multi: pair %d = (%d, %d) outside %d phenotypes x %d variants", i, pairs[2 * i],
                      pairs[2 * i + 1], ny, nv);
            return CRM_ERR_ARG;
        }
    }
    if (bg) {
        if (bg->ctx != ctx || bg->n != n || bg->nrho != 1 || bg->builder) {
            set_error("effects_multi: the background must be a sealed single-grid-point background of %ld cells on this "
                      "context", n);
            return CRM_ERR_ARG;
        }
    }
    const int r = bg ? bg->r[0] : 0;
    if (n <= (long)k0 + r) {
        set_error("effects_multi: %ld cells do not exceed k0 + rank(L) = %d", n, k0 + r);
        return CRM_ERR_UNSUPPORTED;
    }
    if (np == 0) return CRM_OK;
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int P = cW + 1 + k0, KT = P + 1 + k0;
    const long n_pad = bg ? bg->n_pad : round_up(n, CELL_PAD);
    const long ldq = bg ? bg->ldq : 0;
    if ((double)n_pad * (double)std::max(cW + k0, std::max(ny, VARIANT_BLOCK)) * 8.0 > 9.0e18) {
        set_error("effects_multi: sizes overflow");
        return CRM_ERR_ARG;
    }
    if (bg) CRM_TRY(crm_background_require_q0(bg, 0));

    // variants in first-use order, blocked; pairs grouped by block (the results go back in the caller's order)
    std::vector<int> order(np);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return pairs[2 * x + 1] < pairs[2 * y + 1]; });
    std::vector<int> distinct;
    for (int i : order)
        if (distinct.empty() || distinct.back() != pairs[2 * i + 1]) distinct.push_back(pairs[2 * i + 1]);

    const long ldxe = round_up(cW + k0, 128), lde = round_up(k0, 32), ldy = round_up(ny, 128);
    const long ldg = round_up(VARIANT_BLOCK, 128) + 128;
    DevBuf d_xe, d_e, d_y, d_g, d_txe, d_ty, d_tg, d_tu, d_probs, d_pv, d_pp, d_cp, d_px, d_trial, d_fit, d_beta, d_u;
    CRM_TRY(d_xe.ensure(sizeof(double) * n_pad * ldxe));
    CRM_TRY(d_y.ensure(sizeof(double) * n_pad * ldy));
    CRM_TRY(d_g.ensure(sizeof(double) * n_pad * ldg));
    {
        std::vector<double> xe((size_t)n * (cW + k0));
        for (long i = 0; i < n; i++) {
            for (int j = 0; j < cW; j++) xe[(size_t)i * (cW + k0) + j] = W[(size_t)i * cW + j];
            for (int j = 0; j < k0; j++) xe[(size_t)i * (cW + k0) + cW + j] = E0[(size_t)i * k0 + j];
        }
        CRM_TRY(upload_padded(st, d_xe.as<double>(), ldxe, n_pad, xe.data(), cW + k0, n, cW + k0));
        CRM_HIP(hipStreamSynchronize(st));
    }
    CRM_TRY(upload_padded(st, d_y.as<double>(), ldy, n_pad, Y, ny, n, ny));
    if (r > 0) {
        CRM_TRY(d_e.ensure(sizeof(double) * n_pad * lde));
        CRM_TRY(upload_padded(st, d_e.as<double>(), lde, n_pad, E0, k0, n, k0));
        CRM_TRY(d_txe.ensure(sizeof(double) * (cW + k0) * ldq));
        CRM_TRY(d_ty.ensure(sizeof(double) * ny * ldq));
        CRM_TRY(d_tg.ensure(sizeof(double) * VARIANT_BLOCK * ldq));
        CRM_TRY(d_tu.ensure(sizeof(double) * (size_t)VARIANT_BLOCK * k0 * ldq));
        CRM_TRY(d_probs.ensure(sizeof(GemmProblem) * 4));
        // per call: Q_L'[W, E0] and Q_L'Y
        GemmProblem pr[2] = {};
        pr[0].X = d_xe.as<double>(); pr[0].ldx = ldxe; pr[0].M = cW + k0;
        pr[1].X = d_y.as<double>(); pr[1].ldx = ldy; pr[1].M = ny;
        pr[0].C = d_txe.as<double>(); pr[1].C = d_ty.as<double>();
        for (GemmProblem& p : pr) { p.Y = bg->Q0[0].as<double>(); p.ldy = ldq; p.ldc = ldq; p.N = r; }
        CRM_HIP(hipMemcpyAsync(d_probs.ptr, pr, sizeof pr, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs.as<GemmProblem>(), 1, cW + k0, r, n_pad, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, d_probs.as<GemmProblem>() + 1, 1, ny, r, n_pad, false, 0, 1, 0));
        CRM_HIP(hipStreamSynchronize(st));
    }
    const size_t chunk = std::min(np, PAIR_CHUNK);
    CRM_TRY(d_pv.ensure(sizeof(int) * chunk));
    CRM_TRY(d_pp.ensure(sizeof(int) * chunk));
    CRM_TRY(d_cp.ensure(sizeof(double) * chunk * KT * KT));
    CRM_TRY(d_px.ensure(sizeof(double) * chunk * P * P));
    CRM_TRY(d_trial.ensure(sizeof(EffTrial) * chunk * nrho));
    CRM_TRY(d_fit.ensure(sizeof(double) * chunk * 6));
    CRM_TRY(d_beta.ensure(sizeof(double) * chunk * P));
    CRM_TRY(d_u.ensure(sizeof(double) * chunk * k0));

    EffArgs a{};
    a.TXE = d_txe.as<double>(); a.TY = d_ty.as<double>(); a.TG = d_tg.as<double>(); a.TU = d_tu.as<double>();
    a.S = bg ? bg->S0[0].as<double>() : nullptr;
    a.ldq = ldq; a.r = r;
    a.XE = d_xe.as<double>(); a.ldxe = ldxe;
    a.Yd = d_y.as<double>(); a.ldy = ldy;
    a.Gd = d_g.as<double>(); a.ldg = ldg;
    a.n = n; a.cW = cW; a.k0 = k0;
    a.pv = d_pv.as<int>(); a.pp = d_pp.as<int>();
    a.nrho = nrho;
    for (int i = 0; i < nrho; i++) a.rho[i] = rho[i];
    a.Cp = d_cp.as<double>(); a.PX = d_px.as<double>(); a.trial = d_trial.as<EffTrial>();
    a.fit = d_fit.as<double>(); a.beta = d_beta.as<double>(); a.u = d_u.as<double>();
    const int ts = tile_size(KT);

    std::vector<double> gblock((size_t)n * VARIANT_BLOCK);
    std::vector<int> hv, hp, hidx;
    std::vector<double> hfit, hbeta, hu;
    size_t cursor = 0;   // into `order`
    for (size_t v0 = 0; v0 < distinct.size(); v0 += VARIANT_BLOCK) {
        const int vb = (int)std::min<size_t>(VARIANT_BLOCK, distinct.size() - v0);
        for (long i = 0; i < n; i++)
            for (int q = 0; q < vb; q++) gblock[(size_t)i * vb + q] = G[(size_t)i * nv + distinct[v0 + q]];
        CRM_TRY(upload_padded(st, d_g.as<double>(), ldg, n_pad, gblock.data(), vb, n, vb));
        if (r > 0) {
            GemmProblem pr[2] = {};
            pr[0].X = d_g.as<double>(); pr[0].ldx = ldg; pr[0].M = vb; pr[0].C = d_tg.as<double>();
            pr[1].X = d_g.as<double>(); pr[1].ldx = ldg; pr[1].E = d_e.as<double>(); pr[1].lde = lde;
            pr[1].M = vb * k0; pr[1].k0 = k0; pr[1].C = d_tu.as<double>();
            for (GemmProblem& p : pr) { p.Y = bg->Q0[0].as<double>(); p.ldy = ldq; p.ldc = ldq; p.N = r; }
            CRM_HIP(hipMemcpyAsync(d_probs.ptr, pr, sizeof pr, hipMemcpyHostToDevice, st));
            CRM_TRY(launch_gemm_tn(ctx, d_probs.as<GemmProblem>(), 1, vb, r, n_pad, false, 0, 1, 0));
            CRM_TRY(launch_gemm_tn(ctx, d_probs.as<GemmProblem>() + 1, 1, vb * k0, r, n_pad, true, k0, 1, 0));
        }
        // the pairs of this block, in chunks
        std::vector<int> mine;
        while (cursor < order.size() && pairs[2 * order[cursor] + 1] <= distinct[v0 + vb - 1]) mine.push_back(order[cursor++]);
        for (size_t c0 = 0; c0 < mine.size(); c0 += chunk) {
            const int cnt = (int)std::min(chunk, mine.size() - c0);
            hv.resize(cnt); hp.resize(cnt);
            for (int i = 0; i < cnt; i++) {
                const int pi = mine[c0 + i];
                hp[i] = pairs[2 * pi];
                hv[i] = (int)(std::lower_bound(distinct.begin() + v0, distinct.begin() + v0 + vb, pairs[2 * pi + 1]) -
                              (distinct.begin() + v0));
            }
            CRM_HIP(hipMemcpyAsync(d_pv.ptr, hv.data(), sizeof(int) * cnt, hipMemcpyHostToDevice, st));
            CRM_HIP(hipMemcpyAsync(d_pp.ptr, hp.data(), sizeof(int) * cnt, hipMemcpyHostToDevice, st));
            if (ts == 2) CRM_TRY(launch_effects<2>(st, a, cnt));
            else if (ts == 4) CRM_TRY(launch_effects<4>(st, a, cnt));
            else if (ts == 6) CRM_TRY(launch_effects<6>(st, a, cnt));
            else CRM_TRY(launch_effects<9>(st, a, cnt));
            hfit.resize((size_t)cnt * 6); hbeta.resize((size_t)cnt * P); hu.resize((size_t)cnt * k0);
            CRM_HIP(hipMemcpyAsync(hfit.data(), d_fit.ptr, sizeof(double) * hfit.size(), hipMemcpyDeviceToHost, st));
            CRM_HIP(hipMemcpyAsync(hbeta.data(), d_beta.ptr, sizeof(double) * hbeta.size(), hipMemcpyDeviceToHost, st));
            CRM_HIP(hipMemcpyAsync(hu.data(), d_u.ptr, sizeof(double) * hu.size(), hipMemcpyDeviceToHost, st));
            CRM_HIP(hipStreamSynchronize(st));
            for (int i = 0; i < cnt; i++) {
                const int pi = mine[c0 + i];
                std::copy(hfit.begin() + (size_t)i * 6, hfit.begin() + (size_t)(i + 1) * 6, out_fit + (size_t)pi * 6);
                std::copy(hbeta.begin() + (size_t)i * P, hbeta.begin() + (size_t)(i + 1) * P, out_beta + (size_t)pi * P);
                std::copy(hu.begin() + (size_t)i * k0, hu.begin() + (size_t)(i + 1) * k0, out_u + (size_t)pi * k0);
            }
        }
    }
    return CRM_OK;
    });
}
