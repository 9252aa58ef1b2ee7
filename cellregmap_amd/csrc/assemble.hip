// Score statistic Q and mixture matrix F per variant.
//
// Reference: QSCov / PMat / ScoreStatistic, cellregmap/_math.py:40-128, called at
// cellregmap/_cellregmap.py:379-435 with K0 = v0 * Q0 S0 Q0' + v1 * I, X = [W, g],
// half_dK = diag(gtest) E0.  The reference applies K0^-1 to n-vectors with three products
// against Q0; here every bilinear form is taken in the rotated space instead,
//
//     u' K0^-1 v = ( u'v - sum_j d_j (Q0'u)_j (Q0'v)_j ) / v1 ,   d_j = v0 S0_j / (v0 S0_j + v1)
//
// so that with A~ = Q0' diag(gtest) E0 (from the Khatri-Rao contraction) and the n-length
// reductions Z1..Z3 nothing of size n is touched here.  launch_assemble runs, per block of variants:
//   the Gram   : S S' for S = sqrt(d) o [A~ rows ; Q0'W ; Q0'g ; Q0'y]  (one pass over r, FP64 MFMA) -- gram_ext.hip:
//                launch_gram_ext, or wb_gram_fused.hip ahead of this launch
//   woodbury   : (unrelated-donor form) the E1 term folded back by a k1 x k1 capacitance solve: woodbury_yty_kernel,
//                or woodbury_kernel with both substitutions (form "woodbury_ytY" = 0)
//   finalize   : X'K^-1X etc., the (c+1)x(c+1) solve, Q = 1/2 |u|^2,
//                F = 1/2 (D'K^-1 D - D'K^-1 X (X'K^-1X)^-1 X'K^-1 D)
#include "assemble.h"
#include "wave_ops.h"

namespace crm {

namespace {

// Unrelated-donor form (scan_plan.hip: kin_wb).  The Gram Gw of the KT + k1 rows [X ; W ; gx ; y ; E1] was taken over the
// donors k2 positions with the weights of N = v1 I + v0 sum_p s_p(rho) phi_p phi_p' alone, so that
//     M_uv = u'N^-1 v = (u'v - Gw_uv) / v1 ;
// K0 = N + v0 rho E1 E1' then gives, with the k1 x k1 capacitance C = I + v0 rho M_EE (positive definite, >= I),
//     u'K0^-1 v = M_uv - v0 rho M_uE C^-1 M_Ev .
// finalize_kernel reads K0^-1 as (plain - Ge) / v1, so Ge = Gw + v1 v0 rho M_uE C^-1 M_Ev on the leading KT x KT block.
// A variant without a kinship term to speak of (sorted_pos < 0: its X rows of Gw are zero, scan_pass.h: no_kinship_term)
// drops the X part of the correction the same way.  v0 rho = 0 (rho* = 0, or no kinship variance) leaves Gw as it is.
// One workgroup per variant; LDS: M_uE [KT][k1], C [k1][k1], C^-1 M_Ev [k1][KT].
__global__ __launch_bounds__(256) void woodbury_kernel(AssembleArgs a, const double* __restrict__ Gw, int KT,
                                                       double* __restrict__ Gext) {
    extern __shared__ double wsm[];
    const int k1 = a.wb_k1, KW = KT + k1, k0 = a.k0, c = a.c;
    const int b = blockIdx.x, tid = threadIdx.x;
    const NullFitOut fit = a.fit[b];
    const double g = fit.v0 * a.rho[fit.rho_index].rho;
    const double inv = 1.0 / fit.v1;
    const double* __restrict__ G = Gw + (long)b * KW * KW;
    double* __restrict__ out = Gext + (long)b * KT * KT;
    if (!(g > 0.0)) {
        for (int e = tid; e < KT * KT; e += 256) out[e] = G[(long)(e / KT) * KW + e % KT];
        return;
    }
    double* ME = wsm;               // [KT][k1]
    double* Cm = ME + KT * k1;      // [k1][k1]
    double* Z = Cm + k1 * k1;       // [k1][KT]
    const long pos = a.sorted_pos[b];
    for (int e = tid; e < KT * k1; e += 256) {
        const int u = e / k1, f = e - u * k1;
        double plain;
        if (u < k0) plain = pos >= 0 ? a.wb_E1X[(long)f * a.wb_ldE1X + pos * k0 + u] : 0.0;
        else if (u < k0 + c) plain = a.wb_E1yW[(long)f * a.wb_ldE1yW + 1 + (u - k0)];
        else if (u == k0 + c) plain = a.wb_E1g[(long)f * a.wb_ldE1g + b];
        else plain = a.wb_E1yW[(long)f * a.wb_ldE1yW];
        ME[e] = (u < k0 && pos < 0) ? 0.0 : (plain - G[(long)u * KW + KT + f]) * inv;
    }
    for (int e = tid; e < k1 * k1; e += 256) {
        const int i = e / k1, j = e - i * k1;
        Cm[e] = (i == j ? 1.0 : 0.0) + g * (a.wb_EE[e] - G[(long)(KT + i) * KW + KT + j]) * inv;
    }
    __syncthreads();
    // Cholesky C = L L' in place (lower triangle), column by column
    for (int j = 0; j < k1; j++) {
        if (tid == 0) Cm[j * k1 + j] = sqrt(Cm[j * k1 + j]);
        __syncthreads();
        const double l = Cm[j * k1 + j];
        for (int i = j + 1 + tid; i < k1; i += 256) Cm[i * k1 + j] /= l;
        __syncthreads();
        for (int e = tid; e < (k1 - j - 1) * (k1 - j - 1); e += 256) {
            const int i = j + 1 + e / (k1 - j - 1), q = j + 1 + e % (k1 - j - 1);
            if (q <= i) Cm[i * k1 + q] -= Cm[i * k1 + j] * Cm[q * k1 + j];
        }
        __syncthreads();
    }
    // Z = C^-1 M_E. : one column per thread
    for (int u = tid; u < KT; u += 256) {
        for (int i = 0; i < k1; i++) {
            double s = ME[u * k1 + i];
            for (int q = 0; q < i; q++) s -= Cm[i * k1 + q] * Z[q * KT + u];
            Z[i * KT + u] = s / Cm[i * k1 + i];
        }
        for (int i = k1 - 1; i >= 0; i--) {
            double s = Z[i * KT + u];
            for (int q = i + 1; q < k1; q++) s -= Cm[q * k1 + i] * Z[q * KT + u];
            Z[i * KT + u] = s / Cm[i * k1 + i];
        }
    }
    __syncthreads();
    const double scale = fit.v1 * g;
    for (int e = tid; e < KT * KT; e += 256) {
        const int u = e / KT, v = e - u * KT;
        double s = 0.0;
        for (int f = 0; f < k1; f++) s += ME[u * k1 + f] * Z[f * KT + v];
        out[e] = G[(long)u * KW + v] + scale * s;
    }
}

// The same correction without the backward substitution: M_uE C^-1 M_Ev = Y'Y with Y = L^-1 M_E. (k1 x KT), C = L L'.
// Y is what a Cholesky factorisation of the augmented matrix [C ; M_.E] (k1 + KT rows, k1 columns) leaves below L, so the
// factor and the forward substitution are one right-looking sweep: at column j every entry (R, q > j) takes
// -= A[R][j] A[q][j], for the rows of C below the diagonal (R >= q) and for every row of M_.E alike.  The matrix is held
// by columns, AT [k1][LD] with LD odd: a wavefront owns whole columns q = j + 1 + wave, + 4, ..., its lanes the rows R, so
// column j is only read and every other column is touched by one wavefront alone -- one barrier per column.  The
// wavefront that updates column j + 1 also finishes it (square root of the pivot, division of the rest): it works the
// pivot out before it stores anything, and the column is ready when the barrier opens.  Y'Y is then a Gram over
// the k1 rows of Y: 16 x 16 tiles of the upper triangle on the FP64 MFMA (k1 padded with zeros to a multiple of 4),
// mirrored.  LDS: k1 (k1 + KT + 1) doubles at the most, inside woodbury_lds_bytes.
__global__ __launch_bounds__(256) void woodbury_yty_kernel(AssembleArgs a, const double* __restrict__ Gw, int KT,
                                                           double* __restrict__ Gext) {
    extern __shared__ double wsm[];
    const int k1 = a.wb_k1, KW = KT + k1, k0 = a.k0, c = a.c;
    const int NR = k1 + KT, LD = NR | 1;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const NullFitOut fit = a.fit[b];
    const double g = fit.v0 * a.rho[fit.rho_index].rho;
    const double inv = 1.0 / fit.v1;
    const double* __restrict__ G = Gw + (long)b * KW * KW;
    double* __restrict__ out = Gext + (long)b * KT * KT;
    if (!(g > 0.0)) {
        for (int e = tid; e < KT * KT; e += 256) out[e] = G[(long)(e / KT) * KW + e % KT];
        return;
    }
    double* AT = wsm;   // [k1][LD]: column q holds C[R][q] at R in [q, k1) and M_uE[u][q] at R = k1 + u
    const long pos = a.sorted_pos[b];
    for (int e = tid; e < KT * k1; e += 256) {
        const int u = e / k1, f = e - u * k1;
        double plain;
        if (u < k0) plain = pos >= 0 ? a.wb_E1X[(long)f * a.wb_ldE1X + pos * k0 + u] : 0.0;
        else if (u < k0 + c) plain = a.wb_E1yW[(long)f * a.wb_ldE1yW + 1 + (u - k0)];
        else if (u == k0 + c) plain = a.wb_E1g[(long)f * a.wb_ldE1g + b];
        else plain = a.wb_E1yW[(long)f * a.wb_ldE1yW];
        AT[f * LD + k1 + u] = (u < k0 && pos < 0) ? 0.0 : (plain - G[(long)u * KW + KT + f]) * inv;
    }
    for (int e = tid; e < k1 * k1; e += 256) {
        const int i = e / k1, j = e - i * k1;
        if (j <= i) AT[j * LD + i] = (i == j ? 1.0 : 0.0) + g * (a.wb_EE[e] - G[(long)(KT + i) * KW + KT + j]) * inv;
    }
    __syncthreads();
    if (wave == 0) {   // column 0
        const double l = sqrt(AT[0]);
        for (int R = lane; R < NR; R += 64) AT[R] = R == 0 ? l : AT[R] / l;
    }
    __syncthreads();
    for (int j = 0; j + 1 < k1; j++) {
        const double* colj = AT + j * LD;
        // the next pivot, worked out by every lane from the same two numbers before any store of this step: the lane
        // of the diagonal arrives at the same value through its own update
        const double lnext = wave == 0 ? sqrt(fma(-colj[j + 1], colj[j + 1], AT[(j + 1) * LD + j + 1])) : 0.0;
        for (int R = ((j + 1) & ~63) + lane; R < NR; R += 64) {   // (rows up to j have nothing left to take)
            const double aR = R > j ? colj[R] : 0.0;
            for (int q0 = j + 1 + wave; q0 < k1; q0 += 16) {
                double lq[4], cv[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int q = q0 + 4 * m;
                    const bool on = q < k1 && R >= q;
                    lq[m] = on ? colj[q] : 0.0;
                    cv[m] = on ? AT[q * LD + R] : 0.0;
                }
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int q = q0 + 4 * m;
                    if (!(q < k1 && R >= q)) continue;
                    double v = fma(-aR, lq[m], cv[m]);
                    if (q == j + 1) v = R == q ? lnext : v / lnext;   // (wavefront 0: the next pivot column, finished)
                    AT[q * LD + R] = v;
                }
            }
        }
        __syncthreads();
    }
    // out = Gw + v1 g Y'Y on the upper triangle of 16 x 16 tiles, dealt to the wavefronts, mirrored
    const int ts = (KT + 15) / 16, l15 = lane & 15, l4 = lane >> 4;
    const double scale = fit.v1 * g;
    const double* __restrict__ Y = AT + k1;
    int t = 0;
    for (int ti = 0; ti < ts; ti++)
        for (int tj = ti; tj < ts; tj++, t++) {
            if ((t & 3) != wave) continue;
            const int u = 16 * ti + l15, v = 16 * tj + l15;
            v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
            for (int f0 = 0; f0 < k1; f0 += 4) {
                const int f = f0 + l4;
                const double fa = (f < k1 && u < KT) ? Y[f * LD + u] : 0.0;
                const double fb = (f < k1 && v < KT) ? Y[f * LD + v] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc, 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 16 * ti + l4 + 4 * reg;
                if (row < KT && v < KT && v >= row) {
                    const double s = scale * acc[reg];
                    out[(long)row * KT + v] = G[(long)row * KW + v] + s;
                    if (v != row) out[(long)v * KT + row] = G[(long)v * KW + row] + s;
                }
            }
        }
}

constexpr int PMAX = CRM_MAX_COV_XWIDE + 1;

__global__ __launch_bounds__(128) void finalize_kernel(AssembleArgs a, const double* __restrict__ Gext,
                                                        int KT, double* __restrict__ rows, int sym) {
    // per variant: everything below is k0- or (c+1)-sized; LDS carved from the dynamic segment:
    // L [P][P] (Cholesky factor of X'K^-1X), xky [P], uvec [k0], vv, ww [P] each, then dkx [k0][P] (D'K^-1X) and
    // sol [k0][P] -- or, when those two do not fit (many contexts x many covariates), in `rows` (global memory,
    // 2 k0 P doubles per variant: the slower form)
    extern __shared__ double fsm[];
    __shared__ int ok_flag, keep_flag;
    __shared__ double rescale;     // 1 / scale where the fit record asks for the scale to be derived here (fit.scale < 0)
    const int Pd = a.c + 1;
    double* Lm = fsm;
    double* xky = Lm + Pd * Pd;
    double* uvec = xky + Pd;
    double* vv = uvec + a.k0;
    double* ww = vv + Pd;
    double* dkxm = rows ? rows + (size_t)blockIdx.x * 2 * a.k0 * Pd : ww + Pd;
    double* solm = dkxm + a.k0 * Pd;
#define L(i, j) Lm[(i) * Pd + (j)]
#define dkx(j, i) dkxm[(j) * Pd + (i)]
#define sol(j, i) solm[(j) * Pd + (i)]
    const int b = blockIdx.x;
    const NullFitOut fit = a.fit[b];
    const int k0 = a.k0, c = a.c;
    const int P = c + 1;
    const double v1 = fit.v1;
    const double inv = 1.0 / v1;
    const double* __restrict__ Ge = Gext + (long)b * KT * KT;
    const int tid = threadIdx.x;
    auto plain_xx = [&](int i, int j) -> double {  // X'X entries, X = [W, g]
        if (i > j) { int t = i; i = j; j = t; }
        if (j < c) return a.WW[i * c + j];
        if (i < c) return a.gW[(long)b * a.ld_gW + i];
        return a.gg[b];
    };
    auto plain_xy = [&](int i) -> double { return i < c ? a.Wy[i] : a.gy[b]; };

    if (tid == 0) {
        bool ok = true;
        for (int i = 0; i < P; i++) {
            for (int j = 0; j <= i; j++)
                L(i, j) = (plain_xx(i, j) - Ge[(long)(k0 + i) * KT + (k0 + j)]) * inv;
            xky[i] = (plain_xy(i) - Ge[(long)(k0 + i) * KT + (k0 + c + 1)]) * inv;
        }
        // (whether the variant is a column of the projection is PMat's own decision, below -- not the null fit's use_g:
        // the reference's LMM and its PMat apply different rank rules to [W, g])
        bool keep = true;
        for (int j = 0; j < P && ok; j++) {
            double d = L(j, j);
            for (int k = 0; k < j; k++) d -= L(j, k) * L(j, k);
            if (!(d > 0.0)) {
                if (j == c) keep = false;   // no component outside span(W) at all
                else ok = false;
                break;
            }
            const double l = sqrt(d);
            L(j, j) = l;
            for (int i = j + 1; i < P; i++) {
                double s = L(i, j);
                for (int k = 0; k < j; k++) s -= L(i, k) * L(j, k);
                L(i, j) = s / l;
            }
        }
        if (ok && keep) {
            // PMat solves with numpy's lstsq(rcond=None) on X'K^-1X in the basis of X = [W, g] AS GIVEN (_math.py:33-37,
            // :91-93): a singular value below eps * (c + 1) * the largest is cut off -- a rule of its own, apart from the
            // LMM's economic_svd (absolute sqrt(eps) on the singular values of X, use_g above): with columns of norm
            // ~ sqrt(n) a variant can be kept by the null fit and still be cut here.  The matrix at hand is the one of
            // [W', x] with x = g - W' a (a: the block's projection coefficients; none on the collapsed path), i.e.
            // A_given = T' (L L') T, T = [[I, a], [0, 1]] up to an orthogonal change of W's basis, which leaves the
            // singular values alone.  Smallest one: the Rayleigh quotient of the near-null vector (-(a + b), 1), b the
            // K-metric regression of x on W' -- s / (1 + |a + b|^2) with s the Schur complement (last pivot squared);
            // largest one: a few power iterations through the factor.  Cutting that direction leaves the projection of W
            // alone (to the order of the singular-value ratio).
            double nrm2 = 1.0;
            {
                // b = L_WW^-T L(c, 0..c-1)'
                for (int i = c - 1; i >= 0; i--) {
                    double sacc = L(c, i);
                    for (int k = i + 1; k < c; k++) sacc -= L(k, i) * vv[k];
                    vv[i] = sacc / L(i, i);
                }
                for (int j = 0; j < c; j++) {
                    const double t = vv[j] + (a.coef ? a.coef[(long)j * a.ld_coef + b] : 0.0);
                    nrm2 += t * t;
                }
            }
            const double lam_min = L(c, c) * L(c, c) / nrm2;
            // power iteration on T' L L' T
            for (int i = 0; i < P; i++) vv[i] = 1.0;
            double lam_max = 0.0;
            for (int it = 0; it < 12; it++) {
                // u = T v
                const double vl = vv[c];
                for (int j = 0; j < c; j++) ww[j] = vv[j] + (a.coef ? a.coef[(long)j * a.ld_coef + b] : 0.0) * vl;
                ww[c] = vl;
                // w = L' u (in vv), then u = L w (in ww)
                for (int i = 0; i < P; i++) {
                    double sacc = 0.0;
                    for (int k = i; k < P; k++) sacc += L(k, i) * ww[k];
                    vv[i] = sacc;
                }
                for (int i = P - 1; i >= 0; i--) {
                    double sacc = 0.0;
                    for (int k = 0; k <= i; k++) sacc += L(i, k) * vv[k];
                    ww[i] = sacc;
                }
                // v = T' u
                double last = ww[c];
                for (int j = 0; j < c; j++) last += (a.coef ? a.coef[(long)j * a.ld_coef + b] : 0.0) * ww[j];
                double n2 = last * last;
                for (int j = 0; j < c; j++) n2 += ww[j] * ww[j];
                lam_max = sqrt(n2);
                if (!(lam_max > 0.0)) break;
                for (int j = 0; j < c; j++) vv[j] = ww[j] / lam_max;
                vv[c] = last / lam_max;
            }
            if (lam_min <= 2.220446049250313e-16 * (double)P * lam_max) keep = false;
        }
        if (!keep) {  // the projection is the one of W alone
            for (int j = 0; j < c; j++) L(c, j) = 0.0;
            L(c, c) = 1.0;
            xky[c] = 0.0;
        }
        keep_flag = keep ? 1 : 0;
        rescale = 1.0;
        if (ok) {
            for (int i = 0; i < P; i++) {
                double s = xky[i];
                for (int k = 0; k < i; k++) s -= L(i, k) * xky[k];
                xky[i] = s / L(i, i);
            }
            if (fit.scale < 0.0) {
                // A record of (v0, v1) = (1 - delta, delta) without its scale (scan_results.hip: the probes of the flat-optimum flag):
                // the REML scale at that delta is y'Py / df with P of the unit-scale covariance, from what is at hand --
                // y'K^-1y and the forward-substituted X'K^-1y (glimix-core: LMM.scale; nullfit.hip evaluates the same).
                double r = (a.yy - Ge[(long)(k0 + c + 1) * KT + (k0 + c + 1)]) * inv;
                const int used = c + ((fit.use_g && keep) ? 1 : 0);
                for (int i = 0; i < used; i++) r -= xky[i] * xky[i];
                const double df = (double)a.n - (double)(c + (fit.use_g ? 1 : 0));
                rescale = 1.0 / fmax(r / df, 1.4901161193847656e-08);
            }
            for (int i = P - 1; i >= 0; i--) {
                double s = xky[i];
                for (int k = i + 1; k < P; k++) s -= L(k, i) * xky[k];
                xky[i] = s / L(i, i);
            }
        }
        ok_flag = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = ok_flag != 0;
    const bool keep_g = keep_flag != 0;
    // D'K^-1 X rows and their solves, one context per thread
    for (int j = tid; j < k0; j += blockDim.x) {
        double row[PMAX];
        for (int i = 0; i < P; i++) {
            double plain;
            if (i < c) plain = a.Z1[(long)b * a.ldZ1 + (long)(1 + i) * k0 + j];
            else plain = a.Z2[(long)b * a.ldZ2 + j];
            double v = (plain - Ge[(long)j * KT + (k0 + i)]) * inv;
            if (i == c && !keep_g) v = 0.0;
            row[i] = v;
            dkx(j, i) = v;
        }
        for (int i = 0; i < P; i++) {
            double s = row[i];
            for (int k = 0; k < i; k++) s -= L(i, k) * row[k];
            row[i] = s / L(i, i);
        }
        for (int i = P - 1; i >= 0; i--) {
            double s = row[i];
            for (int k = i + 1; k < P; k++) s -= L(k, i) * row[k];
            row[i] = s / L(i, i);
        }
        for (int i = 0; i < P; i++) sol(j, i) = row[i];
        const double dky = (a.Z1[(long)b * a.ldZ1 + j] - Ge[(long)j * KT + (k0 + c + 1)]) * inv;
        double u = dky;
        for (int i = 0; i < P; i++) u -= dkx(j, i) * xky[i];
        uvec[j] = u * rescale;
    }
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (int j = 0; j < k0; j++) q += uvec[j] * uvec[j];
        a.Q[b] = ok ? 0.5 * q : NAN;
    }
    double* __restrict__ F = a.F + (long)b * k0 * k0;
    for (int e = tid; e < k0 * k0; e += blockDim.x) {
        const int j = e / k0, jp = e - j * k0;
        const int lo = j < jp ? j : jp, hi = j < jp ? jp : j;
        // pair index of (lo, hi) in the row-major upper triangle
        const long pidx = (long)lo * k0 - (long)lo * (lo - 1) / 2 + (hi - lo);
        // sym (the Y'Y form of the unrelated-donor correction, whose Ge is mirrored): the lower triangle of F repeats the
        // upper one's arithmetic -- entry (j, j') and entry (j', j) both from Ge(lo, hi), dkx(lo, .) and sol(hi, .) in the same
        // order -- so F comes out exactly symmetric, and its lower triangle rounds differently from what it did.  Otherwise
        // the projection term is taken against the solved rows of j' as it always was, which rounds differently for the
        // two entries (1e-16 of max|F|).
        const int ja = sym ? lo : j, jb = sym ? hi : jp;
        double v = (a.Z3[(long)b * a.ldZ3 + pidx] - Ge[(long)ja * KT + jb]) * inv;
        for (int i = 0; i < P; i++) v -= dkx(ja, i) * sol(jb, i);
        F[e] = ok ? 0.5 * v * rescale : NAN;
    }
}
#undef L
#undef dkx
#undef sol

}  // namespace

size_t woodbury_lds_bytes(int KT, int k1) { return sizeof(double) * ((size_t)2 * KT * k1 + (size_t)k1 * k1); }

size_t assemble_rows_scratch_doubles(int variants, int k0, int c) {
    const size_t P = (size_t)c + 1;
    const size_t lds = sizeof(double) * (P * P + 3 * P + k0 + 2 * (size_t)k0 * P);
    return lds > 150 * 1024 ? (size_t)variants * 2 * k0 * P : 0;
}

int launch_assemble(hipStream_t st, const AssembleArgs& a, int variants, double* Gext, double* fin_rows,
                    long* dma_launches) {
    if (variants <= 0) return CRM_OK;
    const int KT0 = a.k0 + a.c + 2;
    // (unrelated-donor form: the Gram takes the k1 E1 rows as well, the correction folds them back into KT0 x KT0)
    const int KT = KT0 + (a.wb_k1 > 0 ? a.wb_k1 : 0);
    double* const Gfin = Gext;
    if (a.wb_k1 > 0) {
        if (KT > CRM_MAX_GRAM_ROWS || woodbury_lds_bytes(KT0, a.wb_k1) > 150 * 1024 || !a.wb_Gw) {
            set_error("assemble: unrelated-donor form with %d + %d rows outside its supported range", KT0, a.wb_k1);
            return CRM_ERR_INTERNAL;
        }
        Gext = a.wb_Gw;
    }
    const int P = a.c + 1;
    const size_t fin_small = sizeof(double) * ((size_t)P * P + 3 * P + a.k0);
    size_t fin_lds = fin_small + sizeof(double) * 2 * (size_t)a.k0 * P;
    const bool rows_global = fin_lds > 150 * 1024;
    if (rows_global) fin_lds = fin_small;
    if (a.k0 > CRM_MAX_K0 || a.c > CRM_MAX_COV_XWIDE || KT > CRM_MAX_GRAM_ROWS || (rows_global && !fin_rows)) {
        set_error("assemble: k0=%d, c=%d outside the supported range (k0 <= %d, c <= %d, k0 + c + 2 <= %d)", a.k0, a.c,
                  CRM_MAX_K0, CRM_MAX_COV_XWIDE, CRM_MAX_GRAM_ROWS);
        return CRM_ERR_UNSUPPORTED;
    }
    // (the Gram is in wb_Gw already: launch_wb_gram_fused has formed it from the pair products -- a direct-to-LDS form too)
    const bool gram_done = a.wb_k1 > 0 && a.wb_gram_done != 0;
    bool dma = gram_done;
    if (!gram_done) CRM_TRY(launch_gram_ext(st, a, variants, Gext, KT, &dma));
    if (dma && dma_launches) ++*dma_launches;
    const bool yty = a.wb_k1 > 0 && form("woodbury_ytY", 1) != 0;
    if (a.wb_k1 > 0) {
        // form("woodbury_ytY", 0): the factor, then both substitutions, one column of C^-1 M_Ev per thread
        const size_t lds = yty ? sizeof(double) * a.wb_k1 * (size_t)((KT0 + a.wb_k1) | 1) : woodbury_lds_bytes(KT0, a.wb_k1);
        CRM_HIP(yty ? launch_with_lds(woodbury_yty_kernel, dim3(variants), dim3(256), lds, st, lds > 60 * 1024, a, a.wb_Gw, KT0, Gfin)
                    : launch_with_lds(woodbury_kernel, dim3(variants), dim3(256), lds, st, lds > 60 * 1024, a, a.wb_Gw, KT0, Gfin));
    }
    CRM_HIP(launch_with_lds(finalize_kernel, dim3(variants), dim3(128), fin_lds, st, fin_lds > 60 * 1024, a, Gfin, KT0,
                            rows_global ? fin_rows : nullptr, yty ? 1 : 0));
    return CRM_OK;
}

}  // namespace crm
