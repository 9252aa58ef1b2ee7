// Exact tail p-value of the interaction score test: one wavefront per variant.
//
// P(Q > q) for Q = sum_j w_j chi2_1 (the weights SKAT's filter keeps, as eig_davies_kernel filters them) by the
// inverse Laplace transform of exp(K(t) - t q) / t along the parabola t(u) = c + i sigma u + mu u^2 through the saddle
// point c (tools/tail_pvalue_prototype.py states the same procedure in numpy):
//   * c: Newton steps on h(c) = K'(c) - q - 1/c inside a bracket that halves when a step leaves it -- (0, 1/(2 w_max))
//     for q > E[Q], (-(k/2 + 1) 2/q, 0) otherwise (then the contour passes left of the pole and gives P(Q > q) - 1);
//     sums over the weights lane-parallel + a wave total;
//   * the trapezoid rule over u_m = m U / M, m = 1..128, two nodes per lane, the weights read from LDS; every factor
//     1 - w'_j d (w'_j = 2 w_j / (1 - 2 w_j c), d = t - c) taken on the principal branch: it meets the real axis
//     only at d = 0;
//   * exp(K(c) - c q) is kept out of the sum, so log p is formed directly (p below the double range included).
// One kept weight: erfc.  Status per variant (include/crm_hip.h CRM_TAIL_*); no silent fall-back.
#include "nullfit.h"
#include "wave_ops.h"

namespace crm {

namespace {

constexpr double PI = 3.14159265358979323846;
constexpr double TAIL_U = 20.0;       // half-width of the contour in u
constexpr int TAIL_M = 128;           // nodes on (0, U]: two per lane
constexpr double TAIL_KAPPA = 0.1;    // mu = KAPPA / q
constexpr int NEWTON_MAX = 200;

__global__ __launch_bounds__(64) void tail_pvalue_kernel(const double* __restrict__ Qall, const double* __restrict__ lam,
                                                         int k, double* __restrict__ p_out, double* __restrict__ logp_out,
                                                         int* __restrict__ status_out) {
    extern __shared__ double sm[];
    double* w = sm;          // kept weights [k]
    double* wr = sm + k;     // 2 w / (1 - 2 w c) [k]
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* lb = lam + (long)b * k;
    auto finish = [&](double p, double lp, int status) {
        if (lane == 0) {
            p_out[b] = p;
            logp_out[b] = lp;
            status_out[b] = status;
        }
    };
    const double q = Qall[b];
    bool bad = !(fabs(q) < INFINITY);
    double sp = 0.0;
    int np = 0;
    for (int i = lane; i < k; i += 64) {
        const double v = lb[i];
        if (!(fabs(v) < INFINITY)) bad = true;
        if (v >= 0.0) { sp += v; np += 1; }
    }
    if (__any(bad)) {
        finish(NAN, NAN, CRM_TAIL_NON_FINITE);
        return;
    }
    // SKAT Get_Lambda filter, summed as davies.hip sums it: lam > mean(lam[lam >= 0]) / 1e5
    sp = wave_total(sp);
    np = wave_total(np);
    const double thr = np > 0 ? (sp / np) / 100000.0 : INFINITY;
    int r = 0;
    double wmax = 0.0;
    if (lane == 0) {
        for (int i = 0; i < k; i++) {
            const double v = lb[i];
            if (v > thr) {
                w[r++] = v;
                wmax = fmax(wmax, v);
            }
        }
    }
    r = __shfl(r, 0, 64);
    wmax = __shfl(wmax, 0, 64);
    __syncthreads();
    if (r == 0) {
        finish(NAN, NAN, CRM_TAIL_NO_WEIGHTS);
        return;
    }
    if (q <= 0.0) {    // Q >= 0 almost surely
        finish(1.0, 0.0, CRM_TAIL_CONVERGED);
        return;
    }
    if (r == 1) {
        const double x = sqrt(q / (2.0 * w[0]));
        const double p = erfc(x);
        finish(p, p > 1e-300 ? log(p) : log(erfcx(x)) - x * x, CRM_TAIL_CONVERGED);
        return;
    }
    double mean = 0.0;
    for (int i = lane; i < r; i += 64) mean += w[i];
    mean = wave_total(mean);

    // ---- saddle point (wave-uniform) ----
    double lo, hi;
    if (q > mean) {
        lo = 0.0;
        hi = 0.5 / wmax;
    } else {
        lo = -2.0 * (0.5 * r + 1.0) / q;     // h(lo) <= (r/2 + 1) / |lo| - q < 0
        hi = 0.0;
    }
    if (!(fabs(lo) < INFINITY && fabs(hi) < INFINITY && hi > lo)) {
        finish(NAN, NAN, CRM_TAIL_NOT_BRACKETED);
        return;
    }
    double c = 0.5 * (lo + hi);
    bool found = false;
    for (int it = 0; it < NEWTON_MAX; it++) {
        double h = 0.0, dh = 0.0;
        for (int i = lane; i < r; i += 64) {
            const double s = 1.0 - 2.0 * w[i] * c;
            h += w[i] / s;
            dh += 2.0 * w[i] * w[i] / (s * s);
        }
        h = wave_total(h) - q - 1.0 / c;
        dh = wave_total(dh) + 1.0 / (c * c);
        if (h < 0.0) lo = c;
        else hi = c;
        double cn = c - h / dh;
        if (!(lo < cn && cn < hi)) cn = 0.5 * (lo + hi);
        if (fabs(cn - c) <= 1e-14 * fabs(c) || !(hi - lo > 4e-16 * fabs(c))) {
            c = cn;
            found = true;
            break;
        }
        c = cn;
    }
    if (!found) {
        finish(NAN, NAN, CRM_TAIL_NOT_BRACKETED);
        return;
    }

    // ---- contour parameters, K(c) ----
    double kc = 0.0, k2 = 0.0;
    for (int i = lane; i < r; i += 64) {
        const double s = 1.0 - 2.0 * w[i] * c;
        wr[i] = 2.0 * w[i] / s;
        kc += log1p(-2.0 * w[i] * c);
        k2 += 2.0 * w[i] * w[i] / (s * s);
    }
    kc = -0.5 * wave_total(kc);
    k2 = wave_total(k2);
    __syncthreads();
    const double sigma = 1.0 / sqrt(k2 + 1.0 / (c * c));
    const double mu = TAIL_KAPPA / q;
    const double s2 = sigma * sigma;

    // ---- trapezoid sum over the nodes m = lane + 1, lane + 65 ----
    double acc = 0.0;
    for (int half = 0; half < 2; half++) {
        const int m = lane + 1 + 64 * half;
        const double u = m * (TAIL_U / TAIL_M), u2 = u * u;
        const double a2 = s2 + mu * mu * u2;
        double rl = 0.0, il = 0.0;
        for (int j = 0; j < r; j++) {
            const double wj = wr[j];
            rl += log1p(wj * u2 * (wj * a2 - 2.0 * mu));
            il += atan2(-wj * sigma * u, 1.0 - wj * mu * u2);
        }
        // exp(K(t) - K(c) - d q) (sigma - 2 i mu u) / t,  d = mu u^2 + i sigma u,  t = c + d
        const double er = -0.25 * rl - mu * u2 * q, ei = -0.5 * il - sigma * u * q;
        const double mag = exp(er);
        double sn, cs;
        sincos(ei, &sn, &cs);
        const double zr = mag * cs, zi = mag * sn;
        const double ar = zr * sigma + zi * 2.0 * mu * u, ai = zi * sigma - zr * 2.0 * mu * u;
        const double tr = c + mu * u2, ti = sigma * u;
        double term = (ar * tr + ai * ti) / (tr * tr + ti * ti);
        if (m == TAIL_M) term *= 0.5;
        acc += term;
    }
    acc = wave_total(acc);
    const double S = (TAIL_U / TAIL_M) / PI * (0.5 * sigma / c + acc);
    const double A = kc - c * q;
    if (c > 0.0) {
        if (!(S > 0.0 && S < INFINITY)) {
            finish(NAN, NAN, CRM_TAIL_NON_FINITE);
            return;
        }
        const double lp = A + log(S);
        finish(exp(lp), lp, CRM_TAIL_CONVERGED);
        return;
    }
    const double F = -exp(A) * S;    // P(Q <= q)
    if (!(F >= 0.0 && F < 1.0)) {
        finish(NAN, NAN, CRM_TAIL_NON_FINITE);
        return;
    }
    finish(1.0 - F, log1p(-F), CRM_TAIL_CONVERGED);
}

}  // namespace

int launch_tail_pvalue(hipStream_t st, const double* Q, const double* lambda, int count, int k, double* pvalue,
                       double* logp, int* status) {
    if (count <= 0) return CRM_OK;
    if (k < 1 || k > CRM_MAX_K0) {
        set_error("tail p-value: k0=%d (supported 1..%d)", k, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(tail_pvalue_kernel, dim3(count), dim3(64), sizeof(double) * 2 * (size_t)k, st, Q, lambda, k, pvalue,
                       logp, status);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace crm
