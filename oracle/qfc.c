/* Davies (1980), Algorithm AS 155: distribution of a linear combination of
 * chi-squared variables -- CPU oracle (TEST INFRASTRUCTURE ONLY).
 *
 * The reference reaches this through chiscore.davies_pvalue -> chi2comb
 * (C library "chi2comb_cdf", a re-implementation of Davies' qfc); call site
 * /root/reference cellregmap/_cellregmap.py:333,435.  chi2comb is absent from
 * this image, so this file restates the published algorithm (Applied
 * Statistics 29:323-333) in plain C.  The reference holds no golden Davies
 * p-value; what pins this file instead: the published table of AS 155, closed
 * forms and a numerical Imhof integral (tests/test_oracle_davies.py), and, at
 * 2 to 256 weights, the long-double build of this same source -- which takes
 * the same path as the double one and lies within acc = 1e-6 of the exact tail
 * value and of Imhof's integral at 30 digits wherever ifault is 0
 * (tests/test_oracle_davies_widths_cpu.py).
 *
 *   P[ sum_j lb[j] * chi2(n[j], nc[j]) + sigma * N(0,1)  <  c ]
 *
 * ifault: 0 ok; 1 required accuracy not reached within lim terms; 2 round-off
 * possibly significant; 3 invalid parameters; 4 unable to locate integration
 * parameters (evaluation counter exceeded lim).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* One source, two builds (oracle/Makefile): `real` is double, or long double with -DCRM_QFC_LD.  RL() writes a literal
 * and MF() names a math call in that type; the double build's tokens are those of the file before the typedef, so
 * crm_oracle_qfc keeps its bits. */
#ifdef CRM_QFC_LD
typedef long double real;
#define RL(x) x##L
#define MF(f) f##l
#define CRM_LN28 0.0866433975699931636771540151823L /* log(2)/8 */
#define QFC_CORE static int qfc_core
#else
typedef double real;
#define RL(x) x
#define MF(f) f
#define CRM_LN28 0.08664339756999316 /* log(2)/8 */
#define QFC_CORE int crm_oracle_qfc
#endif
#define CRM_PI RL(3.14159265358979323846)

typedef struct {
    const real *lb, *nc;
    const int *n;
    int r, lim, count, ordered, fail, overflow;
    int *th;
    real sigsq, lmax, lmin, mean, c, intl, ersm;
} qf_state;

static real exp_guard(real x) { return x < -RL(50.0) ? RL(0.0) : MF(exp)(x); }

/* log(1+x) when first, else log(1+x) - x; series for small |x| */
static real log1p_variant(real x, int first)
{
    if (MF(fabs)(x) > RL(0.1)) return first ? MF(log)(RL(1.0) + x) : (MF(log)(RL(1.0) + x) - x);
    real y = x / (RL(2.0) + x);
    real term = RL(2.0) * y * y * y;
    real k = RL(3.0);
    real s = (first ? RL(2.0) : -x) * y;
    y = y * y;
    real s1 = s + term / k;
    while (s1 != s) {
        k += RL(2.0);
        term *= y;
        s = s1;
        s1 = s + term / k;
    }
    return s;
}

static void tick(qf_state *q)
{
    q->count++;
    if (q->count > q->lim) q->overflow = 1;
}

/* insertion order of |lb| descending into th */
static void sort_by_abs(qf_state *q)
{
    for (int j = 0; j < q->r; j++) {
        real lj = MF(fabs)(q->lb[j]);
        int k = j - 1;
        while (k >= 0 && lj > MF(fabs)(q->lb[q->th[k]])) {
            q->th[k + 1] = q->th[k];
            k--;
        }
        q->th[k + 1] = j;
    }
    q->ordered = 1;
}

/* bound on tail probability via the mgf; cut-off point returned in *cx */
static real tail_bound(qf_state *q, real u, real *cx)
{
    tick(q);
    real xconst = u * q->sigsq;
    real sum1 = u * xconst;
    u = RL(2.0) * u;
    for (int j = q->r - 1; j >= 0; j--) {
        real nj = q->n[j], lj = q->lb[j], ncj = q->nc[j];
        real x = u * lj, y = RL(1.0) - x;
        xconst += lj * (ncj / y + nj) / y;
        real xy = x / y;
        sum1 += ncj * xy * xy + nj * (x * x / y + log1p_variant(-x, 0));
    }
    *cx = xconst;
    return exp_guard(-RL(0.5) * sum1);
}

/* find cut-off so that P(qf > ctff) < accx (upn>0) or P(qf < ctff) < accx */
static real cutoff(qf_state *q, real accx, real *upn)
{
    real u2 = *upn, u1 = RL(0.0), c1 = q->mean, c2 = RL(0.0), xconst;
    real rb = RL(2.0) * ((u2 > RL(0.0)) ? q->lmax : q->lmin);
    real u = u2 / (RL(1.0) + u2 * rb);
    while (!q->overflow && tail_bound(q, u, &c2) > accx) {
        u1 = u2;
        c1 = c2;
        u2 = RL(2.0) * u2;
        u = u2 / (RL(1.0) + u2 * rb);
    }
    u = (c1 - q->mean) / (c2 - q->mean);
    while (!q->overflow && u < RL(0.9)) {
        u = (u1 + u2) / RL(2.0);
        if (tail_bound(q, u / (RL(1.0) + u * rb), &xconst) > accx) {
            u1 = u;
            c1 = xconst;
        } else {
            u2 = u;
            c2 = xconst;
        }
        u = (c1 - q->mean) / (c2 - q->mean);
    }
    *upn = u2;
    return c2;
}

/* bound on the integration error due to truncation at u */
static real trunc_bound(qf_state *q, real u, real tausq)
{
    tick(q);
    real sum1 = RL(0.0), prod2 = RL(0.0), prod3 = RL(0.0);
    int s = 0;
    real sum2 = (q->sigsq + tausq) * u * u;
    real prod1 = RL(2.0) * sum2;
    u = RL(2.0) * u;
    for (int j = 0; j < q->r; j++) {
        real lj = q->lb[j], ncj = q->nc[j];
        int nj = q->n[j];
        real x = (u * lj) * (u * lj);
        sum1 += ncj * x / (RL(1.0) + x);
        if (x > RL(1.0)) {
            prod2 += nj * MF(log)(x);
            prod3 += nj * log1p_variant(x, 1);
            s += nj;
        } else {
            prod1 += nj * log1p_variant(x, 1);
        }
    }
    sum1 *= RL(0.5);
    prod2 += prod1;
    prod3 += prod1;
    real x = exp_guard(-sum1 - RL(0.25) * prod2) / CRM_PI;
    real y = exp_guard(-sum1 - RL(0.25) * prod3) / CRM_PI;
    real err1 = (s == 0) ? RL(1.0) : x * RL(2.0) / s;
    real err2 = (prod3 > RL(1.0)) ? RL(2.5) * y : RL(1.0);
    if (err2 < err1) err1 = err2;
    x = RL(0.5) * sum2;
    err2 = (x <= y) ? RL(1.0) : y / x;
    return (err1 < err2) ? err1 : err2;
}

/* find u with trunc_bound(u) < accx and trunc_bound(u/RL(1.2)) > accx */
static void find_trunc_point(qf_state *q, real *utx, real accx)
{
    static const real divis[4] = {RL(2.0), RL(1.4), RL(1.2), RL(1.1)};
    real ut = *utx, u = ut / RL(4.0);
    if (trunc_bound(q, u, RL(0.0)) > accx) {
        for (u = ut; !q->overflow && trunc_bound(q, u, RL(0.0)) > accx; u = ut) ut *= RL(4.0);
    } else {
        ut = u;
        for (u = u / RL(4.0); !q->overflow && trunc_bound(q, u, RL(0.0)) <= accx; u = u / RL(4.0)) ut = u;
    }
    for (int i = 0; i < 4; i++) {
        u = ut / divis[i];
        if (trunc_bound(q, u, RL(0.0)) <= accx) ut = u;
    }
    *utx = ut;
}

/* trapezoid sum with nterm+1 terms at step interv; when !mainx the integrand
 * is multiplied by 1 - MF(exp)(-RL(0.5) tausq u^2) */
static void integrate(qf_state *q, int nterm, real interv, real tausq, int mainx)
{
    real inpi = interv / CRM_PI;
    for (int k = nterm; k >= 0; k--) {
        real u = (k + RL(0.5)) * interv;
        real sum1 = -RL(2.0) * u * q->c;
        real sum2 = MF(fabs)(sum1);
        real sum3 = -RL(0.5) * q->sigsq * u * u;
        for (int j = q->r - 1; j >= 0; j--) {
            int nj = q->n[j];
            real x = RL(2.0) * q->lb[j] * u;
            real y = x * x;
            sum3 -= RL(0.25) * nj * log1p_variant(y, 1);
            y = q->nc[j] * x / (RL(1.0) + y);
            real z = nj * MF(atan)(x) + y;
            sum1 += z;
            sum2 += MF(fabs)(z);
            sum3 -= RL(0.5) * x * y;
        }
        real x = inpi * exp_guard(sum3) / u;
        if (!mainx) x *= (RL(1.0) - exp_guard(-RL(0.5) * tausq * u * u));
        sum1 = MF(sin)(RL(0.5) * sum1) * x;
        sum2 = RL(0.5) * sum2 * x;
        q->intl += sum1;
        q->ersm += sum2;
    }
}

/* coefficient of tausq in the error when the convergence factor
 * MF(exp)(-RL(0.5) tausq u^2) is used and the df is evaluated at x */
static real conv_coef(qf_state *q, real x)
{
    tick(q);
    if (!q->ordered) sort_by_abs(q);
    real axl = MF(fabs)(x), sxl = (x > RL(0.0)) ? RL(1.0) : -RL(1.0), sum1 = RL(0.0);
    for (int j = q->r - 1; j >= 0; j--) {
        int t = q->th[j];
        if (q->lb[t] * sxl > RL(0.0)) {
            real lj = MF(fabs)(q->lb[t]);
            real axl1 = axl - lj * (q->n[t] + q->nc[t]);
            real axl2 = lj / CRM_LN28;
            if (axl1 > axl2) {
                axl = axl1;
            } else {
                if (axl > axl2) axl = axl2;
                sum1 = (axl - axl1) / lj;
                for (int k = j - 1; k >= 0; k--) sum1 += (q->n[q->th[k]] + q->nc[q->th[k]]);
                break;
            }
        }
    }
    if (sum1 > RL(100.0)) {
        q->fail = 1;
        return RL(1.0);
    }
    return MF(pow)(RL(2.0), sum1 / RL(4.0)) / (CRM_PI * axl * axl);
}

/* trace[7]: 0 abs-sum, 1 total terms, 2 integrations, 3 main interval,
 * 4 truncation point, 5 sd of convergence factor, 6 counter */
QFC_CORE(const real *lb, const real *nc, const int *n, int r, real sigma,
         real c, int lim, real acc, real *trace, int *ifault, real *res)
{
    static const int rats[4] = {1, 2, 4, 8};
    qf_state q;
    memset(&q, 0, sizeof q);
    q.lb = lb; q.nc = nc; q.n = n; q.r = r; q.lim = lim; q.c = c;
    for (int j = 0; j < 7; j++) trace[j] = RL(0.0);
    *ifault = 0;
    real qfval = -RL(1.0), acc1 = acc, xlim = (real)lim;
    q.th = (int *)malloc((r > 0 ? r : 1) * sizeof(int));
    if (!q.th) { *ifault = 5; *res = qfval; return 5; }

    q.sigsq = sigma * sigma;
    real sd = q.sigsq;
    for (int j = 0; j < r; j++) {
        int nj = n[j];
        real lj = lb[j], ncj = nc[j];
        if (nj < 0 || ncj < RL(0.0)) { *ifault = 3; goto done; }
        sd += lj * lj * (2 * nj + RL(4.0) * ncj);
        q.mean += lj * (nj + ncj);
        if (q.lmax < lj) q.lmax = lj;
        else if (q.lmin > lj) q.lmin = lj;
    }
    if (sd == RL(0.0)) { qfval = (c > RL(0.0)) ? RL(1.0) : RL(0.0); goto done; }
    if (q.lmin == RL(0.0) && q.lmax == RL(0.0) && sigma == RL(0.0)) { *ifault = 3; goto done; }
    sd = MF(sqrt)(sd);
    real almx = (q.lmax < -q.lmin) ? -q.lmin : q.lmax;

    real utx = RL(16.0) / sd, up = RL(4.5) / sd, un = -up, tausq, intv, d1, d2, xnt, xntm;
    find_trunc_point(&q, &utx, RL(0.5) * acc1);
    if (q.overflow) { *ifault = 4; goto done; }
    if (c != RL(0.0) && almx > RL(0.07) * sd) {
        tausq = RL(0.25) * acc1 / conv_coef(&q, c);
        if (q.fail) {
            q.fail = 0;
        } else if (trunc_bound(&q, utx, tausq) < RL(0.2) * acc1) {
            q.sigsq += tausq;
            find_trunc_point(&q, &utx, RL(0.25) * acc1);
            trace[5] = MF(sqrt)(tausq);
        }
        if (q.overflow) { *ifault = 4; goto done; }
    }
    trace[4] = utx;
    acc1 *= RL(0.5);

    for (;;) {
        d1 = cutoff(&q, acc1, &up) - c;
        if (q.overflow) { *ifault = 4; goto done; }
        if (d1 < RL(0.0)) { qfval = RL(1.0); goto done; }
        d2 = c - cutoff(&q, acc1, &un);
        if (q.overflow) { *ifault = 4; goto done; }
        if (d2 < RL(0.0)) { qfval = RL(0.0); goto done; }
        intv = RL(2.0) * CRM_PI / ((d1 > d2) ? d1 : d2);
        xnt = utx / intv;
        xntm = RL(3.0) / MF(sqrt)(acc1);
        if (xnt <= xntm * RL(1.5)) break;
        /* auxiliary integration */
        if (xntm > xlim) { *ifault = 1; goto done; }
        int ntm = (int)MF(floor)(xntm + RL(0.5));
        real intv1 = utx / ntm;
        real x = RL(2.0) * CRM_PI / intv1;
        if (x <= MF(fabs)(c)) break;
        tausq = RL(0.33) * acc1 / (RL(1.1) * (conv_coef(&q, c - x) + conv_coef(&q, c + x)));
        if (q.overflow) { *ifault = 4; goto done; }
        if (q.fail) break;
        acc1 *= RL(0.67);
        integrate(&q, ntm, intv1, tausq, 0);
        xlim -= xntm;
        q.sigsq += tausq;
        trace[2] += RL(1.0);
        trace[1] += ntm + 1;
        find_trunc_point(&q, &utx, RL(0.25) * acc1);
        if (q.overflow) { *ifault = 4; goto done; }
        acc1 *= RL(0.75);
    }

    trace[3] = intv;
    if (xnt > xlim) { *ifault = 1; goto done; }
    {
        int nt = (int)MF(floor)(xnt + RL(0.5));
        integrate(&q, nt, intv, RL(0.0), 1);
        trace[2] += RL(1.0);
        trace[1] += nt + 1;
        qfval = RL(0.5) - q.intl;
        trace[0] = q.ersm;
        real upv = q.ersm, x = upv + acc / RL(10.0);
        for (int j = 0; j < 4; j++)
            if (rats[j] * x == rats[j] * upv) *ifault = 2;
    }

done:
    free(q.th);
    trace[6] = (real)q.count;
    *res = qfval;
    return *ifault;
}

#ifdef CRM_QFC_LD
/* The same algorithm with every variable, constant and math call in long double; arguments and results are doubles,
 * converted here.  *sf = 1 - cdf, formed before the conversion.  The float64 entry is held to this one at every width
 * (tests/test_oracle_davies_widths_cpu.py), and the device to both (tests/test_gpu_davies_widths.py). */
int crm_oracle_qfc_ld(const double *lb, const double *nc, const int *n, int r, double sigma,
                      double c, int lim, double acc, double *trace, int *ifault, double *res, double *sf)
{
    real tr[7], out = -1.0L;
    real *buf = (real *)malloc((r > 0 ? 2 * r : 1) * sizeof(real));
    for (int j = 0; j < 7; j++) trace[j] = 0.0;
    if (!buf) { *ifault = 5; *res = -1.0; *sf = 2.0; return 5; }
    for (int j = 0; j < r; j++) {
        buf[j] = lb[j];
        buf[r + j] = nc[j];
    }
    qfc_core(buf, buf + r, n, r, sigma, c, lim, acc, tr, ifault, &out);
    free(buf);
    for (int j = 0; j < 7; j++) trace[j] = (double)tr[j];
    *res = (double)out;
    *sf = (double)(1.0L - out);
    return *ifault;
}
#endif
