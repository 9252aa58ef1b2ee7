// What the kernels that search over delta have in common around the search itself (brent_search.h): the constants of the
// likelihood, the clamped logistic, the memoised objective that brent_search is given (inline, or called out of line
// where a kernel has no registers for its state), and the end of a fit.  The workgroup kernels (nullfit_wide.hip,
// nullfit_xwide.hip, effects_multi.hip) keep what differs: how the likelihood at one delta is evaluated, with beta and
// scale profiled out.  The register kernels of nullfit.hip use the constants and the logistic only and keep their own
// memo and end of a fit (see there: on this objective they spilled more and one ran slower).
#pragma once
#include "brent_search.h"
#include "nullfit.h"

namespace crm {

constexpr double LOG2PI = 1.8378770664093453;
constexpr double EPS_TINY = 2.220446049250313e-16;    // numpy_sugar.epsilon.tiny
constexpr double EPS_SMALL = 1.4901161193847656e-08;  // numpy_sugar.epsilon.small

__device__ inline double logistic_clamped(double x) {
    double v;
    if (x > 0.0) {
        v = 1.0 / (1.0 + exp(-x));
    } else {
        v = exp(x);
        v = v / (v + 1.0);
    }
    return fmin(fmax(v, EPS_TINY), 1.0 - EPS_TINY);
}

// What a kernel's evaluation at one delta gives back.  ok = false: a factorisation met a non-positive pivot (the other
// fields are not read).  noise: the first-order bound on the rounding noise of lml (NullFitTrial::noise), read only where
// the evaluation was asked for it.
struct DeltaValue {
    bool ok;
    double scale, lml, noise;
};

// f(x) = -lml at delta = logistic(x): the functor of brent_search.  Eval: the kernel's evaluation, (double delta,
// bool noise_now) -> DeltaValue, called by every participating thread in lockstep (it may contain barriers).
//
// The logistic is clamped to [eps, 1 - eps]: every x beyond +-36.7 is the SAME delta, and the objective there the same
// number to the last bit -- a phenotype without a random effect (delta -> 1: half of the genes of an eQTL run) sends the
// reference's bracketing phase through 63, 127, 255, 511, 709 and Brent's iteration after it, dozens of evaluations of
// one value.  The two clamped points are evaluated once and remembered (bit-identical results, fewer evaluations; nfev
// counts the calls, as the reference's does).
template <class Eval>
struct ClampedObjective {
    Eval& eval;
    const bool track;          // the fit bounds the rounding noise of its values: at the clamped points and on want_noise
    bool want_noise = false;   // the next evaluation also bounds the noise of its value
    int nfev = 0;
    double delta = 0.5, scale = 1.0, lml = -INFINITY, noise = NAN;   // of the last evaluation
    // the two clamped points, delta = eps and 1 - eps: scalars per slot, chosen by selects (an array indexed by the slot
    // would keep the whole objective, and what it refers to, in memory wherever it is inline)
    struct Memo {
        bool set = false;
        double f = 0.0, scale = 0.0, lml = 0.0, noise = NAN;
    } at_eps, at_one;
    bool last_clamped = false;   // the last evaluation was one of the two clamped points

    __device__ __forceinline__ ClampedObjective(Eval& e, bool track_) : eval(e), track(track_) {}
    __device__ __forceinline__ bool clamped() const { return last_clamped; }
    __device__ __forceinline__ double operator()(double x) {
        nfev++;
        delta = logistic_clamped(x);
        const bool one = delta == 1.0 - EPS_TINY, eps = !one && delta == EPS_TINY;
        last_clamped = one || eps;
        if (one ? at_one.set : (eps && at_eps.set)) {
            scale = one ? at_one.scale : at_eps.scale;
            lml = one ? at_one.lml : at_eps.lml;
            noise = one ? at_one.noise : at_eps.noise;
            return one ? at_one.f : at_eps.f;
        }
        const bool noise_now = track && (want_noise || last_clamped);
        const DeltaValue e = eval(delta, noise_now);
        double value;
        if (e.ok) {
            scale = e.scale;
            lml = e.lml;
            if (noise_now) noise = e.noise;
            value = -e.lml;
        } else {
            scale = NAN;
            lml = NAN;
            value = INFINITY;
        }
        if (one) at_one = Memo{true, value, scale, lml, noise};
        if (eps) at_eps = Memo{true, value, scale, lml, noise};
        return value;
    }
};

// The same objective called out of line, for the workgroup kernels whose evaluation leaves no registers over
// (nullfit_xwide.hip, effects_multi.hip): one copy of it serves every call of the search and the objective's state lives
// in memory.
template <class Eval>
struct OutOfLineObjective : ClampedObjective<Eval> {
    using ClampedObjective<Eval>::ClampedObjective;
    __device__ __noinline__ double operator()(double x) { return ClampedObjective<Eval>::operator()(x); }
};

// The end of a fit whose search stopped at x: beta and scale refreshed at the optimum (LMM.fit()), and the record.
// Tracked fits first take the objective one stopping tolerance to either side of x -- how flat the likelihood is there
// says how far rounding can move the last parabolic steps (include/crm_hip.h) -- and leave the margin of the search's
// decisions, that curvature and the noise bound of the value at x behind.  Every thread gets the record; which one stores
// it is the kernel's decision.
template <class F>
__device__ __forceinline__ NullFitTrial finish_fit(F& f, double x, const BrentTrace& trace, bool use_g) {
    double f_up = NAN, f_dn = NAN;
    if (f.track) {
        const double tolx = 1e-6 * fabs(x) + 1e-6;
        f_up = f(x + tolx);
        f_dn = f(x - tolx);
    }
    f.want_noise = true;
    const double f_stop = f(x);
    NullFitTrial t;
    t.lml = f.lml;
    t.delta = f.delta;
    t.scale = f.scale;
    t.use_g = use_g ? 1 : 0;
    t.nfev = f.nfev;
    t.margin = NAN;
    t.noise = NAN;
    t.curv = NAN;
    if (f.track) {
        t.margin = fmin(trace.cmp, trace.sign);
        t.curv = 0.5 * (f_up + f_dn) - f_stop;
        t.noise = f.noise;
    }
    return t;
}

}  // namespace crm
