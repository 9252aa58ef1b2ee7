"""The Davies branch of csrc/davies.hip (``qfc_wave`` and what it calls) restated in numpy float64 (plain helper module,
not a test).  The scalar search runs as the wavefront runs it; every sum over the weights is taken lane by lane and then
across the 64 lanes; ``integrate`` forms the kernel's integrand -- one complex product per abscissa, descending j, fused
multiply-adds, powers of two taken out where (j & 3) == 0, the crossings of the negative real axis counted, one atan2 and
one log -- for all abscissas at once.

Two things differ from the device in the last place only: numpy's exp / log / sin / atan2 are the host's, and a fused
multiply-add is taken in the 64-bit significand of long double and then rounded to double, which is the fused result
except at double-rounding ties.

``slip`` imitates one mistake a kernel of this form could make (tests/test_oracle_davies_widths_cpu.py shows that each
falls outside the limit the device is held to):
    "tail_skip64"    weight index 64 left out of tail_bound
    "lost_turn"      one turn lost at one abscissa of the main integration (the heaviest one that has turned at all)
    "rescale_expo"   the exponent of one rescale dropped at that abscissa
    "last_abscissa"  k = nterm omitted from the main integration
    "aux_factor"     1 - exp(-tausq u^2 / 2) missing from the auxiliary integration
    "aux_sigsq"      sigsq not increased after the auxiliary integration
    "turns_on_re"    crossings counted on the real part instead of the imaginary part
"""
import math

import numpy as np

LN28 = 0.08664339756999316
LIM = 10000
ACC = 1e-6
SLIPS = ("tail_skip64", "lost_turn", "rescale_expo", "last_abscissa", "aux_factor", "aux_sigsq", "turns_on_re")

_XOR = [np.arange(64) ^ s for s in (1, 2, 4, 8, 16, 32)]


def _wsum(v):
    """Per-lane partial sums in loop order (lane, lane + 64, ..), then across the lanes by a butterfly."""
    v = np.asarray(v, float)
    n = -(-v.size // 64) * 64
    lanes = np.zeros(n)
    lanes[: v.size] = v
    lanes = np.add.reduce(lanes.reshape(-1, 64), axis=0)
    for idx in _XOR:
        lanes = lanes + lanes[idx]
    return float(lanes[0])


def _exp_guard(x):
    return 0.0 if x < -50.0 else math.exp(x)


def _log1p_variant(x, first):
    """AS 155 "log1", elementwise: log(1 + x) when first, else log(1 + x) - x; its series for |x| <= 0.1."""
    x = np.asarray(x, float)
    big = np.abs(x) > 0.1
    with np.errstate(all="ignore"):
        out = np.where(first, np.log(1.0 + x), np.log(1.0 + x) - x)
        y = x / (2.0 + x)
        term = 2.0 * y * y * y
        k = 3.0
        s = (2.0 if first else -x) * y
        y = y * y
        s1 = s + term / k
        for _ in range(64):
            if np.all((s1 == s) | big):
                break
            k += 2.0
            term = term * y
            s = s1
            s1 = s + term / k
    return np.where(big, out, s)


def _fma(a, b, c):
    return (np.asarray(a, np.longdouble) * b + c).astype(np.float64)


class _Qf:
    pass


def _tick(q):
    q.count += 1
    if q.count > q.lim:
        q.overflow = True


def _tail_bound(q, u):
    _tick(q)
    xconst = u * q.sigsq
    sum1 = u * xconst
    u = 2.0 * u
    lb = q.lb
    x = u * lb
    y = 1.0 - x
    with np.errstate(all="ignore"):
        pc = lb / y
        ps = x * x / y + _log1p_variant(-x, False)
    if q.slip == "tail_skip64" and q.r > 64:
        pc[64] = 0.0
        ps[64] = 0.0
        q.applied = True
    xconst += _wsum(pc)
    sum1 += _wsum(ps)
    return _exp_guard(-0.5 * sum1), xconst


def _cutoff(q, accx, upn):
    u2, u1, c1, c2 = upn, 0.0, q.mean, 0.0
    rb = 2.0 * (q.lmax if u2 > 0.0 else q.lmin)
    u = u2 / (1.0 + u2 * rb)
    while not q.overflow:
        t, c2 = _tail_bound(q, u)
        if not t > accx:
            break
        u1 = u2
        c1 = c2
        u2 = 2.0 * u2
        u = u2 / (1.0 + u2 * rb)
    u = (c1 - q.mean) / (c2 - q.mean)
    while not q.overflow and u < 0.9:
        u = (u1 + u2) / 2.0
        t, xconst = _tail_bound(q, u / (1.0 + u * rb))
        if t > accx:
            u1, c1 = u, xconst
        else:
            u2, c2 = u, xconst
        u = (c1 - q.mean) / (c2 - q.mean)
    return c2, u2


def _trunc_bound(q, u, tausq):
    _tick(q)
    sum2 = (q.sigsq + tausq) * u * u
    prod1 = 2.0 * sum2
    u = 2.0 * u
    x = (u * q.lb) * (u * q.lb)
    over = x > 1.0
    with np.errstate(all="ignore"):
        l1 = _log1p_variant(x, True)
        p1 = np.where(over, 0.0, l1)
        p2 = np.where(over, np.log(np.where(over, x, 1.0)), 0.0)
        p3 = np.where(over, l1, 0.0)
    s = int(over.sum())
    prod1 += _wsum(p1)
    prod2 = _wsum(p2) + prod1
    prod3 = _wsum(p3) + prod1
    x = _exp_guard(-0.25 * prod2) / math.pi
    y = _exp_guard(-0.25 * prod3) / math.pi
    err1 = 1.0 if s == 0 else x * 2.0 / s
    err2 = 2.5 * y if prod3 > 1.0 else 1.0
    if err2 < err1:
        err1 = err2
    x = 0.5 * sum2
    err2 = 1.0 if x <= y else y / x
    return err1 if err1 < err2 else err2


def _find_trunc_point(q, utx, accx):
    ut = utx
    u = ut / 4.0
    if _trunc_bound(q, u, 0.0) > accx:
        u = ut
        while not q.overflow and _trunc_bound(q, u, 0.0) > accx:
            ut *= 4.0
            u = ut
    else:
        ut = u
        u = u / 4.0
        while not q.overflow and _trunc_bound(q, u, 0.0) <= accx:
            ut = u
            u = u / 4.0
    for d in (2.0, 1.4, 1.2, 1.1):
        u = ut / d
        if _trunc_bound(q, u, 0.0) <= accx:
            ut = u
    return ut


def integrand(lb, c, sigsq, nterm, interv, tausq, mainx, slip=None):
    """(a1 terms, a2 terms, whether the slip changed anything) of ``integrate`` at k = nterm, nterm - 1, .., 0 -- lane l
    takes every 64th from the l-th on."""
    applied = False
    r = lb.size
    k = np.arange(nterm, -1, -1, dtype=float)
    u = (k + 0.5) * interv
    sum1 = -2.0 * u * c
    sum2 = np.abs(sum1)
    sum3 = -0.5 * sigsq * u * u
    re = np.ones_like(u)
    im = np.zeros_like(u)
    turns = np.zeros(u.size, np.int64)
    turns_re = np.zeros(u.size, np.int64)
    expo = np.zeros(u.size, np.int64)
    first_e = np.zeros(u.size, np.int64)       # the first non-zero exponent taken out per abscissa ("rescale_expo")
    u2 = 2.0 * u
    for j in range(r - 1, -1, -1):
        x = lb[j] * u2
        nre = _fma(-im, x, re)
        nim = _fma(re, x, im)
        turns += (im >= 0.0) & (nim < 0.0)
        if slip == "turns_on_re":
            turns_re += (re >= 0.0) & (nre < 0.0)
        re, im = nre, nim
        if (j & 3) == 0:
            e = np.frexp(np.maximum(np.abs(re), np.abs(im)))[1].astype(np.int64)
            re = np.ldexp(re, -e)
            im = np.ldexp(im, -e)
            expo += e
            first_e = np.where(first_e == 0, e, first_e)
    if mainx and slip in ("lost_turn", "rescale_expo"):
        with np.errstate(all="ignore"):
            s3 = sum3 - 0.25 * (np.log(re * re + im * im) + 2.0 * 0.6931471805599453 * expo)
            weight = np.where(s3 < -50.0, 0.0, np.exp(s3)) / u
        cand = np.where(turns >= 1 if slip == "lost_turn" else first_e != 0, weight, -1.0)
        if cand.max() > 0:
            i = int(np.argmax(cand))
            applied = True
            if slip == "lost_turn":
                turns[i] -= 1
            else:
                expo[i] -= first_e[i]
    if slip == "turns_on_re":
        differs = turns_re != turns
        turns = turns_re
    theta = np.arctan2(im, re) + 2.0 * math.pi * turns
    logmod2 = np.log(re * re + im * im) + 2.0 * 0.6931471805599453 * expo
    sum1 = sum1 + theta
    sum2 = sum2 + theta
    sum3 = sum3 - 0.25 * logmod2
    with np.errstate(all="ignore"):
        x = (interv / math.pi) * np.where(sum3 < -50.0, 0.0, np.exp(sum3)) / u
        if not mainx and slip != "aux_factor":
            t = -0.5 * tausq * u * u
            x = x * (1.0 - np.where(t < -50.0, 0.0, np.exp(t)))
        elif not mainx:
            applied = True
    if slip == "turns_on_re":
        applied = bool(np.any(differs & (x != 0.0)))
    a1 = np.sin(0.5 * sum1) * x
    a2 = 0.5 * sum2 * x
    if mainx and slip == "last_abscissa":
        a1[0] = 0.0
        a2[0] = 0.0
        applied = True
    return a1, a2, applied


def _integrate(q, nterm, interv, tausq, mainx):
    a1, a2, applied = integrand(q.lb, q.c, q.sigsq, nterm, interv, tausq, mainx, q.slip)
    q.applied = q.applied or applied
    q.intl += _wsum(a1)
    q.ersm += _wsum(a2)
    q.terms += nterm + 1
    q.nint += 1


def _conv_coef(q, x):
    _tick(q)
    axl = abs(x)
    sxl = 1.0 if x > 0.0 else -1.0
    sum1 = 0.0
    for j in range(q.r - 1, -1, -1):
        t = q.r - 1 - j
        lt = float(q.lb[t])
        if lt * sxl > 0.0:
            lj = abs(lt)
            axl1 = axl - lj
            axl2 = lj / LN28
            if axl1 > axl2:
                axl = axl1
            else:
                if axl > axl2:
                    axl = axl2
                sum1 = (axl - axl1) / lj
                sum1 += float(j)
                break
    if sum1 > 100.0:
        q.fail = True
        return 1.0
    return math.pow(2.0, sum1 / 4.0) / (math.pi * axl * axl)


def qfc(lam, c, slip=None):
    """(cdf, ifault, (evaluation counter, terms, integrations)) as ``qfc_wave`` gives them for ascending positive weights;
    with a slip, a fourth entry says whether the slip changed anything on this problem."""
    q = _Qf()
    q.lb = np.ascontiguousarray(lam, float)
    q.r = q.lb.size
    q.c = float(c)
    q.slip = slip
    q.sigsq = q.intl = q.ersm = 0.0
    q.count = q.terms = q.nint = 0
    q.lim = LIM
    q.fail = q.overflow = q.applied = False
    ifault = 0
    acc1, xlim = ACC, float(LIM)

    def out(cdf, fault):
        res = (cdf, fault, (q.count, q.terms, q.nint))
        return res if slip is None else res + (q.applied,)

    sd = _wsum(q.lb * q.lb * 2.0)
    q.mean = _wsum(q.lb)
    q.lmax = max(float(q.lb[-1]), 0.0)
    q.lmin = min(float(q.lb[0]), 0.0)
    assert q.lmin == 0.0 and q.lmax > 0.0, "positive weights only: the mixed-sign loop is not restated"
    sd = math.sqrt(sd)
    almx = q.lmax
    utx, up = 16.0 / sd, 4.5 / sd
    un = -up
    utx = _find_trunc_point(q, utx, 0.5 * acc1)
    if q.overflow:
        return out(-1.0, 4)
    if q.c != 0.0 and almx > 0.07 * sd:
        tausq = 0.25 * acc1 / _conv_coef(q, q.c)
        if q.fail:
            q.fail = False
        elif _trunc_bound(q, utx, tausq) < 0.2 * acc1:
            q.sigsq += tausq
            utx = _find_trunc_point(q, utx, 0.25 * acc1)
        if q.overflow:
            return out(-1.0, 4)
    acc1 *= 0.5
    while True:
        c2, up = _cutoff(q, acc1, up)
        d1 = c2 - q.c
        if q.overflow:
            return out(-1.0, 4)
        if d1 < 0.0:
            return out(1.0, 0)
        c2, un = _cutoff(q, acc1, un)
        d2 = q.c - c2
        if q.overflow:
            return out(-1.0, 4)
        if d2 < 0.0:
            return out(0.0, 0)
        intv = 2.0 * math.pi / (d1 if d1 > d2 else d2)
        xnt = utx / intv
        xntm = 3.0 / math.sqrt(acc1)
        if xnt <= xntm * 1.5:
            break
        if xntm > xlim:
            return out(-1.0, 1)
        ntm = int(math.floor(xntm + 0.5))
        intv1 = utx / ntm
        x = 2.0 * math.pi / intv1
        if x <= abs(q.c):
            break
        tausq = 0.33 * acc1 / (1.1 * (_conv_coef(q, q.c - x) + _conv_coef(q, q.c + x)))
        if q.overflow:
            return out(-1.0, 4)
        if q.fail:
            break
        acc1 *= 0.67
        _integrate(q, ntm, intv1, tausq, False)
        xlim -= xntm
        if slip != "aux_sigsq":
            q.sigsq += tausq
        else:
            q.applied = True
        utx = _find_trunc_point(q, utx, 0.25 * acc1)
        if q.overflow:
            return out(-1.0, 4)
        acc1 *= 0.75
    if xnt > xlim:
        return out(-1.0, 1)
    nt = int(math.floor(xnt + 0.5))
    _integrate(q, nt, intv, 0.0, True)
    qfval = 0.5 - q.intl
    upv = q.ersm
    x = upv + ACC / 10.0
    for rat in (1, 2, 4, 8):
        if rat * x == rat * upv:
            ifault = 2
    return out(qfval, ifault)
