"""An extended-precision checker for the background constructor's decompositions (plain helper module, not a test).

``cellregmap_amd/csrc/background.hip`` returns, per grid point rho,

    Sigma(rho) = rho E1 E1' + (1 - rho) B B' = Q0 diag(S0) Q0'        (Q0: n x r, S0: r)

and, in the thin branch (n > cols = k1 + kb), the mixing matrix with Q0 = H Mix, H = [E1, B].  ``measure`` is given the host
inputs and such a candidate and evaluates, in ``numpy.longdouble`` straight from the half factor

    orthonormality   max |Q0'Q0 - I|
    reconstruction   max |Q0 diag(S0) Q0' - hS hS'|,   hS = [sqrt(rho) E1, sqrt(1 - rho) B]
    spectrum         S0 against LAPACK's: squared singular values of hS (thin; oracle/sugar.py: economic_qs_linear) or
                     eigvalsh of Sigma (n <= cols), and against the prescribed eigenvalues where a family has them
    rank             the documented rule applied to the reference spectrum
    mixing matrix    max |Mix' (H'H) Mix - I| (evaluated as (H Mix)'(H Mix), see ``measure``), |H Mix - Q0| elementwise, exact
                     zeros in the padding

``check`` asserts them.  It imports nothing of the library and needs no GPU.

Tolerances -- all taken from the project, none fitted to what any implementation gives:
  * spectrum and reconstruction: SPECTRUM_TOL * dim * S_max with dim the order of the diagonalised matrix (``_check`` of
    tests/test_gpu_eigh.py); the reconstruction also gets the part the rank rule dropped, which is bounded by its largest
    dropped reference eigenvalue -- itself asserted to be at most rel_tol * S_max (thin) or below sqrt(eps) (n <= cols);
  * orthonormality: ORTHO_CAP (tests/test_gpu_interaction.py: test_constructor_in_phases_with_exchanged_grid_points; the
    constructor's own contract: slab threshold 2e-13, polish target 2e-14);
  * Mix' C Mix - I: MIX_CAP;
  * H Mix - Q0: cols * 2^-52 * (|H| |Mix|), the a-priori bound of a length-cols inner product in float64.

``seal_keeps_mix`` states from the reference spectra what ``seal`` must decide (S_max <= 1e6 S_min at every grid point), and
refuses an input within a factor SEAL_MARGIN of that line.

The rank is a fact about the input, not about rounding: a case is refused (``CaseRefused``) unless every reference
eigenvalue of the grid point is at least RANK_MARGIN away from the cut, as a factor.

Products: everything in longdouble up to order FULL_ORDER.  Beyond it the r x r and n x n products are float64 BLAS (their
own rounding, ~ n * 1e-16, is far inside the caps) and PROBES unit vectors x are pushed through in longdouble:
Sigma x = hS (hS'x) against Q0 (S0 * (Q0'x)), and Q0'(Q0 (Q0'x)) against Q0'x.  For a unit vector
|(A - B) x|_inf <= |A - B|_2, so the probes are held to the same figures as the full products.

The families of tests/test_background_reference_cpu.py and tests/test_gpu_background_reference.py are here as well
(``random_family``, ``prescribed_family``, ``duplicated_family``, ...): both modules check the same inputs.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise RuntimeError("numpy.longdouble on this host has eps %.3g: the background reference needs an extended type "
                       "(eps <= 1e-18) and does not stand in for one with float64" % float(np.finfo(LD).eps))

SQRT_EPS = 1.4901161193847656e-08     # numpy_sugar.epsilon.small: the cut of the n <= cols branch (absolute)
DEFAULT_REL_TOL = 1e-12               # the thin branch's cut relative to the largest eigenvalue
SPECTRUM_TOL = 1e-13                  # x dim x S_max
ORTHO_CAP = 1e-12
MIX_CAP = 1e-12
RANK_MARGIN = 10.0
FULL_ORDER = 400
PROBES = 8
U64 = 2.0 ** -52
RHO_GRID = np.linspace(0, 1, 11)      # the engine's grid (cellregmap_amd/_engine.py: _RHO_GRID), exact 0 and 1


class CaseRefused(ValueError):
    """The input does not decide its own rank: an eigenvalue sits within RANK_MARGIN of the cut."""


def is_thin(E1, B):
    n, k1 = E1.shape
    return n > k1 + (0 if B is None else B.shape[1])


def half_stack(E1, B):
    """H = [E1, B] (float64)."""
    E1 = np.asarray(E1, float)
    return E1 if B is None else np.hstack([E1, np.asarray(B, float)])


def scaled_half(E1, B, rho, dtype=LD):
    """hS(rho) = [sqrt(rho) E1, sqrt(1 - rho) B]; the weights are taken in ``dtype`` from the float64 rho."""
    a = np.sqrt(dtype(rho))
    b = np.sqrt(dtype(1) - dtype(rho))
    E1 = np.asarray(E1, float).astype(dtype)
    if B is None:
        return a * E1
    return np.hstack([a * E1, b * np.asarray(B, float).astype(dtype)])


def reference_spectrum(E1, B, rho):
    """(spectrum, dim): LAPACK's float64 spectrum of Sigma(rho) by the reference's own route for the branch, in the
    order the branch promises -- descending squared singular values of hS (thin), ascending eigvalsh of Sigma."""
    if is_thin(E1, B):
        hS = scaled_half(E1, B, rho, float)
        return np.linalg.svd(hS, compute_uv=False) ** 2, hS.shape[1]
    hS = scaled_half(E1, B, rho)
    if hS.shape[0] <= FULL_ORDER:
        Sigma = (hS @ hS.T).astype(float)
    else:
        h = hS.astype(float)
        Sigma = h @ h.T
    return np.linalg.eigvalsh(Sigma), hS.shape[0]


def rank_rule(lam, thin, rel_tol=None):
    """(rank, cut, margin): the documented rule on a spectrum; margin = the smallest factor between an eigenvalue and
    the cut (inf for an empty or all-zero spectrum)."""
    lam = np.asarray(lam, float)
    if thin:
        cut = (DEFAULT_REL_TOL if not rel_tol or rel_tol <= 0 else rel_tol) * max(lam.max(initial=0.0), 0.0)
        kept = (lam > cut) & (lam > 0)
    else:
        cut = SQRT_EPS
        kept = lam >= cut
    margin = np.inf
    if cut > 0:
        if kept.any():
            margin = min(margin, lam[kept].min() / cut)
        low = lam[~kept]
        low = low[low > 0]
        if low.size:
            margin = min(margin, cut / low.max())
    return int(kept.sum()), cut, float(margin)


SEAL_CONDITION = 1e6      # seal keeps the mixing matrices while S_max <= 1e6 S_min at every grid point
SEAL_MARGIN = 2.0


def seal_keeps_mix(E1, B, rho_grid, rel_tol=None):
    """Whether ``seal`` keeps the mixing matrices of a thin background, from the reference spectra: the largest
    S_max / S_min of a kept spectrum over the grid against SEAL_CONDITION.  Refused within a factor SEAL_MARGIN of it."""
    worst = 1.0
    for rho in rho_grid:
        lam, _ = reference_spectrum(E1, B, float(rho))
        r, _, _ = rank_rule(lam, True, rel_tol)
        if r > 0:
            worst = max(worst, lam[:r].max() / lam[:r].min())
    if max(worst / SEAL_CONDITION, SEAL_CONDITION / worst) < SEAL_MARGIN * (1 - 1e-6):    # (1e-6: the spectra are float64 results)
        raise CaseRefused("S_max / S_min = %.3g is within a factor %g of seal's %g" % (worst, SEAL_MARGIN, SEAL_CONDITION))
    return bool(worst <= SEAL_CONDITION)


def _kept(lam, thin, r):
    lam = np.asarray(lam)
    return lam[:r] if thin else lam[lam.shape[0] - r:]


def _probes(n, seed=20260):
    X = np.random.default_rng(seed).normal(size=(n, PROBES)).astype(LD)
    return X / np.sqrt((X * X).sum(axis=0))


def measure(E1, B, rho, Q0, S0, r, rel_tol=None, Mix=None, prescribed=None):
    """Figures and violations of a candidate decomposition of one grid point.

    ``Mix``: the mixing matrix in the library's layout (ldh x ldq, zero padded) or tight (cols x r); thin branch only.
    ``prescribed``: every eigenvalue of Sigma(rho) as the family prescribes them (any order, zeros may be left out).
    Returns ``(figures, violations)``; raises ``CaseRefused`` when the input does not decide its rank."""
    E1 = np.asarray(E1, float)
    n, k1 = E1.shape
    kb = 0 if B is None else B.shape[1]
    cols = k1 + kb
    thin = n > cols
    tol_rel = DEFAULT_REL_TOL if not rel_tol or rel_tol <= 0 else float(rel_tol)
    bad = []
    fig = {"thin": bool(thin), "n": int(n), "cols": int(cols), "rho": float(rho)}

    lam_ref, dim = reference_spectrum(E1, B, rho)
    s_max = float(max(lam_ref.max(), 0.0))
    r_ref, cut, margin = rank_rule(lam_ref, thin, tol_rel)
    if margin < RANK_MARGIN:
        raise CaseRefused("rho=%g: a reference eigenvalue sits a factor %.3g from the cut %.3g (asked: %g)"
                          % (rho, margin, cut, RANK_MARGIN))
    fig.update(dim=int(dim), s_max=s_max, rank=int(r_ref), rank_margin=margin)
    if prescribed is not None:
        pres = np.sort(np.asarray(prescribed, LD))[::-1]
        p_rank, _, p_margin = rank_rule(pres.astype(float), thin, tol_rel)
        if p_margin < RANK_MARGIN:
            raise CaseRefused("rho=%g: a prescribed eigenvalue sits a factor %.3g from the cut" % (rho, p_margin))
        if p_rank != r_ref:
            bad.append("rank: prescribed spectrum keeps %d, LAPACK's %d" % (p_rank, r_ref))
    if int(r) != r_ref:
        bad.append("rank: %d, the rule keeps %d of the reference spectrum (cut %.3g, margin %.3g)" % (r, r_ref, cut, margin))
    Q0 = np.asarray(Q0, float)
    S0 = np.asarray(S0, float)
    if Q0.shape != (n, r) or S0.shape != (r,):
        bad.append("shape: Q0 %s, S0 %s for n=%d, r=%d" % (Q0.shape, S0.shape, n, r))
        return fig, bad

    # what the rule dropped: bounded by its largest reference eigenvalue, which the rule itself bounds
    low = np.sort(np.abs(np.asarray(lam_ref, float)))[:dim - r_ref] if r_ref < dim else np.zeros(0)
    dropped = float(low.max(initial=0.0))
    if thin and dropped > tol_rel * s_max or (not thin and dropped >= SQRT_EPS):
        bad.append("dropped part %.3g beyond its documented bound" % dropped)
    tol = SPECTRUM_TOL * dim * s_max
    scale = s_max if s_max > 0 else 1.0

    # ---- spectrum: order, LAPACK's values, prescribed values
    if r > 1 and not np.all(np.diff(S0) <= 0 if thin else np.diff(S0) >= 0):
        bad.append("order: S0 is not %s" % ("descending" if thin else "ascending"))
    if r == r_ref and r > 0:
        err = float(np.abs(S0.astype(LD) - _kept(lam_ref, thin, r).astype(LD)).max())
        fig["spectrum"] = err / scale
        if err > tol:
            bad.append("spectrum: |S0 - LAPACK| = %.3g > %.3g" % (err, tol))
        if prescribed is not None and pres.shape[0] >= r:
            want = pres[:r] if thin else pres[:r][::-1]
            err = float(np.abs(S0.astype(LD) - want).max())
            fig["spectrum_prescribed"] = err / scale
            if err > tol:
                bad.append("spectrum: |S0 - prescribed| = %.3g > %.3g" % (err, tol))

    # ---- orthonormality and reconstruction (longdouble while the ORDER of the product is at most FULL_ORDER)
    hS = scaled_half(E1, B, rho)
    X = _probes(n)
    Ql, Sl = Q0.astype(LD), S0.astype(LD)
    if r > 0:
        if r <= FULL_ORDER:
            ortho = float(np.abs(Ql.T @ Ql - np.eye(r, dtype=LD)).max())
        else:
            ortho = float(np.abs(Q0.T @ Q0 - np.eye(r)).max())
            T = Ql.T @ X
            ortho = max(ortho, float(np.abs(Ql.T @ (Ql @ T) - T).max()))
        fig["ortho"] = ortho
        if not ortho <= ORTHO_CAP:
            bad.append("orthonormality: |Q0'Q0 - I| = %.3g > %.3g" % (ortho, ORTHO_CAP))
    if n <= FULL_ORDER:
        recon = float(np.abs((Ql * Sl) @ Ql.T - hS @ hS.T).max())
    else:
        h = hS.astype(float)
        recon = float(np.abs((Q0 * S0) @ Q0.T - h @ h.T).max())
        recon = max(recon, float(np.abs(Ql @ (Sl[:, None] * (Ql.T @ X)) - hS @ (hS.T @ X)).max()))
    fig["reconstruction"] = recon / scale
    fig["dropped"] = dropped / scale
    if not recon <= tol + dropped:
        bad.append("reconstruction: |Q0 S0 Q0' - Sigma| = %.3g > %.3g + %.3g (dropped)" % (recon, tol, dropped))

    # ---- mixing matrix
    if Mix is not None:
        if not thin:
            bad.append("mixing matrix given for the n <= cols branch")
            return fig, bad
        Mix = np.asarray(Mix, float)
        if Mix.shape[0] < cols or Mix.shape[1] < r:
            bad.append("mixing matrix %s smaller than cols x r = %d x %d" % (Mix.shape, cols, r))
            return fig, bad
        if np.any(Mix[cols:, :] != 0) or np.any(Mix[:, r:] != 0):
            bad.append("mixing matrix: non-zero in its padding (rows >= cols or columns >= r)")
        if kb > 0 and rho >= 1.0 and np.any(Mix[k1:cols, :] != 0):
            bad.append("mixing matrix: non-zero in the rows of B at rho = 1")
        if r > 0:
            M = Mix[:cols, :r]
            H = half_stack(E1, B)
            if max(cols, r) <= FULL_ORDER:
                # Mix' C Mix with C = H'H is evaluated as (H Mix)'(H Mix): the same number, but a C rounded once -- even
                # to longdouble -- enters amplified by |Mix|^2 ~ 1 / S_min, which for a spectrum over nine decades is more
                # than the cap; the product H Mix only carries |Mix| ~ S_min^-1/2
                rows = np.arange(n)
                Hl, Ml = H.astype(LD), M.astype(LD)
                Y = Hl @ Ml
                defect = float(np.abs(Y.T @ Y - np.eye(r, dtype=LD)).max())
            else:
                Y64 = H @ M
                defect = float(np.abs(Y64.T @ Y64 - np.eye(r)).max())
                rows = np.unique(np.linspace(0, n - 1, PROBES).astype(int))
                Hl, Ml = H[rows].astype(LD), M.astype(LD)
                Y = Hl @ Ml
            fig["mix_defect"] = defect
            if not defect <= MIX_CAP:
                bad.append("mixing matrix: |Mix' C Mix - I| = %.3g > %.3g" % (defect, MIX_CAP))
            diff = np.abs(Y - Ql[rows])
            bound = cols * LD(U64) * (np.abs(Hl) @ np.abs(Ml))
            share = float((diff / np.where(bound > 0, bound, LD(1))).max()) if np.all(diff[bound == 0] == 0) else np.inf
            fig["h_mix_share"] = share
            if not share <= 1.0:
                bad.append("mixing matrix: |H Mix - Q0| reaches %.3g of cols 2^-52 |H||Mix|" % share)
    return fig, bad


def check(E1, B, rho, Q0, S0, r, rel_tol=None, Mix=None, prescribed=None):
    """``measure`` asserted: the figures, or an AssertionError that names every violated condition."""
    fig, bad = measure(E1, B, rho, Q0, S0, r, rel_tol=rel_tol, Mix=Mix, prescribed=prescribed)
    assert not bad, "rho=%g (n=%d, cols=%d): " % (rho, fig["n"], fig["cols"]) + "; ".join(bad)
    return fig


def check_grid(E1, B, rho_grid, read, rel_tol=None, mixes=None, prescribed=None, points=None):
    """``check`` at every grid point (or at ``points``), the grid points side by side on threads -- numpy's longdouble
    products are plain loops that release the interpreter lock.  ``read(i) -> (Q0, S0, r)``; ``mixes``: per grid point
    or None; ``prescribed(rho) -> eigenvalues`` or None.  Returns the list of figures."""
    from concurrent.futures import ThreadPoolExecutor

    points = list(range(len(rho_grid))) if points is None else list(points)
    got = {i: read(i) for i in points}       # (the library is asked from one thread)

    def one(i):
        Q0, S0, r = got[i]
        return check(E1, B, float(rho_grid[i]), Q0, S0, r, rel_tol=rel_tol, Mix=None if mixes is None else mixes[i],
                     prescribed=None if prescribed is None else prescribed(float(rho_grid[i])))

    with ThreadPoolExecutor(max_workers=min(len(points), 12)) as ex:
        return list(ex.map(one, points))


def worst(figures):
    """Maxima over grid points of the figures ``check`` returned (the record of a case)."""
    out = {}
    for key in ("ortho", "spectrum", "spectrum_prescribed", "reconstruction", "mix_defect", "h_mix_share"):
        vals = [f[key] for f in figures if key in f]
        if vals:
            out[key] = max(vals)
    out["rank_margin"] = min(f["rank_margin"] for f in figures)
    out["ranks"] = [f["rank"] for f in figures]
    return out


# ---- the reference's own decompositions (LAPACK), in the library's conventions ----------------------------------------
def lapack_decomposition(E1, B, rho, rel_tol=None, through_mix=False):
    """(Q0, S0, r, Mix) as the reference forms them -- thin: U and s^2 of LAPACK's SVD of hS, cut by the library's rank
    rule (the reference keeps all of them), and Mix = D(rho) V s^-1 from the same SVD; otherwise ``economic_qs`` of Sigma
    (oracle/sugar.py).  ``through_mix``: Q0 is the float64 product H Mix (the library's form with LAPACK's V) instead
    of U, which equals it only to the SVD's backward error eps S_max^1/2 / S_j^1/2."""
    from oracle.sugar import economic_qs_linear

    E1 = np.asarray(E1, float)
    hS = scaled_half(E1, B, rho, float)
    if is_thin(E1, B):
        U, s, Vt = np.linalg.svd(hS, full_matrices=False)
        (Q,), S = economic_qs_linear(hS, return_q1=False)
        assert np.array_equal(S, s ** 2) and np.array_equal(Q, U)
        r, _, _ = rank_rule(S, True, rel_tol)
        w = np.r_[np.full(E1.shape[1], np.sqrt(rho)), np.full(hS.shape[1] - E1.shape[1], np.sqrt(1.0 - rho))]
        Mix = w[:, None] * Vt[:r].T / s[:r]
        return (half_stack(E1, B) @ Mix if through_mix else U[:, :r]), S[:r], r, Mix
    (Q,), S = economic_qs_linear(hS, return_q1=False)
    return Q, S, S.shape[0], None


# ---- families ---------------------------------------------------------------------------------------------------------
def random_family(n, k1, kb, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, k1)), (rng.normal(size=(n, kb)) if kb else None)


def prescribed_family(n, s1sq, s2sq, seed):
    """E1 = P[:, :k1] diag(s1), B = P[:, k1:] diag(s2) R2' with P'P = I and R2 orthogonal: Sigma(rho) has the eigenvalues
    rho s1^2 and (1 - rho) s2^2 (and zeros).  n <= cols is allowed: P then is n x n and the trailing s2 are unused --
    give len(s1sq) + len(s2sq) <= n for a fully prescribed spectrum there, which makes the case a thin one."""
    rng = np.random.default_rng(seed)
    s1sq, s2sq = np.asarray(s1sq, float), np.asarray(s2sq, float)
    k1, kb = s1sq.shape[0], s2sq.shape[0]
    P, _ = np.linalg.qr(rng.normal(size=(n, k1 + kb)))
    R2, _ = np.linalg.qr(rng.normal(size=(kb, kb)))
    return P[:, :k1] * np.sqrt(s1sq), (P[:, k1:] * np.sqrt(s2sq)) @ R2.T


def prescribed_spectrum(s1sq, s2sq, rho):
    return np.r_[LD(rho) * np.asarray(s1sq, float).astype(LD), (LD(1) - LD(rho)) * np.asarray(s2sq, float).astype(LD)]


def rank_rule_family(rel_tol=None, n=200, k1=6, kb=60, seed=11):
    """Thin, prescribed: eigenvalues at 100 x and 1 / 100 x the cut rel_tol * max (default 1e-12: 1e-10 and 1e-14 of the
    maximum).  E1 carries one kept small value (rank(rho = 1) = k1), B five kept and five dropped ones
    (rank(rho = 0) = kb - 5).  max(rho, 1 - rho) >= 1 / 2 is the largest eigenvalue at every grid point and the small ones
    scale with rho or 1 - rho >= 1 / 10, so on the engine's grid the kept ones stay >= 100 / 9 and the dropped ones
    <= 1 / 100 of the cut."""
    t = DEFAULT_REL_TOL if not rel_tol or rel_tol <= 0 else rel_tol
    s1sq = np.r_[np.linspace(1.0, 0.2, k1 - 1), 100 * t]
    s2sq = np.r_[np.geomspace(1.0, 1e-3, kb - 10), 100 * t * np.array([1.0, 1.5, 2.0, 3.0, 4.0]),
                 t / 100 * np.array([1.0, 0.8, 0.6, 0.4, 0.2])]
    E1, B = prescribed_family(n, s1sq, s2sq, seed)
    return E1, B, s1sq, s2sq


def geometric_family(cols, k1=5, extra=30, decades=9.0, seed=5):
    """Thin, prescribed: a geometric spectrum over ``decades`` in B, well-conditioned values inside it in E1; every
    eigenvalue is kept at every grid point (1e-9 / 9 of the maximum at worst against the cut 1e-12)."""
    kb = cols - k1
    s2sq = np.geomspace(1.0, 10.0 ** -decades, kb)
    s1sq = np.linspace(2e-3, 1e-3, k1)
    E1, B = prescribed_family(cols + extra, s1sq, s2sq, seed)
    return E1, B, s1sq, s2sq


def conditioned_family(cond, n=200, k1=6, kb=60, seed=17):
    """Thin, prescribed, S_max / S_min = cond at the worst grid point: B spans [1 / cond, 1] (that is rho = 0), and
    E1's values lie so that rho s1^2 stays inside (1 - rho) [1 / cond, 1] for rho in [0.1, 0.9]."""
    s2sq = np.geomspace(1.0, 1.0 / cond, kb)
    s1sq = np.linspace(2e-3, 1e-3, k1)
    assert 0.1 * s1sq.min() >= 0.9 / cond and 0.9 * s1sq.max() <= 0.1
    E1, B = prescribed_family(n, s1sq, s2sq, seed)
    return E1, B, s1sq, s2sq


def eigh_prescribed_family(n=60, k1=10, kb=100, seed=23):
    """n <= cols with a known spectrum: E1 and B share an orthonormal P (n x n); E1 = P[:, :k1] diag(s1) and
    B = P[:, k1:] diag(s2) Z' with Z (kb x (n - k1)) of orthonormal columns, so that Sigma(rho) = P diag(rho s1^2,
    (1 - rho) s2^2) P'.  lam_max ~ 1; values at 1.5e-6 (kept) and 1.5e-10 (dropped) on either side of sqrt(eps) -- a factor
    100 / 10 at rho = 0.1 and 0.9."""
    rng = np.random.default_rng(seed)
    P, _ = np.linalg.qr(rng.normal(size=(n, n)))
    Z, _ = np.linalg.qr(rng.normal(size=(kb, n - k1)))
    s1sq = np.r_[np.linspace(1.0, 0.3, k1 - 2), 1.5e-6, 1.5e-10]
    s2sq = np.r_[np.geomspace(1.0, 1e-2, n - k1 - 6), 1.5e-6 * np.array([1.0, 2.0, 3.0]), 1.5e-10 * np.array([1.0, 0.5, 0.25])]
    return P[:, :k1] * np.sqrt(s1sq), (P[:, k1:] * np.sqrt(s2sq)) @ Z.T, s1sq, s2sq


def duplicated_family(n, k1, kb, dup=20, seed=31):
    """Random normal with the last ``dup`` columns of B repeating its first ones: ``dup`` exact null directions."""
    E1, B = random_family(n, k1, kb, seed)
    B[:, kb - dup:] = B[:, :dup]
    return E1, B


def hadamard_family(n, k1, k2, m, seed):
    """(E1, us, hK, B) with B[i, j * m + d] = us[i, j] hK[i, d] written out."""
    rng = np.random.default_rng(seed)
    E1 = rng.normal(size=(n, k1))
    us = rng.normal(size=(n, k2))
    hK = rng.normal(size=(n, m)) / np.sqrt(m)
    B = (us[:, :, None] * hK[:, None, :]).reshape(n, k2 * m)
    return E1, us, hK, B
