// The donor structure of a background's kinship factor (crm_background_set_kinship_groups; objects.h: kin, kin_fold,
// kin_wb): the operands in donor order, the donor-level factor folded into the mixing matrices, and the per-donor
// eigen-decompositions of the unrelated-donor form.
#include <algorithm>
#include <atomic>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace crm {

// One Jacobi rotation (cosine cs, sine sn) in the plane of coordinates p, q: A <- J'A J and V <- V J for k x k row-major
// A and V.  Shared with the orthogonalisation of a gene's covariates (gene.hip), whose sweep skips and stops by other
// rules than jacobi_eigh below: only the rotation is common.
void jacobi_rotate(int k, double* A, double* V, int p, int q, double cs, double sn) {
    for (int r = 0; r < k; r++) {   // columns p, q
        const double arp = A[(size_t)r * k + p], arq = A[(size_t)r * k + q];
        A[(size_t)r * k + p] = cs * arp - sn * arq;
        A[(size_t)r * k + q] = sn * arp + cs * arq;
    }
    for (int r = 0; r < k; r++) {   // rows p, q
        const double apr = A[(size_t)p * k + r], aqr = A[(size_t)q * k + r];
        A[(size_t)p * k + r] = cs * apr - sn * aqr;
        A[(size_t)q * k + r] = sn * apr + cs * aqr;
    }
    for (int r = 0; r < k; r++) {
        const double vrp = V[(size_t)r * k + p], vrq = V[(size_t)r * k + q];
        V[(size_t)r * k + p] = cs * vrp - sn * vrq;
        V[(size_t)r * k + q] = sn * vrp + cs * vrq;
    }
}

// Symmetric eigen-decomposition A = V diag(w) V' of a small k x k matrix (row-major, destroyed) by cyclic Jacobi:
// rotations until every off-diagonal entry is below eps times the root of its two diagonal entries (the relative
// accuracy of the eigenvalues of a positive semidefinite Gram matrix).  V: k x k row-major, columns the eigenvectors.
static void jacobi_eigh(int k, std::vector<double>& A, std::vector<double>& V, std::vector<double>& w) {
    V.assign((size_t)k * k, 0.0);
    for (int i = 0; i < k; i++) V[(size_t)i * k + i] = 1.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < k - 1; p++)
            for (int q = p + 1; q < k; q++) {
                const double apq = A[(size_t)p * k + q], app = A[(size_t)p * k + p], aqq = A[(size_t)q * k + q];
                if (!(std::fabs(apq) > 2.220446049250313e-16 * std::sqrt(std::fabs(app * aqq))) || apq == 0.0) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                jacobi_rotate(k, A.data(), V.data(), p, q, cs, sn);
                A[(size_t)p * k + q] = A[(size_t)q * k + p] = 0.0;
            }
        if (!rotated) break;
    }
    w.resize(k);
    for (int i = 0; i < k; i++) w[i] = A[(size_t)i * k + i];
}

// Unrelated donors (objects.h: kin_wb): is the donor-level kinship hKd hKd' diagonal to rounding?  Then the per-donor
// eigen-decompositions of G_d = us_d'us_d and the rows R = Phi'E1, uploaded once per background.  Any off-diagonal entry
// above 8 m eps sqrt(kappa_d kappa_d') keeps the MixK route; so do k2 > 128, k1 > 64 and donor counts whose test or
// tables would be large.
static int seal_unrelated_donors(crm_background* bg, const double* hKd, long m) {
    bg->kin_wb = false;
    const long groups = bg->kin_groups;
    const int k1 = bg->kin_k1, k2 = bg->kin_k2, KK = k1 + k2;
    if (form("kin_diag", 1) == 0 || k2 > 128 || k1 > 64 || (double)groups * groups * m > 4e9) return CRM_OK;
    std::vector<double> kappa(groups, 0.0);
    for (long d = 0; d < groups; d++)
        for (long q = 0; q < m; q++) kappa[d] += hKd[d * m + q] * hKd[d * m + q];
    const double tol = 8.0 * (double)m * 2.220446049250313e-16;
    for (long d = 0; d < groups; d++)
        for (long e = d + 1; e < groups; e++) {
            double s = 0.0;
            for (long q = 0; q < m; q++) s += hKd[d * m + q] * hKd[e * m + q];
            if (!(std::fabs(s) <= tol * std::sqrt(kappa[d] * kappa[e]))) return CRM_OK;
        }
    crm_ctx* ctx = bg->ctx;
    hipStream_t st = ctx->stream;
    // [us | E1]'[us | E1] per donor over its own cells: G_d, us_d'E1_d and the donor's share of E1'E1
    const long ldc = round_up(KK, 128);
    if (sizeof(double) * (double)groups * KK * ldc > (double)(1ull << 30)) return CRM_OK;
    DevBuf dC, probs_dev;
    CRM_TRY(dC.ensure(sizeof(double) * (size_t)groups * KK * ldc));
    std::vector<GemmProblem> pr((size_t)groups);
    long maxlen = GEMM_BK;
    for (long d = 0; d < groups; d++) {
        GemmProblem p{};
        p.X = bg->kin_Y.as<double>() + bg->kin_row0[d] * bg->kin_ldy; p.ldx = bg->kin_ldy;
        p.Y = p.X; p.ldy = bg->kin_ldy;
        p.C = dC.as<double>() + (size_t)d * KK * ldc; p.ldc = ldc;
        p.M = KK; p.N = KK; p.cells = bg->kin_len[d];
        maxlen = std::max(maxlen, bg->kin_len[d]);
        pr[d] = p;
    }
    CRM_TRY(probs_dev.ensure(sizeof(GemmProblem) * pr.size()));
    CRM_HIP(hipMemcpyAsync(probs_dev.ptr, pr.data(), sizeof(GemmProblem) * pr.size(), hipMemcpyHostToDevice, st));
    CRM_TRY(launch_gemm_tn(ctx, probs_dev.as<GemmProblem>(), (int)groups, KK, KK, maxlen, false, 0, 1, 0));
    std::vector<double> C((size_t)groups * KK * ldc);
    CRM_HIP(hipMemcpyAsync(C.data(), dC.ptr, sizeof(double) * C.size(), hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    const int k2pad = (int)round_up(k2, GEMM_BK);
    const long P = groups * k2, ldp = round_up(P, 128);
    std::vector<double> hU((size_t)groups * k2pad * 128, 0.0), hR((size_t)k1 * ldp, 0.0), hEE((size_t)k1 * k1, 0.0),
        lam((size_t)P, 0.0);
    std::vector<double> A((size_t)k2 * k2), V, w;
    long kept = 0;
    for (long d = 0; d < groups; d++) {
        const double* Cd = C.data() + (size_t)d * KK * ldc;
        for (int i = 0; i < k2; i++)
            for (int j = 0; j < k2; j++) A[(size_t)i * k2 + j] = 0.5 * (Cd[i * ldc + j] + Cd[j * ldc + i]);
        jacobi_eigh(k2, A, V, w);
        double wmax = 0.0;
        for (int j = 0; j < k2; j++) wmax = std::max(wmax, w[j]);
        double* Ud = hU.data() + (size_t)d * k2pad * 128;
        for (int j = 0; j < k2; j++) {
            // (directions of us_d below rounding -- k2 > the donor's cells -- carry no variance: dropped)
            if (!(w[j] > (double)k2 * 2.220446049250313e-16 * wmax)) continue;
            const double sc = 1.0 / std::sqrt(w[j]);
            lam[d * k2 + j] = w[j];
            kept++;
            for (int q = 0; q < k2; q++) Ud[(size_t)q * 128 + j] = V[(size_t)q * k2 + j] * sc;
            for (int a = 0; a < k1; a++) {
                double s = 0.0;
                for (int q = 0; q < k2; q++) s += Ud[(size_t)q * 128 + j] * Cd[q * ldc + k2 + a];
                hR[(size_t)a * ldp + d * k2 + j] = s;
            }
        }
        for (int a = 0; a < k1; a++)
            for (int e = 0; e < k1; e++) hEE[(size_t)a * k1 + e] += Cd[(k2 + a) * ldc + k2 + e];
    }
    CRM_TRY(bg->wb_U.ensure(sizeof(double) * hU.size()));
    CRM_TRY(bg->wb_R.ensure(sizeof(double) * hR.size()));
    CRM_TRY(bg->wb_EE.ensure(sizeof(double) * hEE.size()));
    CRM_HIP(hipMemcpyAsync(bg->wb_U.ptr, hU.data(), sizeof(double) * hU.size(), hipMemcpyHostToDevice, st));
    CRM_HIP(hipMemcpyAsync(bg->wb_R.ptr, hR.data(), sizeof(double) * hR.size(), hipMemcpyHostToDevice, st));
    CRM_HIP(hipMemcpyAsync(bg->wb_EE.ptr, hEE.data(), sizeof(double) * hEE.size(), hipMemcpyHostToDevice, st));
    std::vector<std::vector<double>> s0(bg->nrho, std::vector<double>((size_t)ldp, 0.0));
    for (int i = 0; i < bg->nrho; i++) {
        for (long p = 0; p < P; p++) s0[i][p] = (1.0 - bg->rho[i]) * kappa[p / k2] * lam[p];
        CRM_TRY(bg->wb_S0[i].ensure(sizeof(double) * (size_t)ldp));
        CRM_HIP(hipMemcpyAsync(bg->wb_S0[i].ptr, s0[i].data(), sizeof(double) * (size_t)ldp, hipMemcpyHostToDevice, st));
    }
    CRM_HIP(hipStreamSynchronize(st));
    bg->wb_P = P;
    bg->wb_kept = kept;
    bg->wb_ldp = ldp;
    bg->wb_k2pad = k2pad;
    static std::atomic<unsigned long> wb_tables_made{0};
    bg->wb_gen = ++wb_tables_made;
    bg->kin_wb = true;
    return CRM_OK;
}

}  // namespace crm

extern "C" {

int crm_background_set_kinship_groups(crm_background* bg, const int* group, long groups, const double* hKd, long m,
                                      const double* U, int k2) {
    return crm::guarded_on("crm_background_set_kinship_groups", bg ? bg->ctx : nullptr, [&]() -> int {
    if (!bg || !group || !hKd || !U || groups < 1 || m < 1 || k2 < 1) return CRM_ERR_ARG;
    if (bg->builder) {
        set_error("kinship groups: the background is still under construction");
        return CRM_ERR_ARG;
    }
    const long n = bg->n;
    const int k1 = (int)(bg->cols - (long)k2 * m);
    // only backgrounds that kept their half factor H = [E1, L_1 .. L_k2] (thin branch, well-conditioned spectrum) can use it
    if (!bg->fast_T || !bg->H.ptr || k1 < 1 || k1 + k2 > 2 * CRM_MAX_K0 || groups > 4096) return CRM_OK;   // (kin_operand: one thread per column of [us | E1], <= 1024)
    for (long i = 0; i < n; i++)
        if (group[i] < 0 || group[i] >= groups) {
            set_error("kinship groups: group index %d at cell %ld outside [0, %ld)", group[i], i, groups);
            return CRM_ERR_ARG;
        }
    crm_ctx* ctx = bg->ctx;
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    bg->kin_gen = next_stamp();   // (what the genes keep of the previous structure is rebuilt: crm_gene::tab_key)
    bg->kin = false;   // (a second announcement that fails must not leave the first one's buffers in use)
    struct Undo {      // ... nor keep its own: whatever it allocated goes back unless it ends with bg->kin set
        crm_background* b;
        ~Undo() {
            if (b->kin) return;
            b->kin_fold = false;
            b->kin_wb = false;
            for (DevBuf* x : {&b->kin_map, &b->kin_inv, &b->kin_Y, &b->kin_hKd, &b->wb_U, &b->wb_R, &b->wb_EE}) x->release();
            for (int i = 0; i < b->nrho; i++) b->wb_S0[i].release();
            for (int i = 0; i < b->nrho; i++) b->MixK[i].release();
        }
    } undo{bg};
    // cells in donor order, every donor's run padded to whole stages of the contraction
    std::vector<long> count(groups, 0);
    for (long i = 0; i < n; i++) count[group[i]]++;
    bg->kin_row0.assign(groups, 0);
    bg->kin_len.assign(groups, 0);
    long rows = 0;
    for (long d = 0; d < groups; d++) {
        bg->kin_row0[d] = rows;
        bg->kin_len[d] = round_up(std::max<long>(count[d], 1), GEMM_BK);
        rows += bg->kin_len[d];
    }
    std::vector<int> map(rows, -1);
    std::vector<long> fill(groups, 0);
    for (long i = 0; i < n; i++) {
        const long d = group[i];
        map[bg->kin_row0[d] + fill[d]++] = (int)i;
    }
    // the inverse of the map and the padding rows, behind one another (the fused block pass scatters by the first and clears
    // the second)
    std::vector<int> inv((size_t)bg->n_pad + (size_t)(rows - n), -1);
    for (long k = 0, pads = 0; k < rows; k++) {
        if (map[k] >= 0) inv[map[k]] = (int)k;
        else inv[(size_t)bg->n_pad + pads++] = (int)k;
    }
    bg->kin_pads = rows - n;
    bg->kin_rows = rows;
    bg->kin_groups = groups;
    bg->kin_groups_pad = round_up(groups, GEMM_BK);
    bg->kin_cols = m;
    bg->kin_k1 = k1;
    bg->kin_k2 = k2;
    bg->kin_ldh = round_up(m, 128);
    bg->kin_ldy = round_up(k1 + k2, 128);
    CRM_TRY(bg->kin_map.ensure(sizeof(int) * rows));
    CRM_TRY(bg->kin_Y.ensure(sizeof(double) * rows * bg->kin_ldy));
    CRM_TRY(bg->kin_hKd.ensure(sizeof(double) * bg->kin_groups_pad * bg->kin_ldh));
    DevBuf dU;
    CRM_TRY(dU.ensure(sizeof(double) * n * k2));
    CRM_TRY(bg->kin_inv.ensure(sizeof(int) * inv.size()));
    CRM_HIP(hipMemcpyAsync(bg->kin_map.ptr, map.data(), sizeof(int) * rows, hipMemcpyHostToDevice, st));
    CRM_HIP(hipMemcpyAsync(bg->kin_inv.ptr, inv.data(), sizeof(int) * inv.size(), hipMemcpyHostToDevice, st));
    CRM_HIP(hipMemcpyAsync(dU.ptr, U, sizeof(double) * n * k2, hipMemcpyHostToDevice, st));
    CRM_TRY(upload_padded(st, bg->kin_hKd.as<double>(), bg->kin_ldh, bg->kin_groups_pad, hKd, m, groups, m));
    CRM_TRY(launch_kin_operand(st, dU.as<double>(), k2, bg->H.as<double>(), bg->ldh, k1, bg->kin_map.as<int>(), rows,
                               bg->kin_Y.as<double>(), bg->kin_ldy));
    // the route rests on H[c, k1 + j m + d] = U[c, j] hKd[group(c), d] entry by entry: check it here, once, instead of
    // returning the results of another model when a caller announces a structure its half factor does not have
    DevBuf dgroup, dcheck;
    CRM_TRY(dgroup.ensure(sizeof(int) * n));
    CRM_TRY(dcheck.ensure(2 * sizeof(unsigned long long)));
    unsigned long long check[2] = {0, 0};
    CRM_HIP(hipMemcpyAsync(dgroup.ptr, group, sizeof(int) * n, hipMemcpyHostToDevice, st));
    CRM_HIP(hipMemsetAsync(dcheck.ptr, 0, sizeof check, st));
    CRM_TRY(launch_kin_verify(st, bg->H.as<double>(), bg->ldh, k1, dU.as<double>(), k2, dgroup.as<int>(),
                              bg->kin_hKd.as<double>(), bg->kin_ldh, m, n, dcheck.as<unsigned long long>()));
    CRM_HIP(hipMemcpyAsync(check, dcheck.ptr, sizeof check, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    double dmax, hmax;
    memcpy(&dmax, &check[0], sizeof dmax);
    memcpy(&hmax, &check[1], sizeof hmax);
    if (!(dmax <= 1e-12 * hmax)) {
        set_error("kinship groups: the half factor of this background is not U[c, j] * hKd[group(c), d] (largest difference "
                  "%.3g against entries up to %.3g)", dmax, hmax);
        return CRM_ERR_ARG;
    }
    // the column of ones behind hKd's m columns (objects.h: kin_hKd): the contraction over the donors on the pair products
    // then also gives their sum over the donors (scan_pairs.hip: ScanPass::unfolded_AH).  Written after the check, which reads
    // the m columns alone.
    if (m + 1 <= bg->kin_ldh) {
        std::vector<double> ones((size_t)groups, 1.0);
        CRM_HIP(hipMemcpy2DAsync(bg->kin_hKd.as<double>() + m, sizeof(double) * bg->kin_ldh, ones.data(), sizeof(double),
                                 sizeof(double), groups, hipMemcpyHostToDevice, st));
        CRM_HIP(hipStreamSynchronize(st));   // (ones lives on this stack frame)
    }
    // Fold the donor-level factor into the mixing matrices (objects.h: kin_fold) -- one small product per (grid point, j):
    // MixK[k1 + d' k2 + j, :] = sum_d hKd[d', d] Mix[k1 + j m + d, :], the contraction over d in stages of 16 rows (the
    // rows of hKd' beyond m are zero; the rows of Mix they meet belong to the next j or to Mix's own zero padding, which
    // must exist: cols + padding <= ldh).
    bg->kin_fold = false;
    const long kfold = k1 + groups * (long)k2, m_pad = round_up(m, GEMM_BK);
    const int fold_form = form("kin_fold", 1);   // 0 never, 1 where it pays, 2 also with few columns of us
    // (k2 >= 32: the folded form launches the per-donor sums for the us columns alone, 64 columns wide -- with few of them,
    // config 2's 20, one launch over [us | E1] together and the small contraction over the donors per block is the better
    // form: config 2 463 000 against 451 000 variant-tests/s.  k2 == 1 -- mode B, us a single column -- folds too: its us rows
    // are per-donor sums of the Khatri-Rao rows themselves, a plain batched product, see ScanPass::folded_S)
    if ((double)kfold <= 1.25 * (double)bg->cols && bg->cols + (m_pad - m) <= bg->ldh && (k2 >= 32 || k2 == 1 || fold_form > 1) && fold_form != 0) {
        const long kdim = round_up(kfold, GEMM_BK), ldq = bg->ldq, ld_t = round_up(groups, 128);
        DevBuf hKdT, probs_dev;
        CRM_TRY(hKdT.ensure(sizeof(double) * m_pad * ld_t));
        {
            std::vector<double> t((size_t)m_pad * ld_t, 0.0);
            for (long dd = 0; dd < groups; dd++)
                for (long d = 0; d < m; d++) t[(size_t)d * ld_t + dd] = hKd[dd * m + d];
            CRM_HIP(hipMemcpyAsync(hKdT.ptr, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, st));
            CRM_HIP(hipStreamSynchronize(st));
        }
        std::vector<GemmProblem> pr((size_t)bg->nrho * k2);
        for (int i = 0; i < bg->nrho; i++) {
            CRM_TRY(bg->MixK[i].ensure(sizeof(double) * kdim * ldq));
            CRM_HIP(hipMemsetAsync(bg->MixK[i].ptr, 0, sizeof(double) * kdim * ldq, st));
            CRM_HIP(hipMemcpyAsync(bg->MixK[i].ptr, bg->Mix[i].ptr, sizeof(double) * (size_t)k1 * ldq, hipMemcpyDeviceToDevice, st));
            for (int j = 0; j < k2; j++) {
                GemmProblem p{};
                p.X = hKdT.as<double>(); p.ldx = ld_t;
                p.Y = bg->Mix[i].as<double>() + (size_t)(k1 + (long)j * m) * ldq; p.ldy = ldq;
                p.C = bg->MixK[i].as<double>() + (size_t)(k1 + j) * ldq; p.ldc = (long)k2 * ldq;
                p.M = (int)groups; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
                pr[(size_t)i * k2 + j] = p;
            }
        }
        CRM_TRY(probs_dev.ensure(sizeof(GemmProblem) * pr.size()));
        CRM_HIP(hipMemcpyAsync(probs_dev.ptr, pr.data(), sizeof(GemmProblem) * pr.size(), hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, probs_dev.as<GemmProblem>(), (int)pr.size(), (int)groups, (int)ldq, m_pad, false, 0, 1, 0));
        CRM_HIP(hipStreamSynchronize(st));
        bg->kin_kdim = kdim;
        bg->kin_fold = true;
        CRM_TRY(seal_unrelated_donors(bg, hKd, m));
    }
    bg->kin = true;
    return CRM_OK;
    });
}

int crm_background_kinship_groups(const crm_background* bg) {
    if (!bg) return 0;
    try {
        std::lock_guard<std::recursive_mutex> lock(bg->ctx->mu);
        return bg->kin ? (int)bg->kin_groups : 0;
    } catch (...) {
        return 0;
    }
}

long crm_background_kinship_folded(const crm_background* bg) {
    if (!bg) return 0;
    try {
        std::lock_guard<std::recursive_mutex> lock(bg->ctx->mu);
        return bg->kin && bg->kin_fold ? bg->kin_kdim : 0;
    } catch (...) {
        return 0;
    }
}

}  // extern "C"
