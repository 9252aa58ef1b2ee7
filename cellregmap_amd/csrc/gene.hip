// A gene: one phenotype y with its covariates W and contexts E0 on a background -- crm_gene_create, and the cheaper
// bindings of further phenotypes on the same cohort (crm_gene_create_like, crm_gene_create_batch).
#include <algorithm>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace crm {
// content hash (64-bit words mixed splitmix-style): keys of the shared donor tables
unsigned long content_key(const void* data, size_t bytes, unsigned long seed) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    unsigned long h = seed ^ (0x9E3779B97F4A7C15ul * (bytes + 1));
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        unsigned long w;
        memcpy(&w, p + i, 8);
        h ^= w + 0x9E3779B97F4A7C15ul + (h << 6) + (h >> 2);
        h *= 0xBF58476D1CE4E5B9ul;
        h ^= h >> 29;
    }
    for (; i < bytes; i++) h = (h ^ p[i]) * 0x100000001B3ul;
    return h ? h : 1;
}

void nullfit_gene_args(NullFitArgs& a, const crm_gene* gene, int restricted) {
    const crm_background* bg = gene->bg;
    const crm_ctx* ctx = bg->ctx;
    const long ldq = bg->ldq, slab = (long)(1 + gene->c) * ldq;
    a.nrho = bg->nrho; a.c = gene->c; a.restricted = restricted; a.n = bg->n;
    a.polish = (ctx->polish && gene->c <= CRM_MAX_COV) ? 1 : 0;
    a.exact = (ctx->nullfit_exact || form("nullfit_exact", 0)) ? 1 : 0;
    for (int i = 0; i < bg->nrho; i++) {
        NullFitRho& R = a.rho[i];
        R.ty = gene->rot.as<double>() + (long)i * slab;
        R.tW = R.ty + ldq; R.ldW = ldq;
        R.S0 = bg->S0[i].as<double>();
        R.r = bg->r[i];
    }
    a.WW = gene->WW.as<double>(); a.Wy = gene->Wy.as<double>(); a.yy = gene->yy;
}
}  // namespace crm

__global__ void scatter_column_kernel(const double* __restrict__ src, long lds, int col, double* __restrict__ dst, long ldd, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i * ldd] = src[i * lds + col];
}

// rotations t = Q0(rho)' [y, W] of a gene for every grid point: rows of a [(1+c) x ldq] matrix per grid point
static int gene_rotations(crm_gene* g) {
    crm_background* bg = g->bg;
    crm_ctx* ctx = g->ctx;
    const int c = g->c;
    const long np = bg->n_pad, ldyw = g->ld_yw;
    const int nrho = bg->nrho;
    const long ldq = bg->ldq;
    const long slab = (long)(1 + c) * ldq;
    if (bg->fast_T && ctx->fast_gene_rot) {
        // Q0(rho) = H Mix(rho):  t = Mix(rho)' (H'[y, W]) -- no Q0 needed
        DevBuf thw;
        const long ldh = bg->ldh;
        const long ldt = round_up(1 + c, 128);   // (129 columns at c = CRM_MAX_COV_XWIDE)
        CRM_TRY(thw.ensure(sizeof(double) * ldh * ldt));
        CRM_TRY(g->rot.ensure(sizeof(double) * slab * nrho));
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + 4)));
        CRM_HIP(hipMemsetAsync(thw.ptr, 0, sizeof(double) * ldh * ldt, ctx->stream));
        CRM_HIP(hipMemsetAsync(g->rot.ptr, 0, sizeof(double) * slab * nrho, ctx->stream));
        std::vector<GemmProblem> pr(nrho + 1);
        GemmProblem p0{};
        p0.X = bg->H.as<double>(); p0.ldx = ldh; p0.Y = g->yW.as<double>(); p0.ldy = ldyw;
        p0.C = thw.as<double>(); p0.ldc = ldt; p0.M = (int)bg->cols; p0.N = 1 + c;
        pr[0] = p0;
        for (int i = 0; i < nrho; i++) {
            GemmProblem p{};
            p.X = thw.as<double>(); p.ldx = ldt; p.Y = bg->Mix[i].as<double>(); p.ldy = ldq;
            p.C = g->rot.as<double>() + (long)i * slab; p.ldc = ldq;
            p.M = 1 + c; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            pr[1 + i] = p;
        }
        CRM_HIP(hipMemcpyAsync(ctx->ws_probs.ptr, pr.data(), sizeof(GemmProblem) * (nrho + 1), hipMemcpyHostToDevice, ctx->stream));
        CRM_TRY(launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>(), 1, (int)bg->cols, 1 + c, np, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>() + 1, nrho, 1 + c, (int)ldq, ldh, false, 0, 1, 0));
        CRM_HIP(hipStreamSynchronize(ctx->stream));
        return CRM_OK;
    }
    CRM_TRY(crm_background_require_q0(bg, -1));
    const int ks = split_for(np, (ldq / GEMM_BN) * nrho);
    CRM_TRY(g->rot.ensure(sizeof(double) * slab * nrho * ks));
    std::vector<GemmProblem> probs(nrho);
    for (int i = 0; i < nrho; i++) {
        GemmProblem p{};
        p.X = g->yW.as<double>(); p.ldx = ldyw;
        p.Y = bg->Q0[i].as<double>(); p.ldy = ldq;
        p.C = g->rot.as<double>() + (long)i * slab; p.ldc = ldq;
        p.M = 1 + c; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
        probs[i] = p;
    }
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * CRM_MAX_RHO));
    CRM_HIP(hipMemcpyAsync(ctx->ws_probs.ptr, probs.data(), sizeof(GemmProblem) * nrho, hipMemcpyHostToDevice, ctx->stream));
    // splits write slabs nrho*slab apart
    CRM_HIP(hipMemsetAsync(g->rot.ptr, 0, sizeof(double) * slab * nrho * ks, ctx->stream));
    CRM_TRY(launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>(), nrho, 1 + c, (int)ldq, np, false, 0, ks, slab * nrho));
    CRM_TRY(launch_reduce_splits(ctx->stream, g->rot.as<double>(), slab * nrho, ks, slab * nrho));
    CRM_HIP(hipStreamSynchronize(ctx->stream));
    return CRM_OK;
}

// The covariates as the scans use them, and their inner products.
// The orthogonalisation of the variants against W (blockops.hip: launch_ortho_block) and the null fits work in a basis
// of span(W) with mutually orthogonal columns -- U diag(s) of the thin SVD, the basis glimix-core's LMM holds its
// covariates in, which is what the Python host passes.  Columns that are not orthogonal are brought there here: the
// scans depend on W through its column space only.  W <- W V with V the eigenvectors of W'W by a cyclic Jacobi
// iteration, repeated on the result: a pass leaves the columns orthogonal to ~eps cond(W)^2, and on a nearly diagonal
// Gram matrix Jacobi resolves the small singular values to high relative accuracy, so two or three passes reach the
// 1e-13 the diagonal test asks for up to cond(W) ~ 1e7 -- beyond which the reference's own rank rule
// (numpy_sugar.economic_svd: singular values below sqrt(eps)) is what decides.
// Wused: the n x c columns in use (W itself when its columns are orthogonal as passed); Vtot: the product of the passes' V,
// Wused = W Vtot (empty: W unchanged); WW = Wused'Wused, Wy = Wused'y.
static int orthogonal_covariates(long n, int c, const double* y, const double* W, std::vector<double>& Wused,
                                 std::vector<double>& Vtot, std::vector<double>& WW, std::vector<double>& Wy) {
    WW.assign((size_t)c * c, 0.0);
    Wy.assign(c, 0.0);
    auto inner_products = [&](const double* Wm) {
        std::fill(WW.begin(), WW.end(), 0.0);
        std::fill(Wy.begin(), Wy.end(), 0.0);
        for (long i = 0; i < n; i++)
            for (int a = 0; a < c; a++) {
                Wy[a] += Wm[i * c + a] * y[i];
                for (int b = a; b < c; b++) WW[a * c + b] += Wm[i * c + a] * Wm[i * c + b];
            }
        for (int a = 0; a < c; a++)
            for (int b = 0; b < a; b++) WW[a * c + b] = WW[b * c + a];
    };
    auto is_diagonal = [&]() {
        for (int a = 0; a < c; a++)
            for (int b = a + 1; b < c; b++)
                if (std::fabs(WW[a * c + b]) > 1e-13 * std::sqrt(WW[a * c + a] * WW[b * c + b])) return false;
        return true;
    };
    Wused.assign(W, W + (size_t)n * c);
    Vtot.clear();
    inner_products(Wused.data());
    for (int pass = 0; pass < 4 && !is_diagonal(); pass++) {
        std::vector<double> A(WW), V((size_t)c * c, 0.0);
        for (int a = 0; a < c; a++) V[a * c + a] = 1.0;
        for (int sweep = 0; sweep < 60; sweep++) {
            double offd = 0.0, diag = 0.0;
            for (int a = 0; a < c; a++)
                for (int b = 0; b < c; b++) (a == b ? diag : offd) += A[a * c + b] * A[a * c + b];
            if (offd <= 1e-32 * diag) break;
            for (int pi = 0; pi < c - 1; pi++)
                for (int qi = pi + 1; qi < c; qi++) {
                    const double apq = A[pi * c + qi];
                    if (apq == 0.0) continue;
                    const double theta = (A[qi * c + qi] - A[pi * c + pi]) / (2.0 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                    jacobi_rotate(c, A.data(), V.data(), pi, qi, cs, sn);
                }
        }
        std::vector<double> Wn((size_t)n * c);
        std::vector<double> row(c);
        for (long i = 0; i < n; i++) {
            for (int a = 0; a < c; a++) row[a] = Wused[i * c + a];
            for (int b = 0; b < c; b++) {
                double acc = 0.0;
                for (int a = 0; a < c; a++) acc += row[a] * V[a * c + b];
                Wn[i * c + b] = acc;
            }
        }
        Wused.swap(Wn);
        inner_products(Wused.data());
        if (Vtot.empty()) Vtot = V;
        else {
            std::vector<double> T((size_t)c * c, 0.0);
            for (int a = 0; a < c; a++)
                for (int k = 0; k < c; k++)
                    for (int b = 0; b < c; b++) T[a * c + b] += Vtot[a * c + k] * V[k * c + b];
            Vtot.swap(T);
        }
    }
    if (!is_diagonal()) {
        set_error("gene: the covariates could not be brought to mutually orthogonal columns (W'W stays coupled beyond 1e-13 "
                  "after four passes): pass an orthogonal basis of span(W), e.g. U diag(s) of its thin SVD");
        return CRM_ERR_NUMERIC;
    }
    return CRM_OK;
}

// A new gene on the cohort of `like`: what a gene keeps of W and E0 (device copies, W'W, the projection onto span(W), the
// content keys) copied on the device -- with_rot: the rotations too, for their rows Q0(rho)'W.  Column 0 of [y | W], W'y,
// y'y and the row Q0(rho)'y are the caller's to fill.
static int clone_cohort(const crm_gene* like, bool with_rot, Owned<crm_gene>& out) {
    Owned<crm_gene> g(new crm_gene());
    g->bg = like->bg; g->ctx = like->ctx; g->c = like->c; g->k0 = like->k0;
    g->e0_key = like->e0_key; g->w_key = like->w_key;
    g->ldw = like->ldw; g->lde = like->lde; g->ld_yw = like->ld_yw;
    g->W_host = like->W_host;
    g->W_basis = like->W_basis;
    const DevBuf* src[] = {&like->yW, &like->E0, &like->WW, &like->Wproj, &like->rot};
    DevBuf* dst[] = {&g->yW, &g->E0, &g->WW, &g->Wproj, &g->rot};
    for (int q = 0; q < (with_rot ? 5 : 4); q++) {
        CRM_TRY(dst[q]->ensure(src[q]->bytes));
        CRM_HIP(hipMemcpyAsync(dst[q]->ptr, src[q]->ptr, src[q]->bytes, hipMemcpyDeviceToDevice, g->ctx->stream));
    }
    out = std::move(g);
    return CRM_OK;
}

// y'y and W'y (uploaded) of the phenotype y[i * stride], against the covariates as the gene holds them
static int bind_phenotype(crm_gene* g, const double* y, long stride) {
    const long n = g->bg->n;
    const int c = g->c;
    const double* Wm = g->W_host.data();
    std::vector<double> Wy(c, 0.0);
    g->yy = 0.0;
    for (long i = 0; i < n; i++) g->yy += y[i * stride] * y[i * stride];
    for (long i = 0; i < n; i++)
        for (int a = 0; a < c; a++) Wy[a] += Wm[i * c + a] * y[i * stride];
    CRM_TRY(g->Wy.ensure(sizeof(double) * c));
    CRM_HIP(hipMemcpyAsync(g->Wy.ptr, Wy.data(), sizeof(double) * c, hipMemcpyHostToDevice, g->ctx->stream));
    CRM_HIP(hipStreamSynchronize(g->ctx->stream));   // (Wy lives on this stack frame)
    return CRM_OK;
}

extern "C" {

int crm_gene_create(crm_background* bg, const double* y, const double* W, int c, const double* E0,
                    int k0, crm_gene** out) {
    return crm::guarded_on("crm_gene_create", bg ? bg->ctx : nullptr, [&]() -> int {
    if (!bg || !y || !W || !E0 || !out) return CRM_ERR_ARG;
    *out = nullptr;
    if (bg->builder) {
        set_error("gene: the background is still under construction (crm_background_seal not called)");
        return CRM_ERR_ARG;
    }
    if (c < 1 || c > CRM_MAX_COV_XWIDE) {
        set_error("gene: %d covariate columns (supported 1..%d; the interaction scan up to %d)", c, CRM_MAX_COV_XWIDE, CRM_MAX_COV_WIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    if (k0 < 1 || k0 > CRM_MAX_K0) {
        set_error("gene: %d contexts (supported 1..%d)", k0, CRM_MAX_K0);
        return CRM_ERR_UNSUPPORTED;
    }
    crm_ctx* ctx = bg->ctx;
    CRM_HIP(hipSetDevice(ctx->device));
    const long n = bg->n, np = bg->n_pad;
    for (long i = 0; i < n; i++) {
        bool fin = std::isfinite(y[i]);
        for (int j = 0; j < c && fin; j++) fin = std::isfinite(W[i * c + j]);
        if (!fin) {
            set_error("gene: non-finite values in the outcome or the covariates");
            return CRM_ERR_NUMERIC;
        }
    }
    Owned<crm_gene> g(new crm_gene());
    g->bg = bg;
    g->ctx = bg->ctx;
    g->c = c;
    g->k0 = k0;
    g->e0_key = content_key(E0, sizeof(double) * (size_t)bg->n * k0, (unsigned long)k0);
    g->w_key = content_key(W, sizeof(double) * (size_t)bg->n * c, (unsigned long)c);
    g->ldw = 16;
    g->lde = round_up(k0, 16);
    g->yy = 0.0;
    for (long i = 0; i < n; i++) g->yy += y[i] * y[i];
    std::vector<double> WW, Wy;
    CRM_TRY(orthogonal_covariates(n, c, y, W, g->W_host, g->W_basis, WW, Wy));
    const double* Wuse = g->W_host.data();
    // [y | W] packed as one operand (column 0 = y) for the rotations, plus separate views; 1 + c = 129 columns at
    // c = CRM_MAX_COV_XWIDE
    const long ldyw = round_up(1 + c, 128);
    CRM_TRY(g->yW.ensure(sizeof(double) * np * ldyw));
    CRM_TRY(g->E0.ensure(sizeof(double) * np * g->lde));
    {
        std::vector<double> pack((size_t)n * (1 + c));
        for (long i = 0; i < n; i++) {
            pack[i * (1 + c)] = y[i];
            for (int j = 0; j < c; j++) pack[i * (1 + c) + 1 + j] = Wuse[i * c + j];
        }
        CRM_TRY(upload_padded(ctx->stream, g->yW.as<double>(), ldyw, np, pack.data(), 1 + c, n, 1 + c));
        CRM_HIP(hipStreamSynchronize(ctx->stream));
    }
    g->ld_yw = ldyw;
    CRM_TRY(upload_padded(ctx->stream, g->E0.as<double>(), g->lde, np, E0, k0, n, k0));
    // What the orthogonalisation of the variants against W needs: (W'W)^-1 = diag(1 / s^2), V = I, d^2 = s^2
    {
        constexpr double EPS = 2.220446049250313e-16;
        std::vector<double> proj((size_t)2 * c * c + c, 0.0);
        double* inv = proj.data();
        double* V = inv + (size_t)c * c;
        double* d2 = V + (size_t)c * c;
        for (int a = 0; a < c; a++) {
            if (!(WW[a * c + a] >= EPS)) {
                set_error("gene: the covariates are rank deficient by the reference's rule (a singular value of %.3g, below "
                          "sqrt(eps)): pass a basis of span(W)", std::sqrt(std::max(WW[a * c + a], 0.0)));
                return CRM_ERR_NUMERIC;
            }
            V[a * c + a] = 1.0;
            d2[a] = WW[a * c + a];
            inv[a * c + a] = 1.0 / WW[a * c + a];
        }
        CRM_TRY(g->Wproj.ensure(sizeof(double) * proj.size()));
        CRM_HIP(hipMemcpyAsync(g->Wproj.ptr, proj.data(), sizeof(double) * proj.size(), hipMemcpyHostToDevice, ctx->stream));
        CRM_HIP(hipStreamSynchronize(ctx->stream));   // (proj lives on this stack frame)
    }
    CRM_TRY(g->WW.ensure(sizeof(double) * c * c));
    CRM_TRY(g->Wy.ensure(sizeof(double) * c));
    CRM_HIP(hipMemcpyAsync(g->WW.ptr, WW.data(), sizeof(double) * c * c, hipMemcpyHostToDevice, ctx->stream));
    CRM_HIP(hipMemcpyAsync(g->Wy.ptr, Wy.data(), sizeof(double) * c, hipMemcpyHostToDevice, ctx->stream));
    CRM_HIP(hipStreamSynchronize(ctx->stream));
    CRM_TRY(gene_rotations(g.get()));
    *out = g.release();
    return CRM_OK;
    });
}

// Another phenotype on the cohort of `like`: same background, covariates and contexts -- only y differs.  What a gene
// keeps of W and E0 (device copies, W'W, the projection onto span(W), the content keys that let a multi-phenotype pass check
// that its genes agree) is copied on the device instead of being checked, hashed, orthogonalised and uploaded again: binding
// a phenotype costs its own upload and rotations only (per-gene run_interaction calls of the reference, _cellregmap.py:547-587,
// over many genes of one cohort).  The results are bit for bit those of crm_gene_create with the same W and E0.
int crm_gene_create_like(const crm_gene* like, const double* y, crm_gene** out) {
    return crm::guarded_on("crm_gene_create_like", like ? like->ctx : nullptr, [&]() -> int {
    if (!like || !y || !out) return CRM_ERR_ARG;
    *out = nullptr;
    crm_background* bg = like->bg;
    crm_ctx* ctx = like->ctx;
    CRM_HIP(hipSetDevice(ctx->device));
    const long n = bg->n;
    const int c = like->c;
    if (like->W_host.size() != (size_t)n * c) {
        set_error("gene: the template gene holds no covariates");
        return CRM_ERR_ARG;
    }
    for (long i = 0; i < n; i++)
        if (!std::isfinite(y[i])) {
            set_error("gene: non-finite values in the outcome or the covariates");
            return CRM_ERR_NUMERIC;
        }
    Owned<crm_gene> g;
    CRM_TRY(clone_cohort(like, false, g));
    // column 0 of [y | W]
    CRM_HIP(hipMemcpy2DAsync(g->yW.ptr, sizeof(double) * g->ld_yw, y, sizeof(double), sizeof(double), n, hipMemcpyHostToDevice,
                             ctx->stream));
    CRM_TRY(bind_phenotype(g.get(), y, 1));
    CRM_TRY(gene_rotations(g.get()));
    *out = g.release();
    return CRM_OK;
    });
}

// ngenes phenotypes (the columns of Y: n x ngenes, row-major, leading dimension ldy) on the cohort of `like`, bound in one
// call: what crm_gene_create_like does per phenotype, with the rotations Q0(rho)'y of all of them as ONE product against the
// half factor and one against every mixing matrix -- those operands (0.8 GB + 11 x 0.2 GB at BASELINE config 3) are read once
// per batch instead of once per phenotype.  out: ngenes handles; on failure none is left behind.
int crm_gene_create_batch(const crm_gene* like, const double* Y, long ldy, int ngenes, crm_gene** out) {
    return crm::guarded_on("crm_gene_create_batch", like ? like->ctx : nullptr, [&]() -> int {
    if (!like || !Y || !out || ngenes < 1 || ldy < ngenes) return CRM_ERR_ARG;
    for (int j = 0; j < ngenes; j++) out[j] = nullptr;
    crm_background* bg = like->bg;
    crm_ctx* ctx = like->ctx;
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    const int c = like->c, nrho = bg->nrho;
    if (like->W_host.size() != (size_t)n * c) {
        set_error("gene: the template gene holds no covariates");
        return CRM_ERR_ARG;
    }
    for (long i = 0; i < n; i++)
        for (int j = 0; j < ngenes; j++)
            if (!std::isfinite(Y[i * ldy + j])) {
                set_error("gene: non-finite values in the outcome or the covariates");
                return CRM_ERR_NUMERIC;
            }
    const long ldY = round_up(ngenes, 128);
    DevBuf dY;
    CRM_TRY(dY.ensure(sizeof(double) * np * ldY));
    CRM_TRY(upload_padded(st, dY.as<double>(), ldY, np, Y, ldy, n, ngenes));
    std::vector<Owned<crm_gene>> made(ngenes);
    for (int j = 0; j < ngenes; j++) {
        CRM_TRY(clone_cohort(like, true, made[j]));
        hipLaunchKernelGGL(scatter_column_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dY.as<double>(), ldY, j,
                           made[j]->yW.as<double>(), made[j]->ld_yw, n);
        CRM_TRY(bind_phenotype(made[j].get(), Y + j, ldy));
    }
    CRM_HIP(hipGetLastError());
    const long slab = (long)(1 + c) * ldq;
    if (bg->fast_T && ctx->fast_gene_rot) {
        // t_y = Mix(rho)' (H'y) for all phenotypes at once; the rows Q0(rho)'W came over with the copy of `like`'s rotations
        const long ldh = bg->ldh;
        DevBuf thw, rt;
        CRM_TRY(thw.ensure(sizeof(double) * ldh * ldY));
        CRM_TRY(rt.ensure(sizeof(double) * (size_t)nrho * ngenes * ldq));
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + 4)));
        CRM_HIP(hipMemsetAsync(thw.ptr, 0, sizeof(double) * ldh * ldY, st));
        CRM_HIP(hipMemsetAsync(rt.ptr, 0, sizeof(double) * (size_t)nrho * ngenes * ldq, st));
        std::vector<GemmProblem> pr(nrho + 1);
        GemmProblem p0{};
        p0.X = bg->H.as<double>(); p0.ldx = ldh; p0.Y = dY.as<double>(); p0.ldy = ldY;
        p0.C = thw.as<double>(); p0.ldc = ldY; p0.M = (int)bg->cols; p0.N = ngenes;
        pr[0] = p0;
        for (int i = 0; i < nrho; i++) {
            GemmProblem p{};
            p.X = thw.as<double>(); p.ldx = ldY; p.Y = bg->Mix[i].as<double>(); p.ldy = ldq;
            p.C = rt.as<double>() + (size_t)i * ngenes * ldq; p.ldc = ldq;
            p.M = ngenes; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            pr[1 + i] = p;
        }
        CRM_HIP(hipMemcpyAsync(ctx->ws_probs.ptr, pr.data(), sizeof(GemmProblem) * (nrho + 1), hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>(), 1, (int)bg->cols, ngenes, np, false, 0, 1, 0));
        CRM_TRY(launch_gemm_tn(ctx, ctx->ws_probs.as<GemmProblem>() + 1, nrho, ngenes, (int)ldq, ldh, false, 0, 1, 0));
        for (int j = 0; j < ngenes; j++)     // row 0 of every grid point's [(1 + c) x ldq] block
            CRM_HIP(hipMemcpy2DAsync(made[j]->rot.ptr, sizeof(double) * slab, rt.as<double>() + (size_t)j * ldq,
                                     sizeof(double) * (size_t)ngenes * ldq, sizeof(double) * ldq, nrho, hipMemcpyDeviceToDevice, st));
        CRM_HIP(hipStreamSynchronize(st));
    } else {
        for (auto& g : made) CRM_TRY(gene_rotations(g.get()));
    }
    for (int j = 0; j < ngenes; j++) out[j] = made[j].release();
    return CRM_OK;
    });
}

void crm_gene_destroy(crm_gene* g) {
    try {
    if (!g) return;
    std::lock_guard<std::recursive_mutex> lock(g->ctx->mu);   // (reachable from a finalizer on any thread)
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    delete g;
    } catch (...) {  // (nothing may unwind into the caller; a destroy has no status to return)
    }
}

}  // extern "C"
