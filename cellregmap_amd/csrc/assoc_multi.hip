// Association scans of several phenotypes against one panel (C-ABI crm_association_null_multi,
// crm_scan_association_multi): what does not depend on the phenotype is done once per block of variants.
// Reference: cellregmap/_cellregmap.py:246-314 (per phenotype) and :443-469 (the LRT).
//
// Per block, shared by the genes of the call (genes grouped by the grid index of their null rho*):
//   Gb                      gathered / expanded once
//   gg, g'W, g'y_j          one pass (gg) and one MFMA product [W | y_1 .. y_g]' Gb
//   T_rho = Q0(rho)' Gb     one batched MFMA launch, one problem per distinct rho*  ([r x variants]: the rows of the
//                           products below run over the spectrum)
// Fast path (delta frozen at the null, glimix-core FastScanner): with w_j[k] = 1 / ((1 - delta_j) S0[k] + delta_j),
//   h_u = sum_k T[b,k] x_u[k] w_j[k] + (plain_u - sum_k T[b,k] x_u[k]) / delta_j,  x_u in {tW columns, T[b,:], ty_j}
// and only the weighted sums depend on the gene.  The weights are folded into the right-hand operand, which does not
// depend on the block: per rho group one product
//   C1 = T' [tW | per gene: ty_j, w_j o ty_j, w_j o tW]      (c + g (c + 2) columns)
//   C2 = (T o T)' [1 | per gene: w_j]                         (1 + g columns)
// through the MFMA contraction kernel (gemm_tn.hip), and one thread per (gene, variant) finishes: forward substitution
// with the gene's Cholesky factor (fastscan_prep record), Schur complement, alt lml and the LRT, the statements of
// fastscan_kernel / lrt_kernel (assoc.hip).
// Full refit: the block is orthogonalised against the shared W once; per gene the null-fit kernels run over the block on
// the shared T(rho*) with that gene's y quantities.
// crm_scan_association_multi_effects: the same launches, then the effect sizes of every (gene, variant) from the T(rho*)
// still in place (assoc_effects.hip).
#include <algorithm>

#include "delta_search.h"
#include "lrt_scan.h"

namespace crm {

namespace {

constexpr double DBL_TINY = 2.2250738585072014e-308;
constexpr double DBL_EPS = 2.220446049250313e-16;
constexpr int CMAX = CRM_MAX_COV_XWIDE;   // layout constant of the fastscan_prep record

// One gene of a fast multi-gene pass (device copy).
struct MultiGene {
    const double* ty;     // [r] Q0(rho*)' y
    const double* wts;    // [r] spectrum weights at the null's delta (fastscan_prep)
    const double* prep;   // fastscan_prep record: [0] rss0, [1] logdetK, [3] ok, [8..) zy, [8 + CMAX ..) L
    int group;            // rho group
    int col1, col2;       // first column of the gene in C1 / C2
    int row_y;            // row of g'y_j in the product [W | Y]' Gb
    double inv_d;         // 1 / delta
    double null_lml;
};

struct MultiGroup {
    const double* tW;     // [c x ldW] Q0(rho)' W (first gene of the group)
    long ldW;
    int r, rpad;          // spectrum length, padded to the contraction's stage depth
    int col1, col2;       // first column of the group in C1 / C2 (its tW block / its column of ones)
};

// Right-hand operands of one call (do not depend on the block): rows k < rpad, zero for k >= r.
//   B1[k, col1(group) + u] = tW_u[k];  B1[k, col1(gene) + (0, 1, 2 + u)] = (ty, w ty, w tW_u)[k]
//   B2[k, col2(group)] = 1;            B2[k, col2(gene)] = w[k]
__global__ __launch_bounds__(256) void multi_rhs_kernel(const MultiGene* __restrict__ genes, int ngenes,
                                                        const MultiGroup* __restrict__ groups, int c,
                                                        double* __restrict__ B1, long ld1, double* __restrict__ B2, long ld2) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y;
    if (a < ngenes) {
        const MultiGene g = genes[a];
        const MultiGroup& R = groups[g.group];
        if (k >= R.rpad) return;
        const bool in = k < R.r;
        const double w = in ? g.wts[k] : 0.0;
        double* b1 = B1 + (long)k * ld1 + g.col1;
        b1[0] = in ? g.ty[k] : 0.0;
        b1[1] = in ? w * g.ty[k] : 0.0;
        for (int u = 0; u < c; u++) b1[2 + u] = in ? w * R.tW[(long)u * R.ldW + k] : 0.0;
        B2[(long)k * ld2 + g.col2] = w;
    } else {
        const MultiGroup R = groups[a - ngenes];
        if (k >= R.rpad) return;
        const bool in = k < R.r;
        double* b1 = B1 + (long)k * ld1 + R.col1;
        for (int u = 0; u < c; u++) b1[u] = in ? R.tW[(long)u * R.ldW + k] : 0.0;
        B2[(long)k * ld2 + R.col2] = in ? 1.0 : 0.0;
    }
}

// T2 = T o T over [rpad x variants] of every group (blockIdx.z)
__global__ __launch_bounds__(256) void multi_square_kernel(const double* __restrict__ T, double* __restrict__ T2, long slab,
                                                           long ldt, const MultiGroup* __restrict__ groups, int variants) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    const int z = blockIdx.z;
    if (b >= variants || k >= groups[z].rpad) return;
    const long i = (long)z * slab + (long)k * ldt + b;
    const double t = T[i];
    T2[i] = t * t;
}

// One thread per (gene, variant): the tail of fastscan_kernel on the split sums, then lrt_kernel.
// CR > 0: the forward substitution in registers (c <= CR); CR == 0: in place over the gene's w o tW columns of C1.
template <int CR>
__global__ __launch_bounds__(128) void multi_finish_kernel(const MultiGene* __restrict__ genes, const MultiGroup* __restrict__ groups,
                                                           int c, long n, int variants, double* __restrict__ C1, long ld1,
                                                           const double* __restrict__ C2, long ld2,
                                                           const double* __restrict__ gg, const double* __restrict__ CY, long ldcy,
                                                           double* __restrict__ alt_lml, double* __restrict__ pv, long ld_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y;
    if (b >= variants) return;
    const MultiGene g = genes[a];
    const MultiGroup& R = groups[g.group];
    const double inv_d = g.inv_d;
    double* const row = C1 + (long)b * ld1;
    const double* const s1W = row + R.col1;       // sum_k T tW_u
    double* const gcol = row + g.col1;            // sum_k T ty, sum_k T w ty, sum_k T w tW_u
    const double h_gg = C2[(long)b * ld2 + g.col2] + (gg[b] - C2[(long)b * ld2 + R.col2]) * inv_d;
    const double h_gy = gcol[1] + (CY[(long)g.row_y * ldcy + b] - gcol[0]) * inv_d;
    const double* const zy = g.prep + 8;
    const double* const L = g.prep + 8 + CMAX;
    double zz = 0.0, zzy = 0.0;
    double zr[CR > 0 ? CR : 1];
    for (int i = 0; i < c; i++) {
        double s = gcol[2 + i] + (CY[(long)i * ldcy + b] - s1W[i]) * inv_d;   // h_gW[i]
        for (int k = 0; k < i; k++) s -= L[i * CMAX + k] * (CR > 0 ? zr[k] : gcol[2 + k]);
        s /= L[i * CMAX + i];
        if (CR > 0) zr[i < CR ? i : 0] = s;
        else gcol[2 + i] = s;
        zz += s * s;
        zzy += s * zy[i];
    }
    const double dn = (double)n;
    const double schur = h_gg - zz;
    const double num = h_gy - zzy;
    double rss = g.prep[0];
    if (schur > 1e-12 * h_gg) rss -= num * num / schur;
    const double sc = fmax(rss / dn, EPS_SMALL);
    const double lml = g.prep[3] != 0.0 ? -0.5 * (dn * LOG2PI + dn + dn * log(sc) + g.prep[1]) : NAN;
    alt_lml[(long)a * ld_out + b] = lml;
    double lrs = -2.0 * g.null_lml + 2.0 * lml;
    if (lrs < DBL_TINY) lrs = DBL_TINY;
    double p = erfc(sqrt(0.5 * lrs));
    if (p < DBL_TINY) p = DBL_TINY;
    if (p > 1.0 - DBL_EPS) p = 1.0 - DBL_EPS;
    pv[(long)a * ld_out + b] = p;
}

// lrt_kernel (assoc.hip) for the rows of several genes
__global__ void multi_lrt_kernel(const double* __restrict__ alt_lml, const double* __restrict__ null_lml, int variants,
                                 long ld, double* __restrict__ pv) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y;
    if (b >= variants) return;
    double lrs = -2.0 * null_lml[a] + 2.0 * alt_lml[(long)a * ld + b];
    if (lrs < DBL_TINY) lrs = DBL_TINY;
    double p = erfc(sqrt(0.5 * lrs));
    if (p < DBL_TINY) p = DBL_TINY;
    if (p > 1.0 - DBL_EPS) p = 1.0 - DBL_EPS;
    pv[(long)a * ld + b] = p;
}

}  // namespace

}  // namespace crm

using namespace crm;

extern "C" int crm_association_null_multi(crm_gene* const* genes, int ngenes, double* out_null) {
    return crm::guarded_on("crm_association_null_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    const char* what = "association null multi";
    CRM_TRY(check_shared_genes(what, genes, ngenes, false));
    if (!out_null) {
        set_error("%s: out_null is NULL", what);
        return CRM_ERR_ARG;
    }
    crm_background* bg = genes[0]->bg;
    crm_ctx* ctx = bg->ctx;
    InScan in_scan;
    CRM_TRY(in_scan.enter(ctx, what));
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nrho = bg->nrho, c = genes[0]->c;
    ZeroVariant zero;
    zero.ld_gW = round_up(c, 8);
    NullFitOut* d_fit = nullptr;
    CRM_TRY(carve_workspace(ctx->ws_small, [&](auto& take) {
        take(zero.zero, sizeof(double) * bg->ldq), take(zero.gg, sizeof(double)), take(zero.gy, sizeof(double));
        take(zero.gW, sizeof(double) * zero.ld_gW), take(zero.trial, sizeof(NullFitTrial) * nrho * nrho);
        take(d_fit, sizeof(NullFitOut) * ngenes);
    }));
    // zero T row, gg, gy, gW, which sit in this order in front of the trial records: the fit drops the zero "variant"
    CRM_HIP(hipMemsetAsync(zero.zero, 0, (char*)zero.trial - (char*)zero.zero, st));
    double* xwide = nullptr;
    if (c > CRM_MAX_COV_WIDE) {
        CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(1, nrho, c)));
        xwide = ctx->ws_xwide.as<double>();
    }
    NullFitArgs fa;
    for (int i = 0; i < ngenes; i++) CRM_TRY(launch_gene_null(st, genes[i], zero, d_fit + i, xwide, fa));
    std::vector<NullFitOut> fits(ngenes);
    CRM_HIP(hipMemcpyAsync(fits.data(), d_fit, sizeof(NullFitOut) * ngenes, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < ngenes; i++) CRM_TRY(gene_null_row(what, bg, i, fits[i], out_null + 6 * (size_t)i));
    return CRM_OK;
    });
}

namespace {

// One call of crm_scan_association_multi (eff null: its launches and nothing else) or crm_scan_association_multi_effects
// (assoc_effects.hip: fast, one more launch per block over every (variant, gene); full refit, one per gene after its alt
// fits, whose trial records the next gene overwrites): what is fixed once the checks have passed, one function per stage.
struct AssocMultiScan {
    LrtBlock B;
    crm_gene* const* genes; const int ngenes; const double* null;
    const NullRows& R;
    const AssocEffectsOut* eff;
    crm_background* bg; crm_ctx* ctx; hipStream_t st;
    const int BLK, c, ngrp;
    const bool fast;
    const long n, np, ldq, ldb, slab;
    PhenotypeMatrix Y;
    long rows_cy, ldcy, ldt, tslab, ld1 = 0, ld2 = 0;
    int prep_d, rmax = 0;
    size_t eff_rows;   // per output: [ngenes x BLK], five of doubles, then the status
    std::vector<MultiGroup> groups;
    std::vector<MultiGene> mg;
    double *d_cy = nullptr, *d_alt = nullptr, *d_pv = nullptr, *d_nl = nullptr, *d_prep = nullptr, *d_wts = nullptr, *d_eff = nullptr;
    AssocArgs* d_args = nullptr; MultiGene* d_mg = nullptr; MultiGroup* d_grp = nullptr;
    NullFitTrial* d_trial = nullptr; NullFitOut* d_fit = nullptr; AssocEffectsGene* d_effg = nullptr;
    GemmProblem* d_probs = nullptr; double* Tb = nullptr;
    std::vector<double> null_lml;
    std::vector<AssocArgs> aa;          // (host sources of asynchronous copies: alive until the last sync)
    std::vector<AssocEffectsGene> eg;   // (host source of an asynchronous copy)
    NullFitArgs alt{};
    std::vector<GemmProblem> probs, pp;

    AssocMultiScan(crm_gene* const* genes_, int ngenes_, crm_panel* panel, long first, long count, int fast_, const double* null_,
                   const NullRows& R_, const AssocEffectsOut* eff_)
        : B(genes_[0], panel, first, count, fast_), genes(genes_), ngenes(ngenes_), null(null_), R(R_), eff(eff_), bg(B.bg),
          ctx(B.ctx), st(B.st), BLK(B.BLK), c(B.c), ngrp(R_.ngrp()), fast(B.fast), n(B.n), np(B.np), ldq(B.ldq), ldb(B.ldb),
          slab((long)(1 + B.c) * B.ldq), groups(ngrp), mg(ngenes_), null_lml(ngenes_) {
        Y.plan(genes, ngenes);
        rows_cy = fast ? Y.yoff + ngenes : ngenes;   // full refit: g'W of the orthogonalised block from launch_variant_stats
        ldcy = ldb;
        ldt = ldb;                                   // T_rho: [rpad x ldt] per group (full refit: [variants x ldq])
        tslab = fast ? ldq * ldt : (long)BLK * ldq;
        prep_d = (int)fastscan_prep_doubles();
        eff_rows = (size_t)ngenes * BLK;
        for (int i = 0; i < ngenes; i++) null_lml[i] = null[6 * (size_t)i + 4];
        if (fast) layout();
    }

    // column layout of the fast path's right-hand operands (per group: its own block, then its genes)
    void layout() {
        long col1 = 0, col2 = 0;
        for (int q = 0; q < ngrp; q++) {
            const int k = R.grp_rho[q];
            MultiGroup& G = groups[q];
            G.r = bg->r[k];
            G.rpad = (int)std::max<long>(round_up(G.r, GEMM_BK), GEMM_BK);
            G.ldW = ldq;
            G.col1 = (int)col1; G.col2 = (int)col2;
            G.tW = genes[R.members[q][0]]->rot.as<double>() + (long)k * slab + ldq;
            long a1 = col1 + c, a2 = col2 + 1;
            for (int i : R.members[q]) {
                mg[i].group = q;
                mg[i].col1 = (int)a1; a1 += c + 2;
                mg[i].col2 = (int)a2; a2 += 1;
            }
            col1 = round_up(a1, 16);
            col2 = round_up(a2, 16);
            rmax = std::max(rmax, G.rpad);
        }
        ld1 = col1 + 128;
        ld2 = col2 + 128;
    }

    int workspaces() {
        CRM_TRY(Y.ensure(ctx, np));
        CRM_TRY(Y.clear(st, np));
        CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)ngrp * tslab));
        CRM_TRY(B.ensure());
        if (fast) {
            CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)ngrp * tslab));
            CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)ldq * (ld1 + ld2)));
            CRM_TRY(ctx->ws_F.ensure(sizeof(double) * (size_t)BLK * (ld1 + ld2)));
        }
        CRM_TRY(carve_workspace(ctx->ws_small, [&](auto& take) {
            B.carve(take, !fast);
            take(d_cy, sizeof(double) * rows_cy * ldcy);
            take(d_alt, sizeof(double) * (size_t)ngenes * BLK), take(d_pv, sizeof(double) * (size_t)ngenes * BLK);
            take(d_nl, sizeof(double) * ngenes);
            take(d_prep, fast ? sizeof(double) * (size_t)ngenes * prep_d : 0), take(d_wts, fast ? sizeof(double) * (size_t)ngenes * ldq : 0);
            take(d_args, fast ? sizeof(AssocArgs) * ngenes : 0), take(d_mg, fast ? sizeof(MultiGene) * ngenes : 0);
            take(d_grp, fast ? sizeof(MultiGroup) * ngrp : 0);
            take(d_trial, !fast ? sizeof(NullFitTrial) * BLK : 0), take(d_fit, !fast ? sizeof(NullFitOut) * BLK : 0);
            take(Y.d_srcs, Y.srcs_bytes());
            take(d_eff, eff ? (sizeof(double) * 5 + sizeof(int)) * eff_rows : 0), take(d_effg, eff ? sizeof(AssocEffectsGene) * ngenes : 0);
        }));
        CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (size_t)(3 * ngrp + 2)));
        d_probs = ctx->ws_probs.as<GemmProblem>();
        Tb = ctx->ws_T.as<double>();
        return CRM_OK;
    }

    // what does not depend on the block: the null lmls, the phenotype matrix, the fast path's records and right-hand
    // operands, the shared arguments of the refits, the records of the effects launch
    int operands() {
        CRM_HIP(hipMemcpyAsync(d_nl, null_lml.data(), sizeof(double) * ngenes, hipMemcpyHostToDevice, st));
        CRM_TRY(Y.fill(st, np));
        if (fast) CRM_TRY(fast_operands());
        else CRM_TRY(refit_operands());
        if (eff) CRM_TRY(effects_operands());
        return CRM_OK;
    }

    int fast_operands() {
        aa.resize(ngenes);
        for (int i = 0; i < ngenes; i++) {
            crm_gene* g = genes[i];
            const int k = R.ri[i];
            AssocArgs& A = aa[i];
            A.ty = g->rot.as<double>() + (long)k * slab;
            A.tW = A.ty + ldq; A.ldW = ldq; A.S0 = bg->S0[k].as<double>();
            A.r = bg->r[k]; A.c = c; A.n = n; A.delta0 = null[6 * (size_t)i + 5];
            A.WW = g->WW.as<double>(); A.Wy = g->Wy.as<double>(); A.yy = g->yy;
            MultiGene& M = mg[i];
            M.ty = A.ty;
            M.wts = d_wts + (size_t)i * ldq;
            M.prep = d_prep + (size_t)i * prep_d;
            M.row_y = (int)(Y.yoff + i);
            M.inv_d = 1.0 / A.delta0;
            M.null_lml = null_lml[i];
        }
        CRM_HIP(hipMemcpyAsync(d_args, aa.data(), sizeof(AssocArgs) * ngenes, hipMemcpyHostToDevice, st));
        CRM_HIP(hipMemcpyAsync(d_mg, mg.data(), sizeof(MultiGene) * ngenes, hipMemcpyHostToDevice, st));
        CRM_HIP(hipMemcpyAsync(d_grp, groups.data(), sizeof(MultiGroup) * ngrp, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_fastscan_prep_batch(st, d_args, ngenes, c, d_prep, prep_d, d_wts, ldq));
        double* B1 = ctx->ws_A.as<double>();
        double* B2 = B1 + (size_t)ldq * ld1;
        CRM_HIP(hipMemsetAsync(B1, 0, sizeof(double) * (size_t)ldq * (ld1 + ld2), st));
        hipLaunchKernelGGL(multi_rhs_kernel, dim3((rmax + 255) / 256, ngenes + ngrp), dim3(256), 0, st, (const MultiGene*)d_mg,
                           ngenes, (const MultiGroup*)d_grp, c, B1, ld1, B2, ld2);
        CRM_HIP(hipGetLastError());
        return CRM_OK;
    }

    // the shared full-refit arguments: the null's rho per gene, the block's shared quantities
    int refit_operands() {
        alt.nrho = 1; alt.c = c; alt.restricted = 0;
        alt.polish = (ctx->polish && c <= CRM_MAX_COV) ? 1 : 0;
        alt.exact = (ctx->nullfit_exact || form("nullfit_exact", 0)) ? 1 : 0;
        alt.n = n;
        alt.gg = B.d_gg; alt.gW = B.d_gW; alt.ld_gW = B.ld_gW;
        alt.g_drop = B.d_drop;
        alt.trial = d_trial; alt.out = d_fit;
        if (c > CRM_MAX_COV_WIDE) {
            CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(BLK, B.nrho, c)));
            alt.xwide = ctx->ws_xwide.as<double>();
        }
        return CRM_OK;
    }

    // the per-gene records of the effects launch; fast: in the order of the rho groups, so that the tests that read one
    // row of T are neighbours in the grid (record q writes the rows of gene eff_gene[q])
    int effects_operands() {
        eg.resize(ngenes);
        std::vector<int> eff_gene(ngenes);
        for (int i = 0; i < ngenes; i++) eff_gene[i] = i;
        if (fast)
            std::stable_sort(eff_gene.begin(), eff_gene.end(),
                             [&](int x, int y) { return R.grp_of_rho[R.ri[x]] < R.grp_of_rho[R.ri[y]]; });
        for (int q = 0; q < ngenes; q++) {
            const int i = eff_gene[q], k = R.ri[i];
            crm_gene* g = genes[i];
            AssocEffectsGene& E = eg[q];
            E.T = Tb + (size_t)R.grp_of_rho[k] * tslab;
            E.t_sb = fast ? 1 : ldq; E.t_sk = fast ? ldt : 1;
            E.ty = g->rot.as<double>() + (long)k * slab;
            E.tW = E.ty + ldq; E.ldW = ldq; E.S0 = bg->S0[k].as<double>();
            E.r = bg->r[k]; E.c = c; E.n = n;
            E.WW = g->WW.as<double>(); E.Wy = g->Wy.as<double>(); E.yy = g->yy;
            E.gg = B.d_gg;
            if (fast) {
                E.gy = d_cy + (size_t)(Y.yoff + i) * ldcy;
                E.gW = d_cy; E.gW_sb = 1; E.gW_su = ldcy;
                E.prep = d_prep + (size_t)i * prep_d;
                E.wts = d_wts + (size_t)i * ldq;
                E.delta0 = null[6 * (size_t)i + 5];
            } else {
                E.gy = d_cy + (size_t)i * ldcy;
                E.gW = B.d_gW; E.gW_sb = B.ld_gW; E.gW_su = 1;
                E.trial = alt.trial;
            }
            E.alt_lml = d_alt + (size_t)i * BLK;
            E.null_lml = null_lml[i];
            double* o = d_eff + (size_t)i * BLK;
            E.out_beta = o; E.out_se = o + eff_rows; E.out_delta = o + 2 * eff_rows; E.out_scale = o + 3 * eff_rows;
            E.out_logp = o + 4 * eff_rows;
            E.out_status = (int*)(d_eff + 5 * eff_rows) + (size_t)i * BLK;
        }
        CRM_HIP(hipMemcpyAsync(d_effg, eg.data(), sizeof(AssocEffectsGene) * ngenes, hipMemcpyHostToDevice, st));
        return CRM_OK;
    }

    // one batched launch: g'y_j (fast: g'W too) against the phenotype matrix, and T_rho of every rho group
    int block_products(int nb) {
        probs.clear();
        GemmProblem p{};
        if (fast) {   // (gg came from the one column reduction of the block's preparation)
            p.X = Y.XY; p.ldx = Y.ldxy; p.Y = B.Gb; p.ldy = ldb; p.C = d_cy; p.ldc = ldcy; p.M = (int)rows_cy; p.N = nb;
            probs.push_back(p);
            for (int q = 0; q < ngrp; q++) {
                GemmProblem t{};
                t.X = bg->Q0[R.grp_rho[q]].as<double>(); t.ldx = ldq; t.Y = B.Gb; t.ldy = ldb;
                t.C = Tb + (size_t)q * tslab; t.ldc = ldt; t.M = groups[q].rpad; t.N = nb;
                probs.push_back(t);
            }
        } else {
            p.X = Y.XY + Y.yoff; p.ldx = Y.ldxy; p.Y = B.Gx; p.ldy = ldb; p.C = d_cy; p.ldc = ldcy; p.M = ngenes; p.N = nb;
            probs.push_back(p);
            for (int q = 0; q < ngrp; q++) probs.push_back(B.rotation(R.grp_rho[q], nb, Tb + (size_t)q * tslab, ldq));
        }
        int max_m = 0, max_n = 0;
        for (const GemmProblem& q : probs) { max_m = std::max(max_m, q.M); max_n = std::max(max_n, q.N); }
        CRM_HIP(hipMemcpyAsync(d_probs, probs.data(), sizeof(GemmProblem) * probs.size(), hipMemcpyHostToDevice, st));
        return launch_gemm_tn(ctx, d_probs, (int)probs.size(), max_m, max_n, np, false, 0, 1, 0);
    }

    // fast: T o T, the two weighted products per rho group, one thread per (gene, variant) to finish
    int fast_tests(int nb) {
        double* T2 = ctx->ws_G2.as<double>();
        hipLaunchKernelGGL(multi_square_kernel, dim3((nb + 255) / 256, rmax, ngrp), dim3(256), 0, st, Tb, T2, tslab, ldt,
                           (const MultiGroup*)d_grp, nb);
        CRM_HIP(hipGetLastError());
        double* B1 = ctx->ws_A.as<double>();
        double* B2 = B1 + (size_t)ldq * ld1;
        double* C1 = ctx->ws_F.as<double>();
        double* C2 = C1 + (size_t)BLK * ld1;
        pp.clear();
        int mn = 0;
        for (int q = 0; q < ngrp; q++) {
            const MultiGroup& G = groups[q];
            const int n1 = (q + 1 < ngrp ? groups[q + 1].col1 : (int)ld1 - 128) - G.col1;
            const int n2 = (q + 1 < ngrp ? groups[q + 1].col2 : (int)ld2 - 128) - G.col2;
            GemmProblem a{};
            a.X = Tb + (size_t)q * tslab; a.ldx = ldt; a.Y = B1 + G.col1; a.ldy = ld1; a.C = C1 + G.col1; a.ldc = ld1;
            a.M = nb; a.N = n1; a.cells = G.rpad;
            GemmProblem b = a;
            b.X = T2 + (size_t)q * tslab; b.Y = B2 + G.col2; b.ldy = ld2; b.C = C2 + G.col2; b.ldc = ld2; b.N = n2;
            pp.push_back(a);
            pp.push_back(b);
            mn = std::max(mn, std::max(n1, n2));
        }
        GemmProblem* d_pp = d_probs + probs.size();
        CRM_HIP(hipMemcpyAsync(d_pp, pp.data(), sizeof(GemmProblem) * pp.size(), hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_pp, (int)pp.size(), nb, mn, rmax, false, 0, 1, 0));
        const dim3 grid((nb + 127) / 128, ngenes);
        if (c <= 8)
            hipLaunchKernelGGL(multi_finish_kernel<8>, grid, dim3(128), 0, st, (const MultiGene*)d_mg, (const MultiGroup*)d_grp, c, n,
                               nb, C1, ld1, C2, ld2, B.d_gg, d_cy, ldcy, d_alt, d_pv, (long)BLK);
        else
            hipLaunchKernelGGL(multi_finish_kernel<0>, grid, dim3(128), 0, st, (const MultiGene*)d_mg, (const MultiGroup*)d_grp, c, n,
                               nb, C1, ld1, C2, ld2, B.d_gg, d_cy, ldcy, d_alt, d_pv, (long)BLK);
        CRM_HIP(hipGetLastError());
        if (eff) CRM_TRY(launch_assoc_effects(st, d_effg, ngenes, nb, c, true));
        return CRM_OK;
    }

    // full refit: per gene the null-fit kernels over the block on the shared T(rho*), then the LRT of all genes
    int refit_tests(int nb) {
        for (int i = 0; i < ngenes; i++) {
            crm_gene* g = genes[i];
            const int k = R.ri[i];
            NullFitRho& A = alt.rho[0];
            A.T = Tb + (size_t)R.grp_of_rho[k] * tslab; A.ldT = ldq;
            A.ty = g->rot.as<double>() + (long)k * slab;
            A.tW = A.ty + ldq; A.ldW = ldq;
            A.S0 = bg->S0[k].as<double>();
            A.r = bg->r[k];
            alt.WW = g->WW.as<double>(); alt.Wy = g->Wy.as<double>(); alt.yy = g->yy;
            alt.gy = d_cy + (size_t)i * ldcy;
            CRM_TRY(launch_nullfit(st, alt, nb));
            CRM_TRY(launch_gather_trial_lml(st, alt.trial, nb, d_alt + (size_t)i * BLK));
            if (eff) CRM_TRY(launch_assoc_effects(st, d_effg + i, 1, nb, c, false));
        }
        hipLaunchKernelGGL(multi_lrt_kernel, dim3((nb + 255) / 256, ngenes), dim3(256), 0, st, d_alt, d_nl, nb, (long)BLK, d_pv);
        CRM_HIP(hipGetLastError());
        return CRM_OK;
    }

    // the block's rows, gene-major on the host: row i of [ngenes x count]
    template <class T>
    int copy_rows(T* out, long done, int nb, const T* d_rows) {
        if (out)
            CRM_HIP(hipMemcpy2DAsync(out + done, sizeof(T) * B.count, d_rows, sizeof(T) * BLK, sizeof(T) * nb, ngenes,
                                     hipMemcpyDeviceToHost, st));
        return CRM_OK;
    }
    int copy_out(long done, int nb, double* out_pvalue, double* out_alt_lml) {
        CRM_TRY(copy_rows(out_pvalue, done, nb, d_pv));
        CRM_TRY(copy_rows(out_alt_lml, done, nb, d_alt));
        if (!eff) return CRM_OK;
        double* const outs[5] = {eff->beta, eff->se, eff->delta, eff->scale, eff->logp};
        for (int q = 0; q < 5; q++) CRM_TRY(copy_rows(outs[q], done, nb, d_eff + q * eff_rows));
        return copy_rows(eff->status, done, nb, (const int*)(d_eff + 5 * eff_rows));
    }
};

int scan_association_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, int fast,
                           const double* null, double* out_pvalue, double* out_alt_lml, const AssocEffectsOut* eff) {
    const char* what = "association multi";
    CRM_TRY(check_shared_genes(what, genes, ngenes, false));
    if (!panel || !null) {
        set_error("%s: %s is NULL", what, panel ? "null" : "panel");
        return CRM_ERR_ARG;
    }
    crm_background* bg = genes[0]->bg;
    CRM_TRY(check_panel_range(what, bg, panel, first, count));
    NullRows R;
    CRM_TRY(R.read(what, bg, null, ngenes, fast != 0));
    if (genes[0]->c > CMAX) {
        set_error("%s: %d covariate columns (supported up to %d)", what, genes[0]->c, CMAX);
        return CRM_ERR_UNSUPPORTED;
    }
    if (count == 0) return CRM_OK;
    InScan in_scan;
    CRM_TRY(in_scan.enter(bg->ctx, what));
    CRM_HIP(hipSetDevice(bg->ctx->device));
    CRM_TRY(R.group(bg));
    AssocMultiScan S(genes, ngenes, panel, first, count, fast, null, R, eff);
    CRM_TRY(S.workspaces());
    CRM_TRY(S.operands());
    for (long done = 0; done < count; done += S.BLK) {
        const int nb = S.B.nb_at(done);
        CRM_TRY(S.B.prepare(done, nb, fast ? 1 : S.c));   // (fast: g'W and g'y_j come from the product below)
        CRM_TRY(S.block_products(nb));
        CRM_TRY(fast ? S.fast_tests(nb) : S.refit_tests(nb));
        CRM_TRY(S.copy_out(done, nb, out_pvalue, out_alt_lml));
        CRM_HIP(hipStreamSynchronize(S.st));
        S.ctx->report(done + nb, count);
    }
    return CRM_OK;
}

}  // namespace

extern "C" int crm_scan_association_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                                          int fast, const double* null, double* out_pvalue, double* out_alt_lml) {
    return crm::guarded_on("crm_scan_association_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    return scan_association_multi(genes, ngenes, panel, first, count, fast, null, out_pvalue, out_alt_lml, nullptr);
    });
}

extern "C" int crm_scan_association_multi_effects(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                                                  int fast, const double* null, double* out_pvalue, double* out_alt_lml,
                                                  double* out_beta, double* out_se, double* out_delta, double* out_scale,
                                                  double* out_logp, int* out_status) {
    return crm::guarded_on("crm_scan_association_multi_effects", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    const AssocEffectsOut eff{out_beta, out_se, out_delta, out_scale, out_logp, out_status};
    return scan_association_multi(genes, ngenes, panel, first, count, fast, null, out_pvalue, out_alt_lml, &eff);
    });
}
