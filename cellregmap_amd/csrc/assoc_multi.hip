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
#include "objects.h"

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

// XY[i, dst[q]] = src[q][i * ld[q]] for the columns q of [W | y_1 .. y_g] (cells_pad rows: the sources are zero padded)
struct ColumnSource {
    const double* src;
    long ld;
    long dst;
};
__global__ __launch_bounds__(256) void multi_columns_kernel(const ColumnSource* __restrict__ cols, long rows, double* __restrict__ XY,
                                                            long ldxy) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const ColumnSource s = cols[blockIdx.y];
    XY[i * ldxy + s.dst] = s.src[i * s.ld];
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

// The null model of crm_scan_association (ML, X = W, over the rho grid) with the same arguments, into *out.
int association_null_fit(crm_gene* gene, double* d_zero, double* d_gg, double* d_gy, double* d_gW, long ld_gW,
                         NullFitTrial* d_trial, NullFitOut* d_fit, double* xwide) {
    NullFitArgs fa{};
    nullfit_gene_args(fa, gene, 0);
    for (int i = 0; i < fa.nrho; i++) { fa.rho[i].T = d_zero; fa.rho[i].ldT = 0; }
    fa.gg = d_gg; fa.gy = d_gy; fa.gW = d_gW; fa.ld_gW = ld_gW;
    fa.trial = d_trial; fa.out = d_fit;
    fa.xwide = xwide;
    return launch_nullfit(gene->ctx->stream, fa, 1);
}

int check_genes(crm_gene* const* genes, int ngenes, const char* what) {
    if (!genes || ngenes <= 0) {
        set_error("%s: no genes", what);
        return CRM_ERR_ARG;
    }
    for (int i = 0; i < ngenes; i++)
        if (!genes[i] || !genes[i]->bg) {
            set_error("%s: gene %d is NULL", what, i);
            return CRM_ERR_ARG;
        }
    const crm_gene* g0 = genes[0];
    for (int i = 1; i < ngenes; i++) {
        const crm_gene* g = genes[i];
        // the shared pass takes g'W, T(rho)'W and the orthogonalisation from the first gene: the others must hold the same W
        if (g->bg != g0->bg || g->ctx != g0->ctx || g->c != g0->c || g->w_key != g0->w_key) {
            set_error("%s: genes of one call must share the background and W (gene %d differs from gene 0)", what, i);
            return CRM_ERR_ARG;
        }
    }
    return CRM_OK;
}

}  // namespace

}  // namespace crm

using namespace crm;

extern "C" int crm_association_null_multi(crm_gene* const* genes, int ngenes, double* out_null) {
    return crm::guarded_on("crm_association_null_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    CRM_TRY(check_genes(genes, ngenes, "association null multi"));
    if (!out_null) {
        set_error("association null multi: out_null is NULL");
        return CRM_ERR_ARG;
    }
    crm_background* bg = genes[0]->bg;
    crm_ctx* ctx = bg->ctx;
    if (ctx->in_scan) {
        set_error("association null multi: a scan is running on this context (started from a progress callback?)");
        return CRM_ERR_UNSUPPORTED;
    }
    struct InScan { crm_ctx* c; explicit InScan(crm_ctx* c_) : c(c_) { c->in_scan = true; } ~InScan() { c->in_scan = false; } } in_scan(ctx);
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long ldq = bg->ldq;
    const int nrho = bg->nrho, c = genes[0]->c;
    const long ld_gW = round_up(c, 8);
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_zero = carve(sizeof(double) * ldq), o_gg = carve(sizeof(double)), o_gy = carve(sizeof(double)),
                 o_gW = carve(sizeof(double) * ld_gW), o_trial = carve(sizeof(NullFitTrial) * nrho * nrho),
                 o_fit = carve(sizeof(NullFitOut) * ngenes);
    CRM_TRY(ctx->ws_small.ensure(off));
    char* sm = ctx->ws_small.as<char>();
    double* d_zero = (double*)(sm + o_zero);
    NullFitOut* d_fit = (NullFitOut*)(sm + o_fit);
    CRM_HIP(hipMemsetAsync(sm, 0, o_trial, st));   // zero T row, gg, gy, gW: the fit drops the zero "variant"
    double* xwide = nullptr;
    if (c > CRM_MAX_COV_WIDE) {
        CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(1, nrho, c)));
        xwide = ctx->ws_xwide.as<double>();
    }
    for (int i = 0; i < ngenes; i++)
        CRM_TRY(association_null_fit(genes[i], d_zero, (double*)(sm + o_gg), (double*)(sm + o_gy), (double*)(sm + o_gW), ld_gW,
                                     (NullFitTrial*)(sm + o_trial), d_fit + i, xwide));
    std::vector<NullFitOut> fits(ngenes);
    CRM_HIP(hipMemcpyAsync(fits.data(), d_fit, sizeof(NullFitOut) * ngenes, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < ngenes; i++) {
        const NullFitOut& f = fits[i];
        if (f.rho_index < 0 || f.rho_index >= nrho) {
            set_error("association null multi: the null model's fit of gene %d did not run (grid index %d)", i, f.rho_index);
            return CRM_ERR_NUMERIC;
        }
        const double rho = bg->rho[f.rho_index];
        double* o = out_null + 6 * (size_t)i;
        o[0] = rho;
        o[1] = f.v0 * rho;
        o[2] = f.v0 * (1 - rho);
        o[3] = f.v1;
        o[4] = f.lml;
        o[5] = f.delta;
    }
    return CRM_OK;
    });
}

namespace {

// The scan behind crm_scan_association_multi (eff null: its launches and nothing else) and
// crm_scan_association_multi_effects (assoc_effects.hip: fast, one more launch per block over every (variant, gene); full
// refit, one per gene after its alt fits, whose trial records the next gene overwrites).
int scan_association_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, int fast,
                           const double* null, double* out_pvalue, double* out_alt_lml, const AssocEffectsOut* eff) {
    CRM_TRY(check_genes(genes, ngenes, "association multi"));
    if (!panel || !null) {
        set_error("association multi: %s is NULL", panel ? "null" : "panel");
        return CRM_ERR_ARG;
    }
    crm_gene* g0 = genes[0];
    crm_background* bg = g0->bg;
    crm_ctx* ctx = bg->ctx;
    if (panel->ctx != ctx || panel->n != bg->n) {
        set_error("association multi: genes and panel do not match (context / cell count: %ld against %ld)", panel->n, bg->n);
        return CRM_ERR_ARG;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("association multi: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    const int nrho = bg->nrho, c = g0->c;
    std::vector<int> ri(ngenes);
    for (int i = 0; i < ngenes; i++) {
        const double* row = null + 6 * (size_t)i;
        ri[i] = -1;
        for (int k = 0; k < nrho; k++)
            if (bg->rho[k] == row[0]) { ri[i] = k; break; }
        if (ri[i] < 0) {
            set_error("association multi: null row %d has rho1 = %.17g, not a point of the background's grid", i, row[0]);
            return CRM_ERR_ARG;
        }
        if (!std::isfinite(row[4])) {
            set_error("association multi: null row %d has a non-finite lml (the null model could not be fitted)", i);
            return CRM_ERR_ARG;
        }
        if (fast && !(row[5] > 0.0 && row[5] <= 1.0)) {
            set_error("association multi: null row %d has delta = %g outside (0, 1]", i, row[5]);
            return CRM_ERR_ARG;
        }
    }
    if (c > CMAX) {
        set_error("association multi: %d covariate columns (supported up to %d)", c, CMAX);
        return CRM_ERR_UNSUPPORTED;
    }
    if (count == 0) return CRM_OK;
    if (ctx->in_scan) {
        set_error("association multi: another scan is running on this context (started from a progress callback?)");
        return CRM_ERR_UNSUPPORTED;
    }
    struct InScan { crm_ctx* c; explicit InScan(crm_ctx* c_) : c(c_) { c->in_scan = true; } ~InScan() { c->in_scan = false; } } in_scan(ctx);
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    const int BLK = (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : CRM_DEFAULT_BLOCK,
                                        round_up(std::max<long>(count, 1), 128));
    const long ldb = BLK + 128;   // (column tiles of 128 over the variants stay inside every [.. x variants] buffer)
    const long ld_gW = round_up(c, 8);
    const long slab = (long)(1 + c) * ldq;

    // rho groups: the distinct grid indices of the genes' null models, in grid order
    std::vector<int> grp_of_rho(nrho, -1), grp_rho;
    for (int i = 0; i < ngenes; i++) grp_of_rho[ri[i]] = 0;
    for (int k = 0; k < nrho; k++)
        if (grp_of_rho[k] == 0) { grp_of_rho[k] = (int)grp_rho.size(); grp_rho.push_back(k); }
    const int ngrp = (int)grp_rho.size();
    for (int k : grp_rho) CRM_TRY(crm_background_require_q0(bg, k));

    // [W | y_1 .. y_g] (cells x ldxy): W at columns 0 .. c-1, the phenotypes from column yoff
    const long yoff = round_up(c, 16);
    const long ldxy = round_up(yoff + ngenes, 128) + 128;   // (column tiles read from column 0 or from yoff stay inside a row)
    CRM_TRY(ctx->ws_XG.ensure(sizeof(double) * (size_t)np * ldxy));
    double* XY = ctx->ws_XG.as<double>();
    CRM_HIP(hipMemsetAsync(XY, 0, sizeof(double) * (size_t)np * ldxy, st));
    std::vector<ColumnSource> srcs;
    for (int u = 0; u < c; u++) srcs.push_back({g0->yW.as<double>() + 1 + u, g0->ld_yw, u});
    for (int i = 0; i < ngenes; i++) srcs.push_back({genes[i]->yW.as<double>(), genes[i]->ld_yw, yoff + i});
    const long rows_cy = fast ? yoff + ngenes : ngenes;   // full refit: g'W of the orthogonalised block from launch_variant_stats

    // column layout of the fast path's right-hand operands (per group: its own block, then its genes)
    std::vector<MultiGroup> groups(ngrp);
    std::vector<MultiGene> mg(ngenes);
    long ld1 = 0, ld2 = 0;
    if (fast) {
        long col1 = 0, col2 = 0;
        for (int q = 0; q < ngrp; q++) {
            const int k = grp_rho[q];
            MultiGroup& R = groups[q];
            R.r = bg->r[k];
            R.rpad = (int)std::max<long>(round_up(R.r, GEMM_BK), GEMM_BK);
            R.ldW = ldq;
            R.col1 = (int)col1; R.col2 = (int)col2;
            int first_gene = -1;
            for (int i = 0; i < ngenes; i++)
                if (ri[i] == k && first_gene < 0) first_gene = i;
            R.tW = genes[first_gene]->rot.as<double>() + (long)k * slab + ldq;
            long a1 = col1 + c, a2 = col2 + 1;
            for (int i = 0; i < ngenes; i++)
                if (ri[i] == k) {
                    mg[i].group = q;
                    mg[i].col1 = (int)a1; a1 += c + 2;
                    mg[i].col2 = (int)a2; a2 += 1;
                }
            col1 = round_up(a1, 16);
            col2 = round_up(a2, 16);
        }
        ld1 = col1 + 128;
        ld2 = col2 + 128;
    }

    // device work buffers
    const long ldt = ldb;                    // T_rho: [rpad x ldt] per group (full refit: [variants x ldq])
    const long tslab = fast ? ldq * ldt : (long)BLK * ldq;
    CRM_TRY(ctx->ws_T.ensure(sizeof(double) * (size_t)ngrp * tslab));
    CRM_TRY(ctx->ws_Gb.ensure(sizeof(double) * (size_t)np * ldb));
    if (!fast) CRM_TRY(ctx->ws_Gx.ensure(sizeof(double) * (size_t)np * ldb));
    if (fast) {
        CRM_TRY(ctx->ws_G2.ensure(sizeof(double) * (size_t)ngrp * tslab));
        CRM_TRY(ctx->ws_A.ensure(sizeof(double) * (size_t)ldq * (ld1 + ld2)));
        CRM_TRY(ctx->ws_F.ensure(sizeof(double) * (size_t)BLK * (ld1 + ld2)));
    }
    const long ldcy = ldb;
    const int prep_d = (int)fastscan_prep_doubles();
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_cy = carve(sizeof(double) * rows_cy * ldcy), o_gg = carve(sizeof(double) * BLK),
                 o_gy = carve(sizeof(double) * BLK), o_gW = carve(sizeof(double) * BLK * ld_gW),
                 o_part = carve(variant_stats_workspace(BLK, std::min(c, CRM_MAX_COV))),
                 o_alt = carve(sizeof(double) * (size_t)ngenes * BLK), o_pv = carve(sizeof(double) * (size_t)ngenes * BLK),
                 o_nl = carve(sizeof(double) * ngenes),
                 o_prep = fast ? carve(sizeof(double) * (size_t)ngenes * prep_d) : 0,
                 o_wts = fast ? carve(sizeof(double) * (size_t)ngenes * ldq) : 0,
                 o_args = fast ? carve(sizeof(AssocArgs) * ngenes) : 0,
                 o_mg = fast ? carve(sizeof(MultiGene) * ngenes) : 0, o_grp = fast ? carve(sizeof(MultiGroup) * ngrp) : 0,
                 o_trial = !fast ? carve(sizeof(NullFitTrial) * BLK) : 0, o_fit = !fast ? carve(sizeof(NullFitOut) * BLK) : 0,
                 o_coef = !fast ? carve(sizeof(double) * (size_t)c * ldb) : 0, o_thr = !fast ? carve(sizeof(double) * BLK) : 0,
                 o_drop = !fast ? carve(sizeof(int) * BLK) : 0, o_src = carve(sizeof(ColumnSource) * srcs.size());
    const size_t eff_rows = (size_t)ngenes * BLK;   // per output: [ngenes x BLK], five of doubles, then the status
    const size_t o_eff = eff ? carve((sizeof(double) * 5 + sizeof(int)) * eff_rows) : 0,
                 o_effg = eff ? carve(sizeof(AssocEffectsGene) * ngenes) : 0;
    CRM_TRY(ctx->ws_small.ensure(off));
    char* sm = ctx->ws_small.as<char>();
    double* d_cy = (double*)(sm + o_cy);
    double* d_gg = (double*)(sm + o_gg);
    double* d_gy = (double*)(sm + o_gy);
    double* d_gW = (double*)(sm + o_gW);
    double* d_part = (double*)(sm + o_part);
    double* d_alt = (double*)(sm + o_alt);
    double* d_pv = (double*)(sm + o_pv);
    double* d_nl = (double*)(sm + o_nl);
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (size_t)(3 * ngrp + 2)));
    GemmProblem* d_probs = ctx->ws_probs.as<GemmProblem>();
    std::vector<double> null_lml(ngenes);
    for (int i = 0; i < ngenes; i++) null_lml[i] = null[6 * (size_t)i + 4];
    CRM_HIP(hipMemcpyAsync(d_nl, null_lml.data(), sizeof(double) * ngenes, hipMemcpyHostToDevice, st));
    const double* d_W = g0->yW.as<double>() + 1;
    double* Tb = ctx->ws_T.as<double>();
    CRM_HIP(hipMemcpyAsync(sm + o_src, srcs.data(), sizeof(ColumnSource) * srcs.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(multi_columns_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)srcs.size()), dim3(256), 0, st,
                       (const ColumnSource*)(sm + o_src), np, XY, ldxy);
    CRM_HIP(hipGetLastError());

    // the per-gene records of the fast path and the right-hand operands (once per call)
    std::vector<AssocArgs> aa(fast ? ngenes : 0);   // (host sources of asynchronous copies: alive until the last sync)
    if (fast) {
        double* d_prep = (double*)(sm + o_prep);
        double* d_wts = (double*)(sm + o_wts);
        for (int i = 0; i < ngenes; i++) {
            crm_gene* g = genes[i];
            const int k = ri[i];
            AssocArgs& A = aa[i];
            A.ty = g->rot.as<double>() + (long)k * slab;
            A.tW = A.ty + ldq; A.ldW = ldq; A.S0 = bg->S0[k].as<double>();
            A.r = bg->r[k]; A.c = c; A.n = n; A.delta0 = null[6 * (size_t)i + 5];
            A.WW = g->WW.as<double>(); A.Wy = g->Wy.as<double>(); A.yy = g->yy;
            MultiGene& M = mg[i];
            M.ty = A.ty;
            M.wts = d_wts + (size_t)i * ldq;
            M.prep = d_prep + (size_t)i * prep_d;
            M.row_y = (int)(yoff + i);
            M.inv_d = 1.0 / A.delta0;
            M.null_lml = null_lml[i];
        }
        CRM_HIP(hipMemcpyAsync(sm + o_args, aa.data(), sizeof(AssocArgs) * ngenes, hipMemcpyHostToDevice, st));
        CRM_HIP(hipMemcpyAsync(sm + o_mg, mg.data(), sizeof(MultiGene) * ngenes, hipMemcpyHostToDevice, st));
        CRM_HIP(hipMemcpyAsync(sm + o_grp, groups.data(), sizeof(MultiGroup) * ngrp, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_fastscan_prep_batch(st, (const AssocArgs*)(sm + o_args), ngenes, c, d_prep, prep_d, d_wts, ldq));
        double* B1 = ctx->ws_A.as<double>();
        double* B2 = B1 + (size_t)ldq * ld1;
        int rmax = 0;
        for (const MultiGroup& R : groups) rmax = std::max(rmax, R.rpad);
        CRM_HIP(hipMemsetAsync(B1, 0, sizeof(double) * (size_t)ldq * (ld1 + ld2), st));
        hipLaunchKernelGGL(multi_rhs_kernel, dim3((rmax + 255) / 256, ngenes + ngrp), dim3(256), 0, st,
                           (const MultiGene*)(sm + o_mg), ngenes, (const MultiGroup*)(sm + o_grp), c, B1, ld1, B2, ld2);
        CRM_HIP(hipGetLastError());
    }

    // the shared full-refit arguments: the null's rho per gene, the block's shared quantities
    NullFitArgs alt{};
    if (!fast) {
        alt.nrho = 1; alt.c = c; alt.restricted = 0;
        alt.polish = (ctx->polish && c <= CRM_MAX_COV) ? 1 : 0;
        alt.exact = (ctx->nullfit_exact || form("nullfit_exact", 0)) ? 1 : 0;
        alt.n = n;
        alt.gg = d_gg; alt.gW = d_gW; alt.ld_gW = ld_gW;
        alt.g_drop = (int*)(sm + o_drop);
        alt.trial = (NullFitTrial*)(sm + o_trial); alt.out = (NullFitOut*)(sm + o_fit);
        if (c > CRM_MAX_COV_WIDE) {
            CRM_TRY(ctx->ws_xwide.ensure(sizeof(double) * nullfit_xwide_scratch_doubles(BLK, nrho, c)));
            alt.xwide = ctx->ws_xwide.as<double>();
        }
    }

    // the per-gene records of the effects launch; fast: in the order of the rho groups, so that the tests that read one
    // row of T are neighbours in the grid (record q writes the rows of gene eff_gene[q])
    std::vector<AssocEffectsGene> eg(eff ? ngenes : 0);   // (host source of an asynchronous copy)
    double* d_eff = eff ? (double*)(sm + o_eff) : nullptr;
    const AssocEffectsGene* d_effg = eff ? (const AssocEffectsGene*)(sm + o_effg) : nullptr;
    if (eff) {
        std::vector<int> eff_gene(ngenes);
        for (int i = 0; i < ngenes; i++) eff_gene[i] = i;
        if (fast) std::stable_sort(eff_gene.begin(), eff_gene.end(), [&](int x, int y) { return grp_of_rho[ri[x]] < grp_of_rho[ri[y]]; });
        for (int q = 0; q < ngenes; q++) {
            const int i = eff_gene[q], k = ri[i];
            crm_gene* g = genes[i];
            AssocEffectsGene& E = eg[q];
            E.T = Tb + (size_t)grp_of_rho[k] * tslab;
            E.t_sb = fast ? 1 : ldq; E.t_sk = fast ? ldt : 1;
            E.ty = g->rot.as<double>() + (long)k * slab;
            E.tW = E.ty + ldq; E.ldW = ldq; E.S0 = bg->S0[k].as<double>();
            E.r = bg->r[k]; E.c = c; E.n = n;
            E.WW = g->WW.as<double>(); E.Wy = g->Wy.as<double>(); E.yy = g->yy;
            E.gg = d_gg;
            if (fast) {
                E.gy = d_cy + (size_t)(yoff + i) * ldcy;
                E.gW = d_cy; E.gW_sb = 1; E.gW_su = ldcy;
                E.prep = (const double*)(sm + o_prep) + (size_t)i * prep_d;
                E.wts = (const double*)(sm + o_wts) + (size_t)i * ldq;
                E.delta0 = null[6 * (size_t)i + 5];
            } else {
                E.gy = d_cy + (size_t)i * ldcy;
                E.gW = d_gW; E.gW_sb = ld_gW; E.gW_su = 1;
                E.trial = alt.trial;
            }
            E.alt_lml = d_alt + (size_t)i * BLK;
            E.null_lml = null_lml[i];
            double* o = d_eff + (size_t)i * BLK;
            E.out_beta = o; E.out_se = o + eff_rows; E.out_delta = o + 2 * eff_rows; E.out_scale = o + 3 * eff_rows;
            E.out_logp = o + 4 * eff_rows;
            E.out_status = (int*)(d_eff + 5 * eff_rows) + (size_t)i * BLK;
        }
        CRM_HIP(hipMemcpyAsync(sm + o_effg, eg.data(), sizeof(AssocEffectsGene) * ngenes, hipMemcpyHostToDevice, st));
    }

    std::vector<GemmProblem> probs, pp;
    for (long done = 0; done < count; done += BLK) {
        const int nb = (int)std::min<long>(BLK, count - done);
        double* Gb = ctx->ws_Gb.as<double>();
        if (panel->grouped)
            CRM_TRY(launch_expand_block(st, panel->Gd.as<double>() + first + done, panel->ld, panel->group.as<int>(),
                                        np, n, nullptr, nb, Gb, ldb, (int)ldb));
        else
            CRM_TRY(launch_gather_block(st, panel->G.as<double>() + first + done, panel->ld, np, n, nullptr, nullptr,
                                        nb, Gb, ldb, (int)ldb));
        probs.clear();
        if (fast) {
            // gg (the one column reduction); g'W and g'y_j from the product below
            CRM_TRY(launch_variant_stats(st, Gb, ldb, np, nb, g0->yW.as<double>(), d_W, g0->ld_yw, 1, d_part, d_gg, d_gy,
                                         d_gW, ld_gW));
            GemmProblem p{};
            p.X = XY; p.ldx = ldxy; p.Y = Gb; p.ldy = ldb; p.C = d_cy; p.ldc = ldcy; p.M = (int)rows_cy; p.N = nb;
            probs.push_back(p);
            for (int q = 0; q < ngrp; q++) {
                GemmProblem t{};
                t.X = bg->Q0[grp_rho[q]].as<double>(); t.ldx = ldq; t.Y = Gb; t.ldy = ldb;
                t.C = Tb + (size_t)q * tslab; t.ldc = ldt; t.M = groups[q].rpad; t.N = nb;
                probs.push_back(t);
            }
        } else {
            double* Gx = ctx->ws_Gx.as<double>();
            CRM_TRY(launch_variant_stats(st, Gb, ldb, np, nb, g0->yW.as<double>(), d_W, g0->ld_yw, c, d_part, d_gg, d_gy,
                                         d_gW, ld_gW));
            CRM_TRY(launch_ortho_block(st, Gb, ldb, np, nb, (int)ldb, d_W, g0->ld_yw, c, g0->Wproj.as<double>(), d_gW, ld_gW,
                                       (double*)(sm + o_coef), ldb, (double*)(sm + o_thr), Gx, ldb));
            CRM_TRY(launch_variant_stats(st, Gx, ldb, np, nb, g0->yW.as<double>(), d_W, g0->ld_yw, c, d_part, d_gg, d_gy,
                                         d_gW, ld_gW));
            CRM_TRY(launch_ortho_rank(st, d_gg, (double*)(sm + o_thr), nb, (int*)(sm + o_drop)));
            Gb = Gx;
            GemmProblem p{};
            p.X = XY + yoff; p.ldx = ldxy; p.Y = Gb; p.ldy = ldb; p.C = d_cy; p.ldc = ldcy; p.M = ngenes; p.N = nb;
            probs.push_back(p);
            for (int q = 0; q < ngrp; q++) {
                const int k = grp_rho[q];
                GemmProblem t{};
                t.X = Gb; t.ldx = ldb; t.Y = bg->Q0[k].as<double>(); t.ldy = ldq;
                t.C = Tb + (size_t)q * tslab; t.ldc = ldq; t.M = nb; t.N = bg->r[k] > 0 ? bg->r[k] : 1;
                probs.push_back(t);
            }
        }
        int max_m = 0, max_n = 0;
        for (const GemmProblem& p : probs) { max_m = std::max(max_m, p.M); max_n = std::max(max_n, p.N); }
        CRM_HIP(hipMemcpyAsync(d_probs, probs.data(), sizeof(GemmProblem) * probs.size(), hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, (int)probs.size(), max_m, max_n, np, false, 0, 1, 0));

        if (fast) {
            const MultiGroup* d_grp = (const MultiGroup*)(sm + o_grp);
            double* T2 = ctx->ws_G2.as<double>();
            int rmax = 0;
            for (const MultiGroup& R : groups) rmax = std::max(rmax, R.rpad);
            hipLaunchKernelGGL(multi_square_kernel, dim3((nb + 255) / 256, rmax, ngrp), dim3(256), 0, st, Tb, T2, tslab, ldt,
                               d_grp, nb);
            CRM_HIP(hipGetLastError());
            double* B1 = ctx->ws_A.as<double>();
            double* B2 = B1 + (size_t)ldq * ld1;
            double* C1 = ctx->ws_F.as<double>();
            double* C2 = C1 + (size_t)BLK * ld1;
            pp.clear();
            int mn = 0;
            for (int q = 0; q < ngrp; q++) {
                const MultiGroup& R = groups[q];
                const int n1 = (q + 1 < ngrp ? groups[q + 1].col1 : (int)ld1 - 128) - R.col1;
                const int n2 = (q + 1 < ngrp ? groups[q + 1].col2 : (int)ld2 - 128) - R.col2;
                GemmProblem a{};
                a.X = Tb + (size_t)q * tslab; a.ldx = ldt; a.Y = B1 + R.col1; a.ldy = ld1; a.C = C1 + R.col1; a.ldc = ld1;
                a.M = nb; a.N = n1; a.cells = R.rpad;
                GemmProblem b = a;
                b.X = T2 + (size_t)q * tslab; b.Y = B2 + R.col2; b.ldy = ld2; b.C = C2 + R.col2; b.ldc = ld2; b.N = n2;
                pp.push_back(a);
                pp.push_back(b);
                mn = std::max(mn, std::max(n1, n2));
            }
            GemmProblem* d_pp = d_probs + probs.size();
            CRM_HIP(hipMemcpyAsync(d_pp, pp.data(), sizeof(GemmProblem) * pp.size(), hipMemcpyHostToDevice, st));
            CRM_TRY(launch_gemm_tn(ctx, d_pp, (int)pp.size(), nb, mn, rmax, false, 0, 1, 0));
            const dim3 grid((nb + 127) / 128, ngenes);
            if (c <= 8)
                hipLaunchKernelGGL(multi_finish_kernel<8>, grid, dim3(128), 0, st, (const MultiGene*)(sm + o_mg), d_grp, c, n, nb,
                                   C1, ld1, C2, ld2, d_gg, d_cy, ldcy, d_alt, d_pv, (long)BLK);
            else
                hipLaunchKernelGGL(multi_finish_kernel<0>, grid, dim3(128), 0, st, (const MultiGene*)(sm + o_mg), d_grp, c, n, nb,
                                   C1, ld1, C2, ld2, d_gg, d_cy, ldcy, d_alt, d_pv, (long)BLK);
            CRM_HIP(hipGetLastError());
            if (eff) CRM_TRY(launch_assoc_effects(st, d_effg, ngenes, nb, c, true));
        } else {
            for (int i = 0; i < ngenes; i++) {
                crm_gene* g = genes[i];
                const int k = ri[i];
                NullFitRho& R = alt.rho[0];
                R.T = Tb + (size_t)grp_of_rho[k] * tslab; R.ldT = ldq;
                R.ty = g->rot.as<double>() + (long)k * slab;
                R.tW = R.ty + ldq; R.ldW = ldq;
                R.S0 = bg->S0[k].as<double>();
                R.r = bg->r[k];
                alt.WW = g->WW.as<double>(); alt.Wy = g->Wy.as<double>(); alt.yy = g->yy;
                alt.gy = d_cy + (size_t)i * ldcy;
                CRM_TRY(launch_nullfit(st, alt, nb));
                CRM_TRY(launch_gather_trial_lml(st, alt.trial, nb, d_alt + (size_t)i * BLK));
                if (eff) CRM_TRY(launch_assoc_effects(st, d_effg + i, 1, nb, c, false));
            }
            hipLaunchKernelGGL(multi_lrt_kernel, dim3((nb + 255) / 256, ngenes), dim3(256), 0, st, d_alt, d_nl, nb, (long)BLK,
                               d_pv);
            CRM_HIP(hipGetLastError());
        }
        if (out_pvalue)
            CRM_HIP(hipMemcpy2DAsync(out_pvalue + done, sizeof(double) * count, d_pv, sizeof(double) * BLK, sizeof(double) * nb,
                                     ngenes, hipMemcpyDeviceToHost, st));
        if (out_alt_lml)
            CRM_HIP(hipMemcpy2DAsync(out_alt_lml + done, sizeof(double) * count, d_alt, sizeof(double) * BLK,
                                     sizeof(double) * nb, ngenes, hipMemcpyDeviceToHost, st));
        if (eff) {
            double* const outs[5] = {eff->beta, eff->se, eff->delta, eff->scale, eff->logp};
            for (int q = 0; q < 5; q++)
                if (outs[q])
                    CRM_HIP(hipMemcpy2DAsync(outs[q] + done, sizeof(double) * count, d_eff + q * eff_rows, sizeof(double) * BLK,
                                             sizeof(double) * nb, ngenes, hipMemcpyDeviceToHost, st));
            if (eff->status)
                CRM_HIP(hipMemcpy2DAsync(eff->status + done, sizeof(int) * count, (const int*)(d_eff + 5 * eff_rows),
                                         sizeof(int) * BLK, sizeof(int) * nb, ngenes, hipMemcpyDeviceToHost, st));
        }
        CRM_HIP(hipStreamSynchronize(st));
        ctx->report(done + nb, count);
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
