// What the association LRTs (assoc_host.hip, assoc_multi.hip) and the fixed-effect GxC context tests (context_host.hip,
// context_multi.hip) have in common on the host: the checks of a call, the workspace carver, the gene-level null fit on a
// zero "variant", the rows of fitted nulls and their rho groups, the phenotype matrix [W | y_1 .. y_P], and the
// preparation of a block of variants.  Each scan keeps its own sequence of launches; these are the steps that are the same
// statement in all of them (lrt_scan.hip).
#pragma once
#include <algorithm>
#include <cstdio>
#include <vector>

#include "nullfit.h"
#include "objects.h"

namespace crm {

// ---- checks -----------------------------------------------------------------------------------------------------------
// The gene(s) and the panel live on one context and hold the same cells; [first, first + count) lies inside the panel.
int check_panel_range(const char* what, const crm_background* bg, const crm_panel* panel, long first, long count);
// Non-null genes of one background and context with the same covariates (c, w_key); contexts_too: the same contexts as
// well (k0, e0_key).  The shared passes take g'W, the orthogonalisation and the context tables from the first gene.
int check_shared_genes(const char* what, crm_gene* const* genes, int ngenes, bool contexts_too);

// ---- workspaces -------------------------------------------------------------------------------------------------------
// Variants per block of the association and context scans, and the leading dimension of every [.. x variants] buffer
// (column tiles of 128 over the variants stay inside a row).
inline int lrt_block_variants(const crm_ctx* ctx, long count) {
    return (int)std::min<long>(ctx->block_variants > 0 ? ctx->block_variants : CRM_DEFAULT_BLOCK,
                               round_up(std::max<long>(count, 1), 128));
}

// One buffer cut into arrays that each start on a 256-byte boundary.  `list(take)` names them, take(pointer, bytes) in
// turn; it runs twice: to add up the offsets, and, once the buffer has that size (*total), to set the pointers.
template <class List>
int carve_workspace(DevBuf& buf, List&& list, size_t* total = nullptr) {
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](auto*& ptr, size_t bytes) {
        ptr = base ? reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + off) : nullptr;
        off += (bytes + 255) / 256 * 256;
    };
    list(take);
    CRM_TRY(buf.ensure(off));
    if (total) *total = off;
    base = buf.as<char>();
    off = 0;
    list(take);
    return CRM_OK;
}

// ---- the gene-level null: ML fit with X = W over the rho grid (_cellregmap.py:250-266) ------------------------------------
// A zero "variant" (T = a row of zeros with ldT = 0, g'g = g'y = g'W = 0) makes [W, g] rank deficient, so the fit kernel
// drops g: exactly LMM(y, W).
struct ZeroVariant {
    double *zero = nullptr, *gg = nullptr, *gy = nullptr, *gW = nullptr;   // [ldq], [1], [1], [ld_gW]
    long ld_gW = 0;
    NullFitTrial* trial = nullptr;
};
// fa = the gene's null-fit arguments on the zero variant, fit into *d_fit; launches it
int launch_gene_null(hipStream_t st, crm_gene* gene, const ZeroVariant& z, NullFitOut* d_fit, double* xwide, NullFitArgs& fa);
// the fit's grid index checked (gene >= 0: named in the refusal) and its row (rho, v0 rho, v0 (1 - rho), v1, lml, delta)
// written (row may be null)
int gene_null_row(const char* what, const crm_background* bg, int gene, const NullFitOut& fit, double* row);
// The single-gene scans: the four clears, the fit, its copy and the wait, the row.  xwide: the call's own scratch of the
// 63..128-column kernel for `variants` variants (the alt fits use it too).
int fit_gene_null(const char* what, crm_gene* gene, const ZeroVariant& z, NullFitOut* d_fit, int variants, DevBuf& xwide,
                  NullFitArgs& fa, NullFitOut& null, double* out_row);

// ---- rows of fitted nulls (crm_association_null_multi's output, six doubles per gene) -----------------------------------
struct NullRows {
    std::vector<int> ri;           // grid index of every gene's rho*
    std::vector<int> grp_of_rho;   // [nrho] rho group of a grid index, -1: no gene of the call sits there
    std::vector<int> grp_rho;      // the groups' grid indices, in grid order
    std::vector<std::vector<int>> members;   // the genes of every group, in the order given
    int ngrp() const { return (int)grp_rho.size(); }
    // rho1 a grid point, a finite lml, fast: delta in (0, 1]
    int read(const char* what, const crm_background* bg, const double* null, int ngenes, bool fast);
    // the rho groups, and Q0 of every group formed
    int group(crm_background* bg);
};

// ---- the phenotype matrix [W | y_1 .. y_P] (cells_pad x ldxy): W at columns 0 .. c - 1, the phenotypes from column yoff ---
struct ColumnSource {   // XY[i, dst] = src[i * ld]
    const double* src;
    long ld, dst;
};
struct PhenotypeMatrix {
    long yoff = 0, ncol = 0, ldxy = 0;
    double* XY = nullptr;   // ctx->ws_XG
    std::vector<ColumnSource> srcs;
    ColumnSource* d_srcs = nullptr;   // carved by the caller: srcs_bytes()
    void plan(crm_gene* const* genes, int ngenes);
    size_t srcs_bytes() const { return sizeof(ColumnSource) * srcs.size(); }
    int ensure(crm_ctx* ctx, long cells_pad);
    int clear(hipStream_t st, long cells_pad);   // (the sources are zero padded; so are the columns between)
    int fill(hipStream_t st, long cells_pad);
};

// ---- a block of variants ----------------------------------------------------------------------------------------------
// Columns [first + done, + nb) of the panel in ws_Gb with their plain products g'g, g'y, g'W against the first gene; full
// refit: also in the basis of economic_svd([W, g]) (glimix-core LMM) -- the block orthogonalised against W in the cell axis,
// as in the interaction scan -- in ws_Gx, with the products of that and the reference's rank rule.  The fast path's lstsq
// keeps the raw columns: Gx = Gb.
struct LrtBlock {
    crm_gene* g0; crm_panel* panel;
    crm_background* bg; crm_ctx* ctx; hipStream_t st;
    long first, count;
    bool fast;
    long n, np, ldq;
    int nrho, c, BLK;
    long ldb, ld_gW;
    double *d_gg = nullptr, *d_gy = nullptr, *d_gW = nullptr, *d_part = nullptr;
    double *d_coef = nullptr, *d_thr = nullptr;   // full refit
    int* d_drop = nullptr;                        // full refit
    double *Gb = nullptr, *Gx = nullptr;          // of the block last prepared

    LrtBlock(crm_gene* g0_, crm_panel* panel_, long first_, long count_, int fast_)
        : g0(g0_), panel(panel_), bg(g0_->bg), ctx(bg->ctx), st(ctx->stream), first(first_), count(count_), fast(fast_ != 0),
          n(bg->n), np(bg->n_pad), ldq(bg->ldq), nrho(bg->nrho), c(g0_->c), BLK(lrt_block_variants(ctx, count_)),
          ldb(BLK + 128), ld_gW(round_up(g0_->c, 8)) {}
    int nb_at(long done) const { return (int)std::min<long>(BLK, count - done); }
    int ensure();   // ws_Gb; full refit: ws_Gx
    // the tables, in a carve_workspace list; refit: those of the full refit too
    template <class Take>
    void carve(Take& take, bool refit) {
        take(d_gg, sizeof(double) * BLK), take(d_gy, sizeof(double) * BLK), take(d_gW, sizeof(double) * BLK * ld_gW);
        take(d_part, variant_stats_workspace(BLK, std::min(c, CRM_MAX_COV)));
        take(d_coef, refit ? sizeof(double) * (size_t)c * ldb : 0), take(d_thr, refit ? sizeof(double) * BLK : 0);
        take(d_drop, refit ? sizeof(int) * BLK : 0);
    }
    // plain_cols: covariate columns of the raw block's products (c; 1 where g'W comes from a product of the caller's)
    int prepare(long done, int nb, int plain_cols);
    // T_g = Q0(rho_k)'gx of the block last prepared: [nb x ldc] at C
    GemmProblem rotation(int k, int nb, double* C, long ldc) const;
};

// ---- the context tests' tables (context_host.hip, context_multi.hip; DESIGN.md sections 12 to 14) ------------------------
// The contexts as operands -- C (rows padded to whole 128-column tiles: the Khatri-Rao operand), C^2 and, for the joint
// test, the pair products C_i o C_j, i >= j -- and a block's plain products against them:
//   x_j'x_j = (g o g)'C_j^2,   x_j'g = (g o gx)'C_j (gx: the column that stands for g),   x_i'x_j = (g o g)'(C_i o C_j)
// T_x, the rotated candidates, is the large buffer (variants x k x ldq doubles), so a block is cut into sub-ranges of SUB
// variants that keep it within a byte budget.
constexpr size_t CONTEXT_BUDGET = (size_t)8 << 30;
constexpr int CONTEXT_SLOTS = 8;   // of ws_probs: 0 T_g, 1 / 2 the squared block's products, 3 / 4 the two Khatri-Rao contractions, 5 x_i'x_j
struct ContextTables {
    int k, npair;
    bool joint, v_global;   // v_global: the joint test's V in global memory, not LDS
    long ld_k, ld_cq, ld_pp, v_slab;
    int SUB;
    size_t tests;           // (variant, context) pairs of a sub-range
    double *Cq = nullptr, *C2 = nullptr, *CC = nullptr;
    double *d_xx = nullptr, *d_xg = nullptr, *d_xxp = nullptr;   // carved by the caller: [BLK x ld_k] twice, [BLK x ld_pp]

    // the supported shapes; then the sizes
    static int check(const char* what, int c, int k, bool joint);
    ContextTables(const LrtBlock& B, int k_, bool joint_);
    int ensure(const LrtBlock& B);     // ws_G2, full refit: ws_GG, ws_A, ws_ctxE
    int operands(const LrtBlock& B);   // Cq, C2, CC from the first gene's contexts
    // G2 = g o g (full refit: also GG = g o gx) of the block last prepared, and the three products as problems 1, 2, 5 of pr
    int block_products(const LrtBlock& B, int nb, GemmProblem* pr) const;
    // the Khatri-Rao problem of variants [b0, b0 + ns) of the block against Y: [ns k x N] at C
    GemmProblem khatri_rao(const LrtBlock& B, int b0, int ns, const double* Y, long ldy, int N, double* C, long ldc) const;
    // the contraction T_x = Q0(rho*)'(g o C_j), the launch the kernel timer brackets; r: the spectrum's length
    int launch_rotated(const LrtBlock& B, const GemmProblem* d_p, const GemmProblem& p, int r, int ns) const;
};

}  // namespace crm
