// Host orchestration of the interaction scan behind the C-ABI: the scan plan and the per-block kernel pipeline
//   stats -> T(rho) = G' Q0(rho) -> null fits + rho* -> sort by rho* -> Khatri-Rao contraction
//   -> side contractions -> assemble (Q, F) -> eigenvalues + Davies.
// Here: the driver of a pass and the entry points; the plan and the stages are declared in scan_pass.h.
// Reference loop being replaced: cellregmap/_cellregmap.py:340-436.  The objects it works on are built elsewhere:
// background.hip, kinship.hip, gene.hip, panel.hip, donor_tables.hip.
#include <algorithm>

#include "scan_pass.h"

using namespace crm;

namespace crm {

// One pass over variants [first, first + count) for one or several genes that share the background,
// the covariates W and the contexts E0 (several phenotypes against one panel).  What does not depend
// on the phenotype is done once per block: the block copies, T(rho) = G'Q0(rho), the Khatri-Rao
// contraction per (variant, rho) pair that at least one gene selected, and the y-free side
// contractions.  Per gene: g'y, the null fits, E'(g o y), assembly, eigenvalues and Davies.
//
// allow_collapse = false keeps a grouped panel on the dense path; near_out (collapsed passes only) receives the positions
// (relative to `first`) of the variants that are nearly collinear with the covariates -- scan_core repeats those on the
// dense path, where the block is orthogonalised against W in the cell axis (blockops.hip: launch_ortho_block).
static int scan_pass(const std::vector<crm_gene*>& genes, crm_panel* panel, long first, long count,
                     const int* idx_E, const int* idx_G, const std::vector<ScanOut>& outs, bool allow_collapse,
                     std::vector<long>* near_out) {
    crm_gene* g0 = genes[0];
    crm_background* bg = g0->bg;
    crm_ctx* ctx = bg->ctx;
    if (panel->ctx != ctx) {
        set_error("scan: gene and panel live on different contexts");
        return CRM_ERR_ARG;
    }
    if (panel->n != bg->n) {
        set_error("scan: panel has %ld cells, background has %ld", panel->n, bg->n);
        return CRM_ERR_ARG;
    }
    if (panel->grouped && panel->m + 1 > BLOCK_SLACK_MAX) {
        set_error("scan: grouped panel with %ld groups (supported up to %d)", panel->m, BLOCK_SLACK_MAX - 1);
        return CRM_ERR_UNSUPPORTED;
    }
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("scan: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    for (crm_gene* g : genes) {
        // the shared pass computes g'W, the context features and the donor tables once, from the first
        // gene's W and E0: the others must hold the same values, not just the same shapes
        if (g->bg != bg || g->c != g0->c || g->k0 != g0->k0 || g->w_key != g0->w_key || g->e0_key != g0->e0_key) {
            set_error("scan: genes of one call must share the background, W and E0 (contents, not only shapes)");
            return CRM_ERR_ARG;
        }
    }
    if (count == 0) return CRM_OK;
    InScan in_scan;
    CRM_TRY(in_scan.enter(ctx, "scan"));
    // (the Gram kernel stages all k0 + c + 2 rows of a variant in LDS: refused here, before anything is launched, with
    // the limit named; past 144 rows / 128 contexts the scan runs through the slower forms of its per-variant kernels)
    if (g0->k0 + g0->c + 2 > CRM_MAX_GRAM_ROWS) {
        set_error("interaction scan: %d contexts with %d covariate columns (supported: contexts + covariates + 2 <= %d; "
                  "the association scans take up to %d covariate columns)", g0->k0, g0->c, CRM_MAX_GRAM_ROWS,
                  CRM_MAX_COV_XWIDE);
        return CRM_ERR_UNSUPPORTED;
    }
    if (ctx->polish && g0->c > CRM_MAX_COV) {
        set_error("interaction scan: the null-fit polish is only built for up to %d covariate columns", CRM_MAX_COV);
        return CRM_ERR_UNSUPPORTED;
    }
    CRM_HIP(hipSetDevice(ctx->device));
    const long n = bg->n;
    for (long i = 0; i < n; i++) {
        if ((idx_E && (idx_E[i] < 0 || idx_E[i] >= n)) || (idx_G && (idx_G[i] < 0 || idx_G[i] >= n))) {
            set_error("scan: permutation index out of range at position %ld", i);
            return CRM_ERR_ARG;
        }
    }
    if ((int)bg->s0_max.size() != bg->nrho) {   // (filled when the background was sealed / created)
        set_error("scan: the background was not sealed");
        return CRM_ERR_INTERNAL;
    }
    ScanPass S(genes, panel, first, count, idx_E, idx_G, outs, allow_collapse, near_out);
    const ScanPlan& P = S.P;
    CRM_TRY(S.workspaces());
    CRM_TRY(S.prepare_contexts());
    CRM_TRY(S.prepare_kinship());
    CRM_TRY(S.prepare_woodbury());
    // The side stream (scan_side.hip): whatever way the pass ends -- the null-fit probe's early return, an error -- it ends
    // with the side stream idle, so that the buffers its launches read and write can be reused or freed
    S.side_form = S.side_serves() ? std::max(0, std::min(3, form("side_stream", 1))) : 0;
    struct SideIdle { crm_ctx* c; bool on; ~SideIdle() { if (on) (void)hipStreamSynchronize(c->side_stream); } } side_idle{ctx, S.side_form != 0};
    for (long done = 0; done < count; done += P.BLK) {
        Block B;
        B.done = done;
        B.col0 = first + done;
        B.nb = (int)std::min<long>(P.BLK, count - done);
        TraceRange range_block("crm scan block");
        CRM_TRY(S.copy_block(B));
        CRM_TRY(S.block_stats(B));
        if (!P.fastT && !P.collapsed()) CRM_TRY(crm_background_require_q0(bg, -1));
        if (ctx->replay_mode == 2) {
            CRM_TRY(S.replay_block(B));
            if (P.wb()) CRM_TRY(S.woodbury_phi(B));
        } else {
            CRM_TRY(S.rotations(B));   // (unrelated-donor form: with Phi'gx, woodbury_phi)
            CRM_TRY(S.null_fits(B));
            if (ctx->probe_on) return CRM_OK;   // (test hook: the pass ends with this block's records)
        }
        if (P.wb()) ctx->unrelated_donor_blocks++;
        CRM_TRY(S.collect_fits(B));
        for (int b0 = 0; b0 < B.nb;) {
            const SubRange R = S.sub_range(B, b0);
            Pairs Q;
            CRM_TRY(S.select_pairs(B, R, Q));
            CRM_TRY(S.form_A(B, R, Q));
            if (S.side_form != 0) {   // (Z2, Z3 and Z1 come from the side stream: the join before the assembly)
                CRM_TRY(S.side_join(B));
            } else {
                CRM_TRY(S.side_contractions(B, R));
                CRM_TRY(S.z1_products(B, R));
            }
            for (int gi = 0; gi < S.ng; gi++) CRM_TRY(S.gene_results(B, R, gi));
            b0 += R.nb;
        }
        ctx->report(done + B.nb, count);   // (the reference's tqdm, :340)
    }
    return CRM_OK;
}

// The scan of [first, first + count): one pass, plus -- after a collapsed pass -- a dense pass over every run of variants
// the collapsed one marked as nearly collinear with the covariates (their results are overwritten).
static int scan_core(const std::vector<crm_gene*>& genes, crm_panel* panel, long first, long count,
                     const int* idx_E, const int* idx_G, const std::vector<ScanOut>& outs) {
    std::vector<long> near;
    CRM_TRY(scan_pass(genes, panel, first, count, idx_E, idx_G, outs, true, &near));
    crm_ctx* ctx = genes[0]->ctx;
    if (near.empty() || ctx->probe_on) return CRM_OK;
    const int k0 = genes[0]->k0;
    struct Quiet {   // (the repeated variants were reported as done by the first pass)
        crm_ctx* c;
        explicit Quiet(crm_ctx* c_) : c(c_) { c->progress_muted = true; }
        ~Quiet() { c->progress_muted = false; }
    } quiet(ctx);
    ctx->dense_repeats += (long)near.size();
    // runs of marked variants, neighbours closer than 32 variants merged (a dense pass has a fixed cost of a few
    // milliseconds whatever its length); a panel that is marked on more than a quarter of its variants is simply scanned
    // again as a whole
    if ((long)near.size() * 4 > count) {
        near.resize((size_t)count);
        for (long v = 0; v < count; v++) near[(size_t)v] = v;
    }
    for (size_t i = 0; i < near.size();) {
        size_t j = i + 1;
        while (j < near.size() && near[j] <= near[j - 1] + 32) j++;
        const long off = near[i], len = near[j - 1] - near[i] + 1;
        std::vector<ScanOut> shifted;
        for (const ScanOut& o : outs) shifted.push_back(o.advanced(off, k0));   // (every array: scan_pass.h)
        CRM_TRY(scan_pass(genes, panel, first + off, len, idx_E, idx_G, shifted, false, nullptr));
        i = j;
    }
    return CRM_OK;
}

}  // namespace crm

extern "C" {

int crm_scan_interaction(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                         const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2,
                         double* out_g2, double* out_eps2, double* out_Q, double* out_lml,
                         double* out_delta, double* out_scale, double* out_lambda, double* out_F) {
    return crm::guarded_on("crm_scan_interaction", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    std::vector<ScanOut> outs{{out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q, out_lml, out_delta,
                               out_scale, out_lambda, out_F}};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

int crm_scan_interaction_tail(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                              const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2,
                              double* out_g2, double* out_eps2, double* out_Q, double* out_lml,
                              double* out_delta, double* out_scale, double* out_lambda, double* out_F,
                              double* out_logp, int* out_status) {
    return crm::guarded_on("crm_scan_interaction_tail", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q, out_lml, out_delta, out_scale, out_lambda, out_F};
    o.exact = true;
    o.logp = out_logp;
    o.status = out_status;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

int crm_scan_interaction_info(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E,
                              const int* idx_G, double* out_pvalue, int* out_ifault, double* out_liu_pvalue,
                              int* out_model_flags) {
    return crm::guarded_on("crm_scan_interaction_info", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    o.ifault = out_ifault;
    o.liu = out_liu_pvalue;
    o.flags = out_model_flags;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

// B permutations of one scan (include/crm_hip.h): the first permutation's pass records, per block, the fits and the rows
// T(rho*); the others replay them.  The panel is walked in chunks that keep the record within REPLAY_CAP_BYTES.
static int scan_permuted(crm_gene* gene, crm_panel* panel, long first, long count, int nperm, const int* idx_E,
                         const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                         double* out_eps2, double* out_Q, bool exact, double* out_logp, int* out_status) {
    if (!gene || !panel || nperm < 1 || !out_pvalue) return CRM_ERR_ARG;
    if (first < 0 || count < 0 || first + count > panel->p) {
        set_error("scan: variants [%ld, %ld) outside the panel (p = %ld)", first, first + count, panel->p);
        return CRM_ERR_ARG;
    }
    crm_ctx* ctx = gene->ctx;
    if (ctx->replay_mode != 0 || ctx->in_scan) {
        set_error("scan: another scan is running on this context");
        return CRM_ERR_UNSUPPORTED;
    }
    const long n = gene->bg->n;
    constexpr double REPLAY_CAP_BYTES = 8.0 * (1ull << 30);
    // (whole blocks of the scan as one call over all `count` variants would cut them: the same launches, the same bits)
    const long blk = scan_block_variants(ctx, gene, count);
    const long chunk_cap = std::max<long>(blk, (long)(REPLAY_CAP_BYTES / (sizeof(double) * (double)gene->bg->ldq)) / blk * blk);
    struct Clear { crm_ctx* c; ~Clear() { c->replay_clear(); } } clear{ctx};
    std::vector<crm_gene*> genes{gene};
    for (long at = 0; at < count; at += chunk_cap) {
        const long len = std::min(chunk_cap, count - at);
        ctx->replay_clear();
        for (int q = 0; q < nperm; q++) {
            ctx->replay_mode = q == 0 ? 1 : 2;
            ctx->replay_cursor = 0;
            // (rho*, the variance components and the fit do not depend on the permutation: written by the first pass)
            ScanOut o{out_pvalue + (size_t)q * count + at, nullptr, nullptr, nullptr, nullptr,
                      out_Q ? out_Q + (size_t)q * count + at : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (q == 0) {
                o.rho1 = out_rho1 ? out_rho1 + at : nullptr; o.e2 = out_e2 ? out_e2 + at : nullptr;
                o.g2 = out_g2 ? out_g2 + at : nullptr; o.eps2 = out_eps2 ? out_eps2 + at : nullptr;
            }
            o.exact = exact;
            o.logp = out_logp ? out_logp + (size_t)q * count + at : nullptr;
            o.status = out_status ? out_status + (size_t)q * count + at : nullptr;
            std::vector<ScanOut> outs{o};
            const int rc = scan_core(genes, panel, first + at, len, idx_E ? idx_E + (size_t)q * n : nullptr,
                                     idx_G ? idx_G + (size_t)q * n : nullptr, outs);
            if (rc != CRM_OK) return rc;
        }
    }
    return CRM_OK;
}

int crm_scan_interaction_permuted(crm_gene* gene, crm_panel* panel, long first, long count, int nperm, const int* idx_E,
                                  const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                                  double* out_eps2, double* out_Q) {
    return crm::guarded_on("crm_scan_interaction_permuted", gene ? gene->ctx : nullptr, [&]() -> int {
    return scan_permuted(gene, panel, first, count, nperm, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2,
                         out_Q, false, nullptr, nullptr);
    });
}

int crm_scan_interaction_permuted_tail(crm_gene* gene, crm_panel* panel, long first, long count, int nperm,
                                       const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                                       double* out_e2, double* out_g2, double* out_eps2, double* out_Q,
                                       double* out_logp, int* out_status) {
    return crm::guarded_on("crm_scan_interaction_permuted_tail", gene ? gene->ctx : nullptr, [&]() -> int {
    return scan_permuted(gene, panel, first, count, nperm, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2,
                         out_Q, true, out_logp, out_status);
    });
}

int crm_scan_interaction_bounds(crm_gene* gene, crm_panel* panel, long first, long count, const int* idx_E, const int* idx_G,
                                double* out_pvalue, int* out_ifault, double* out_liu_pvalue, int* out_model_flags,
                                double* out_bound_Q, double* out_bound_p) {
    return crm::guarded_on("crm_scan_interaction_bounds", gene ? gene->ctx : nullptr, [&]() -> int {
    if (!gene || !panel || !out_model_flags) return CRM_ERR_ARG;
    std::vector<crm_gene*> genes{gene};
    ScanOut o{out_pvalue, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    o.ifault = out_ifault;
    o.liu = out_liu_pvalue;
    o.flags = out_model_flags;
    o.bound_Q = out_bound_Q;
    o.bound_p = out_bound_p;
    std::vector<ScanOut> outs{o};
    return scan_core(genes, panel, first, count, idx_E, idx_G, outs);
    });
}

static int scan_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count, const int* idx_E,
                      const int* idx_G, double* out_pvalue, double* out_rho1, double* out_e2, double* out_g2,
                      double* out_eps2, double* out_Q, bool exact, double* out_logp, int* out_status) {
    if (!genes || ngenes < 1 || !panel) return CRM_ERR_ARG;
    std::vector<crm_gene*> gs(genes, genes + ngenes);
    for (crm_gene* g : gs)
        if (!g) return CRM_ERR_ARG;
    std::vector<ScanOut> outs(ngenes);
    for (int i = 0; i < ngenes; i++) {
        auto at = [&](double* base) { return base ? base + (size_t)i * count : nullptr; };
        outs[i] = ScanOut{at(out_pvalue), at(out_rho1), at(out_e2), at(out_g2), at(out_eps2), at(out_Q),
                          nullptr, nullptr, nullptr, nullptr, nullptr};
        outs[i].exact = exact;
        outs[i].logp = at(out_logp);
        outs[i].status = out_status ? out_status + (size_t)i * count : nullptr;
    }
    return scan_core(gs, panel, first, count, idx_E, idx_G, outs);
}

int crm_scan_interaction_multi(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                               const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                               double* out_e2, double* out_g2, double* out_eps2, double* out_Q) {
    return crm::guarded_on("crm_scan_interaction_multi", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr, [&]() -> int {
    return scan_multi(genes, ngenes, panel, first, count, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q,
                      false, nullptr, nullptr);
    });
}

int crm_scan_interaction_multi_tail(crm_gene* const* genes, int ngenes, crm_panel* panel, long first, long count,
                                    const int* idx_E, const int* idx_G, double* out_pvalue, double* out_rho1,
                                    double* out_e2, double* out_g2, double* out_eps2, double* out_Q, double* out_logp,
                                    int* out_status) {
    return crm::guarded_on("crm_scan_interaction_multi_tail", (genes && ngenes > 0 && genes[0]) ? genes[0]->ctx : nullptr,
                           [&]() -> int {
    return scan_multi(genes, ngenes, panel, first, count, idx_E, idx_G, out_pvalue, out_rho1, out_e2, out_g2, out_eps2, out_Q,
                      true, out_logp, out_status);
    });
}

}  // extern "C"
