// The side stream of a scan pass (scan_pass.h: ScanPass): the products of a block that depend on the
// block alone -- Z2, Z3 and Z1, and the per-donor pair products P_d = G_d'(E (x) E)_d -- taken out of the pair stage,
// where they ran behind the host's round trip for the fits, and placed where the chip has room for them.  The same
// launches on the same inputs: only the order of launches that do not depend on each other changes.
//
// Z2, Z3 and Z1 go to the context's second, lowest-priority stream, forked behind the batched rotation launch: they run
// beside the spectrum tails (a few workgroups, bound by load latency) and the null fits (vector ALU, 120 KB of LDS per CU)
// and are done before the Gram starts.  The pair products stay on the main stream, enqueued in collect_fits between the
// copy of the fits and the host's wait for it: they run while the host reads the fits and enqueues the pair stage, and the
// Gram follows them in stream order.  (On the side stream too they ran beside the null fits, but what was left of the
// side work then shared the CUs with the Gram, one workgroup of each per CU instead of two of the Gram: DESIGN.md
// section 6 has the placements that were measured.)
//
// Fork: ev_fork on the main stream behind the rotation launch; everything the side work reads (the block, G2, GG) was
// written by block_stats before it, and its records were uploaded ahead of the rotations.  Join: the main stream waits on
// ev_side before the assembly (scan.hip), so a block ends -- gene_results synchronises the main stream -- with its side
// work done, and the next block's block_stats may rewrite what it read.  Between fork and join the side stream alone
// writes ws_Z (Z1, Z2, Z3 and their split slabs) and, in a block that kept the copy, ws_G2 and ws_GG; the main stream
// writes ws_T, ws_Tcut, ws_WB, ws_small, ws_Gk, ws_Pd, ws_AH, ws_S and ws_A there, none of which the side work touches.
#include "scan_pass.h"

namespace crm {

// One phenotype on the unrelated-donor form in block order (a block is then one sub-range, known before its fits), no
// permutation replay, and no launch in the pass that could take the persistent Khatri-Rao form, whose generation wait
// counts on having the chip to itself: without the pair products the folded form forms its per-donor sums and, without
// pair features, its E1 rows by Khatri-Rao launches (pair_stage) -- asked here at their largest
bool ScanPass::side_serves() const {
    if (!P.wb() || ng != 1 || !P.wb_block || ctx->replay_mode != 0) return false;
    if (probed.donor_pairs) return true;
    const long row_tiles = ((long)P.BLK * k0 + GEMM_BM - 1) / GEMM_BM;
    if (bg->kin_k2 != 1 && kr_launch_persistent(ctx, row_tiles * ((bg->kin_k2 + 127) / 128) * bg->kin_groups, np, 128)) return false;
    if (!P.e1_pairs && kr_launch_persistent(ctx, row_tiles * ((bg->kin_k1 + 127) / 128) * P.fold_split6, np, 128)) return false;
    return true;
}

// The block's records of these launches -- [donors] pair products, Z2, Z3, Z1 -- uploaded on the main stream ahead of the
// rotations: the host is not to wait on the side stream's queue, and the fork orders the upload before every launch that
// reads it.  side_recs lives as long as the pass and is written again only after gene_results has synchronised the main
// stream.
int ScanPass::side_prepare(const Block& B) {
    if (side_form == 0) return CRM_OK;
    const long groups = bg->kin_groups;
    const SubRange R = sub_range(B, 0);
    side_recs.assign((size_t)P.side_probs, GemmProblem{});
    if (early_pairs()) {
        DonorCols D;
        CRM_TRY(donor_columns(B, R, Pairs{}, D, nullptr));
        GemmProblem p{};
        p.X = D.Gk; p.ldx = D.ldk; p.Y = g0->kinEE.as<double>(); p.ldy = g0->ld_ee; p.C = ctx->ws_Pd.as<double>(); p.ldc = P.ldPd;
        p.M = D.ncol; p.N = P.npair;
        side_maxlen = donor_run_records(bg, p, P.pd_slab, side_recs.data());
    }
    side_records(R, side_recs.data() + groups);
    z1_records(B, R, side_recs.data() + groups + 2);
    return upload(P.side_slot(), side_recs.data(), side_recs.size());
}

// the fork, behind the batched rotation launch (rotations); form 3 (side last) leaves the launches to the join
int ScanPass::side_fork(const Block& B) {
    if (side_form == 0) return CRM_OK;
    side_enqueued = false;
    CRM_HIP(hipEventRecord(ctx->ev_fork, st));
    CRM_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    ctx->side_stream_blocks++;
    if (side_form != 3) CRM_TRY(side_enqueue(B));
    if (side_form == 2) CRM_TRY(side_join(B));   // (side first: the main stream goes on once all of it is done)
    return CRM_OK;
}

int ScanPass::side_enqueue(const Block& B) {
    hipStream_t ss = ctx->side_stream;
    const SubRange R = sub_range(B, 0);
    const GemmProblem* d_z = d_probs + P.side_slot() + bg->kin_groups;
    CRM_TRY(side_launches(B, R, ss, d_z));
    CRM_TRY(z1_launches(R, ss, d_z + 2));
    CRM_HIP(hipEventRecord(ctx->ev_side, ss));
    side_enqueued = true;
    return CRM_OK;
}

// The join, before the assembly.  Form 3 enqueues the side work only here, behind an event the main stream records now: it
// then starts when the main stream has nothing left to do but wait for it.
int ScanPass::side_join(const Block& B) {
    if (side_form == 0) return CRM_OK;
    if (!side_enqueued) {
        CRM_HIP(hipEventRecord(ctx->ev_main, st));
        CRM_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_main, 0));
        CRM_TRY(side_enqueue(B));
    }
    CRM_HIP(hipStreamWaitEvent(st, ctx->ev_side, 0));
    return CRM_OK;
}

// The pair products on the main stream, from the block's side records (collect_fits: behind the copy of the fits, ahead
// of the host's wait for it); a block that kept the copy gathers its test direction in donor order first
int ScanPass::launch_early_pairs(const Block& B) {
    DonorCols D;
    CRM_TRY(donor_columns(B, sub_range(B, 0), Pairs{}, D, st));
    return launch_gemm_tn(ctx, d_probs + P.side_slot(), (int)bg->kin_groups, D.ncol, P.npair, side_maxlen, false, 0, 1, 0);
}

}  // namespace crm
