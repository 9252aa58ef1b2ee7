// The pair stage of a scan (scan_pass.h: ScanPass): steps 5-9 over a sub-range of a block -- the (variant, rho*) pairs, A~, the side
// contractions and Z1.
#include "scan_pass.h"

namespace crm {

// The pair stage runs over sub-ranges of the block: one unless several phenotypes ask for more (variant, rho*) pairs
// than the pair-ordered buffers hold
SubRange ScanPass::sub_range(const Block& B, int b0) const {
    SubRange R;
    R.b0 = b0;
    R.nb = B.nb - b0;
    R.done = B.done + b0;
    if (ng > 1) {
        long pairs = 0;
        int take = 0;
        for (; b0 + take < B.nb; take++) {
            unsigned seen = 0;
            for (int gi = 0; gi < ng; gi++) {
                const NullFitOut& f = h_fit[(size_t)gi * P.BLK + b0 + take];
                if (!no_kinship_term(f)) seen |= 1u << f.rho_index;
            }
            const int here = __builtin_popcount(seen);
            if (take > 0 && pairs + here > P.pair_cap) break;
            pairs += here;
        }
        R.nb = take;
    }
    return R;
}

// 5. the (rho, variant) pairs some gene selected, ordered by rho; the sub-range's columns of the block in that order (Gs)
int ScanPass::select_pairs(const Block& B, const SubRange& R, Pairs& Q) {
    const int nb = R.nb, BLK = P.BLK;
    const NullFitOut* fit = h_fit.data() + R.b0;
    std::fill(pair_of.begin(), pair_of.end(), -1);
    long with_pair = 0;
    for (int gi = 0; gi < ng; gi++)
        for (int b = 0; b < nb; b++) {
            const NullFitOut& f = fit[(size_t)gi * BLK + b];
            if (no_kinship_term(f)) continue;
            pair_of[(size_t)f.rho_index * BLK + b] = 0;
            with_pair++;
        }
    ctx->tests_without_pair += (long)ng * nb - with_pair;
    // (a sub-range without any pair keeps its first test's: the launches below always have something to do)
    if (with_pair == 0) pair_of[(size_t)fit[0].rho_index * BLK] = 0;
    for (int i = 0; i < nrho; i++) {
        Q.start[i] = Q.npairs;
        for (int b = 0; b < nb; b++) {
            if (pair_of[(size_t)i * BLK + b] == 0) {
                pair_of[(size_t)i * BLK + b] = Q.npairs;
                h_ord[Q.npairs++] = b;
            }
        }
        Q.cnt[i] = Q.npairs - Q.start[i];
    }
    Q.start[nrho] = Q.npairs;
    for (int gi = 0; gi < ng; gi++)
        for (int b = 0; b < nb; b++) {
            const NullFitOut& f = fit[(size_t)gi * BLK + b];
            h_pos[(size_t)gi * BLK + b] = no_kinship_term(f) ? -1 : pair_of[(size_t)f.rho_index * BLK + b];
        }
    if (P.wb_block && ng == 1) {
        // (the position of a test is its variant's place in the block; the sorted copy Gs is not formed: donor_columns)
        for (int b = 0; b < nb; b++)
            if (h_pos[b] >= 0) h_pos[b] = b;
        CRM_HIP(hipMemcpyAsync(d_pos, h_pos.data(), sizeof(int) * (size_t)BLK, hipMemcpyHostToDevice, st));
        return CRM_OK;
    }
    CRM_HIP(hipMemcpyAsync(d_pos, h_pos.data(), sizeof(int) * (size_t)BLK * ng, hipMemcpyHostToDevice, st));
    if (P.wb() && ng > 1) {   // (S in block order: a variant's rows of the rotated S sit at its own position)
        std::vector<int> h_posw((size_t)BLK * ng, -1);
        for (int gi = 0; gi < ng; gi++)
            for (int b = 0; b < nb; b++)
                if (h_pos[(size_t)gi * BLK + b] >= 0) h_posw[(size_t)gi * BLK + b] = b;
        CRM_HIP(hipMemcpyAsync(d_posw, h_posw.data(), sizeof(int) * h_posw.size(), hipMemcpyHostToDevice, st));
        CRM_HIP(hipStreamSynchronize(st));   // (h_posw lives on this scope)
    }
    CRM_HIP(hipMemcpyAsync(d_ord, h_ord.data(), sizeof(int) * Q.npairs, hipMemcpyHostToDevice, st));
    return launch_gather_block(st, B.Gt + R.b0, B.ldt, P.xrows, P.xrows, nullptr, d_ord, Q.npairs, ctx->ws_Gs.as<double>(),
                               P.ldp, (int)P.ldp);
}

// Splits of the direct route's A~ launch along the cell axis (few rounds: see kr_split_for), and its spectrum tails.
// A spectrum a little longer than a multiple of the 128-column tile (config 3: r = 5000 = 39 tiles + 8 columns)
// would pay a whole last column of tiles -- 1 / 40 of the launch -- for those few columns: the last 128 + rem
// columns (rem <= 32) go into a second launch of 160-column tiles instead, cut along the cell axis to fill its
// rounds (38 x 128 + 160 = 5024 columns computed instead of 5120).
int ScanPass::direct_splits(const Pairs& Q, AGroups& A, bool* tail_of) {
    A.a_slab = (size_t)P.pair_cap * k0 * P.ldA;
    long row_tiles = 0;
    int mn = 1;
    for (int i = 0; i < nrho; i++)
        if (Q.cnt[i] > 0) { row_tiles += ((long)Q.cnt[i] * k0 + GEMM_BM - 1) / GEMM_BM; mn = std::max(mn, bg->r[i]); }
    const int cap = (int)std::min<size_t>(8, ((size_t)16 << 30) / std::max<size_t>(sizeof(double) * A.a_slab, 1));
    A.kr_split = kr_split_for(ctx, row_tiles, mn, 1, np, std::max(cap, 1));
    if (A.kr_split > 1) CRM_TRY(ctx->ws_A.ensure(sizeof(double) * A.a_slab * A.kr_split));
    if (A.kr_split > 1 || !ctx->tune.glds || ctx->tune.bn == 64 || ctx->tune.bn == 160 || form("kr_no_tail", 0)) return CRM_OK;
    long tail_row_tiles = 0, main_tiles = 0;
    for (int i = 0; i < nrho; i++) {
        if (Q.cnt[i] == 0) continue;
        const int N = bg->r[i], rem = N % 128;
        const long rt = ((long)Q.cnt[i] * k0 + GEMM_BM - 1) / GEMM_BM;
        main_tiles += rt * ((N + 127) / 128);
        if (N >= 1024 && rem > 0 && rem <= 32) {
            tail_of[i] = true;
            tail_row_tiles += rt;
            A.tail_maxn = std::max(A.tail_maxn, 128 + rem);
        }
    }
    if (tail_row_tiles == 0 || main_tiles <= 1024) {
        std::fill(tail_of, tail_of + CRM_MAX_RHO, false);
    } else {
        const int saved_bn = ctx->tune.bn;
        ctx->tune.bn = 160;
        A.tail_split = kr_split_for(ctx, tail_row_tiles, A.tail_maxn, 1, np, std::max(cap, 1));
        ctx->tune.bn = saved_bn;
        // (before the problem records take addresses inside ws_A: growing the buffer does not keep its contents)
        if (A.tail_split > 1) CRM_TRY(ctx->ws_A.ensure(sizeof(double) * A.a_slab * A.tail_split));
    }
    return CRM_OK;
}

// the problems of step 6, one per non-empty rho group of pairs, into probs[0, nz) (none on the unrelated-donor route)
void ScanPass::a_records(const Pairs& Q, bool via_H, const bool* tail_of, AGroups& A) {
    const double kin_rows = P.folded() ? bg->kin_k1 + bg->kin_groups * (long)bg->kin_k2 : bg->cols;   // (rows of the Mix products)
    for (int i = 0; i < nrho; i++) {
        if (Q.cnt[i] == 0 || P.wb()) continue;   // (unrelated-donor form: no A~ at all)
        GemmProblem p{};
        p.X = ctx->ws_Gs.as<double>() + Q.start[i]; p.ldx = P.ldp;
        p.C = ctx->ws_A.as<double>() + (size_t)Q.start[i] * k0 * P.ldA;
        if (P.collapsed()) {
            // A~(b) = sum_d gamma_d,b * Bd(rho)[d]: rows of Bd are (k0 x ldq) slabs per donor
            p.Y = tab->Bd.as<double>() + (size_t)i * P.mp * k0 * ldq; p.ldy = (long)k0 * ldq; p.ldc = (long)k0 * P.ldA;
            p.M = Q.cnt[i]; p.N = (int)((long)k0 * ldq);
        } else if (via_H) {
            if (P.kin() && ng == 1) {   // (AH / S is in pair order already, see folded_S / unfolded_AH)
                p.X = (P.folded() ? ctx->ws_S.as<double>() : ctx->ws_AH.as<double>()) + (size_t)Q.start[i] * k0; p.ldx = P.ld_ah;
            } else {
                p.X = ctx->ws_XG.as<double>() + (size_t)Q.start[i] * k0; p.ldx = P.ld_xg;
            }
            p.Y = P.folded() ? bg->MixK[i].as<double>() : bg->Mix[i].as<double>(); p.ldy = ldq; p.ldc = P.ldA;
            p.M = Q.cnt[i] * k0; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            A.kr_flops += 2.0 * kin_rows * (double)bg->r[i] * (double)k0 * (double)Q.cnt[i];
        } else {
            p.E = d_Ep; p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->Q0[i].as<double>(); p.ldy = ldq; p.ldc = P.ldA;
            p.M = Q.cnt[i] * k0; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            A.kr_flops += 2.0 * (double)n * (double)bg->r[i] * (double)k0 * (double)Q.cnt[i];
            if (tail_of[i]) {
                GemmProblem t = p;
                const int rem = 128 + p.N % 128;
                p.N -= rem;
                t.Y = p.Y + p.N; t.C = p.C + p.N; t.N = rem;
                A.tails.push_back(t);
            }
        }
        // The mixing-matrix products of the kinship-structure route: a spectrum a little longer than a multiple of the
        // 128-column tile (config 3: r = 5000 = 39 tiles + 8 columns) would pay a whole last column of tiles -- 1 / 40 of
        // the launch -- for those few columns; they go through one pass over the operand instead (launch_skinny_tn).
        if (P.kin() && p.N >= 1024 && p.N % 128 > 0 && p.N % 128 <= 16 && p.ldx % 2 == 0 &&
            (reinterpret_cast<uintptr_t>(p.X) & 15) == 0 && !form("kr_no_tail", 0)) {
            GemmProblem t = p;
            const int rem = p.N % 128;
            A.kr_flops -= 2.0 * kin_rows * (double)rem * (double)k0 * (double)Q.cnt[i];   // (the timed launch is the tiled one alone)
            p.N -= rem;
            t.Y = p.Y + p.N; t.C = p.C + p.N; t.N = rem;
            A.spectrum_tails.push_back(t);
        }
        A.max_m = std::max(A.max_m, p.M);
        A.max_n = std::max(A.max_n, p.N);
        probs[A.nz++] = p;
    }
}

// The kinship routes' operand columns in donor order (Gk): one phenotype takes them in the rho*-sorted pair order (Gs)
// straight away, so that the result is the operand of the Mix products as it stands; several phenotypes share a
// variant between pairs: block order, then the pair gather.  The unrelated-donor form has no Mix product: block order
// `on`: the stream of the gather; null: the columns' places alone (the gather is launched elsewhere, or was)
int ScanPass::donor_columns(const Block& B, const SubRange& R, const Pairs& Q, DonorCols& D, hipStream_t on) {
    D.in_pair_order = ng == 1 && !P.wb_block;
    D.G = D.in_pair_order ? ctx->ws_Gs.as<double>() : B.Gt + R.b0;
    D.ldg = D.in_pair_order ? P.ldp : B.ldt;
    D.Gk = ctx->ws_Gk.as<double>();
    D.ldk = D.in_pair_order ? P.ldp : P.ldb;
    D.ncol = D.in_pair_order ? Q.npairs : R.nb;
    if (B.fused && !D.in_pair_order) {   // (block_stats' fused pass has written it; a fused block has one sub-range: fused_pass)
        D.Gk = ctx->ws_Gkt.as<double>();
        return CRM_OK;
    }
    if (!on) return CRM_OK;
    const int blk_cols = (int)(P.ldb - R.b0);   // (columns of the block buffers from the sub-range's first one on)
    return launch_gather_rows(on, D.G, D.ldg, bg->kin_map.as<int>(), bg->kin_rows, D.in_pair_order ? (int)D.ldg : blk_cols,
                              ctx->ws_Gk.as<double>(), D.ldk);
}
int ScanPass::gather_pairs(const double* src, long rows, const Pairs& Q) {   // (several phenotypes: the operand in pair order, XG)
    const int xg_cols = (int)std::min<long>(P.ld_xg, round_up((long)Q.npairs * k0, 128) + 128);
    return launch_gather_slabs(st, src, P.ld_ah, rows, d_ord, Q.npairs, k0, ctx->ws_XG.as<double>(), P.ld_xg, xg_cols);
}

// Folded form (objects.h: kin_fold): S = [E1 rows ; (donor, us_j) rows] of "H'(g o E0) before the contraction over
// the donors", which MixK carries.  (a) the block in donor order; (b) per donor d' the Khatri-Rao contraction over
// its own cells against us (transposed store into rows k1 + d' k2 + j); (c) the E1 rows by one Khatri-Rao
// contraction over ALL cells against the E1 columns of the half factor, cut into slices along the cell axis so
// that its few output tiles fill the chip, summed, and copied into rows [0, k1).
int ScanPass::folded_S(const Block& B, const SubRange& R, const Pairs& Q) {
    DonorCols D;
    CRM_TRY(donor_columns(B, R, Q, D, early_pairs() ? nullptr : st));   // (launch_early_pairs has gathered them)
    double* S = ctx->ws_S.as<double>();
    const int k1 = bg->kin_k1, k2 = bg->kin_k2, ncol = D.ncol, npair = P.npair;
    const long groups = bg->kin_groups, ld_ah = P.ld_ah;
    // (the pair products were launched from the block's side records, in collect_fits: this stage uploads no records, so
    // the host does not wait here)
    if (early_pairs()) return pair_stage(B, R, Q, D, nullptr, 0, GEMM_BK, 0);
    std::vector<GemmProblem> kp((size_t)groups + P.fold_split6);
    GemmProblem p{};
    p.X = D.Gk; p.ldx = D.ldk;
    if (probed.donor_pairs) {   // per donor G_d' (E (x) E)_d, then the rows of S and the E1 rows from it
        p.Y = g0->kinEE.as<double>(); p.ldy = g0->ld_ee; p.C = ctx->ws_Pd.as<double>(); p.ldc = P.ldPd;
        p.M = ncol; p.N = npair;
    } else if (k2 == 1) {  // plain product G_d'' (us o E0)_d': C[b, i] = row k1 + d' of S at column b k0 + i
        p.Y = g0->kinUE.as<double>(); p.ldy = g0->ld_ep; p.C = S + (size_t)k1 * ld_ah; p.ldc = k0; p.M = ncol; p.N = k0;
    } else {
        p.E = g0->kinEp.as<double>(); p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->kin_Y.as<double>(); p.ldy = bg->kin_ldy;
        p.C = S + (size_t)k1 * ld_ah; p.ldc = ld_ah; p.M = ncol * k0; p.N = k2;
    }
    const long maxlen = donor_run_records(bg, p, probed.donor_pairs ? P.pd_slab : (long)k2 * ld_ah, kp.data());
    // slices of whole stages along the cell axis, the last one shorter
    const long stages_all = np / GEMM_BK, per = (stages_all + P.fold_split6 - 1) / P.fold_split6;
    const long e1_slab = (long)k1 * ld_ah;
    int slices = 0;
    long chunk_max = GEMM_BK;
    if (P.e1_pairs) {
        GemmProblem& e = kp[groups];
        e.X = D.G; e.ldx = D.ldg; e.Y = g0->kinP.as<double>(); e.ldy = P.ldP;
        e.C = ctx->ws_AH.as<double>(); e.ldc = P.ldP; e.M = ncol; e.N = k1 * k0;
        if (probed.e1_sym) { e.Y = d_EE; e.ldy = g0->ld_ee; e.N = npair; }
    }
    for (int sps = 0; sps < P.fold_split6 && !P.e1_pairs; sps++) {
        const long s0 = sps * per, s1 = std::min(stages_all, s0 + per);
        if (s1 <= s0) break;
        GemmProblem& e = kp[groups + slices++];
        e.X = D.G + s0 * GEMM_BK * D.ldg; e.ldx = D.ldg;
        e.E = d_Ep + s0 * GEMM_BK * g0->ld_ep; e.lde = g0->ld_ep; e.k0 = k0;
        e.Y = bg->H.as<double>() + s0 * GEMM_BK * bg->ldh; e.ldy = bg->ldh;
        e.C = ctx->ws_AH.as<double>() + (size_t)sps * e1_slab; e.ldc = ld_ah;
        e.M = ncol * k0; e.N = k1; e.cells = (s1 - s0) * GEMM_BK;
        chunk_max = std::max(chunk_max, e.cells);
    }
    kp.resize((size_t)groups + std::max(slices, 1));
    return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int { return pair_stage(B, R, Q, D, d_kp, maxlen, chunk_max, slices); });
}

// ... its launches, from the records at d_kp (null: the pair products are in the stream's queue already, collect_fits)
int ScanPass::pair_stage(const Block& B, const SubRange& R, const Pairs& Q, const DonorCols& D, GemmProblem* d_kp, long maxlen,
                         long chunk_max, int slices) {
    double* S = ctx->ws_S.as<double>();
    const int k1 = bg->kin_k1, k2 = bg->kin_k2, ncol = D.ncol, npair = P.npair;
    const long groups = bg->kin_groups, ld_ah = P.ld_ah, e1_slab = (long)k1 * ld_ah;
    double* AH = ctx->ws_AH.as<double>();
    if (probed.donor_pairs) {
        if (d_kp) CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, npair, maxlen, false, 0, 1, 0));
        // One phenotype, no second assembly from the rotated S (flags: flat_probes) and no replay: the Gram of the
        // assembly straight from the pair products, the rotated S stays in LDS (wb_gram_fused.hip)
        if (probed.wb_rotate && may_fuse_gram() && R.b0 == 0 && R.nb == B.nb) {
            const AssembleArgs aa = assemble_args(R, 0);
            const WbFusedArgs fa{ctx->ws_Pd.as<double>(), P.pd_slab, P.ldPd, bg->wb_U.as<double>(), (long)bg->wb_k2pad * 128, 128,
                                 AH, P.pd_slab, (int)groups, P.donor_pair_splits, bg->wb_k2pad};
            if (wb_gram_fused_serves(aa, fa, nrho)) {
                CRM_TRY(launch_wb_gram_fused(st, aa, fa, nrho, ncol));
                gram_fused = true;
                ctx->wb_gram_fused_blocks++;
            }
        }
        if (!gram_fused && P.wb()) CRM_TRY(ctx->ws_A.ensure(ws_A_bytes()));   // (workspaces() left it to the fused Gram)
        if (gram_fused) {
        } else if (probed.wb_rotate)   // (the rotated S straight from the pair products: the rows of S are not formed)
            CRM_TRY(launch_donor_pairs_rotate(st, ctx->ws_Pd.as<double>(), P.pd_slab, P.ldPd, (int)groups, ncol, k0,
                                              bg->wb_U.as<double>(), (long)bg->wb_k2pad * 128, 128, bg->wb_k2pad,
                                              ctx->ws_A.as<double>(), P.ldAw, AH, P.pd_slab, P.donor_pair_splits));
        else
            CRM_TRY(launch_donor_pairs_expand(st, ctx->ws_Pd.as<double>(), P.pd_slab, P.ldPd, (int)groups, ncol, k0, k1, S, ld_ah,
                                              AH, P.pd_slab, P.donor_pair_splits));
        CRM_TRY(launch_reduce_splits(st, AH, (long)ncol * P.ldPd, P.donor_pair_splits, P.pd_slab));
        CRM_TRY(launch_pair_rows_sym(st, AH, P.ldPd, ncol, k0, S, ld_ah));
        ctx->donor_pair_blocks++;
    } else {
        if (k2 == 1) CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, k0, maxlen, false, 0, 1, 0));
        else CRM_TRY(launch_kr_transposed(ctx, d_kp, (int)groups, ncol * k0, k2, maxlen, k0));
        if (P.e1_pairs) {
            const long p_slab = (long)(std::max<long>(P.BLK, P.pair_cap) + 128) * P.ldP;
            CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, 1, ncol, probed.e1_sym ? npair : k1 * k0, np, false, 0, P.fold_split6, p_slab));
            CRM_TRY(launch_reduce_splits(st, AH, (long)ncol * P.ldP, P.fold_split6, p_slab));
            if (probed.e1_sym) CRM_TRY(launch_pair_rows_sym(st, AH, P.ldP, ncol, k0, S, ld_ah));
            else CRM_TRY(launch_pair_rows(st, AH, P.ldP, ncol, k1, k0, S, ld_ah));
        } else {
            CRM_TRY(launch_kr_transposed(ctx, d_kp + groups, slices, ncol * k0, k1, chunk_max, k0));
            CRM_TRY(launch_reduce_splits(st, AH, e1_slab, slices, e1_slab));
            CRM_HIP(hipMemcpyAsync(S, AH, sizeof(double) * (size_t)e1_slab, hipMemcpyDeviceToDevice, st));
        }
    }
    // (2 kin_rows k2 k0 + 2 n k1 k0 flops per variant, outside the timed pair: the roofline figure is the MixK product's own;
    // bench.py's whole_path counts them)
    if (!D.in_pair_order && !P.wb()) CRM_TRY(gather_pairs(S, P.kdim, Q));
    return CRM_OK;
}

// AH = H'(g o E0) without an n-length contraction against the cols columns of H:
// (a) the block in donor order; (b) per donor d' the Khatri-Rao contraction over its own cells against
// [us | E1] (transposed store: S[(d' KK + q), (b, i)]); (c) the L rows: for every j a contraction over the
// donors with hKd, AH[(k1 + j m + d), .] = sum_d' hKd[d', d] S[(d' KK + j), .]; (d) the E1 rows: sums over d'
int ScanPass::unfolded_AH(const Block& B, const SubRange& R, const Pairs& Q) {
    DonorCols D;
    CRM_TRY(donor_columns(B, R, Q, D, st));
    double* S = ctx->ws_S.as<double>();
    double* AH = ctx->ws_AH.as<double>();
    const int k1 = bg->kin_k1, k2 = bg->kin_k2, ncol = D.ncol, npair = P.npair;
    const long groups = bg->kin_groups, mk = bg->kin_cols, KK = P.KK, ld_ah = P.ld_ah;
    GemmProblem p{};
    p.X = D.Gk; p.ldx = D.ldk;
    if (probed.pairs_unfolded) {
        // P_d = G_d'(E (x) E)_d per donor; Z = [hKd | 1]' P over the donors (in ws_S: the per-donor blocks are not formed);
        // rows k1 + j m + c of AH from Z_c, rows [0, k1) from the sums over the donors Z_m
        double* Pd = ctx->ws_Pd.as<double>();
        double* Z = S;
        std::vector<GemmProblem> kp((size_t)groups + 1);
        p.Y = g0->kinEE.as<double>(); p.ldy = g0->ld_ee; p.C = Pd; p.ldc = P.ldPd; p.M = ncol; p.N = npair;
        const long maxlen = donor_run_records(bg, p, P.pd_slab, kp.data());
        GemmProblem& z = kp[groups];
        z.X = bg->kin_hKd.as<double>(); z.ldx = bg->kin_ldh;   // (column m of hKd: ones)
        z.Y = Pd; z.ldy = P.pd_slab; z.C = Z; z.ldc = P.pd_slab; z.M = (int)mk + 1; z.N = (int)((long)ncol * P.ldPd);
        return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
            CRM_TRY(launch_gemm_tn(ctx, d_kp, (int)groups, ncol, npair, maxlen, false, 0, 1, 0));
            CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, 1, (int)mk + 1, (int)((long)ncol * P.ldPd), bg->kin_groups_pad, false, 0, 1, 0));
            CRM_TRY(launch_donor_pairs_expand(st, Z, P.pd_slab, P.ldPd, (int)mk, ncol, k0, k1, AH, ld_ah, Pd, P.pd_slab, 1, 1, mk));
            CRM_TRY(launch_pair_rows_sym(st, Z + (size_t)mk * P.pd_slab, P.ldPd, ncol, k0, AH, ld_ah));
            ctx->donor_pair_blocks++;
            if (!D.in_pair_order) CRM_TRY(gather_pairs(AH, bg->ldh, Q));
            return CRM_OK;
        });
    }
    std::vector<GemmProblem> kp((size_t)groups + k2);
    p.E = g0->kinEp.as<double>(); p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->kin_Y.as<double>(); p.ldy = bg->kin_ldy;
    p.C = S; p.ldc = ld_ah; p.M = ncol * k0; p.N = (int)KK;
    const long maxlen = donor_run_records(bg, p, KK * ld_ah, kp.data());
    for (int j = 0; j < k2; j++) {
        GemmProblem& q = kp[groups + j];
        q.X = bg->kin_hKd.as<double>(); q.ldx = bg->kin_ldh; q.Y = S + (size_t)j * ld_ah; q.ldy = KK * ld_ah;
        q.C = AH + (size_t)(k1 + (long)j * mk) * ld_ah; q.ldc = ld_ah; q.M = (int)mk; q.N = ncol * k0;
    }
    return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) -> int {
        CRM_TRY(launch_kr_transposed(ctx, d_kp, (int)groups, ncol * k0, (int)KK, maxlen, k0));
        CRM_TRY(launch_gemm_tn(ctx, d_kp + groups, k2, (int)mk, ncol * k0, bg->kin_groups_pad, false, 0, 1, 0));
        CRM_TRY(launch_kin_sum_e1(st, S, ld_ah, (int)KK, k2, k1, (int)groups, (long)ncol * k0, AH, ld_ah));
        // (2 kin_rows KK k0 + 2 groups_pad m k2 k0 flops per variant, outside the timed pair: the roofline figure is the Mix
        // product's own; bench.py's whole_path counts them)
        if (!D.in_pair_order) CRM_TRY(gather_pairs(AH, bg->ldh, Q));
        return CRM_OK;
    });
}

// several phenotypes on the direct route through H: AH = H'(g o E0) over all cells, then the pair gather
int ScanPass::direct_AH(const Block& B, const SubRange& R, const Pairs& Q, AGroups& A) {
    GemmProblem p{};
    p.X = B.Gt + R.b0; p.ldx = B.ldt; p.E = d_Ep; p.lde = g0->ld_ep; p.k0 = k0; p.Y = bg->H.as<double>(); p.ldy = bg->ldh;
    p.C = ctx->ws_AH.as<double>(); p.ldc = P.ld_ah; p.M = R.nb * k0; p.N = (int)bg->cols;
    CRM_TRY(upload(SLOT_ONE, &p, 1));
    CRM_TRY(launch_kr_transposed(ctx, d_probs + SLOT_ONE, 1, p.M, p.N, np, k0));
    A.kr_flops += 2.0 * (double)n * (double)bg->cols * (double)k0 * (double)R.nb;
    return gather_pairs(ctx->ws_AH.as<double>(), bg->ldh, Q);
}

// Unrelated-donor form: the rotated S, rows (col k0 + i) over the donors k2 positions -- per donor
// (U_d Lambda_d^-1/2)' S_d, stored transposed into ws_A; col = the pair (one phenotype) or the block position
int ScanPass::woodbury_S(const SubRange& R, const Pairs& Q) {
    CRM_TRY(ctx->ws_A.ensure(ws_A_bytes()));   // (workspaces() leaves it out where the fused Gram may serve)
    const long groups = bg->kin_groups;
    const int ncol = P.wb_block ? R.nb : Q.npairs;
    std::vector<GemmProblem> kp((size_t)groups);
    GemmProblem p{};
    p.X = ctx->ws_S.as<double>() + (size_t)bg->kin_k1 * P.ld_ah; p.ldx = P.ld_ah;
    p.C = ctx->ws_A.as<double>(); p.ldc = P.ldAw; p.M = ncol * k0;
    woodbury_records(bg, p, (long)bg->kin_k2 * P.ld_ah, kp.data());
    return with_records(SLOT_KIN, kp, [&](GemmProblem* d_kp) {
        return launch_gemm_tn(ctx, d_kp, (int)groups, ncol * k0, bg->kin_k2, bg->wb_k2pad, false, 0, 1, 0);
    });
}

// 6. A~ = KR(Gs, Ep)' Q0(rho), one problem per non-empty rho group of pairs.
//    Several genes can select several rho* for one variant; with Q0(rho) = H Mix(rho) the
//    n-length Khatri-Rao contraction is then done once per variant against H (stored transposed)
//    and every (variant, rho) pair costs a cols-length product with Mix(rho) instead.
int ScanPass::form_A(const Block& B, const SubRange& R, const Pairs& Q) {
    gram_fused = false;   // (set by folded_S where the fused Gram serves the sub-range)
    bool via_H = P.kin();
    if (P.fastT && ng > 1 && !P.kin()) {
        double direct = 0.0, via = (double)R.nb * (double)bg->cols * (double)n;
        for (int i = 0; i < nrho; i++) {
            direct += (double)Q.cnt[i] * bg->r[i] * (double)n;
            via += (double)Q.cnt[i] * bg->r[i] * (double)bg->ldh;
        }
        via_H = ctx->tune.shared_h < 0 ? via < 0.9 * direct : ctx->tune.shared_h > 0;
    }
    const bool direct = !P.collapsed() && !via_H;
    if (direct)
        for (int i = 0; i < nrho; i++)
            if (Q.cnt[i] > 0) CRM_TRY(crm_background_require_q0(bg, i));
    AGroups A;
    bool tail_of[CRM_MAX_RHO] = {false};
    if (direct) CRM_TRY(direct_splits(Q, A, tail_of));
    a_records(Q, via_H, tail_of, A);
    const bool timing = !P.wb() && ctx->timing && ctx->timed_used < 65536;  // bounded: a forgotten timer cannot grow for ever
    // (kinship-structure route: the pair brackets the dominant launch alone, the Mix(rho*)' product further down)
    if (timing) CRM_TRY(kernel_timer_open(ctx, st, !P.kin()));
    if (P.folded()) CRM_TRY(folded_S(B, R, Q));
    else if (P.kin()) CRM_TRY(unfolded_AH(B, R, Q));
    else if (via_H) CRM_TRY(direct_AH(B, R, Q, A));
    CRM_TRY(upload(SLOT_ONE, probs.data(), A.nz));
    GemmProblem* d_A = d_probs + SLOT_ONE;
    if (P.collapsed()) {
        CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, (int)((long)k0 * ldq), P.mp, false, 0, 1, 0));
    } else if (P.wb()) {
        if (!probed.wb_rotate) CRM_TRY(woodbury_S(R, Q));   // (else the rotated S is in ws_A already: launch_donor_pairs_rotate)
    } else if (P.kin()) {
        if (timing) CRM_HIP(hipEventRecord(ctx->timed[ctx->timed_used].first, st));
        struct Restore { crm_ctx* c; ~Restore() { c->tune.tag = 0; } } restore{ctx};
        ctx->tune.tag = 1;
        CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, P.kdim, false, 0, 1, 0));
    } else if (via_H) {
        CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, P.kdim, false, 0, 1, 0));
    } else {
        CRM_TRY(launch_gemm_tn(ctx, d_A, A.nz, A.max_m, A.max_n, np, true, k0, A.kr_split, (long)A.a_slab));
        CRM_TRY(launch_reduce_splits(st, ctx->ws_A.as<double>(), (long)Q.npairs * k0 * P.ldA, A.kr_split, (long)A.a_slab));
        if (!A.tails.empty()) {
            const int saved_bn = ctx->tune.bn;
            ctx->tune.bn = 160;
            struct Restore { crm_ctx* c; int bn; ~Restore() { c->tune.bn = bn; } } restore{ctx, saved_bn};
            CRM_TRY(upload(A.nz, A.tails.data(), A.tails.size()));
            CRM_TRY(launch_gemm_tn(ctx, d_probs + A.nz, (int)A.tails.size(), A.max_m, A.tail_maxn, np, true, k0, A.tail_split, (long)A.a_slab));
            ctx->tail_launches++;
            for (const GemmProblem& t : A.tails)
                CRM_TRY(launch_reduce_splits_band(st, t.C, (long)t.M, t.ldc, 0, t.N, A.tail_split, (long)A.a_slab));
        }
    }
    if (timing) {
        CRM_TRY(kernel_timer_close(ctx, st));
        ctx->kr_flops += A.kr_flops;
    }
    if (!A.spectrum_tails.empty()) {
        CRM_TRY(upload(A.nz, A.spectrum_tails.data(), A.spectrum_tails.size()));
        CRM_TRY(launch_skinny_tn(st, d_probs + A.nz, (int)A.spectrum_tails.size(), A.max_m, P.kdim));
        ctx->spectrum_tail_launches++;
        CRM_HIP(hipStreamSynchronize(st));   // (the records live on this stack frame)
    }
    return CRM_OK;
}

// 7. elementwise products for the side contractions
// 8. y-free side contractions: Z2 = (Gt o G)' E, Z3 = (Gt o Gt)' (E (x) E)
// (the records -- Z2, Z3 -- and the launches apart: the side stream's are uploaded ahead of the fork, scan_side.hip)
void ScanPass::side_records(const SubRange& R, GemmProblem* out) const {
    double* G2 = ctx->ws_G2.as<double>();
    double* GG = !P.collapsed() ? ctx->ws_GG.as<double>() : G2;   // (test direction) o (fixed-effect role)
    GemmProblem p{};
    p.ldx = P.ldb; p.M = R.nb;
    p.X = GG; p.Y = P.collapsed() ? tab->Z2.as<double>() : d_Ep; p.ldy = g0->ld_ep; p.C = dZ2; p.ldc = P.ldZ2; p.N = k0;
    out[0] = p;
    p.X = G2; p.Y = P.collapsed() ? tab->Z3.as<double>() : d_EE; p.ldy = g0->ld_ee; p.C = dZ3; p.ldc = P.ldZ3; p.N = P.npair;
    out[1] = p;
}
int ScanPass::side_launches(const Block& B, const SubRange& R, hipStream_t on, const GemmProblem* d_recs) {
    const long ldb = P.ldb;
    const int nb = R.nb;
    double* G2 = ctx->ws_G2.as<double>();
    double* GG = !P.collapsed() ? ctx->ws_GG.as<double>() : nullptr;
    // (a fused block: block_stats' pass has written both, from the same products)
    if (!B.fused) CRM_TRY(launch_square_block(on, B.Gt + R.b0, B.Gx + R.b0, ldb, ldb, P.xrows, (int)(ldb - R.b0), G2, GG, ldb));
    const int s2 = P.collapsed() ? 1 : P.ks2, s3 = P.collapsed() ? 1 : P.ks3;
    if (P.cross) {
        CRM_TRY(launch_donor_cross(on, nb, B.Gb + R.b0, ldb, (int)panel->m, tab->Z2.as<double>(), P.ldZ2, k0, dZ2, P.ldZ2));
    } else {
        CRM_TRY(launch_gemm_tn(ctx, on, d_recs, 1, nb, k0, P.xrows, false, 0, s2, z2_sz));
        CRM_TRY(launch_reduce_splits(on, dZ2, z2_sz, s2, z2_sz));
    }
    CRM_TRY(launch_gemm_tn(ctx, on, d_recs + 1, 1, nb, P.npair, P.xrows, false, 0, s3, z3_sz));
    return launch_reduce_splits(on, dZ3, z3_sz, s3, z3_sz);
}
int ScanPass::side_contractions(const Block& B, const SubRange& R) {
    side_records(R, probs.data() + 1);
    CRM_TRY(upload(SLOT_RHO, probs.data() + 1, 2));
    return side_launches(B, R, st, d_probs + SLOT_RHO);
}

// 9. Z1 = Gt' [y o E, W o E] of every phenotype, one launch (ScanPlan::ks1)
void ScanPass::z1_records(const Block& B, const SubRange& R, GemmProblem* out) const {
    for (int gi = 0; gi < ng; gi++) {
        crm_gene* g = genes[gi];
        GemmProblem p{};
        p.X = B.Gt + R.b0; p.ldx = B.ldt; p.Y = P.collapsed() ? g->dt_Z1.as<double>() : g->YE.as<double>(); p.ldy = g->ld_ye;
        p.C = dZ1 + (size_t)gi * z1_sz * P.ks1; p.ldc = P.ldZ1; p.M = R.nb; p.N = k0 * (1 + c);
        out[gi] = p;
    }
}
int ScanPass::z1_launches(const SubRange& R, hipStream_t on, const GemmProblem* d_recs) {
    const int s1 = P.collapsed() ? 1 : P.ks1;
    CRM_TRY(launch_gemm_tn(ctx, on, d_recs, ng, R.nb, k0 * (1 + c), P.xrows, false, 0, s1, z1_sz));
    for (int gi = 0; gi < ng; gi++)
        CRM_TRY(launch_reduce_splits(on, dZ1 + (size_t)gi * z1_sz * P.ks1, z1_sz, s1, z1_sz));
    return CRM_OK;
}
int ScanPass::z1_products(const Block& B, const SubRange& R) {
    std::vector<GemmProblem> zp((size_t)ng);
    z1_records(B, R, zp.data());
    CRM_TRY(upload(P.z1_slot(), zp.data(), zp.size()));
    return z1_launches(R, st, d_probs + P.z1_slot());
}

}  // namespace crm
