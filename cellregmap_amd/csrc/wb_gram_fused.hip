// Unrelated-donor form, one phenotype: the weighted Gram Gw of [rotated S ; W ; gx ; y ; E1] straight from the per-donor pair
// products -- donor_pairs_rotate_kernel (blockops.hip) and gram_ext_dma_wide_kernel (gram_ext.hip) in one launch, so that the
// rotated S (ws_A: variants x k0 rows x donors k2 positions) is neither written nor read back.
//
// One workgroup per variant of the block walks the donors.  A donor d owns the positions [k0 d, k0 d + k0) of the Gram's
// contraction; the Gram sums positions in groups of four from position 0 in one accumulator per output, so the walk is cut at
// the multiples of four: chunk d is [start_d, end_d), start_d = 4 floor(k0 d / 4), end_d = start_(d + 1) (the last one:
// 4 ceil(donors k0 / 4), zeros past the end).  With k0 even a chunk is k0 - 2, k0 or k0 + 2 positions and every group of
// four is the two launches' group: Gw has their bits (up to the sign of a zero).  Per donor:
//   rotation  A_d = S_d Psi_d (k0 x k0) on the FP64 MFMA as donor_pairs_rotate_kernel forms it (symmetric lookup into the
//             donor's pair products, k ascending in groups of four, one accumulator per output), written into the Gram's
//             LDS image; the donor sums Psum are accumulated from the same LDS copy of P_d;
//   Gram      over the chunk's columns of the image: rows [0, k0) the rotated S, rows [k0, KT) the other operand rows
//             brought in by LDS-DMA; the weight d_j = s / (1 + s), s = (v0 / v1) S0_j, goes onto the B operand; the upper
//             triangle of 16 x 16 tiles dealt to the four wavefronts as in gram_ext_dma_wide_kernel.
// LDS image of the Gram: row R at R * RS doubles, RS = (k0 + 4) | 2 (an odd multiple of two: the sixteen rows of a fragment
// read start two 8-byte slots apart); a position p of chunk d sits in column p - start_d + c0_d, c0_d = 2 - (k0 d - start_d),
// so that A_d[., j] is column j + 2 in every chunk -- except the last two of a donor whose chunk ends two short (k0 = 2 mod 4,
// d even): they belong to chunk d + 1 and go to its columns 0 and 1, which chunk d does not read and the rotation of d + 1
// does not write.  Columns that no chunk fills are zeros: written once for the rotated rows, and by every DMA for the
// others (lanes off the chunk read a row of zeros, AssembleArgs::A_none).
// Every buffer is single: a load is issued behind the barrier that frees its buffer and waited for (vmcnt(0), written out:
// dma_barrier, wave_ops.h) before the next barrier, so it is in flight during the MFMAs of the phase between the two --
//     rotation d | wait + barrier | issue P, Psi, S0 of d + 1 | Gram d | wait + barrier | issue the other rows of d + 1 | rotation d + 1 ...
// (two of everything would not fit two workgroups per CU: 79 KB per workgroup at k0 = 50 as it is), and the second
// workgroup of the CU fills what is left.  With the form "wb_gram_spread" (the default) the issues do not stand in a bunch
// behind the barrier but one by one among the MFMAs of the phase that follows it, behind the same barrier as before --
//     rotation d, the other rows of d piece by piece | wait + barrier | Gram d, P, Psi, S0 of d + 1 piece by piece | wait + barrier | rotation d + 1 ...
// The loop holds no ordinary global load: each would be waited for together with every LDS-DMA in flight.
#include <type_traits>

#include "assemble.h"
#include "gram_common.h"

namespace crm {

namespace {

constexpr int WF_MAXQ_P = 10, WF_MAXQ_O = 9, WF_PSUM = 6;   // DMA instructions per wavefront (P, Psi, S0 / other rows); sums per thread
// what may cross the marks around a spread piece (__builtin_amdgcn_sched_barrier): vector and scalar ALU, LDS -- not a load, not an MFMA
constexpr int WF_PIN = 0x2 | 0x4 | 0x80 | 0x100 | 0x200;
constexpr int WF_UW = 56;   // LDS row of Psi_d: a constant, so that the fragment reads carry their offsets as immediates (k0 <= 54)
constexpr int WF_MAXKS = 14;   // k-steps of the rotation and of the longest chunk: (k0 + 2) / 4, k0 <= 54

}  // namespace

WbFusedLayout wb_gram_fused_layout(int k0, int KT, long ldp) {
    WbFusedLayout L;
    const int KS = (k0 + 3) / 4;
    L.urows = 4 * KS;
    L.UW = WF_UW;
    L.RS = (k0 + 4) | 2;
    L.nP = (int)(ldp / 128);
    L.nU = (L.urows * (L.UW / 2) + 63) / 64;
    L.rows_o = KT - k0;
    L.nO = (L.rows_o * (L.RS / 2) + 63) / 64;
    L.off_P = k0 * L.RS + L.nO * 128;
    L.off_U = L.off_P + L.nP * 128;
    L.off_S0 = L.off_U + L.nU * 128;
    L.off_d = L.off_S0 + 128;
    L.off_rp = L.off_d + 64;
    L.total = L.off_rp + ((L.rows_o + 1) & ~1);
    return L;
}

namespace {

// STRIPS (form "gram_strips", the default): the tiles are dealt in strips (tile_gram.h: kStripDeal) and the Gram phase is
// written out per role and k-step; false: the round-robin deal, one k-loop for every role.  Every accumulator receives the
// same operands in the same order either way.
// SPREAD (form "wb_gram_spread", the default; with STRIPS only): a donor's LDS-DMA instructions are issued one by one among
// the MFMAs of the phase that they used to stand in front of -- P, Psi of d + 1 behind the first MFMA of the Gram's k-steps
// 0, 1, ... of donor d, the other rows of d behind the MFMA pairs of the rotation's first k-steps of donor d; what is left
// when the steps run out follows the last step.  Which barrier frees a piece's buffer and which one waits for it does not
// change, and no accumulator sees another operand.  false: every piece in a bunch behind the barrier, the earlier order.
template <int NTL, bool STRIPS, bool SPREAD>
__global__ __launch_bounds__(256, NTL <= 7 ? 2 : 1) void wb_gram_fused_kernel(AssembleArgs a, WbFusedArgs f, WbFusedLayout L, int KT) {
    static_assert(STRIPS || !SPREAD, "the pieces are spread among the k-steps of the strip deal only");
    constexpr int NTILES = NTL * (NTL + 1) / 2, MAXT = (NTILES + 3) / 4;
    constexpr int MAXKS = WF_MAXKS;
    extern __shared__ __align__(16) double smem[];
    double* const img = smem;                      // [KT][RS] (+ what the last DMA instruction overshoots)
    double* const Pl = smem + L.off_P;             // the donor's pair products of this variant
    double* const Ul = smem + L.off_U;             // Psi_d [urows][UW]
    double* const S0l = smem + L.off_S0;           // S0 of the chunk, by column
    double* const dS = smem + L.off_d;             // d_j of the chunk, by column
    const double** const rowp = reinterpret_cast<const double**>(smem + L.off_rp);
    const int b = blockIdx.x;
    const NullFitOut fit = a.fit[b];
    const AssembleRho R = a.rho[fit.rho_index];
    const double ratio = fit.v0 / fit.v1;
    const bool has_A = a.sorted_pos[b] >= 0;       // (block order: the position is the variant's own; none: rows of zeros)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int k0 = a.k0, RS = L.RS;
    constexpr int UW = WF_UW;
    const int npair = k0 * (k0 + 1) / 2, KS = (k0 + 3) / 4, JT = (k0 + 15) / 16;
    const int D = f.donors, Ptot = D * k0;
    const double* __restrict__ zeros = a.A_none;

    for (int e = tid; e < k0 * RS; e += 256) img[e] = 0.0;
    for (int t = tid; t < L.rows_o; t += 256) rowp[t] = gram_other_row(a, R, b, t);
    // what each DMA instruction of this lane reads: instruction I = wave + 4 q carries the 16-byte units 64 I .. 64 I + 63 of
    // its LDS region.  P, Psi, S0: an element offset (P: into the variant's row; Psi: k ldu + column; S0: the column);
    // the other rows: (row << 8) | column, -1 off the rows
    const int nPU = L.nP + L.nU + 1;
    int poff[WF_MAXQ_P], ocode[WF_MAXQ_O];
#pragma unroll
    for (int q = 0; q < WF_MAXQ_P; q++) {
        const int I = wave + 4 * q;
        if (I < L.nP) poff[q] = 128 * I + 2 * lane;
        else if (I < L.nP + L.nU) {
            const int u = 64 * (I - L.nP) + lane, k = u / (UW / 2), cu = u - k * (UW / 2);
            poff[q] = k < L.urows ? k * (int)f.ldu + 2 * cu : 0;
        } else poff[q] = 2 * lane;
    }
#pragma unroll
    for (int q = 0; q < WF_MAXQ_O; q++) {
        const int u = 64 * (wave + 4 * q) + lane, t = u / (RS / 2), cu = u - t * (RS / 2);
        // (SPREAD: not the row but the place of its pointer in LDS, in bytes from the start, other_row; off the rows: row 0, a
        // column off every chunk)
        if constexpr (SPREAD) ocode[q] = t < L.rows_o ? ((8 * (L.off_rp + t)) << 8) | (2 * cu) : ((8 * L.off_rp) << 8) | 255;
        else ocode[q] = t < L.rows_o ? (t << 8) | (2 * cu) : -1;
    }
    // SPREAD: P and Psi as unsigned byte offsets from the donor's wave-uniform P_d and Psi_d, so that a piece is its one
    // instruction on a scalar base; P, Psi and S0 are one LDS region, instruction I at Pl + 128 I
    const int nPsi = L.nP + L.nU;
    unsigned pbyte[WF_MAXQ_P];
    if constexpr (SPREAD) {
#pragma unroll
        for (int q = 0; q < WF_MAXQ_P; q++) pbyte[q] = 8u * (unsigned)poff[q];
    }
    // the chunk of donor d: positions [start, end) at columns c0 .., the columns [c0, c0 + lim - start) hold data
    auto chunk = [&](int d, int& start, int& end, int& c0, int& lim) __attribute__((always_inline)) {
        start = (k0 * d) & ~3;
        end = d + 1 < D ? (k0 * (d + 1)) & ~3 : (Ptot + 3) & ~3;
        c0 = 2 - (k0 * d - start);
        lim = end < Ptot ? end : Ptot;
    };
    auto issue_pus = [&](int d) __attribute__((always_inline)) {
        int start, end, c0, lim;
        chunk(d, start, end, c0, lim);
        const double* __restrict__ Pd = f.P + (size_t)d * f.p_slab + (long)b * f.ldp;
        const double* __restrict__ Ud = f.U + (size_t)d * f.u_slab;
        const double* __restrict__ S0 = R.S0 + (start - c0);
#pragma unroll
        for (int q = 0; q < WF_MAXQ_P; q++) {
            const int I = wave + 4 * q;
            if (I < L.nP) gram_dma16(Pd + poff[q], Pl + 128 * I);
            else if (I < L.nP + L.nU) gram_dma16(Ud + poff[q], Ul + 128 * (I - L.nP));
            else if (I < nPU) {
                const int col = poff[q];
                gram_dma16(col >= c0 && start - c0 + col < lim ? S0 + col : zeros, S0l);
            }
        }
    };
    auto issue_others = [&](int d) __attribute__((always_inline)) {
        int start, end, c0, lim;
        chunk(d, start, end, c0, lim);
        const int shift = start - c0;
#pragma unroll
        for (int q = 0; q < WF_MAXQ_O; q++) {
            const int I = wave + 4 * q;
            if (I < L.nO) {
                const int code = ocode[q], col = code & 255;
                const bool in = code >= 0 && col >= c0 && shift + col < lim;
                const double* src = zeros;
                if (in) src = rowp[code >> 8] + (shift + col);
                gram_dma16(src, img + k0 * RS + 128 * I);
            }
        }
    };
    // SPREAD: the same pieces one at a time.  The donor that the Gram phase brings in: its P_d and Psi_d, and how many of
    // the instructions 0 .. nPsi - 1 there are to issue (none behind the last donor)
    const char* Pnext = nullptr;
    const char* Unext = nullptr;
    int n_next = 0;
    auto set_next = [&](int d) __attribute__((always_inline)) {
        Pnext = reinterpret_cast<const char*>(f.P + (size_t)d * f.p_slab + (long)b * f.ldp);
        Unext = reinterpret_cast<const char*>(f.U + (size_t)d * f.u_slab);
        n_next = d < D ? nPsi : 0;
    };
    auto pu_piece = [&](auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        if constexpr (q < WF_MAXQ_P) {
            // (I and the offset pass through empty asm: what follows from them is a few scalar instructions beside the
            // piece, not a table of flags and 64-bit offsets kept across the donor loop in registers that are not there)
            int I = wave + 4 * q;
            asm volatile("" : "+s"(I));
            if (I < n_next) {
                unsigned off = pbyte[q];
                asm volatile("" : "+v"(off));
                gram_dma16(reinterpret_cast<const double*>((I < L.nP ? Pnext : Unext) + off), Pl + 128 * I);
            }
        }
    };
    // S0 of chunk d (instruction nPsi, one wavefront's): its lanes choose between two sources, so it goes first in its phase
    auto s0_piece = [&](int d) __attribute__((always_inline)) {
        if (d < D && ((nPsi - wave) & 3) == 0) {
            int start, end, c0, lim;
            chunk(d, start, end, c0, lim);
            const int col = 2 * lane;
            gram_dma16(col >= c0 && start - c0 + col < lim ? R.S0 + (start - c0) + col : zeros, S0l);
        }
    };
    // the other rows: the row's address is looked up (other_row) a step ahead of the piece that adds the chunk's shift
    // (a lane is on the chunk when its column is one of the o_width from o_c0: one unsigned compare, both sources formed
    // and one selected -- no branch among the MFMAs)
    int n_other = 0, o_c0 = 0, o_shift = 0, o_width = 0;
    auto set_others = [&](int d, bool on) __attribute__((always_inline)) {
        int start, end, lim;
        chunk(d, start, end, o_c0, lim);
        o_shift = start - o_c0;
        o_width = lim - start;
        n_other = on ? L.nO : 0;
    };
    // (the shift is written out: left to the compiler it is taken out of the donor loop, and the nine addresses that it
    // yields are kept across the loop in vector registers that are not there)
    auto other_row = [&](int q) __attribute__((always_inline)) {
        unsigned at;
        asm volatile("v_lshrrev_b32 %0, 8, %1" : "=v"(at) : "v"(ocode[q]));
        return *reinterpret_cast<const double* const*>(reinterpret_cast<const char*>(smem) + at);
    };
    auto other_piece = [&](int q, const double* row) __attribute__((always_inline)) {     // (q: a constant once unrolled)
        int I = wave + 4 * q;
        asm volatile("" : "+s"(I));
        if (I < n_other) {
            const int col = ocode[q] & 255;
            const double* src = row + (unsigned)(o_shift + col);
            asm volatile("" : "+v"(src));
            gram_dma16((unsigned)(col - o_c0) < (unsigned)o_width ? src : zeros, img + k0 * RS + 128 * I);
        }
    };
    // rotation fragments: lane (l15, lq) of k-step ks reads S_d[k = 4 ks + lq, i = 16 w + l15] (pair (0, 0) off the matrix)
    const int iw = 16 * wave + l15;
    int pidx[MAXKS];
#pragma unroll
    for (int ks = 0; ks < MAXKS; ks++) {
        const int k = 4 * ks + lq, lo = k < iw ? k : iw, hi = k < iw ? iw : k;
        pidx[ks] = k < k0 && iw < k0 ? lo * k0 - lo * (lo - 1) / 2 + (hi - lo) : 0;
    }
    const unsigned st_base = 8u * (unsigned)((16 * wave + lq) * RS + l15 + 2);     // (the rotation's stores: byte offset of A_d[16 wave + lq, l15] in the image)
    // tiles of this wavefront, as gram_ext_dma_wide_kernel deals them (gram_common.h; rows past KT read row 0: never stored).
    // Round-robin: listed here, for the fragment offsets; strips: a tile row's fragments start at r_off[row], and the list
    // is made behind the loop, for the store alone
    const int first = gram_wave_first(wave, b);
    const int ntw = gram_wave_ntiles<NTL, STRIPS>(first);
    int t_i[MAXT], t_j[MAXT], t_ij[MAXT], r_off[NTL];
#pragma unroll
    for (int i = 0; i < NTL; i++) {
        const int row = 16 * i + l15;
        r_off[i] = (row < KT ? row : 0) * RS + lq;
    }
    if constexpr (!STRIPS) {
        gram_wave_tiles<NTL, false>(first, t_ij);
#pragma unroll
        for (int t = 0; t < MAXT; t++) {
            const int ri = 16 * (t_ij[t] & 255) + l15, rj = 16 * (t_ij[t] >> 8) + l15;
            t_i[t] = (ri < KT ? ri : 0) * RS + lq;
            t_j[t] = (rj < KT ? rj : 0) * RS + lq;
        }
    }
    v4d acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; t++) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    double psum[WF_PSUM];
#pragma unroll
    for (int q = 0; q < WF_PSUM; q++) psum[q] = 0.0;
    // the donor sums by ranges of donors, as donor_pairs_rotate_kernel's grid splits them
    const int per = (D + f.splits - 1) / f.splits;
    int split = 0;

    auto gram = [&](int col0, int nks, auto nt_tag) __attribute__((always_inline)) {
        constexpr int NT = decltype(nt_tag)::value;
        const double* __restrict__ S = img + col0;
        const double* __restrict__ Dw = dS + col0 + lq;
        // one set of fragments: an MFMA has read its operands when it is issued, so the reads of k-step ks + 1 follow the
        // MFMAs of ks into the same registers and land while those run (16 passes each); the other workgroup of the CU
        // covers what is left.  Two sets would cost 4 NT registers beside the accumulators.
        // (tile by tile: the reads of tile t for k-step ks + 1 go out behind its MFMA of ks and have the other tiles' MFMAs
        // to land in; the weight is multiplied in just before the use)
        double fa[NT], fr[NT];
        double dk = Dw[0];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            fa[t] = S[t_i[t]];
            fr[t] = S[t_j[t]];
        }
        for (int ks = 0; ks < nks; ks++) {
            const bool more = ks + 1 < nks;
            const int nx = more ? 4 * (ks + 1) : 4 * ks;     // (the last step re-reads its own fragments: no branch in the loop)
            const double dn = Dw[nx];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fr[t] * dk, acc[t], 0, 0, 0);
                fa[t] = S[t_i[t] + nx];
                fr[t] = S[t_j[t] + nx];
            }
            dk = dn;
        }
    };
    // The same for one role of the strip deal, every k-step written out: a step reads each operand tile row of the role
    // once, at register base + immediate offset, and forms the weighted fragment once per column of the role.  One set of
    // fragments as above: the read of a row for step ks + 1 follows the last MFMA of step ks that takes it.  Behind the
    // chunk's last step that read goes up to four columns past the chunk (at most column k0 + 5 of a row of RS >= k0 + 4
    // doubles: the next row's first columns or, behind the image's last row, the region that follows it in LDS) and is
    // dropped; each step stands behind a wave-uniform compare with the chunk's step count (nks <= MAXKS).
    auto gram_strips = [&](int col0, int nks, auto role_tag) __attribute__((always_inline)) {
        constexpr int ROLE = decltype(role_tag)::value;
        constexpr int NT = kStripDeal<NTL>.n[ROLE];
        const double* __restrict__ S = img + col0;
        const double* __restrict__ Dw = dS + col0 + lq;
        const double* rows[NTL];
        double fr[NTL], fw[NTL];
        static_for<0, NTL>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (kStripDeal<NTL>.reads(ROLE, i)) {
                rows[i] = S + r_off[i];
                fr[i] = rows[i][0];
            }
        });
        double dk = Dw[0];
        // (SPREAD: k-step ks carries piece ks of P and Psi of the next donor behind its first MFMA, held there against the
        // scheduler: neither a load nor an MFMA crosses the two marks)
        auto step = [&](int off, auto kc) __attribute__((always_inline)) {
            static_for<0, NTL>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if constexpr (kStripDeal<NTL>.is_b(ROLE, j)) {
                    fw[j] = fr[j] * dk;
                    if constexpr (kStripDeal<NTL>.last_a(ROLE, j) < 0) fr[j] = rows[j][off + 4];
                }
            });
            static_for<0, NT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[kStripDeal<NTL>.ti[ROLE][t]], fw[kStripDeal<NTL>.tj[ROLE][t]], acc[t], 0, 0, 0);
                if constexpr (SPREAD && t == 0) {
                    __builtin_amdgcn_sched_barrier(WF_PIN);
                    pu_piece(kc);
                    __builtin_amdgcn_sched_barrier(WF_PIN);
                }
                static_for<0, NTL>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    if constexpr (kStripDeal<NTL>.last_a(ROLE, i) == t) fr[i] = rows[i][off + 4];
                });
            });
            dk = Dw[off + 4];
        };
        static_for<0, MAXKS>([&](auto kc) {
            constexpr int ks = decltype(kc)::value;
            if (ks < nks) step(4 * ks, kc);
            else if constexpr (SPREAD) pu_piece(kc);     // (more pieces than steps, nks = 0: the rest behind the last step)
        });
    };

    __syncthreads();   // (the row pointers are read by the first loads)
    if constexpr (!SPREAD) {
        issue_pus(0);
        issue_others(0);
    } else {
        set_next(0);
        s0_piece(0);
        static_for<0, WF_MAXQ_P>(pu_piece);
        set_others(0, true);
#pragma unroll
        for (int q = 0; q < WF_MAXQ_O; q++) other_piece(q, other_row(q));
    }
    dma_barrier();     // (P, Psi, S0 and the other rows of donor 0 have landed)
    for (int d = 0; d < D; d++) {
        int start, end, c0, lim;
        chunk(d, start, end, c0, lim);
        if constexpr (SPREAD) set_others(d, d > 0);     // (this rotation phase issues the other rows of its own chunk)
        // ---- rotation phase: weights, donor sums, A_d into the image (the other rows of chunk d are in flight) ----
        if (tid < RS) dS[tid] = gram_weight(ratio, S0l[tid]);     // (zeros off the chunk: d = 0)
#pragma unroll
        for (int q = 0; q < WF_PSUM; q++)
            if (tid + 256 * q < npair) psum[q] += Pl[tid + 256 * q];
        if (d + 1 == D || d + 1 == (split + 1) * per) {
            double* __restrict__ out = f.Psum + (size_t)split * f.psum_slab + (long)b * f.ldp;
            // (the thread's index through empty asm: the offsets and the masks of these stores, which a split runs once, are
            // then formed here and not kept across the donor loop)
            int at = tid;
            asm volatile("" : "+v"(at));
#pragma unroll
            for (int q = 0; q < WF_PSUM; q++)
                if (at + 256 * q < npair) { out[at + 256 * q] = psum[q]; psum[q] = 0.0; }
            split++;
        }
        if (has_A && wave < JT) {
            unsigned uo = (unsigned)(lq * UW + l15);
            asm volatile("" : "+v"(uo));
            const double* __restrict__ ub = Ul + uo;
            // column of A_d[., j]: j + 2, or -- past the chunk's end -- columns 0, 1 of the next chunk
            const int jcut = end - k0 * d;
            // The counts that the passes compare with pass through empty asm in every donor's turn: a compare with a
            // constant is then one scalar compare beside its branch.  Left loop-invariant, each of them (some forty: a k-step
            // there is, a k-step two ahead, a column tile, a row or a column below k0) is formed once in front of the donor
            // loop as a mask in two scalar registers and kept across it -- a hundred scalar registers more than there are,
            // kept in the lanes of vector registers and read back lane by lane among the MFMAs.
            // (the k-step count twice over, ksn for "this step exists" and ksf for "a fragment two steps ahead": of one count
            // the compiler keeps the second compare of step ks as a mask for the first of step ks + 2, six scalar instructions
            // a step where two compares and two branches do)
            int ksn = KS, ksf = KS, jtn = JT, k0n = k0, rsn = RS;
            asm volatile("" : "+s"(ksn), "+s"(ksf), "+s"(jtn), "+s"(k0n), "+s"(rsn));
            // Where a pass stores: A_d[16 wave + lq + 4 reg, 16 tile + l15] at st + 32 RS reg + 128 tile bytes of the image, the
            // two columns past jcut 8 (jcut + 2) bytes back.  One address from in front of the loop (through empty asm as
            // well: the sixteen that follow from it were kept across the loop, in vector registers that are not there) and
            // scalar offsets; a row or a column is below k0 when lq or l15 is below a scalar.
            unsigned st = st_base;
            asm volatile("" : "+v"(st));
            const int rows_below = k0n - 16 * wave;
            // One pass: NT (1 or 2) column tiles from tile TH on, every k-step (two tiles at a time: four would hold 32 more
            // registers beside the Gram's accumulators).  NT is the pass's own, so no MFMA stands behind a branch of its own
            // and an accumulator is one register tuple from its first MFMA (on zeros, an inline constant) to its store.
            auto rotate = [&](auto th_tag, auto nt_tag) __attribute__((always_inline)) {
                constexpr int TH = decltype(th_tag)::value, NT = decltype(nt_tag)::value;
                v4d cr[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) cr[t] = (v4d){0.0, 0.0, 0.0, 0.0};
                // the fragments of k-step ks + 2 are read before the MFMAs of ks are issued (two MFMAs a step: one step
                // ahead would leave a read 128 cycles to land), and no further (the scheduler would pull every read up front)
                double af[3], bf[3][NT];
                auto frag = [&](int ks, int slot) __attribute__((always_inline)) {
                    af[slot] = Pl[pidx[ks]];
#pragma unroll
                    for (int t = 0; t < NT; t++) bf[slot][t] = ub[4 * ks * UW + 16 * (TH + t)];
                };
                frag(0, 0);
                if (1 < ksf) frag(1, 1);
#pragma unroll
                for (int ks = 0; ks < MAXKS; ks++) {
                    if (ks > 0 && ks >= ksn) break;     // (there is a first k-step: k0 >= 1)
                    // (SPREAD: the first pass over the k-steps carries piece ks of the other rows behind the MFMAs of
                    // step ks, its row looked up ahead of them)
                    const bool piece = SPREAD && TH == 0 && ks < WF_MAXQ_O;
                    const double* row = nullptr;
                    if (piece) row = other_row(ks);
                    if (ks + 2 < MAXKS && ks + 2 < ksf) frag(ks + 2, (ks + 2) % 3);
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks % 3], bf[ks % 3][t], cr[t], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (piece) {
                        other_piece(ks, row);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if constexpr (SPREAD && TH == 0) {     // (the pieces of the k-steps that k0 does not have follow the last step)
                    if (ksn < WF_MAXQ_O) {
#pragma unroll
                        for (int q = 1; q < WF_MAXQ_O; q++)
                            if (q >= ksn) other_piece(q, other_row(q));
                    }
                }
                bool below[NT];
                unsigned back[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    below[t] = l15 < k0n - 16 * (TH + t);
                    back[t] = l15 < jcut - 16 * (TH + t) ? 0u : 8u * (unsigned)(jcut + 2);
                }
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    if (lq < rows_below - 4 * reg) {
                        const unsigned at = st + (unsigned)(32 * reg) * (unsigned)rsn;
#pragma unroll
                        for (int t = 0; t < NT; t++)
                            if (below[t])
                                *reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (at - back[t] + 128u * (TH + t))) = cr[t][reg];
                    }
                }
            };
            if (jtn >= 2) rotate(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
            else rotate(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
            if (jtn >= 4) rotate(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
            else if (jtn == 3) rotate(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{});
        } else if constexpr (SPREAD) {     // (no rotation of its own -- a variant without a kinship term, wave >= JT: in a bunch)
#pragma unroll
            for (int q = 0; q < WF_MAXQ_O; q++) other_piece(q, other_row(q));
        }
        dma_barrier();     // (A_d and the weights are written; P_d, Psi_d and S0 are free; the other rows of chunk d, issued
                           // behind the previous barrier -- SPREAD: in this phase --, are waited for here: nothing else of
                           // this wavefront is in flight)
        if constexpr (!SPREAD) {
            if (d + 1 < D) issue_pus(d + 1);
        } else {
            set_next(d + 1);
            s0_piece(d + 1);
        }
        // ---- Gram phase ----
        const int nks = (end - start) / 4;
        if constexpr (STRIPS) {
            if (SPREAD || nks > 0) {     // (SPREAD: a chunk without a step still issues the next donor's pieces)
                if (first == 0) gram_strips(c0, nks, std::integral_constant<int, 0>{});
                else if (first == 1) gram_strips(c0, nks, std::integral_constant<int, 1>{});
                else if (first == 2) gram_strips(c0, nks, std::integral_constant<int, 2>{});
                else gram_strips(c0, nks, std::integral_constant<int, 3>{});
            }
        } else {
            if (ntw == MAXT) gram(c0, nks, std::integral_constant<int, MAXT>{});
            else gram(c0, nks, std::integral_constant<int, MAXT - 1>{});
        }
        dma_barrier();     // (the image is free; P, Psi and S0 of d + 1 are waited for)
        if constexpr (!SPREAD) {
            if (d + 1 < D) issue_others(d + 1);
        }
    }
    // ranges of donors that hold no donor (more splits than ranges): zeros, so that the sum over the splits is the sum
    for (; split < f.splits; split++) {
        double* __restrict__ out = f.Psum + (size_t)split * f.psum_slab + (long)b * f.ldp;
        for (int e = tid; e < npair; e += 256) out[e] = 0.0;
    }
    if constexpr (STRIPS) gram_wave_tiles<NTL, true>(first, t_ij);
    gram_store_tiles(a.wb_Gw + (long)b * KT * KT, KT, t_ij, ntw, acc, lq, l15);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// Does the fused launch serve this assembly?  One phenotype in block order on the pair-rotation form, an even context count
// (whole groups of four positions per pair of donors), 5 to 8 tile rows, every DMA source on a 16-byte boundary
bool wb_gram_fused_serves(const AssembleArgs& a, const WbFusedArgs& f, int nrho) {
    const int k0 = a.k0, KT = k0 + a.c + 2 + a.wb_k1, ts = (KT + 15) / 16;
    if (form("wb_gram_fused", 1) == 0 || form("gram_staged", 0) != 0) return false;
    if (a.wb_k1 <= 0 || k0 % 2 != 0 || !donor_pairs_rotate_serves(k0) || ts < 5 || ts > 8 || f.donors < 1 || f.splits < 1) return false;
    if (f.ldp % 128 != 0 || f.ldp < k0 * (k0 + 1) / 2 || f.p_slab % 2 != 0 || f.u_slab % 2 != 0 || f.ldu % 2 != 0 || f.ldu < 4 * ((k0 + 3) / 4) ||
        f.k2pad < 4 * ((k0 + 3) / 4) || !aligned16(f.P) || !aligned16(f.U) || !aligned16(a.A_none) || !a.wb_Gw)
        return false;
    if (a.wb_ldR % 2 != 0 || !aligned16(a.wb_R)) return false;
    for (int i = 0; i < nrho; i++) {
        const AssembleRho& R = a.rho[i];
        if (R.r != f.donors * k0 || R.ldW % 2 != 0 || R.ldT % 2 != 0 || !aligned16(R.ty) || !aligned16(R.tW) || !aligned16(R.T) ||
            !aligned16(R.S0))
            return false;
    }
    const WbFusedLayout L = wb_gram_fused_layout(k0, KT, f.ldp);
    return k0 + 2 <= 4 * WF_MAXKS && L.nP + L.nU + 1 <= 4 * WF_MAXQ_P && L.nO <= 4 * WF_MAXQ_O && L.RS <= 64 && k0 * (k0 + 1) / 2 <= 256 * WF_PSUM &&
           sizeof(double) * (size_t)L.total <= 160 * 1024;
}

int launch_wb_gram_fused(hipStream_t st, const AssembleArgs& a, const WbFusedArgs& f, int nrho, int variants) {
    if (variants <= 0) return CRM_OK;
    if (!wb_gram_fused_serves(a, f, nrho)) {
        set_error("fused unrelated-donor Gram: k0=%d, c=%d outside the supported range", a.k0, a.c);
        return CRM_ERR_INTERNAL;
    }
    const int KT = a.k0 + a.c + 2 + a.wb_k1, ts = (KT + 15) / 16;
    const WbFusedLayout L = wb_gram_fused_layout(a.k0, KT, f.ldp);
    const size_t lds = sizeof(double) * (size_t)L.total;
    const bool strips = form("gram_strips", 1) != 0;
    const bool spread = strips && form("wb_gram_spread", 1) != 0;     // (the round-robin deal keeps its pieces in a bunch)
    // (the limit is raised whatever the size: 79 KB at k0 = 50)
    auto fused = [&](auto ntl) {
        constexpr int NTL = decltype(ntl)::value;
        if (spread) return launch_with_lds(wb_gram_fused_kernel<NTL, true, true>, dim3(variants), dim3(256), lds, st, true, a, f, L, KT);
        return strips ? launch_with_lds(wb_gram_fused_kernel<NTL, true, false>, dim3(variants), dim3(256), lds, st, true, a, f, L, KT)
                      : launch_with_lds(wb_gram_fused_kernel<NTL, false, false>, dim3(variants), dim3(256), lds, st, true, a, f, L, KT);
    };
    if (ts == 5) CRM_HIP(fused(std::integral_constant<int, 5>{}));
    else if (ts == 6) CRM_HIP(fused(std::integral_constant<int, 6>{}));
    else if (ts == 7) CRM_HIP(fused(std::integral_constant<int, 7>{}));   // (config 3: 50 + 3 + 50 rows)
    else CRM_HIP(fused(std::integral_constant<int, 8>{}));
    return CRM_OK;
}

}  // namespace crm
