// What the four Gram kernels of the score statistic share around their inner MFMA loops (gram_ext.hip: gram_ext_kernel,
// gram_ext_dma_kernel, gram_ext_dma_wide_kernel; wb_gram_fused.hip: wb_gram_fused_kernel): where an operand row lives, the
// spectrum weight, the deal of the upper-triangle tiles to the four wavefronts, the store with its mirror and the LDS-DMA.
// The tests hold these kernels to each other bit for bit; what must be the same in all of them is stated here once.
// Device code only: every helper is inlined, with compile-time indices into the arrays it is handed (an array indexed at
// run time would go to scratch).
#pragma once
#include "assemble.h"
#include "tile_gram.h"
#include "wave_ops.h"

namespace crm {

// ---- operand rows ---------------------------------------------------------------------------------
// Row t past the k0 test-direction rows: the c rows Q0'W, Q0'g of variant b, Q0'y, then (unrelated-donor form) the E1 rows.
__device__ __forceinline__ const double* gram_other_row(const AssembleArgs& a, const AssembleRho& R, int b, int t) {
    const int c = a.c;
    if (t > c + 1) return a.wb_R + (long)(t - c - 2) * a.wb_ldR;
    return t < c ? R.tW + (long)t * R.ldW : (t == c ? R.T + (long)b * R.ldT : R.ty);
}

// What a workgroup of the launch_gram_ext kernels reads of its variant b before anything else.
struct GramVariant {
    AssembleRho R;           // the grid point of the variant's fit
    double ratio;            // v0 / v1
    const double* Arows;     // test-direction row i at Arows + i a_stride
    long a_stride;           // (no position in the sorted buffer: every row is the row of zeros)
};
__device__ __forceinline__ GramVariant gram_variant(const AssembleArgs& a, int b) {
    GramVariant v;
    const NullFitOut fit = a.fit[b];
    v.R = a.rho[fit.rho_index];
    v.ratio = fit.v0 / fit.v1;
    const long pos = a.sorted_pos[b];
    v.Arows = pos >= 0 ? a.A + pos * a.k0 * a.ldA : a.A_none;
    v.a_stride = pos >= 0 ? a.ldA : 0;
    return v;
}
// Row `row` of the KT operand rows, for the direct-to-LDS kernels, which load whole tile rows: rows past KT read row 0 (their
// outputs are never stored).
__device__ __forceinline__ const double* gram_row(const AssembleArgs& a, const GramVariant& v, int b, int KT, int row) {
    if (row >= KT) row = 0;
    return row < a.k0 ? v.Arows + (long)row * v.a_stride : gram_other_row(a, v.R, b, row - a.k0);
}

// ---- the spectrum weight d_j = s / (1 + s), s = (v0 / v1) S0_j --------------------------------------
// Two roundings of 1 + s exist, and each kernel keeps the one it has always had -- its results are its bits:
//   gram_weight      the product rounded on its own, then the sum: gram_ext_dma_wide_kernel and wb_gram_fused_kernel, which
//                    are held to each other bit for bit (tests/test_gpu_wb_gram_fused.py);
//   gram_weight_fma  1 + s as fma(ratio, S0_j, 1) -- what the compiler's contraction made of the staged kernel and of
//                    gram_ext_dma_kernel, which are held to each other (tests/test_gpu_pinned.py: test_gram_forms); the
//                    last bit of the denominator may differ from gram_weight's.
// Both are pinned here (no contraction left to the compiler), so a change of the surrounding code cannot move them.
// (on = false: a position past the spectrum's end, whose S0 is not one: weight 0)
__device__ __forceinline__ double gram_weight(double ratio, double s0, bool on = true) {
#pragma clang fp contract(off)
    const double s = on ? ratio * s0 : 0.0;
    return s / (1.0 + s);
}
__device__ __forceinline__ double gram_weight_fma(double ratio, double s0) {
#pragma clang fp contract(off)
    const double s = ratio * s0;
    return s / fma(ratio, s0, 1.0);
}

// ---- the deal of the NTL (NTL + 1) / 2 upper-triangle tiles ------------------------------------------
// A tile is kept as ti | tj << 8.  Entry e of the row-major upper triangle:
template <int NTL>
__device__ __forceinline__ int gram_tile_of(int e) {
    int ti = 0, rem = e;
    while (rem >= NTL - ti) { rem -= NTL - ti; ti++; }
    return ti | ((ti + rem) << 8);
}
// The place of a wavefront in the deal, rotated by the block index so that the SIMDs of a CU see the same load: under the
// round-robin deal it takes the entries first, first + 4, ...; under the strip deal `first` is its role of kStripDeal<NTL>.
__device__ __forceinline__ int gram_wave_first(int wave, int b) { return (wave + b) & 3; }
// how many tiles that is (MAXT = ceil(tiles / 4) or, round-robin, MAXT - 1 at the least)
template <int NTL, bool STRIPS>
__device__ __forceinline__ int gram_wave_ntiles(int first) {
    if constexpr (!STRIPS) return (NTL * (NTL + 1) / 2 - first + 3) / 4;
    else return first == 0 ? kStripDeal<NTL>.n[0] : first == 1 ? kStripDeal<NTL>.n[1] : first == 2 ? kStripDeal<NTL>.n[2] : kStripDeal<NTL>.n[3];
}
// and which, in the order of the wavefront's accumulators (entries past its count: tile (0, 0) round-robin, unused)
template <int NTL, bool STRIPS, int MAXT>
__device__ __forceinline__ void gram_wave_tiles(int first, int (&t_ij)[MAXT]) {
    static_for<0, MAXT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if constexpr (!STRIPS) {
            t_ij[t] = gram_tile_of<NTL>(first + 4 * t < NTL * (NTL + 1) / 2 ? first + 4 * t : 0);
        } else {
            constexpr int i0 = kStripDeal<NTL>.ti[0][t], i1 = kStripDeal<NTL>.ti[1][t], i2 = kStripDeal<NTL>.ti[2][t], i3 = kStripDeal<NTL>.ti[3][t];
            constexpr int j0 = kStripDeal<NTL>.tj[0][t], j1 = kStripDeal<NTL>.tj[1][t], j2 = kStripDeal<NTL>.tj[2][t], j3 = kStripDeal<NTL>.tj[3][t];
            t_ij[t] = (first == 0 ? i0 : first == 1 ? i1 : first == 2 ? i2 : i3) | ((first == 0 ? j0 : first == 1 ? j1 : first == 2 ? j2 : j3) << 8);
        }
    });
}

// ---- the store --------------------------------------------------------------------------------------
// Entry `reg` of a lane's four of a 16 x 16 accumulator tile ij (lane (l15, lq) holds rows lq + 4 reg, column l15) into the
// KT x KT matrix `out`, with its mirror below the diagonal; and the whole tile.
__device__ __forceinline__ void gram_store_entry(double* __restrict__ out, int KT, int ij, int reg, double v, int lq, int l15) {
    const int ri = (ij & 255) * 16, cj = (ij >> 8) * 16;
    const int row = ri + lq + 4 * reg, col = cj + l15;
    if (row < KT && col < KT) {
        out[(long)row * KT + col] = v;
        if (ri != cj) out[(long)col * KT + row] = v;
    }
}
__device__ __forceinline__ void gram_store_tile(double* __restrict__ out, int KT, int ij, const v4d& acc, int lq, int l15) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) gram_store_entry(out, KT, ij, reg, acc[reg], lq, l15);
}
// the first ntw tiles of a wavefront
template <int MAXT>
__device__ __forceinline__ void gram_store_tiles(double* __restrict__ out, int KT, const int (&t_ij)[MAXT], int ntw,
                                                 const v4d (&acc)[MAXT], int lq, int l15) {
#pragma unroll
    for (int t = 0; t < MAXT; t++)
        if (t < ntw) gram_store_tile(out, KT, t_ij[t], acc[t], lq, l15);
}

// ---- LDS-DMA ----------------------------------------------------------------------------------------
// global_load_lds: every lane brings 16 (4) bytes from its own address to the wave-uniform LDS address + 16 (4) lane.
// (__device__ functions: the builtin does not exist in the host pass, which would drop a kernel's host stub)
typedef const double __attribute__((address_space(1))) * gram_gptr_t;
typedef __attribute__((address_space(3))) void* gram_lptr_t;
__device__ __forceinline__ void gram_dma16(const double* src, double* lds_wave_uniform) {
    __builtin_amdgcn_global_load_lds((gram_gptr_t)src, (gram_lptr_t)lds_wave_uniform, 16, 0, 0);
}
__device__ __forceinline__ void gram_dma4(const float* src, double* lds_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const float __attribute__((address_space(1)))*)src, (gram_lptr_t)lds_wave_uniform, 4, 0, 0);
}

}  // namespace crm
