// The Gram of many columns over a long axis, and the packed factorisation behind it, for the 256-thread workgroups that
// evaluate a likelihood with more columns than registers hold (nullfit_wide.hip, nullfit_xwide.hip, effects_multi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace crm {

// KT x KT Gram of scaled rows in TS x TS register tiles (16 x 16 threads), CH positions per staging step (32 or 64).
// `scale(start, q, lpart)` (called by the threads q < CH for the positions start + q < len) gives the factor of position
// start + q and may add that position's logarithm to lpart; `value(row, position)` gives the unscaled entry (not read where
// the factor is zero).  by_row: consecutive threads stage consecutive positions of one row (spectrum rows are contiguous);
// else consecutive rows of one position (cell-axis operands are row-major).  `sink(row, col, v)` gets every entry from the
// thread that holds it.  Positions are added one by one inside a step and step by step.
// Where the factor of a position is zero, `value` is not called and a zero is staged: the same as the product for finite
// entries (an accumulator that starts at +0 never becomes -0), but not for a non-finite entry or a non-finite D behind the
// factor, where a product would stage a NaN and this stages 0.  Beyond `len` the factor is zero by construction.
// LDS: S [16 TS][CH + 1], sd [CH]; red [256] and scal [8] for the sum of the logarithms, which is returned (thread 0 adds
// the CH partial sums in ascending order; scal[1] carries it) -- red = null: no logarithms, no sum, 0 is returned.
template <int TS, int CH, class Len, class Scale, class Value, class Sink>
__device__ inline double gram_tiles(double* S, double* sd, double* red, double* scal, int KT, Len len, bool by_row,
                                    Scale&& scale, Value&& value, Sink&& sink) {
    const int tid = threadIdx.x;
    const int ti = tid >> 4, tj = tid & 15;
    double acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.0;
    double lpart = 0.0;
    constexpr int UNR = CH / 16;   // (2 at 32 positions per step, 4 at 64)
    for (Len c0 = 0; c0 < len; c0 += CH) {
        if (tid < CH) sd[tid] = c0 + tid < len ? scale(c0, tid, lpart) : 0.0;
        __syncthreads();
        for (int e = tid; e < 16 * TS * CH; e += 256) {
            int row, q;
            if (by_row) { row = e / CH; q = e - row * CH; }
            else { q = e / (16 * TS); row = e - q * (16 * TS); }
            double v = 0.0;
            if (row < KT && c0 + q < len && sd[q] != 0.0) v = value(row, c0 + q) * sd[q];
            S[row * (CH + 1) + q] = v;
        }
        __syncthreads();
#pragma unroll UNR
        for (int q = 0; q < CH; q++) {
            double x[TS], y[TS];
#pragma unroll
            for (int i = 0; i < TS; i++) {
                x[i] = S[(ti + 16 * i) * (CH + 1) + q];
                y[i] = S[(tj + 16 * i) * (CH + 1) + q];
            }
#pragma unroll
            for (int i = 0; i < TS; i++)
#pragma unroll
                for (int j = 0; j < TS; j++) acc[i][j] += x[i] * y[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TS; i++) {
        const int row = ti + 16 * i;
#pragma unroll
        for (int j = 0; j < TS; j++) {
            const int col = tj + 16 * j;
            if (row < KT && col < KT) sink(row, col, acc[i][j]);
        }
    }
    if (!red) return 0.0;
    red[tid] = lpart;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < CH; i++) s += red[i];
        scal[1] = s;
    }
    __syncthreads();
    return scal[1];
}

// The upper triangle of NTL x NTL 16 x 16 MFMA tiles dealt to four wavefronts in strips (gram_ext_dma_wide_kernel,
// wb_gram_fused_kernel; form "gram_strips").  A tile (i, j), i <= j, takes tile row i as its A operand and the weighted
// tile row j as its B operand.  A role owns whole columns j of the triangle where the balance allows, so that a k-step
// forms one weighted fragment per column it owns (one or two, three in one role at NTL 9) and reads every operand row
// once, whichever of the role's tiles use it.  No role holds more than ceil(tiles / 4) tiles, the bound of the
// round-robin deal, so the accumulators take the registers they took.
struct StripSeg { int j, i0, i1; };     // the tiles (i0 .. i1 - 1, j)
struct StripDeal {
    static constexpr int MAXN = 12;     // (NTL 9: 45 tiles)
    int ntl;
    int n[4];
    int ti[4][MAXN], tj[4][MAXN];
    // is tile row `row` read by role w as a B operand / at all; the last tile of w that takes it as its A operand (-1: none)
    constexpr bool is_b(int w, int row) const {
        for (int t = 0; t < n[w]; t++)
            if (tj[w][t] == row) return true;
        return false;
    }
    constexpr int last_a(int w, int row) const {
        int last = -1;
        for (int t = 0; t < n[w]; t++)
            if (ti[w][t] == row) last = t;
        return last;
    }
    constexpr bool reads(int w, int row) const { return is_b(w, row) || last_a(w, row) >= 0; }
    // every tile of the triangle exactly once, no role above the round-robin bound
    constexpr bool valid() const {
        const int maxt = (ntl * (ntl + 1) / 2 + 3) / 4;
        for (int w = 0; w < 4; w++)
            if (n[w] < 1 || n[w] > maxt) return false;
        for (int i = 0; i < ntl; i++)
            for (int j = i; j < ntl; j++) {
                int seen = 0;
                for (int w = 0; w < 4; w++)
                    for (int t = 0; t < n[w]; t++) seen += ti[w][t] == i && tj[w][t] == j;
                if (seen != 1) return false;
            }
        int total = 0;
        for (int w = 0; w < 4; w++) total += n[w];
        return total == ntl * (ntl + 1) / 2;
    }
};
constexpr StripDeal make_strip_deal(int ntl, const StripSeg (&segs)[4][3]) {
    StripDeal d{};
    d.ntl = ntl;
    for (int w = 0; w < 4; w++)
        for (int s = 0; s < 3; s++)
            for (int i = segs[w][s].i0; i < segs[w][s].i1; i++) {
                d.ti[w][d.n[w]] = i;
                d.tj[w][d.n[w]] = segs[w][s].j;
                d.n[w]++;
            }
    return d;
}
template <int NTL> inline constexpr StripDeal kStripDeal = {};
// 15 tiles, 4 + 4 + 4 + 3: column 4 is cut above its diagonal tile
template <> inline constexpr StripDeal kStripDeal<5> =
    make_strip_deal(5, {{{4, 0, 4}, {}, {}}, {{3, 0, 4}, {}, {}}, {{2, 0, 3}, {0, 0, 1}, {}}, {{1, 0, 2}, {4, 4, 5}, {}}});
// 21 tiles, 6 + 5 + 5 + 5
template <> inline constexpr StripDeal kStripDeal<6> =
    make_strip_deal(6, {{{5, 0, 6}, {}, {}}, {{4, 0, 5}, {}, {}}, {{3, 0, 4}, {0, 0, 1}, {}}, {{2, 0, 3}, {1, 0, 2}, {}}});
// 28 tiles, 7 each: {6}, {5, 0}, {4, 1}, {3, 2}
template <> inline constexpr StripDeal kStripDeal<7> =
    make_strip_deal(7, {{{6, 0, 7}, {}, {}}, {{5, 0, 6}, {0, 0, 1}, {}}, {{4, 0, 5}, {1, 0, 2}, {}}, {{3, 0, 4}, {2, 0, 3}, {}}});
// 36 tiles, 9 each: {7, 0}, {6, 1}, {5, 2}, {4, 3}
template <> inline constexpr StripDeal kStripDeal<8> =
    make_strip_deal(8, {{{7, 0, 8}, {0, 0, 1}, {}}, {{6, 0, 7}, {1, 0, 2}, {}}, {{5, 0, 6}, {2, 0, 3}, {}}, {{4, 0, 5}, {3, 0, 4}, {}}});
// 45 tiles, 12 + 11 + 11 + 11: {8, 1, 0}, {7, 2}, {6, 3}, {5, 4}
template <> inline constexpr StripDeal kStripDeal<9> =
    make_strip_deal(9, {{{8, 0, 9}, {1, 0, 2}, {0, 0, 1}}, {{7, 0, 8}, {2, 0, 3}, {}}, {{6, 0, 7}, {3, 0, 4}, {}}, {{5, 0, 6}, {4, 0, 5}, {}}});
static_assert(kStripDeal<5>.valid() && kStripDeal<6>.valid() && kStripDeal<7>.valid() && kStripDeal<8>.valid() && kStripDeal<9>.valid(),
              "a strip deal holds every tile of the upper triangle once and no role more than ceil(tiles / 4)");

// f(std::integral_constant<int, I>) for I = 0 .. N - 1: indices that stay constant expressions inside f
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Packed lower-triangular storage: entry (i, k), k <= i, and the row of entry e.
__device__ inline int tri(int i, int k) { return i * (i + 1) / 2 + k; }
__device__ inline int tri_row(int e) {
    int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while (tri(i + 1, 0) <= e) i++;
    while (tri(i, 0) > e) i--;
    return i;
}

// In-place Cholesky of the leading P x P block in packed lower storage, all threads.  false on a non-positive pivot.
// (static, not inline: whether a kernel inlines its calls stays the compiler's choice, call by call)
static __device__ bool packed_cholesky(double* H, int P, double* scal, double& logdet) {
    const int tid = threadIdx.x;
    logdet = 0.0;
    for (int j = 0; j < P; j++) {
        __syncthreads();
        if (tid == 0) {
            double d = H[tri(j, j)];
            for (int k = 0; k < j; k++) d -= H[tri(j, k)] * H[tri(j, k)];
            scal[0] = d;
        }
        __syncthreads();
        const double d = scal[0];
        if (!(d > 0.0)) return false;
        const double l = sqrt(d);
        logdet += 2.0 * log(l);
        for (int i = j + 1 + tid; i < P; i += blockDim.x) {
            double s = H[tri(i, j)];
            for (int k = 0; k < j; k++) s -= H[tri(i, k)] * H[tri(j, k)];
            H[tri(i, j)] = s / l;
        }
        if (tid == 0) H[tri(j, j)] = l;
        __syncthreads();
    }
    return true;
}

}  // namespace crm
