// The Gram of many columns over a long axis, and the packed factorisation behind it, for the 256-thread workgroups that
// evaluate a likelihood with more columns than registers hold (nullfit_wide.hip, nullfit_xwide.hip, effects_multi.hip).
#pragma once
#include <hip/hip_runtime.h>

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
