// The Gram of the score statistic's operand rows over the spectrum (assemble.hip has the formulas it serves):
//     Gext = S S',   S = sqrt(d) o [A~ rows ; Q0'W ; Q0'g ; Q0'y ; (unrelated-donor form) R],   d_j = s / (1 + s), s = (v0 / v1) S0_j
// per variant, KT x KT, both triangles, on the FP64 MFMA in 16 x 16 tiles of the upper triangle.  Three kernels behind
// launch_gram_ext:
//   gram_ext_dma_kernel       up to 64 rows: direct-to-LDS loads, every wavefront keeps every tile over a quarter of the columns
//   gram_ext_dma_wide_kernel  65 to 144 rows: direct-to-LDS loads, the tiles dealt to the wavefronts (in strips, or round-robin)
//   gram_ext_kernel           any row count, any alignment: rows staged through registers, scaled on the way in (past 144
//                             rows in two or four workgroups per variant); the reference the other two are tested against
// What they share with each other and with wb_gram_fused.hip -- row pointers, weights, tile deal, store -- is gram_common.h;
// the inner loops are each kernel's own (tuned one by one, and different on purpose).
#include <type_traits>

#include "assemble.h"
#include "gram_common.h"

namespace crm {

namespace {

constexpr int CH = 64;   // spectrum entries staged per step
constexpr int SLD = 66;  // LDS row length: 16 rows x 2 columns of a fragment read land on 32 distinct bank pairs

// S S' with S = sqrt(d) o [A~ rows ; Q0'W ; Q0'g ; Q0'y] (KT x r) on the FP64 matrix pipe.  One
// workgroup per variant; S is staged through LDS in chunks of 64 spectrum entries (scaled on the way
// in, next chunk prefetched into registers during the MFMAs).  Only the upper triangle of 16x16
// output tiles is computed; the tiles are dealt round-robin to the four wavefronts, rotated by the
// block index so that the SIMDs of a CU see the same load.  NG > 1 (more than 144 rows: the slower form for many contexts +
// covariates): NG workgroups per variant, workgroup g of them takes the tiles g, g + NG, ... of the list -- every one
// stages all rows, the accumulators of a wavefront stay within its registers.
template <int NTL, int NG = 1>
__global__ __launch_bounds__(256) void gram_ext_kernel(AssembleArgs a, double* __restrict__ Gext, int KT) {
    constexpr int ROWS = 16 * NTL, NTILES = NTL * (NTL + 1) / 2, NLOC = (NTILES + NG - 1) / NG, MAXT = (NLOC + 3) / 4,
                  RPT = ROWS / 4;
    extern __shared__ double Ss[];  // [ROWS][SLD]
    __shared__ int tile_ij[NTILES];
    __shared__ const double* tail_ptr[ROWS];   // (rows past k0: KT - k0 <= ROWS)
    const int b = blockIdx.x;
    const GramVariant V = gram_variant(a, b);
    const AssembleRho& R = V.R;
    const int r = R.r;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int k0 = a.k0;

    for (int e = tid; e < NTILES; e += 256) tile_ij[e] = gram_tile_of<NTL>(e);
    for (int t = tid; t < KT - k0; t += 256) tail_ptr[t] = gram_other_row(a, R, b, t);
    __syncthreads();
    // tiles of this wavefront: the entries first, first + 4, ... of this workgroup's list (MAXT or MAXT - 1 of them)
    const int grp = NG > 1 ? (int)blockIdx.y : 0;
    const int first = gram_wave_first(wave, b);
    const int nloc = (NTILES - grp + NG - 1) / NG;
    const int ntw = (nloc - first + 3) / 4;
    int t_i[MAXT], t_j[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; t++) {
        const int idx = grp + NG * (first + 4 * t);
        const int ij = tile_ij[idx < NTILES ? idx : 0];
        t_i[t] = ((ij & 255) * 16 + l15) * SLD + lq;
        t_j[t] = ((ij >> 8) * 16 + l15) * SLD + lq;
    }
    v4d acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; t++) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

    const int cc = lane;          // column of the chunk this thread stages
    auto fetch = [&](int c0, double (&v)[RPT]) __attribute__((always_inline)) {
        const int j = c0 + cc;
        const bool okj = j < r;
        double sdv = 0.0;
        if (okj) sdv = sqrt(gram_weight_fma(V.ratio, R.S0[j]));
#pragma unroll
        for (int i = 0; i < RPT; i++) {
            const int row = wave + 4 * i;
            double x = 0.0;
            if (okj && row < KT) {
                const double* __restrict__ p = row < k0 ? V.Arows + (long)row * V.a_stride : tail_ptr[row - k0];
                x = p[j];
            }
            v[i] = x * sdv;
        }
    };
    auto stash = [&](const double (&v)[RPT]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < RPT; i++) Ss[(wave + 4 * i) * SLD + cc] = v[i];
    };
    // MFMAs of one staged chunk for NT tiles; operand fragments are read one k-step ahead
    auto chunk_mma = [&](auto nt_tag) __attribute__((always_inline)) {
        constexpr int NT = decltype(nt_tag)::value;
        if constexpr (NT > 0) {
            double fa[2][NT], fb[2][NT];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                fa[0][t] = Ss[t_i[t]];
                fb[0][t] = Ss[t_j[t]];
            }
#pragma unroll
            for (int ks = 0; ks < CH / 4; ks++) {
                const int cur = ks & 1, nx = cur ^ 1;
                if (ks + 1 < CH / 4) {
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        fa[nx][t] = Ss[t_i[t] + 4 * (ks + 1)];
                        fb[nx][t] = Ss[t_j[t] + 4 * (ks + 1)];
                    }
                }
#pragma unroll
                for (int t = 0; t < NT; t++)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][t], fb[cur][t], acc[t], 0, 0, 0);
            }
        }
    };

    // chunk ch sits in LDS while chunk ch + 1 is in registers / in flight: the kernel streams 8 (KT r) bytes per variant and
    // needs the loads outstanding during the MFMAs  (measured: two chunks ahead costs occupancy, 146 VGPRs, and gains nothing)
    const int nchunks = (r + CH - 1) / CH;
    double bA[RPT];
    fetch(0, bA);
    stash(bA);
    __syncthreads();
    fetch(CH, bA);
    for (int ch = 0; ch < nchunks; ch++) {
        if (ntw == MAXT) chunk_mma(std::integral_constant<int, MAXT>{});
        else chunk_mma(std::integral_constant<int, MAXT - 1>{});
        __syncthreads();
        if (ch + 1 < nchunks) {
            stash(bA);
            __syncthreads();
            fetch((ch + 2) * CH, bA);
        }
    }
    double* __restrict__ out = Gext + (long)b * KT * KT;
#pragma unroll
    for (int t = 0; t < MAXT; t++) {
        const int idx = grp + NG * (first + 4 * t);
        if (idx < NTILES) gram_store_tile(out, KT, tile_ij[idx], acc[t], lq, l15);
    }
}

// The same Gram with the operand rows brought in by direct-to-LDS loads (global_load_lds_dwordx4), for 16 NTL rows
// with NTL even.  The staged kernel above spends a third of its issue slots on the way into LDS -- per chunk and
// thread sixteen 8-byte loads with 64-bit address arithmetic, a square root and a division for sqrt(d_j), sixteen
// products and sixteen ds_write -- none of which can overlap an FP64 MFMA, and two barriers per chunk.  Here a
// wave-instruction carries two rows of a chunk (lanes 0-31 row q, lanes 32-63 row q + ROWS/2, 64 columns each) straight
// into LDS, two buffers deep, one barrier per chunk; the spectrum weights go in as d_j (not sqrt d_j) on ONE operand,
// a product per fragment read:  S S' = sum_j a_ij d_j a_i'j.  LDS image: instruction q at q * 130 doubles (its two
// rows 64 doubles apart), so the sixteen rows of a fragment read start two 8-byte slots apart -- conflict-free like the
// 66-double rows of the staged kernel.  A last, partial chunk is loaded through registers with per-element guards.
constexpr int GRAM_QLD = 130;   // doubles per DMA instruction slot: 1 KB of operand rows + 2 of padding (both kernels)
// dynamic LDS of gram_ext_dma_kernel<NTL>, in doubles: two chunk buffers of 8 NTL instruction slots, d [2][CH]
constexpr int gram_dma_lds_doubles(int ntl) { return 2 * (8 * ntl) * GRAM_QLD + 2 * CH; }

template <int NTL>
__global__ __launch_bounds__(256) void gram_ext_dma_kernel(AssembleArgs a, double* __restrict__ Gext, int KT) {
    static_assert(NTL % 2 == 0, "row pairs of one DMA instruction must fall into different 16-row tiles");
    constexpr int ROWS = 16 * NTL, HALF = ROWS / 2, NTILES = NTL * (NTL + 1) / 2;
    constexpr int QLD = GRAM_QLD;            // doubles per DMA instruction slot (2 x 64 + 2 of padding)
    constexpr int BUF = HALF * QLD;          // doubles per chunk buffer
    static_assert(gram_dma_lds_doubles(NTL) == 2 * BUF + 2 * CH, "the launch allocates what the kernel lays out");
    constexpr int IPW = HALF / 4;            // DMA instructions per wavefront and chunk
    constexpr int KSW = CH / 16;             // k-steps per wavefront and chunk (the four wavefronts split the chunk's columns)
    static_assert(2 * BUF >= 2 * NTILES * 256, "the accumulators of two wavefronts must fit the chunk buffers");
    extern __shared__ double Ss[];           // [2][BUF] + d [2][64]
    double* const dS = Ss + 2 * BUF;
    const int b = blockIdx.x;
    const GramVariant V = gram_variant(a, b);
    const AssembleRho& R = V.R;
    const int r = R.r;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;

    auto row_ptr = [&](int row) { return gram_row(a, V, b, KT, row); };
    auto row_off = [](int row) { return row < HALF ? row * QLD : (row - HALF) * QLD + 64; };
    // this lane's source addresses (column pair 2 * (lane & 31) of the row its half-wave carries)
    const double* src[IPW];
#pragma unroll
    for (int q = 0; q < IPW; q++) {
        const int inst = wave + 4 * q;
        src[q] = row_ptr(inst + (lane >> 5) * HALF) + 2 * (lane & 31);
    }
    // Every wavefront accumulates ALL upper-triangle tiles over its quarter of the columns of each chunk (an even
    // split whatever the tile count; the fragment of a 16-row block serves as the A operand and, times d_j, as the B
    // operand of every tile that touches the block: NTL reads and NTL products per k-step for NTILES MFMAs); the four
    // partial sums meet through LDS once per variant, in a fixed order.
    int f_off[NTL];
#pragma unroll
    for (int t = 0; t < NTL; t++) f_off[t] = row_off(16 * t + l15) + 4 * KSW * wave + lq;
    v4d acc[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; t++) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

    const int nfull = r / CH, nchunks = (r + CH - 1) / CH;
    auto weights = [&](int ch, int buf) __attribute__((always_inline)) {   // d_j of chunk ch (wavefront 0)
        if (wave == 0) {
            const int j = ch * CH + lane;
            double d = 0.0;
            if (j < r) d = gram_weight_fma(V.ratio, R.S0[j]);
            dS[buf * CH + lane] = d;
        }
    };
    auto issue = [&](int ch, int buf) __attribute__((always_inline)) {
        if (ch < nfull) {
#pragma unroll
            for (int q = 0; q < IPW; q++)
                gram_dma16(src[q] + (long)ch * CH, Ss + buf * BUF + (wave + 4 * q) * QLD);
        } else {   // the partial chunk: guarded element loads, zeros past r
            for (int e = tid; e < ROWS * CH; e += 256) {
                const int row = e / CH, col = e - row * CH;
                const int j = ch * CH + col;
                Ss[buf * BUF + row_off(row) + col] = (j < r && row < KT) ? row_ptr(row)[j] : 0.0;
            }
        }
    };
    auto chunk_mma = [&](int buf) __attribute__((always_inline)) {
        const double* __restrict__ S = Ss + buf * BUF;
        const double* __restrict__ D = dS + buf * CH + 4 * KSW * wave + lq;
        double fa[2][NTL], fb[2][NTL];
        {
            const double dk = D[0];
#pragma unroll
            for (int t = 0; t < NTL; t++) {
                fa[0][t] = S[f_off[t]];
                fb[0][t] = fa[0][t] * dk;
            }
        }
#pragma unroll
        for (int ks = 0; ks < KSW; ks++) {
            const int cur = ks & 1, nx = cur ^ 1;
            if (ks + 1 < KSW) {
                const double dk = D[4 * (ks + 1)];
#pragma unroll
                for (int t = 0; t < NTL; t++) {
                    fa[nx][t] = S[f_off[t] + 4 * (ks + 1)];
                    fb[nx][t] = fa[nx][t] * dk;
                }
            }
            int idx = 0;
#pragma unroll
            for (int ti = 0; ti < NTL; ti++)
#pragma unroll
                for (int tj = ti; tj < NTL; tj++, idx++)
                    acc[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][ti], fb[cur][tj], acc[idx], 0, 0, 0);
        }
    };
    issue(0, 0);
    weights(0, 0);
    __syncthreads();   // (drains the LDS-DMA: vmcnt(0) precedes the barrier)
    for (int ch = 0; ch < nchunks; ch++) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) {
            issue(ch + 1, buf ^ 1);
            weights(ch + 1, buf ^ 1);
        }
        chunk_mma(buf);
        __syncthreads();
    }
    // (wave 0 + wave 2) + (wave 1 + wave 3): two exchanges through the chunk buffers
    double* const red = Ss + (wave & 1) * NTILES * 256;
    if (wave >= 2) {
#pragma unroll
        for (int t = 0; t < NTILES; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) red[(t * 4 + reg) * 64 + lane] = acc[t][reg];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int t = 0; t < NTILES; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) acc[t][reg] += red[(t * 4 + reg) * 64 + lane];
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
        for (int t = 0; t < NTILES; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) red[(t * 4 + reg) * 64 + lane] = acc[t][reg];
    }
    __syncthreads();
    if (wave != 0) return;
    double* __restrict__ out = Gext + (long)b * KT * KT;
    int idx = 0;
#pragma unroll
    for (int ti = 0; ti < NTL; ti++) {
#pragma unroll
        for (int tj = ti; tj < NTL; tj++, idx++) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                gram_store_entry(out, KT, ti | (tj << 8), reg, acc[idx][reg] + (Ss + NTILES * 256)[(idx * 4 + reg) * 64 + lane], lq, l15);
        }
    }
}

// The direct-to-LDS Gram for 5 to 9 tile rows (65-144 rows).  Keeping every tile in every wavefront, as the kernel above
// does, would take 426 registers at 6 tile rows; here the upper-triangle tiles are dealt to the four wavefronts as in the
// staged kernel (7 of 28 at 7 tile rows, a wavefront's tiles over all columns: no reduction at the end), which leaves
// room for two wavefronts per SIMD up to 8 tile rows.  Chunks of 32 spectrum entries, so that two buffers of 128 rows
// (65 KB) fit a CU twice.  A wave-instruction carries row q of four consecutive 16-row tiles (sixteen lanes each); LDS
// image: instruction slot (16 * (tile / 4) + row in tile) at 130 doubles, the four tiles 32 doubles apart -- the sixteen
// rows of a fragment read again start two 8-byte slots apart.  Tile rows are loaded in fours (rows past KT read row 0),
// only the NTL (NTL + 1) / 2 tiles that exist are computed.
// What is left on the table: every chunk ends in a __syncthreads(), which waits for the next chunk's DMA -- the loads
// overlap the MFMAs of one chunk, no more (a third buffer with a counted vmcnt and a raw barrier was not tried); and the
// tile rows loaded past KT are re-reads of row 0 (at 103 rows 25 of 128, a quarter of the DMA instructions' traffic).
constexpr int GRAM_WCH = 32;    // spectrum entries per chunk of gram_ext_dma_wide_kernel
// dynamic LDS of gram_ext_dma_wide_kernel<NTL>, in doubles: two chunk buffers of 16 ceil(NTL / 4) instruction slots,
// d [2][GRAM_WCH], S0 as loaded [2][GRAM_WCH]
constexpr int gram_dma_wide_lds_doubles(int ntl) { return 2 * (16 * ((ntl + 3) / 4)) * GRAM_QLD + 4 * GRAM_WCH; }

// STRIPS (form "gram_strips", the default): the tiles are dealt in strips (tile_gram.h: kStripDeal), a k-step reads every
// operand tile row of the wavefront's role once and weights one fragment per column of the role; false: the round-robin
// deal with two reads and a product per tile.  Every accumulator receives the same operands in the same order either way.
template <int NTL, bool STRIPS>
__global__ __launch_bounds__(256, NTL <= 8 ? 2 : 1) void gram_ext_dma_wide_kernel(AssembleArgs a, double* __restrict__ Gext,
                                                                                  int KT) {
    constexpr int WCH = GRAM_WCH;                  // spectrum entries per chunk
    constexpr int SLOTS = 16 * ((NTL + 3) / 4);    // DMA instructions per chunk
    constexpr int NTILES = NTL * (NTL + 1) / 2, MAXT = (NTILES + 3) / 4;
    constexpr int QLD = GRAM_QLD;                  // doubles per DMA instruction slot (4 x 32 + 2 of padding)
    constexpr int BUF = SLOTS * QLD;               // doubles per chunk buffer
    static_assert(gram_dma_wide_lds_doubles(NTL) == 2 * BUF + 4 * WCH, "the launch allocates what the kernel lays out");
    constexpr int IPW = SLOTS / 4;                 // DMA instructions per wavefront and chunk
    extern __shared__ double Ss[];                 // [2][BUF] + d [2][WCH] + S0 [2][WCH]
    double* const dS = Ss + 2 * BUF;
    const int b = blockIdx.x;
    const GramVariant V = gram_variant(a, b);
    const AssembleRho& R = V.R;
    const int r = R.r;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;

    auto row_ptr = [&](int row) { return gram_row(a, V, b, KT, row); };
    auto row_off = [](int row) { return (16 * (row >> 6) + (row & 15)) * QLD + ((row >> 4) & 3) * WCH; };
    // this lane's source addresses (column pair 2 * (lane & 15) of the row its sixteen lanes carry)
    const double* src[IPW];
#pragma unroll
    for (int q = 0; q < IPW; q++) {
        const int slot = wave + 4 * q;
        src[q] = row_ptr(64 * (slot >> 4) + 16 * lq + (slot & 15)) + 2 * l15;
    }
    // tiles of this wavefront (gram_common.h), MAXT or fewer of them.  Round-robin: listed here, for the fragment offsets;
    // strips: the fragments of tile row i start at row_off(16 i + l15) + lq, a constant past the lane's own part, and the
    // list is made behind the loop, for the store alone
    const int first = gram_wave_first(wave, b);
    const int ntw = gram_wave_ntiles<NTL, STRIPS>(first);
    int t_i[MAXT], t_j[MAXT], t_ij[MAXT];
    if constexpr (!STRIPS) {
        gram_wave_tiles<NTL, false>(first, t_ij);
#pragma unroll
        for (int t = 0; t < MAXT; t++) {
            t_i[t] = row_off(16 * (t_ij[t] & 255) + l15) + lq;
            t_j[t] = row_off(16 * (t_ij[t] >> 8) + l15) + lq;
        }
    }
    v4d acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; t++) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

    const int nfull = r / WCH, nchunks = (r + WCH - 1) / WCH;
    // d_j of a chunk (wavefront 0).  An ordinary load of S0 inside the loop would make the compiler wait for every LDS-DMA
    // in flight where its result is first touched, so S0 comes in by LDS-DMA as well: 64 lanes x 4 bytes two chunks
    // ahead (lanes past r re-read entry r - 1), turned into d_j one chunk ahead, a barrier after each step.
    double* const sS = dS + 2 * WCH;               // S0 as loaded [2][WCH]
    auto issue_s0 = [&](int ch) __attribute__((always_inline)) {
        if (wave == 0 && ch < nchunks) {
            const int j = ch * WCH + (lane >> 1);
            gram_dma4(reinterpret_cast<const float*>(R.S0 + (j < r ? j : r - 1)) + (lane & 1), sS + (ch & 1) * WCH);
        }
    };
    auto weights = [&](int ch, double s0) __attribute__((always_inline)) {
        dS[(ch & 1) * WCH + lane] = gram_weight(V.ratio, s0, ch * WCH + lane < r);
    };
    auto issue = [&](int ch, int buf) __attribute__((always_inline)) {
        if (ch < nfull) {
#pragma unroll
            for (int q = 0; q < IPW; q++)
                gram_dma16(src[q] + (long)ch * WCH, Ss + buf * BUF + (wave + 4 * q) * QLD);
        } else {   // the partial chunk: guarded element loads, zeros past r
            for (int e = tid; e < 16 * NTL * WCH; e += 256) {
                const int row = e / WCH, col = e - row * WCH;
                const int j = ch * WCH + col;
                Ss[buf * BUF + row_off(row) + col] = (j < r && row < KT) ? row_ptr(row)[j] : 0.0;
            }
        }
    };
    // MFMAs of one chunk for NT tiles; operand fragments are read one k-step ahead, the weight goes onto the B operand
    auto chunk_mma = [&](int buf, auto nt_tag) __attribute__((always_inline)) {
        constexpr int NT = decltype(nt_tag)::value;
        const double* __restrict__ S = Ss + buf * BUF;
        const double* __restrict__ D = dS + buf * WCH + lq;
        double fa[2][NT], fb[2][NT];
        {
            const double dk = D[0];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                fa[0][t] = S[t_i[t]];
                fb[0][t] = S[t_j[t]] * dk;
            }
        }
#pragma unroll
        for (int ks = 0; ks < WCH / 4; ks++) {
            const int cur = ks & 1, nx = cur ^ 1;
            if (ks + 1 < WCH / 4) {
                const double dk = D[4 * (ks + 1)];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    fa[nx][t] = S[t_i[t] + 4 * (ks + 1)];
                    fb[nx][t] = S[t_j[t] + 4 * (ks + 1)] * dk;
                }
            }
#pragma unroll
            for (int t = 0; t < NT; t++)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][t], fb[cur][t], acc[t], 0, 0, 0);
        }
    };
    // one role of the strip deal: two sets of row fragments and of weighted fragments, read one k-step ahead
    auto chunk_mma_strips = [&](int buf, auto role_tag) __attribute__((always_inline)) {
        constexpr int ROLE = decltype(role_tag)::value;
        constexpr int NT = kStripDeal<NTL>.n[ROLE];
        const double* __restrict__ S = Ss + buf * BUF + l15 * QLD + lq;
        const double* __restrict__ D = dS + buf * WCH + lq;
        double fr[2][NTL], fw[2][NTL];
        auto fragments = [&](int set, int ks) __attribute__((always_inline)) {
            const double dk = D[4 * ks];
            static_for<0, NTL>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (kStripDeal<NTL>.reads(ROLE, i)) {
                    fr[set][i] = S[16 * (i >> 2) * QLD + (i & 3) * WCH + 4 * ks];
                    if constexpr (kStripDeal<NTL>.is_b(ROLE, i)) fw[set][i] = fr[set][i] * dk;
                }
            });
        };
        fragments(0, 0);
        static_for<0, WCH / 4>([&](auto kc) {
            constexpr int ks = decltype(kc)::value, cur = ks & 1;
            if constexpr (ks + 1 < WCH / 4) fragments(cur ^ 1, ks + 1);
            static_for<0, NT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[cur][kStripDeal<NTL>.ti[ROLE][t]], fw[cur][kStripDeal<NTL>.tj[ROLE][t]], acc[t], 0, 0, 0);
            });
        });
    };
    if (wave == 0 && lane < WCH) weights(0, lane < r ? R.S0[lane] : 0.0);
    issue_s0(1);
    issue(0, 0);
    __syncthreads();   // (drains the LDS-DMA: vmcnt(0) precedes the barrier)
    for (int ch = 0; ch < nchunks; ch++) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) {
            if (wave == 0 && lane < WCH) weights(ch + 1, sS[(buf ^ 1) * WCH + lane]);
            issue(ch + 1, buf ^ 1);
        }
        issue_s0(ch + 2);
        if constexpr (STRIPS) {
            if (first == 0) chunk_mma_strips(buf, std::integral_constant<int, 0>{});
            else if (first == 1) chunk_mma_strips(buf, std::integral_constant<int, 1>{});
            else if (first == 2) chunk_mma_strips(buf, std::integral_constant<int, 2>{});
            else chunk_mma_strips(buf, std::integral_constant<int, 3>{});
        } else {
            if (ntw == MAXT) chunk_mma(buf, std::integral_constant<int, MAXT>{});
            else chunk_mma(buf, std::integral_constant<int, MAXT - 1>{});
        }
        __syncthreads();
    }
    if constexpr (STRIPS) gram_wave_tiles<NTL, true>(first, t_ij);
    gram_store_tiles(Gext + (long)b * KT * KT, KT, t_ij, ntw, acc, lq, l15);
}

template <int N>
using int_c = std::integral_constant<int, N>;

}  // namespace

int launch_gram_ext(hipStream_t st, const AssembleArgs& a, int variants, double* Gext, int KT, bool* dma_served) {
    const int ts = (KT + 15) / 16;
    // LDS-DMA forms: 16-byte loads, so every row must start on a 16-byte boundary and hold an even number of doubles
    bool dma = ts <= 9 && a.ldA % 2 == 0 && (reinterpret_cast<uintptr_t>(a.A) & 15) == 0 && !form("gram_staged", 0);
    for (int i = 0; dma && i < CRM_MAX_RHO; i++) {
        const AssembleRho& R = a.rho[i];
        if (R.r <= 0 && !R.ty) continue;
        dma = R.ldW % 2 == 0 && R.ldT % 2 == 0 && ((reinterpret_cast<uintptr_t>(R.ty) | reinterpret_cast<uintptr_t>(R.tW) |
                                                    reinterpret_cast<uintptr_t>(R.T)) & 15) == 0;
    }
    if (a.wb_k1 > 0) dma = dma && a.wb_ldR % 2 == 0 && (reinterpret_cast<uintptr_t>(a.wb_R) & 15) == 0;
    *dma_served = dma;
    const bool strips = form("gram_strips", 1) != 0;
    const dim3 block(256);
    // every kernel asks for its LDS limit where it needs more than the 64 KB a kernel gets unasked; the grouped ones always
    auto narrow = [&](auto ntl) {
        constexpr int NTL = decltype(ntl)::value;
        const size_t lds = sizeof(double) * gram_dma_lds_doubles(NTL);
        return launch_with_lds(gram_ext_dma_kernel<NTL>, dim3(variants), block, lds, st, lds > 60 * 1024, a, Gext, KT);
    };
    auto wide = [&](auto ntl) {
        constexpr int NTL = decltype(ntl)::value;
        const size_t lds = sizeof(double) * gram_dma_wide_lds_doubles(NTL);
        return strips ? launch_with_lds(gram_ext_dma_wide_kernel<NTL, true>, dim3(variants), block, lds, st, lds > 60 * 1024, a, Gext, KT)
                      : launch_with_lds(gram_ext_dma_wide_kernel<NTL, false>, dim3(variants), block, lds, st, lds > 60 * 1024, a, Gext, KT);
    };
    auto staged = [&](auto ntl, auto ng) {
        constexpr int NTL = decltype(ntl)::value, NG = decltype(ng)::value;
        const size_t lds = sizeof(double) * 16 * NTL * SLD;
        return launch_with_lds(gram_ext_kernel<NTL, NG>, NG > 1 ? dim3(variants, NG) : dim3(variants), block, lds, st,
                               NG > 1 || lds > 60 * 1024, a, Gext, KT);
    };
    if (dma) {
        // (up to 4 tile rows every wavefront keeps every tile; past that the tiles are dealt to the wavefronts)
        if (ts <= 2) CRM_HIP(narrow(int_c<2>{}));
        else if (ts <= 4) CRM_HIP(narrow(int_c<4>{}));
        else if (ts == 5) CRM_HIP(wide(int_c<5>{}));
        else if (ts == 6) CRM_HIP(wide(int_c<6>{}));
        else if (ts == 7) CRM_HIP(wide(int_c<7>{}));   // (unrelated-donor form at config 3: 50 + 3 + 50 rows)
        else if (ts == 8) CRM_HIP(wide(int_c<8>{}));
        else CRM_HIP(wide(int_c<9>{}));
    } else if (ts <= 2) CRM_HIP(staged(int_c<2>{}, int_c<1>{}));
    else if (ts <= 4) CRM_HIP(staged(int_c<4>{}, int_c<1>{}));
    else if (ts <= 6) CRM_HIP(staged(int_c<6>{}, int_c<1>{}));
    else if (ts <= 7) CRM_HIP(staged(int_c<7>{}, int_c<1>{}));
    else if (ts <= 9) CRM_HIP(staged(int_c<9>{}, int_c<1>{}));
    else if (ts <= 12) CRM_HIP(staged(int_c<12>{}, int_c<2>{}));
    else if (ts <= 15) CRM_HIP(staged(int_c<15>{}, int_c<4>{}));
    else CRM_HIP(staged(int_c<18>{}, int_c<4>{}));
    return CRM_OK;
}

}  // namespace crm
