// Per-donor tables of the collapsed path (grouped panels): their kernels, the build, and the launchers of the two kernels
// the scan starts itself.
#include <algorithm>

#include "objects.h"

using namespace crm;

namespace crm {

// sums[d][q] over the cells of donor d: q = 0 count, 1 y, 2.. the covariate columns.  One workgroup per (donor, q):
// its threads stride over the cells and meet in a fixed order (the same bits whatever the launch).
__global__ __launch_bounds__(256) void donor_sums_kernel(const int* __restrict__ group, long cells, int m,
                                                         const double* __restrict__ yW, long ldw, int c,
                                                         double* __restrict__ sums) {
    __shared__ double part[256];
    const int d = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    double acc = 0.0;
    for (long i = tid; i < cells; i += 256)
        if (group[i] == d) acc += q == 0 ? 1.0 : yW[i * ldw + (q - 1)];
    part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) sums[d * DT_SUMS_LD + q] = part[0];
}

__global__ void permute_group_kernel(const int* __restrict__ group, const int* __restrict__ idx, long n,
                                     int* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = group[idx[i]];
}

// Z2[b, j] = sum_{d, d'} gamma_{d,b} gamma_{d',b} C[(d, d'), j]  with  C[(d, d'), :] = sum_i z'_d[i] z_d'[i] E[i, :]
// (test direction carried by the permuted indicators z', fixed effect by the unpermuted ones)
__global__ __launch_bounds__(128) void donor_cross_kernel(const double* __restrict__ Gam, long ld_gam, int m,
                                                           const double* __restrict__ C, long ldc, int k0,
                                                           double* __restrict__ Z2, long ldz2) {
    __shared__ double gam[BLOCK_SLACK_MAX > 256 ? 256 : BLOCK_SLACK_MAX];
    const int b = blockIdx.x;
    for (int d = threadIdx.x; d < m; d += blockDim.x) gam[d] = Gam[(long)d * ld_gam + b];
    __syncthreads();
    for (int j = threadIdx.x; j < k0; j += blockDim.x) {
        double acc = 0.0;
        for (int d = 0; d < m; d++) {
            const double gd = gam[d];
            if (gd == 0.0) continue;
            double inner = 0.0;
            const double* row = C + (long)d * m * ldc + j;
            for (int e = 0; e < m; e++) inner += gam[e] * row[(long)e * ldc];
            acc += gd * inner;
        }
        Z2[(long)b * ldz2 + j] = acc;
    }
}

// Per-donor tables of the collapsed path: every n-length contraction of the scan is linear in
// diag(g) (or diag(g)^2 = sum_d gamma_d^2 diag(z_d) for donor-constant g), so it is taken once per donor
// indicator z_d with the same kernels and afterwards combined with the donor dosages gamma.
int build_donor_tables(crm_gene* gene, const crm_panel* panel, crm_donor_tables* shared, const double* d_Ep,
                              const double* d_EE, const double* Zt, bool cross) {
    // shared != nullptr: also (re)build the phenotype-free tables (TZ, Bd, Z2, Z3) into *shared.
    // Zt: indicators of the test direction (rows permuted by idx_G, else the panel's own);
    // cross: Z2 becomes the m*m-row table of the mixed products z'_d o z_d'.
    crm_background* bg = gene->bg;
    crm_ctx* ctx = bg->ctx;
    hipStream_t st = ctx->stream;
    const long n = bg->n, np = bg->n_pad, ldq = bg->ldq;
    const int nrho = bg->nrho, c = gene->c, k0 = gene->k0;
    const long m = panel->m, mp = panel->m_pad;
    const int npair = k0 * (k0 + 1) / 2;
    const long ldZ1 = gene->ld_ye, ldZ2 = gene->ld_ep, ldZ3 = gene->ld_ee;
    const bool full = shared != nullptr;
    CRM_TRY(ctx->ws_probs.ensure(sizeof(GemmProblem) * (CRM_MAX_RHO + 4)));
    GemmProblem* d_probs = ctx->ws_probs.as<GemmProblem>();
    std::vector<GemmProblem> probs(CRM_MAX_RHO + 4);
    const double* Z = panel->Z.as<double>();
    if (full) CRM_TRY(crm_background_require_q0(bg, -1));   // the tables are contractions against every Q0(rho)
    if (full) {
        CRM_TRY(shared->TZ.ensure(sizeof(double) * (size_t)nrho * mp * ldq));
        CRM_TRY(shared->Bd.ensure(sizeof(double) * (size_t)nrho * mp * k0 * ldq));
        CRM_HIP(hipMemsetAsync(shared->TZ.ptr, 0, sizeof(double) * (size_t)nrho * mp * ldq, st));
        CRM_HIP(hipMemsetAsync(shared->Bd.ptr, 0, sizeof(double) * (size_t)nrho * mp * k0 * ldq, st));
        for (int i = 0; i < nrho; i++) {
            GemmProblem p{};
            p.X = Z; p.ldx = panel->ldz; p.Y = bg->Q0[i].as<double>(); p.ldy = ldq;
            p.C = shared->TZ.as<double>() + (size_t)i * mp * ldq; p.ldc = ldq;
            p.M = (int)m; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            probs[i] = p;
        }
        CRM_HIP(hipMemcpyAsync(d_probs, probs.data(), sizeof(GemmProblem) * nrho, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, nrho, (int)m, (int)ldq, np, false, 0, 1, 0));
        CRM_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < nrho; i++) {
            GemmProblem p{};
            p.X = Zt; p.ldx = panel->ldz; p.E = d_Ep; p.lde = gene->ld_ep; p.k0 = k0;
            p.Y = bg->Q0[i].as<double>(); p.ldy = ldq;
            p.C = shared->Bd.as<double>() + (size_t)i * mp * k0 * ldq; p.ldc = ldq;
            p.M = (int)m * k0; p.N = bg->r[i] > 0 ? bg->r[i] : 1;
            probs[i] = p;
        }
        CRM_HIP(hipMemcpyAsync(d_probs, probs.data(), sizeof(GemmProblem) * nrho, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, nrho, (int)m * k0, (int)ldq, np, true, k0, 1, 0));
        CRM_HIP(hipStreamSynchronize(st));
    }
    // side tables (split over the cell axis: only one M tile)
    DevBuf unused;
    struct Side { DevBuf* buf; const double* Y; long ldy; int N; long ld; bool needed; } side[3] = {
        {&gene->dt_Z1, gene->YE.as<double>(), gene->ld_ye, k0 * (1 + c), ldZ1, true},
        {full ? &shared->Z2 : &unused, d_Ep, gene->ld_ep, k0, ldZ2, full},
        {full ? &shared->Z3 : &unused, d_EE, gene->ld_ee, npair, ldZ3, full}};
    if (full && cross) {
        // C[(d*m + d'), :] = KR(Zt, Z)' Ep : the Khatri-Rao contraction with the indicators as "contexts"
        side[1].needed = false;
        const long rows = m * m;
        CRM_TRY(shared->Z2.ensure(sizeof(double) * (size_t)rows * ldZ2));
        CRM_HIP(hipMemsetAsync(shared->Z2.ptr, 0, sizeof(double) * (size_t)rows * ldZ2, st));
        GemmProblem p{};
        p.X = Zt; p.ldx = panel->ldz; p.E = Z; p.lde = panel->ldz; p.k0 = (int)m;
        p.Y = d_Ep; p.ldy = gene->ld_ep; p.C = shared->Z2.as<double>(); p.ldc = ldZ2;
        p.M = (int)rows; p.N = k0;
        CRM_HIP(hipMemcpyAsync(d_probs, &p, sizeof p, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, 1, (int)rows, k0, np, true, (int)m, 1, 0));
        CRM_HIP(hipStreamSynchronize(st));
    }
    for (auto& sd : side) {
        if (!sd.needed) continue;
        const int ks = split_for(np, sd.ld / GEMM_BN);
        const long sz = mp * sd.ld;
        CRM_TRY(sd.buf->ensure(sizeof(double) * (size_t)sz * ks));
        CRM_HIP(hipMemsetAsync(sd.buf->ptr, 0, sizeof(double) * (size_t)sz * ks, st));
        GemmProblem p{};
        p.X = Zt; p.ldx = panel->ldz; p.Y = sd.Y; p.ldy = sd.ldy; p.C = sd.buf->as<double>(); p.ldc = sd.ld;
        p.M = (int)m; p.N = sd.N;
        CRM_HIP(hipMemcpyAsync(d_probs, &p, sizeof p, hipMemcpyHostToDevice, st));
        CRM_TRY(launch_gemm_tn(ctx, d_probs, 1, (int)m, sd.N, np, false, 0, ks, sz));
        CRM_TRY(launch_reduce_splits(st, sd.buf->as<double>(), sz, ks, sz));
        CRM_HIP(hipStreamSynchronize(st));
    }
    CRM_TRY(gene->dt_sums.ensure(sizeof(double) * mp * DT_SUMS_LD));
    CRM_HIP(hipMemsetAsync(gene->dt_sums.ptr, 0, sizeof(double) * mp * DT_SUMS_LD, st));
    hipLaunchKernelGGL(donor_sums_kernel, dim3((unsigned)m, c + 2), dim3(256), 0, st,
                       panel->group.as<int>(), n, (int)m, gene->yW.as<double>(), gene->ld_yw, c,
                       gene->dt_sums.as<double>());
    CRM_HIP(hipGetLastError());
    CRM_HIP(hipStreamSynchronize(st));
    return CRM_OK;
}

int launch_permute_group(hipStream_t st, const int* group, const int* idx, long n, int* out) {
    hipLaunchKernelGGL(permute_group_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, group, idx, n, out);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

int launch_donor_cross(hipStream_t st, int nb, const double* Gam, long ld_gam, int m, const double* C, long ldc, int k0,
                       double* Z2, long ldz2) {
    hipLaunchKernelGGL(donor_cross_kernel, dim3(nb), dim3(128), 0, st, Gam, ld_gam, m, C, ldc, k0, Z2, ldz2);
    CRM_HIP(hipGetLastError());
    return CRM_OK;
}

}  // namespace crm
