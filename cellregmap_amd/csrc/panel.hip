// Genotype panels: dense (one row per cell) or grouped (donor-constant: one row per donor, a donor index per cell and its
// 0/1 indicator matrix), from float64 matrices or int8 dosages.
#include <algorithm>
#include <atomic>

#include "nullfit.h"
#include "objects.h"

using namespace crm;

namespace crm {

// flags[0] |= any non-finite entry; flags[1] |= any cell differing from its group's representative
__global__ void verify_panel_kernel(const double* __restrict__ G, long ld, long p, const int* __restrict__ group,
                                    const long* __restrict__ rep, int* __restrict__ flags) {
    const long i = blockIdx.x;
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= p) return;
    const double v = G[i * ld + j];
    if (!(fabs(v) < INFINITY)) atomicOr(&flags[0], 1);
    if (group) {
        const double r = G[rep[group[i]] * ld + j];
        if (__double_as_longlong(v) != __double_as_longlong(r)) atomicOr(&flags[1], 1);
    }
}

__global__ void gather_rows_kernel(const double* __restrict__ G, long ld, const long* __restrict__ rep,
                                   double* __restrict__ Gd) {
    const long d = blockIdx.x;
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x;
    if (j < ld) Gd[d * ld + j] = G[rep[d] * ld + j];
}

// One workgroup per variant: mean and standard deviation of the EXPANDED column (every donor's dosage weighted by
// its number of cells; population variance, as numpy's std / the reference simulator's column_normalize,
// cellregmap/_simulate.py:50-54), then the standardised donor-level column in float64.
__global__ __launch_bounds__(256) void standardise_dosages_kernel(const signed char* __restrict__ D, long ldd, long m, long p,
                                                                  const double* __restrict__ cells_of, double n, int standardise,
                                                                  double* __restrict__ Gd, long ldg, int* __restrict__ flags) {
    __shared__ double red[2][4];
    const long j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s1 = 0.0, s2 = 0.0;
    for (long d = tid; d < m; d += blockDim.x) {
        const double g = (double)D[d * ldd + j], w = cells_of[d];
        s1 += w * g;
        s2 += w * g * g;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64); }
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    s1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    s2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double mean = s1 / n;
    double var = 0.0;   // second pass in the centred form (the raw-moment difference cancels for rare alleles)
    for (long d = tid; d < m; d += blockDim.x) {
        const double c = (double)D[d * ldd + j] - mean;
        var += cells_of[d] * c * c;
    }
    for (int off = 32; off > 0; off >>= 1) var += __shfl_xor(var, off, 64);
    __syncthreads();
    if (lane == 0) red[0][wave] = var;
    __syncthreads();
    var = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / n;
    const double sd = sqrt(var);
    if (standardise && !(sd > 0.0)) {
        if (tid == 0) atomicOr(&flags[0], 1);   // monomorphic column: the reference's normalisation divides by zero
        return;
    }
    for (long d = tid; d < m; d += blockDim.x) {
        const double g = (double)D[d * ldd + j];
        Gd[d * ldg + j] = standardise ? (g - mean) / sd : g;
    }
}

static unsigned long next_panel_uid() {
    static std::atomic<unsigned long> counter{0};
    return ++counter;
}

// a panel of n cells and p variants with nothing on the device yet
static Owned<crm_panel> new_panel(crm_ctx* ctx, long n, long p) {
    Owned<crm_panel> P(new crm_panel());
    P->ctx = ctx;
    P->uid = next_panel_uid();
    P->n = n;
    P->n_pad = round_up(n, CELL_PAD);
    P->p = p;
    P->ld = round_up(p, 128);
    return P;
}

// Give a panel its donor structure: m groups, cell i in group[i] (on_device: the same index already in device memory).  Gd is
// allocated -- the caller fills it -- and the index, its content key and the indicator matrix are put in place on `st`,
// which the caller synchronises.
static int panel_set_groups(crm_panel* P, const int* group, const int* on_device, long m, hipStream_t st) {
    P->grouped = true;
    P->m = m;
    P->m_pad = round_up(m, GEMM_BK);
    P->ldz = round_up(m, 128) + 128;
    CRM_TRY(P->Gd.ensure(sizeof(double) * P->m_pad * P->ld));
    CRM_TRY(P->group.ensure(sizeof(int) * P->n));
    CRM_TRY(P->Z.ensure(sizeof(double) * P->n_pad * P->ldz));
    CRM_HIP(hipMemcpyAsync(P->group.ptr, on_device ? on_device : group, sizeof(int) * P->n,
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    P->group_key = content_key(group, sizeof(int) * P->n, (unsigned long)m);
    return launch_indicator(st, P->group.as<int>(), P->n, P->n_pad, (int)m, P->Z.as<double>(), P->ldz);
}

}  // namespace crm

extern "C" {

// (No lock of the context: the upload touches none of its work buffers and runs on a stream of its own, so that a panel
// can go to the device from one thread while another thread's constructor holds the context -- 8 GB over PCIe beside
// the eleven decompositions.  The copy is complete when the call returns.)
int crm_panel_create(crm_ctx* ctx, long n, const double* G, long ldg, long p, crm_panel** out) {
    return crm::guarded("crm_panel_create", [&]() -> int {
    if (!ctx || !G || !out || n <= 0 || p <= 0 || ldg < p) return CRM_ERR_ARG;
    *out = nullptr;
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->upload_stream ? ctx->upload_stream : ctx->stream;
    Owned<crm_panel> P = new_panel(ctx, n, p);
    CRM_TRY(P->G.ensure(sizeof(double) * P->n_pad * P->ld));
    CRM_TRY(upload_padded(st, P->G.as<double>(), P->ld, P->n_pad, G, ldg, n, p));
    CRM_HIP(hipStreamSynchronize(st));
    *out = P.release();
    return CRM_OK;
    });
}

void crm_panel_destroy(crm_panel* P) {
    try {
    if (!P) return;
    std::lock_guard<std::recursive_mutex> lock(P->ctx->mu);   // (reachable from a finalizer on any thread)
    (void)hipSetDevice(P->ctx->device);
    (void)hipStreamSynchronize(P->ctx->stream);
    delete P;
    } catch (...) {  // (nothing may unwind into the caller; a destroy has no status to return)
    }
}

// ---- grouped (donor-constant) panels ---------------------------------------------------------------
int crm_panel_create_grouped(crm_ctx* ctx, long n, const int* group, long m, const double* Gd, long ldg,
                             long p, crm_panel** out) {
    return crm::guarded_on("crm_panel_create_grouped", ctx, [&]() -> int {
    if (!ctx || !group || !Gd || !out || n <= 0 || m <= 0 || p <= 0 || ldg < p) return CRM_ERR_ARG;
    *out = nullptr;
    for (long i = 0; i < n; i++) {
        if (group[i] < 0 || group[i] >= m) {
            set_error("grouped panel: group index %d at cell %ld outside [0, %ld)", group[i], i, m);
            return CRM_ERR_ARG;
        }
    }
    CRM_HIP(hipSetDevice(ctx->device));
    Owned<crm_panel> P = new_panel(ctx, n, p);
    CRM_TRY(panel_set_groups(P.get(), group, nullptr, m, ctx->stream));
    CRM_TRY(upload_padded(ctx->stream, P->Gd.as<double>(), P->ld, P->m_pad, Gd, ldg, m, p));
    CRM_HIP(hipStreamSynchronize(ctx->stream));
    *out = P.release();
    return CRM_OK;
    });
}

int crm_panel_create_grouped_i8(crm_ctx* ctx, long n, const int* group, long m, const signed char* dosage,
                                long ldd, long p, int standardise, crm_panel** out) {
    return crm::guarded_on("crm_panel_create_grouped_i8", ctx, [&]() -> int {
    if (!ctx || !group || !dosage || !out || n <= 0 || m <= 0 || p <= 0 || ldd < p) return CRM_ERR_ARG;
    *out = nullptr;
    std::vector<double> cells_of(m, 0.0);
    for (long i = 0; i < n; i++) {
        if (group[i] < 0 || group[i] >= m) {
            set_error("grouped panel: group index %d at cell %ld outside [0, %ld)", group[i], i, m);
            return CRM_ERR_ARG;
        }
        cells_of[group[i]] += 1.0;
    }
    CRM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Owned<crm_panel> P = new_panel(ctx, n, p);
    CRM_TRY(panel_set_groups(P.get(), group, nullptr, m, st));
    DevBuf dD, dCells, dFlags;
    CRM_TRY(dD.ensure((size_t)m * p));
    CRM_TRY(dCells.ensure(sizeof(double) * m));
    CRM_TRY(dFlags.ensure(sizeof(int)));
    int h_flag = 0;
    CRM_HIP(hipMemsetAsync(P->Gd.ptr, 0, sizeof(double) * P->m_pad * P->ld, st));
    CRM_HIP(hipMemsetAsync(dFlags.ptr, 0, sizeof(int), st));
    CRM_HIP(hipMemcpy2DAsync(dD.ptr, p, dosage, ldd, p, m, hipMemcpyHostToDevice, st));   // 1 byte per dosage over PCIe
    CRM_HIP(hipMemcpyAsync(dCells.ptr, cells_of.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(standardise_dosages_kernel, dim3((unsigned)p), dim3(256), 0, st, dD.as<signed char>(), p, m, p,
                       dCells.as<double>(), (double)n, standardise ? 1 : 0, P->Gd.as<double>(), P->ld, dFlags.as<int>());
    CRM_HIP(hipGetLastError());
    CRM_HIP(hipMemcpyAsync(&h_flag, dFlags.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    if (h_flag) {
        set_error("panel: a monomorphic variant cannot be standardised (zero variance)");
        return CRM_ERR_NUMERIC;
    }
    *out = P.release();
    return CRM_OK;
    });
}

// Upload an expanded genotype matrix, check it for non-finite entries and -- when a candidate
// grouping is given (group_hint[i] in [0, m_hint), rep_rows[d] = a row carrying group d) -- verify ON THE
// DEVICE that every cell equals its group's representative in every variant; if so the panel is stored
// donor-level (grouped), otherwise dense.  Replaces the host-side isfinite pass and the host-side
// verification of detect_groups (both O(n p) memory passes that dominated short scans).
int crm_panel_create_auto(crm_ctx* ctx, long n, const double* G, long ldg, long p, const int* group_hint,
                          long m_hint, const long* rep_rows, crm_panel** out, int* out_grouped) {
    return crm::guarded("crm_panel_create_auto", [&]() -> int {   // (no lock of the context, like crm_panel_create)
    if (!ctx || !G || !out || n <= 0 || p <= 0 || ldg < p) return CRM_ERR_ARG;
    if (out_grouped) *out_grouped = 0;
    crm_panel* dense = nullptr;
    CRM_TRY(crm_panel_create(ctx, n, G, ldg, p, &dense));
    Owned<crm_panel> P(dense);
    hipStream_t st = ctx->upload_stream ? ctx->upload_stream : ctx->stream;
    DevBuf flags, dgroup, drep;
    CRM_TRY(flags.ensure(sizeof(int) * 2));
    const bool hinted = group_hint && rep_rows && m_hint > 0 && m_hint < BLOCK_SLACK_MAX - 1;
    if (hinted) {
        for (long i = 0; i < n; i++)
            if (group_hint[i] < 0 || group_hint[i] >= m_hint) return CRM_ERR_ARG;
        for (long d = 0; d < m_hint; d++)
            if (rep_rows[d] < 0 || rep_rows[d] >= n) return CRM_ERR_ARG;
        CRM_TRY(dgroup.ensure(sizeof(int) * n));
        CRM_TRY(drep.ensure(sizeof(long) * m_hint));
        CRM_HIP(hipMemcpyAsync(dgroup.ptr, group_hint, sizeof(int) * n, hipMemcpyHostToDevice, st));
        CRM_HIP(hipMemcpyAsync(drep.ptr, rep_rows, sizeof(long) * m_hint, hipMemcpyHostToDevice, st));
    }
    CRM_HIP(hipMemsetAsync(flags.ptr, 0, sizeof(int) * 2, st));
    hipLaunchKernelGGL(verify_panel_kernel, dim3((unsigned)n, (unsigned)((p + 255) / 256)), dim3(256), 0, st,
                       P->G.as<double>(), P->ld, p, hinted ? dgroup.as<int>() : nullptr,
                       hinted ? drep.as<long>() : nullptr, flags.as<int>());
    int h_flags[2] = {0, 0};
    CRM_HIP(hipGetLastError());
    CRM_HIP(hipMemcpyAsync(h_flags, flags.ptr, sizeof h_flags, hipMemcpyDeviceToHost, st));
    CRM_HIP(hipStreamSynchronize(st));
    if (h_flags[0]) {
        set_error("panel: non-finite values in the genotype matrix");
        return CRM_ERR_NUMERIC;
    }
    if (hinted && !h_flags[1]) {
        // collapse: gather the representative rows, drop the dense copy
        CRM_TRY(panel_set_groups(P.get(), group_hint, dgroup.as<int>(), m_hint, st));
        CRM_HIP(hipMemsetAsync(P->Gd.ptr, 0, sizeof(double) * P->m_pad * P->ld, st));
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)m_hint, (unsigned)((P->ld + 255) / 256)), dim3(256), 0,
                           st, P->G.as<double>(), P->ld, drep.as<long>(), P->Gd.as<double>());
        CRM_HIP(hipStreamSynchronize(st));
        P->G.release();
        if (out_grouped) *out_grouped = 1;
    }
    *out = P.release();
    return CRM_OK;
    });
}

// ---- read-back hooks (include/crm_hip_test.h) -------------------------------------------------------
int crm_test_panel_layout(const crm_panel* P, long* out) {
    return crm::guarded("crm_test_panel_layout", [&]() -> int {
    if (!P || !out) return CRM_ERR_ARG;
    const long v[8] = {P->n, P->n_pad, P->p, P->ld, P->grouped ? 1L : 0L, P->m, P->m_pad, P->ldz};
    std::copy(v, v + 8, out);
    return CRM_OK;
    });
}

int crm_test_panel_read(crm_panel* P, int what, void* dst, size_t bytes) {
    return crm::guarded_on("crm_test_panel_read", P ? P->ctx : nullptr, [&]() -> int {
    if (!P || !dst) return CRM_ERR_ARG;
    static const char* const names[4] = {"G", "Gd", "group", "Z"};
    const DevBuf* src = nullptr;
    size_t size = 0;
    switch (what) {
    case 0: src = &P->G; size = sizeof(double) * P->n_pad * P->ld; break;
    case 1: src = &P->Gd; size = sizeof(double) * P->m_pad * P->ld; break;
    case 2: src = &P->group; size = sizeof(int) * P->n; break;
    case 3: src = &P->Z; size = sizeof(double) * P->n_pad * P->ldz; break;
    default:
        set_error("crm_test_panel_read: buffer %d is none of 0 (G), 1 (Gd), 2 (group), 3 (Z)", what);
        return CRM_ERR_ARG;
    }
    if (!src->ptr || (what == 0) == P->grouped) {
        set_error("crm_test_panel_read: a %s panel holds no %s", P->grouped ? "grouped" : "dense", names[what]);
        return CRM_ERR_ARG;
    }
    if (bytes != size || src->bytes < size) {
        set_error("crm_test_panel_read: %s is %zu bytes, the caller asked for %zu", names[what], size, bytes);
        return CRM_ERR_ARG;
    }
    CRM_HIP(hipSetDevice(P->ctx->device));
    CRM_HIP(hipStreamSynchronize(P->ctx->stream));
    if (P->ctx->upload_stream) CRM_HIP(hipStreamSynchronize(P->ctx->upload_stream));
    CRM_HIP(hipMemcpy(dst, src->ptr, size, hipMemcpyDeviceToHost));
    return CRM_OK;
    });
}

int crm_set_donor_collapse(crm_ctx* ctx, int on) {
    return crm::guarded_on("crm_set_donor_collapse", ctx, [&]() -> int {
    if (!ctx) return CRM_ERR_ARG;
    ctx->collapse = on != 0;
    return CRM_OK;
    });
}

}  // extern "C"
