// The score statistic's assembly: its argument records and launches (assemble.hip, gram_ext.hip, wb_gram_fused.hip).
#pragma once
#include "nullfit.h"

namespace crm {

// ---- score statistic assembly (assemble.hip) ------------------------------------------------------
struct AssembleRho {
    const double* ty;
    const double* tW;
    const double* S0;
    const double* T;  // [variants x ldT] in block order
    long ldW, ldT;
    int r;
    int pad_;
    double rho;       // the grid point (unrelated-donor form: the weight v0 rho of the E1 term)
};

struct AssembleArgs {
    AssembleRho rho[CRM_MAX_RHO];
    const NullFitOut* fit;    // [variants] block order
    const int* sorted_pos;    // [variants] position of variant b inside the rho*-sorted A~ buffer; < 0: none was formed
    const double* A;          // [variants*k0 x ldA]  rows (pos*k0 + j) = Q0(rho*)' (gtest o E_j)
    long ldA;
    const double* A_none;     // ldA zeros: the rows of a variant without a position (scan_pass.h: no_kinship_term)
    int k0, c;
    long n;
    // n-length reductions, block order
    const double* Z1; long ldZ1;   // [variants x k0*(1+c)]  E' (gt o y), E' (gt o W_i)
    const double* Z2; long ldZ2;   // [variants x k0]        E' (gt o g)
    const double* Z3; long ldZ3;   // [variants x k0(k0+1)/2] E' diag(gt^2) E (upper, row-major pairs)
    const double* WW; const double* Wy; double yy;
    const double* gg; const double* gy; const double* gW; long ld_gW;
    const double* coef; long ld_coef;   // [c x ld_coef] projection coefficients of the block's variants onto W
                                        // (launch_ortho_block; null where the block was not orthogonalised)
    double* Q;   // [variants]
    double* F;   // [variants x k0 x k0]
    // Unrelated-donor form (scan_plan.hip: kin_wb, assemble.hip: woodbury_kernel), wb_k1 > 0: the Gram runs over donors k2
    // positions with k1 more rows R = Phi'E1 behind the k0 + c + 2 of the spectral form, and the E1 term is added back by
    // a k1 x k1 capacitance solve before the finalize.  Plain E1 products: E1'X (rows of the folded S), E1'[y, W] (gene),
    // E1'gx (block), E1'E1.
    int wb_k1;
    const double* wb_R; long wb_ldR;         // [k1 x ldR]
    const double* wb_E1X; long wb_ldE1X;     // [k1 x ld]: column pos k0 + i
    const double* wb_E1yW; long wb_ldE1yW;   // [k1 x ld]: column 0 y, 1.. W
    const double* wb_E1g; long wb_ldE1g;     // [k1 x ld]: column b
    const double* wb_EE;                     // [k1 x k1]
    double* wb_Gw;                           // workspace [variants x (k0 + c + 2 + k1)^2]
    int wb_gram_done;                        // wb_Gw holds the Gram already (launch_wb_gram_fused): the assembly starts behind it
};

// Gext: workspace [variants x (k0+c+2)^2]; fin_rows: assemble_rows_scratch_doubles(...) doubles (0: not needed -- the
// per-variant rows D'K^-1X and their solves fit LDS); *dma_launches grows by one when the Gram went through a
// direct-to-LDS kernel
int launch_assemble(hipStream_t st, const AssembleArgs& a, int variants, double* Gext, double* fin_rows = nullptr,
                    long* dma_launches = nullptr);
size_t assemble_rows_scratch_doubles(int variants, int k0, int c);
// LDS of the unrelated-donor correction (assemble.hip: woodbury_kernel) for KT = k0 + c + 2 rows and k1 E1 columns
size_t woodbury_lds_bytes(int KT, int k1);

// ---- the Gram of the KT operand rows over the spectrum (gram_ext.hip) -----------------------------
// Gext [variants x KT x KT] = S S' with S = sqrt(d) o [A~ rows ; Q0'W ; Q0'g ; Q0'y ; (unrelated-donor form) R], both
// triangles.  KT <= CRM_MAX_GRAM_ROWS (the caller has checked).  *dma_served: a direct-to-LDS kernel took the launch (up to
// 144 rows on 16-byte aligned operands unless form("gram_staged") asks for the staged kernel).
int launch_gram_ext(hipStream_t st, const AssembleArgs& a, int variants, double* Gext, int KT, bool* dma_served);

// ---- the unrelated-donor Gram straight from the per-donor pair products (wb_gram_fused.hip) -------
// The operands of launch_donor_pairs_rotate that the assembly's arguments do not hold: P [donors][variants x ldp] pair
// products (the variant's row is its place in the block), U [donors][k2pad x ldu] = Psi_d, the donor sums Psum [splits] slabs
struct WbFusedArgs {
    const double* P; long p_slab, ldp;
    const double* U; long u_slab, ldu;
    double* Psum; long psum_slab;
    int donors, splits, k2pad;
};
// LDS of wb_gram_fused_kernel, in doubles (tools/wb_gram_fused_prototype.py walks the same table): the Gram's image
// [KT][RS] from 0 (rows from k0 on in nO DMA instructions of 128 doubles), the variant's pair products at off_P (nP
// instructions), Psi_d [urows][UW] at off_U (nU), S0 and d_j of the chunk by column, the row pointers of the rows_o other rows
struct WbFusedLayout { int RS, UW, urows, rows_o, nP, nU, nO, off_P, off_U, off_S0, off_d, off_rp, total; };
WbFusedLayout wb_gram_fused_layout(int k0, int KT, long ldp);
bool wb_gram_fused_serves(const AssembleArgs& a, const WbFusedArgs& f, int nrho);
// wb_Gw of every variant of the block (a.fit, a.sorted_pos, a.rho[.].{ty, tW, T, S0, r}, a.wb_R, a.A_none as the assembly
// reads them) and the donor sums as launch_donor_pairs_rotate leaves them
int launch_wb_gram_fused(hipStream_t st, const AssembleArgs& a, const WbFusedArgs& f, int nrho, int variants);

}  // namespace crm
