// bm_center.h - the small kernels of the centred update: offsets o_l as running means of the positive
// phase, one scalar a_{l,b} = (x_{l,b} - o_l).o_l per row and layer, and the bias corrections r_l as row-weighted column sums
// fused with the bias update.  The centred weight gradient itself is grad_kernel's CEN flavour (bm_kernels.h).  Every
// reduction runs in a fixed order, nothing here uses atomics, and every operation that enters a stored value is an explicit
// round-to-nearest intrinsic or an expression copied from the plain kernel it stands in for, so that zero offsets reproduce
// the plain update bit for bit.
#pragma once
#include "bm_kernels.h"

namespace bm {

constexpr int CEN_LAYERS = 1 + 4;                 // the visible layer + BM_DBM_MAX_LAYERS hidden ones

// o <- (1 - nu) o + nu * (s / N)  from the positive phase's column sum s over N rows
__device__ __forceinline__ float cen_ema(float o, float nu, float s, float N) {
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, nu), o), __fmul_rn(nu, __fdiv_rn(s, N)));
}

// ---- DBM: offsets and plain bias gradients from the column sums launch_dbm_colsums left (blockIdx.y = layer)
struct CenEmaJob { const float *s_pos, *s_neg; float *o, *g; int n; float nu; };
struct CenEmaArgs { CenEmaJob job[CEN_LAYERS]; float N, M; };
__global__ void cen_ema_kernel(CenEmaArgs a) {
    const CenEmaJob &j = a.job[blockIdx.y];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= j.n) return;
    j.o[c] = cen_ema(j.o[c], j.nu, j.s_pos[c], a.N);
    j.g[c] = j.s_pos[c] / a.N - j.s_neg[c] / a.M;            // dbm_bias_update's g, before the sparsity term
}

// ---- RBM: the column sums themselves (block_colsum: the canonical sequential order over the rows), the raw tail the plain
// update publishes, the plain bias gradients and the offsets.  One workgroup per 64 columns, visible groups first.
struct RbmCenStatsArgs {
    const float *X, *vs, *h0m, *hm;     // [B][V] pitch ldx / ldv, [B][H] pitch ldh0 / ldh
    int ldx, ldv, ldh0, ldh, B, V, H;
    int hm_negated;                     // 1: `hm` points at -h_k
    float *raw_tail;                    // [V | H | H]: sum(X - v_k), sum(h0 - h_k), sum(h_k)
    float *ov, *oh, *gv, *gh;
    float nu_v, nu_h, N;
};
__global__ __launch_bounds__(NT) void rbm_cen_stats_kernel(RbmCenStatsArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[CS_SMEM_FLOATS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
    const int nv = (a.V + 63) / 64, wv = blockIdx.x;
    f32x4 s1, s2, sp, unused;
    if (wv < nv) {
        const int c0 = wv * 64;
        block_colsum(a.X, a.ldx, a.vs, a.ldv, c0, a.V, a.B, false, smem, s1, s2);           // sum(X - v_k)
        block_colsum(a.X, a.ldx, nullptr, 0, c0, a.V, a.B, false, smem, sp, unused);        // sum(X)
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + w * 16 + g * 4 + r;
                if (c < a.V) {
                    a.raw_tail[c] = s1[r];
                    a.gv[c] = s1[r] / a.N;
                    a.ov[c] = cen_ema(a.ov[c], a.nu_v, sp[r], a.N);
                }
            }
        }
    } else {
        const int c0 = (wv - nv) * 64;
        block_colsum(a.h0m, a.ldh0, a.hm, a.ldh, c0, a.H, a.B, true, smem, s1, s2, a.hm_negated != 0);   // sum(h0 - h_k), sum(h_k)
        block_colsum(a.h0m, a.ldh0, nullptr, 0, c0, a.H, a.B, false, smem, sp, unused);                   // sum(h0)
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + w * 16 + g * 4 + r;
                if (c < a.H) {
                    a.raw_tail[a.V + c] = s1[r];
                    a.raw_tail[a.V + a.H + c] = s2[r];
                    a.gh[c] = s1[r] / a.N;
                    a.oh[c] = cen_ema(a.oh[c], a.nu_h, sp[r], a.N);
                }
            }
        }
    }
}

// ---- row scalars a_b = sum_c (x_bc - o_c) * o_c: one wave per row, lane-strided partial sums (columns lane, lane + 64, ...
// in ascending order, product and sum rounded separately), then the xor butterfly 32, 16, ... 1 - a fixed order
struct CenRowJob { const float *X; const float *o; float *out; int ld, rows, cols, negated; };
constexpr int CEN_ROWJOBS = 2 * CEN_LAYERS;
struct CenRowArgs { CenRowJob job[CEN_ROWJOBS]; int first_blk[CEN_ROWJOBS + 1]; int njobs; };
__global__ __launch_bounds__(256) void cen_rowscal_kernel(CenRowArgs a) {
    int jb = 0;
    while (jb + 1 < a.njobs && (int)blockIdx.x >= a.first_blk[jb + 1]) ++jb;
    const CenRowJob &J = a.job[jb];
    const int row = ((int)blockIdx.x - a.first_blk[jb]) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= J.rows) return;
    float s = 0.f;
    for (int c = lane; c < J.cols; c += 64) {
        float x = J.X[(size_t)row * J.ld + c];
        if (J.negated) x = -x;
        const float o = J.o[c];
        s = __fadd_rn(s, __fmul_rn(__fsub_rn(x, o), o));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
    if (lane == 0) J.out[row] = s;
}

// ---- bias corrections fused with the bias update.
// sum_b (x_bc - o_c) * w_b for 64 columns [c0, c0 + 64) by one 256-thread workgroup, w_b = w0[b] + w1[b] (an absent
// neighbour counts 0): block_colsum's chain with the row weight as the MFMA's second operand in place of 1.0f, so the sum
// is ONE fma chain over the rows in ascending order.  sA: CS_ROWS x CS_LD floats, sW: CS_ROWS floats.  Lanes with
// (lane & 15) == 0 hold the results: [r] is column c0 + 16 wave + 4 (lane >> 4) + r.
__device__ __forceinline__ f32x4 block_wcolsum(const float *A, int lda, bool negA, const float *o, const float *w0, const float *w1,
                                               int c0, int ncols, int nrows, float *sA, float *sW) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, co = w * 16 + (lane & 15);
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < nrows; r0 += CS_ROWS) {
        const int nr = (nrows - r0 < CS_ROWS) ? nrows - r0 : CS_ROWS;
        for (int e = tid; e < CS_ROWS * 64; e += NT) {
            const int row = e >> 6, cc = e & 63, c = c0 + cc;
            float d = 0.f;
            if (row < nr && c < ncols) {
                float x = A[(size_t)(r0 + row) * lda + c];
                if (negA) x = -x;
                d = __fsub_rn(x, o[c]);
            }
            sA[row * CS_LD + cc] = d;
        }
        for (int row = tid; row < CS_ROWS; row += NT) {
            float wt = 0.f;
            if (row < nr) wt = __fadd_rn(w0 ? w0[r0 + row] : 0.f, w1 ? w1[r0 + row] : 0.f);
            sW[row] = wt;
        }
        wg_barrier();
        const int nsteps = (nr + 3) / 4;            // rows >= nr are zero in LDS
        for (int s = 0; s < nsteps; ++s) {
            const int k = 4 * s + g;
            sum = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[k * CS_LD + co], sW[k], sum, 0, 0, 0);
        }
        wg_barrier();
    }
    return sum;
}

// one layer's job: r = wsum_pos / N - wsum_neg / M, then the layer's bias update from g - r.  `rbm`: the update is
// rbm_bias_apply's (r; the column is a visible one when rbm_hidden == 0), else dbm_bias_apply's (d) - the plain updates' own.
struct CenBiasJob {
    const float *pos, *neg;             // [N][n] pitch ldp, [M][n] pitch ldn
    int ldp, ldn, neg_negated, n;
    const float *wp0, *wp1, *wn0, *wn1; // row scalars of the layer below / above, positive and negative rows (null: no such layer)
    const float *o, *g;                 // [n] offsets and plain bias gradients
    int rbm, rbm_hidden;
    RbmBiasArgs r;
    DbmBiasArgs d;
};
struct CenBiasArgs { CenBiasJob job[CEN_LAYERS]; int first_blk[CEN_LAYERS + 1]; int njobs; int N, M; };

__global__ __launch_bounds__(NT) void cen_bias_kernel(CenBiasArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[CS_ROWS * CS_LD];
    __shared__ float sW[CS_ROWS];
    int jb = 0;
    while (jb + 1 < a.njobs && (int)blockIdx.x >= a.first_blk[jb + 1]) ++jb;
    const CenBiasJob &J = a.job[jb];
    const int c0 = ((int)blockIdx.x - a.first_blk[jb]) * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
    const f32x4 sp = block_wcolsum(J.pos, J.ldp, false, J.o, J.wp0, J.wp1, c0, J.n, a.N, sA, sW);
    const f32x4 sn = block_wcolsum(J.neg, J.ldn, J.neg_negated != 0, J.o, J.wn0, J.wn1, c0, J.n, a.M, sA, sW);
    if ((lane & 15) != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + w * 16 + g * 4 + r;
        if (c >= J.n) continue;
        const float corr = __fsub_rn(__fdiv_rn(sp[r], (float)a.N), __fdiv_rn(sn[r], (float)a.M));
        const float gc = __fsub_rn(J.g[c], corr);
        if (J.rbm) rbm_bias_apply(J.r, J.rbm_hidden != 0, c, gc);
        else dbm_bias_apply(J.d, c, gc);
    }
}

static inline void launch_cen_rowscal(CenRowArgs &a, hipStream_t st) {
    a.first_blk[0] = 0;
    for (int j = 0; j < a.njobs; ++j) a.first_blk[j + 1] = a.first_blk[j] + (a.job[j].rows + 3) / 4;
    hipLaunchKernelGGL(cen_rowscal_kernel, dim3(a.first_blk[a.njobs]), dim3(256), 0, st, a);
}
static inline void launch_cen_bias(CenBiasArgs &a, hipStream_t st) {
    a.first_blk[0] = 0;
    for (int j = 0; j < a.njobs; ++j) a.first_blk[j + 1] = a.first_blk[j] + (a.job[j].n + 63) / 64;
    hipLaunchKernelGGL(cen_bias_kernel, dim3(a.first_blk[a.njobs]), dim3(NT), 0, st, a);
}

}  // namespace bm
