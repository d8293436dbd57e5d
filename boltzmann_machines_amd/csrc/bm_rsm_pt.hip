// bm_rsm_pt.hip - parallel tempering over replicated softmax visible units (bm_rbm_rsm_pt_*): the instantiations of
// act_kernel's DB + RT flavour - the prop-up with a temperature and a document length per row that leaves the slot partials of
// h . (vW + D hb) - for exactly the geometries DB has, the start kernel and the re-scoring kernel of the visible half of the swap
// energy.  A translation unit of its own, as bm_softmax_pt.hip is beside bm_softmax_v.hip: the kernels of every other unit are
// compiled exactly as before.  Compiled into libbm355.so next to bm355.hip.  bm_rsm.h fixes the operation sequences.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_rsm.h"

namespace bm {

void launch_act_dbpt_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_as<FL_DB | FL_RT>(geo, a, st); }

// ---- rsm_pt_start_kernel (RsmPtStartArgs).  One wave per row (four rows per workgroup); every store is bounded by rows and V
__global__ __launch_bounds__(256) void rsm_pt_start_kernel(RsmPtStartArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                    // wave-uniform
    const int c = row / a.R, r = row % a.R;
    if (a.V0) {
        const float *v0 = a.V0 + (size_t)c * a.V;
        float *v = a.v + (size_t)row * a.ld;
        for (int i = lane; i < a.V; i += 64) v[i] = v0[i];
    }
    if (lane == 0) {
        const float D = a.chain_len[c];
        a.row_mult[row] = a.beta[r]; a.idx[row] = r; a.len[row] = D;
        if (a.V0_len && r == 0 && a.V0_len[c] != D) atomicOr(a.bad, RSM_BAD_MISMATCH);
    }
}
void launch_rsm_pt_start(const RsmPtStartArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(rsm_pt_start_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
}

// ---- rsm_pt_rescore_kernel (bm_rsm.h).  One workgroup of 256 threads per row; thread tid owns the runs p * 256 + tid, p < 4
// (V <= RSM_MAX_V = 4 * 256 * 16), as in multinomial_counts_kernel; level 1 in the first 64 threads, level 2 in thread 0
__global__ __launch_bounds__(256) void rsm_pt_rescore_kernel(const float *x, int ld, int rows, int V, const float *vb, float *part, int ld_part) {
    __shared__ double s_dr[4 * 256], s_db[64];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= rows) return;                      // (uniform over the workgroup)
    const float *xr = x + (size_t)row * ld;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i0 = (p * 256 + tid) * 16;
        double r = 0.0;
        if (i0 < V) {
            for (int k = 0; k < 16; ++k)
                if (i0 + k < V) r = r + (double)xr[i0 + k] * (double)vb[i0 + k];
        }
        s_dr[p * 256 + tid] = r;
    }
    __syncthreads();
    if (tid < 64) {                               // level 1: the 16 runs of block `tid` in ascending order
        double b = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) b = b + s_dr[tid * 16 + q];
        s_db[tid] = b;
    }
    __syncthreads();
    if (tid == 0) {                               // level 2: the blocks in ascending order
        double s = 0.0;
        for (int b = 0; b < 64; ++b) s = s + s_db[b];
        const float hi = (float)s, lo = (float)(s - (double)hi);
        part[row] = hi;
        part[(size_t)ld_part + row] = lo;
    }
}
void launch_rsm_pt_rescore(const float *x, int ld, int rows, int V, const float *vb, float *part, int ld_part, hipStream_t st) {
    if (rows < 1) return;
    hipLaunchKernelGGL(rsm_pt_rescore_kernel, dim3(rows), dim3(256), 0, st, x, ld, rows, V, vb, part, ld_part);
}

}  // namespace bm
