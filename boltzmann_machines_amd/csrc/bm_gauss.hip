// bm_gauss.hip - Gaussian visible units as one joint model (bm_rbm_gauss_ais, bm_rbm_gauss_free_energy_rows, bm_rbm_gauss_pt_*;
// DESIGN.md 3.30): the instantiations of act_kernel's RT + GT flavour - the prop-down whose row j draws around an untempered mean
// with the standard deviation of its own temperature and leaves the slot partials of -1/2 (s - c)^2 - and the small kernels of the
// three entries.  A translation unit of its own, as bm_softmax_pt.hip is: the kernels of every other unit are compiled exactly as
// before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_gauss.h"

namespace bm {

void launch_act_gtpt_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_RT | FL_GT>(geo, a, st); }

// the standard normal of flat index idx on `key`: draw4's per-element mapping (word pair (idx & 3) >> 1 of block idx >> 2, sin first)
__device__ __forceinline__ float gauss_normal_at(const PhiloxKey &key, unsigned long long idx) {
    uint32_t wds[4];
    philox_block(key, idx >> 2, wds);
    float n0, n1;
    const int pr = (int)(idx & 3) >> 1;
    box_muller(wds[2 * pr], wds[2 * pr + 1], n0, n1);
    return (idx & 1) ? n1 : n0;
}

// the slot partial of -1/2 (u - c)^2 over the 16-column slot `slot` in the order of the GT flavour; u_at(i) supplies (and may store)
// column i of the row
template <class F>
__device__ __forceinline__ float gauss_sq_slot(int slot, int V, const float *c, F u_at) {
    float q[4];
    for (int g = 0; g < 4; ++g) {
        float acc = 0.f;
        for (int r = 0; r < 4; ++r) {
            const int i = slot * 16 + 4 * g + r;
            if (i >= V) break;
            const float d = __fsub_rn(u_at(i), c[i]);
            acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(-0.5f, d), d));
        }
        q[g] = acc;
    }
    return __fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3]));
}

// ---- gauss_prep_kernel
__global__ __launch_bounds__(256) void gauss_prep_kernel(const float *vb, const float *sigma, int V, float *c, float *ones) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) {
        c[i] = __fdiv_rn(vb[i], sigma[i]);
        ones[i] = 1.0f;
    }
}
void launch_gauss_prep(const float *vb, const float *sigma, int V, float *c, float *ones, hipStream_t st) {
    hipLaunchKernelGGL(gauss_prep_kernel, dim3((V + 255) / 256), dim3(256), 0, st, vb, sigma, V, c, ones);
}

// ---- gauss_ais_start_kernel (GaStartArgs).  One wave per row (four rows per workgroup), the layout of rbm_ais_init_kernel.  Every
// store is bounded by rows, V and nslot
__global__ __launch_bounds__(256) void gauss_ais_start_kernel(GaStartArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                    // wave-uniform
    const unsigned long long base = (a.row0 + (unsigned long long)row) * (unsigned long long)a.V;
    float s = 0.f;
    for (int i = lane; i < a.V; i += 64) {
        const float x = __fadd_rn(a.abase[i], gauss_normal_at(a.key, base + (unsigned long long)i));
        a.v[(size_t)row * a.ld + i] = x;
        s += x * a.dvec[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) a.part[row] = s;
    for (int q = 1 + lane; q < a.nslot; q += 64) a.part[(size_t)q * a.ld_part + row] = 0.f;
}
void launch_gauss_ais_start(const GaStartArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(gauss_ais_start_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
}

// ---- gauss_fe_rows_kernel.  One wave per row (four rows per workgroup), the layout of rbm_fe_rows_kernel; u - c is formed in double
// (exact: both are floats), so the quadratic term carries no rounding of its own beyond the double sums
__global__ __launch_bounds__(256) void gauss_fe_rows_kernel(const float *U, int ldu, int rows, int V, const float *c, const float *part,
                                                            int ld_part, int nslot, double *out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                      // wave-uniform
    double s = 0.0;
    for (int i = lane; i < V; i += 64) {
        const double d = (double)U[(size_t)row * ldu + i] - (double)c[i];
        s += 0.5 * d * d;
    }
    for (int q = lane; q < nslot; q += 64) s -= (double)part[(size_t)q * ld_part + row];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = s;
}
void launch_gauss_fe_rows(const float *U, int ldu, int rows, int V, const float *c, const float *part, int ld_part, int nslot, double *out,
                          hipStream_t st) {
    hipLaunchKernelGGL(gauss_fe_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, U, ldu, rows, V, c, part, ld_part, nslot, out);
}

// ---- gauss_pt_init_kernel (GpStartArgs).  One wave per row (four rows per workgroup), a lane per 16-column slot in turn: the slot's
// 16 states, their stores and its partial; no lane reads what another lane wrote.  Every store is bounded by rows, V and the slot count
__global__ __launch_bounds__(256) void gauss_pt_init_kernel(GpStartArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                    // wave-uniform
    const int r = row % a.R;
    float *v = a.v + (size_t)row * a.ld;
    const float *v0 = a.V0 ? a.V0 + (size_t)(row / a.R) * a.V : nullptr;
    const float sd = a.sd[r];
    const unsigned long long base = (a.row0 + (unsigned long long)row) * (unsigned long long)a.V;
    const int nslot = (a.V + 15) / 16;
    for (int slot = lane; slot < nslot; slot += 64)
        a.part[(size_t)slot * a.ld_part + row] = gauss_sq_slot(slot, a.V, a.c, [&](int i) {
            const float u = v0 ? __fdiv_rn(v0[i], a.sigma[i])
                               : __fadd_rn(a.c[i], __fmul_rn(gauss_normal_at(a.key, base + (unsigned long long)i), sd));
            v[i] = u;
            return u;
        });
    if (lane == 0) { a.row_mult[row] = a.beta[r]; a.idx[row] = r; }
}
void launch_gauss_pt_init(const GpStartArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(gauss_pt_init_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
}

// ---- gauss_pt_rows_kernel (GpRowsArgs): the same layout; every store is bounded by J, V and the slot count
__global__ __launch_bounds__(256) void gauss_pt_rows_kernel(GpRowsArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.J) return;                       // wave-uniform
    const float *z = a.Z + (size_t)row * a.ldz;
    float *s = a.states + (size_t)row * a.ld_states;
    const float sd = a.sd[a.idx[row]];
    const unsigned long long base = (unsigned long long)(a.row0 + row) * (unsigned long long)a.V;
    const int nslot = (a.V + 15) / 16;
    for (int slot = lane; slot < nslot; slot += 64)
        a.part[(size_t)slot * a.ld_part + row] = gauss_sq_slot(slot, a.V, a.c, [&](int i) {
            const float m = __fadd_rn(z[i], a.c[i]);
            const float u = __fadd_rn(m, __fmul_rn(gauss_normal_at(a.key, base + (unsigned long long)i), sd));
            s[i] = u;
            return u;
        });
}
void launch_gauss_pt_rows(const GpRowsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(gauss_pt_rows_kernel, dim3((a.J + 3) / 4), dim3(256), 0, st, a);
}

// ---- gauss_scale_rows_kernel
__global__ __launch_bounds__(256) void gauss_scale_rows_kernel(float *x, int rows, int V, const float *sigma) {
    const size_t n = (size_t)rows * V;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) x[e] = __fmul_rn(x[e], sigma[e % (size_t)V]);
}
void launch_gauss_scale_rows(float *x, int rows, int V, const float *sigma, hipStream_t st) {
    const size_t n = (size_t)rows * V;
    hipLaunchKernelGGL(gauss_scale_rows_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, st, x, rows, V, sigma);
}

}  // namespace bm
