// bm_softmax_ais.hip - AIS over softmax visible units (bm_rbm_groups_ais): the instantiations of act_kernel's
// SM + SA flavour - the tempered softmax-group prop-down that holds absent groups at zero and leaves the slot partials of
// state . dot_vec, for exactly the geometries SM has - the start kernel and the row-dot kernel of the generic route.  A translation
// unit of its own, as bm_softmax_cl.hip is beside bm_softmax_v.hip: the kernels of every other unit are compiled exactly as before.
// Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_softmax_ais.h"

namespace bm {

void launch_act_smais_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_SM | FL_SA>(geo, a, st); }

// ---- softmax_ais_start_kernel (SaStartArgs).  One wave per row (four rows per workgroup), a lane per group in turn, the K units
// of a group walked three times as softmax_groups_kernel walks them: maximum, S, then the draw.  Every store is bounded by rows, V
// (g K + k < V: V % K == 0) and nslot
__global__ __launch_bounds__(256) void softmax_ais_start_kernel(SaStartArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                    // wave-uniform
    float *v = a.v + (size_t)row * a.ld;
    const int G = a.V / a.K;
    float s = 0.f;
    for (int g = lane; g < G; g += 64) {
        const int i0 = g * a.K;
        if (a.absent && a.absent[i0] != 0.f) {    // not part of this run's model: zeros
            for (int k = 0; k < a.K; ++k) v[i0 + k] = 0.f;
            continue;
        }
        float mx = -3.402823466e38f;
        for (int k = 0; k < a.K; ++k) mx = fmaxf(mx, a.abase[i0 + k]);
        float S = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - a.abase[i0 + k];
            if (d > 80.0f) d = 80.0f;
            S = S + exp_neg(d);
        }
        const float u = philox_uniform_at(a.key, (a.row0 + (unsigned long long)row) * (unsigned long long)a.V + (unsigned long long)i0);
        const float t = u * S;
        float c = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - a.abase[i0 + k];
            if (d > 80.0f) d = 80.0f;
            const float cp = c;
            c = c + exp_neg(d);
            const float sv = (c > t && !(cp > t)) ? 1.0f : 0.0f;
            v[i0 + k] = sv;
            s += sv * a.dvec[i0 + k];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) a.part[row] = s;
    for (int q = 1 + lane; q < a.nslot; q += 64) a.part[(size_t)q * a.ld_part + row] = 0.f;
}

void launch_softmax_ais_start(const SaStartArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(softmax_ais_start_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
}

// ---- softmax_ais_dot_kernel: a thread per (slot, row), consecutive threads on consecutive rows (the stores are full lines)
__global__ __launch_bounds__(256) void softmax_ais_dot_kernel(const float *x, int ldx, int rows, int V, const float *dvec, float *part,
                                                              int ld_part) {
    const int nslot = (V + 15) / 16;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * nslot) return;
    const int slot = (int)(e / rows), row = (int)(e % rows);
    const float *xr = x + (size_t)row * ldx;
    float q[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float acc = 0.f;
        for (int r = 0; r < 4; ++r) {
            const int c = slot * 16 + 4 * g + r;
            if (c >= V) break;
            acc += xr[c] * dvec[c];
        }
        q[g] = acc;
    }
    part[(size_t)slot * ld_part + row] = (q[0] + q[1]) + (q[2] + q[3]);
}

void launch_softmax_ais_dot(const float *x, int ldx, int rows, int V, const float *dvec, float *part, int ld_part, hipStream_t st) {
    const long long n = (long long)rows * ((V + 15) / 16);
    hipLaunchKernelGGL(softmax_ais_dot_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, ldx, rows, V, dvec, part, ld_part);
}

}  // namespace bm
