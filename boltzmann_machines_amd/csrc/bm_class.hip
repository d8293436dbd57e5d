// bm_class.hip - the class head of a Bernoulli RBM: the instantiations of act_kernel's CR flavour, and the
// three fixed-order kernels behind it (bm_class.h lists the launches of one update).  A translation unit of its own, as
// bm_grad_cen.hip is: the kernels of the plain update are compiled exactly as before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_class.h"

namespace bm {

void launch_act_cr_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_as<FL_CR>(geo, a, st); }      // (bm_launch.h)

// ---- class_row_kernel: one wave per row.  s_c = yb_c + the row's slots in ascending order, in double; logsumexp in double over
// lane-strided classes + butterflies (a fixed order).  Labels are read through ordinary bounds logic: one outside [0, C) indexes
// nothing, zeroes the row's coefficients and raises the flag
__device__ __forceinline__ double class_score(const ClassRowArgs &a, int row, int c) {
    double s = (double)a.yb[c];
    const float *p = a.part + (size_t)c * a.nslots * a.ldp + row;
    for (int q = 0; q < a.nslots; ++q) s += (double)p[(size_t)q * a.ldp];
    return s;
}
__global__ __launch_bounds__(256) void class_row_kernel(ClassRowArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.B) return;
    // the row's maximum and the first class that attains it
    double best = -1e300;
    int arg = a.C;
    for (int c = lane; c < a.C; c += 64) {
        const double s = class_score(a, row, c);
        if (s > best) { best = s; arg = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    double sum = 0.0;
    for (int c = lane; c < a.C; c += 64) sum += exp(class_score(a, row, c) - best);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const double lse = best + log(sum);
    int t = -1;
    if (a.y) {
        const int lab = a.y[row];
        if (lab >= 0 && lab < a.C) t = lab;
        else if (lane == 0) *a.bad = 1;
    }
    for (int c = lane; c < a.C; c += 64) {
        const double lp = class_score(a, row, c) - lse;
        const size_t o = (size_t)row * a.C + c;
        const float p = (float)exp(lp);
        a.logp[o] = (float)lp;
        a.prob[o] = p;
        if (a.y) {
            a.coef[o] = (t < 0) ? 0.f : __fsub_rn(c == t ? 1.0f : 0.0f, p);
            if (c == t) a.rowlp[row] = (float)lp;
        }
    }
    if (a.y && lane == 0) {
        a.tl[row] = t;
        a.rowhit[row] = (t >= 0 && arg == t) ? 1.0f : 0.0f;
        if (t < 0) a.rowlp[row] = 0.f;
    }
}
void launch_class_row(const ClassRowArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_row_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
}

// ---- class_hidden_kernel: elementwise over [B][H].  pos = sigmoid(t + U[t_j]), negm = -sum_c p_c sigmoid(t + U[c]), the classes
// in ascending order; a row without a valid label gets zeros in both (it contributes nothing to the outer products and sums)
__global__ __launch_bounds__(256) void class_hidden_kernel(ClassHiddenArgs a) {
    const long long n = (long long)a.B * a.H;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / a.H), i = (int)(e - (long long)j * a.H);
        const int t = a.tl[j];
        float pos = 0.f, negm = 0.f;
        if (t >= 0) {
            const float x = a.T[(size_t)j * a.ldt + i];
            pos = sigmoid(__fadd_rn(x, a.U[(size_t)t * a.ldu + i]));
            for (int c = 0; c < a.C; ++c)
                negm = __fmaf_rn(-a.prob[(size_t)j * a.C + c], sigmoid(__fadd_rn(x, a.U[(size_t)c * a.ldu + i])), negm);
        }
        a.pos[(size_t)j * a.ld + i] = pos;
        a.negm[(size_t)j * a.ld + i] = negm;
    }
}
void launch_class_hidden(const ClassHiddenArgs &a, hipStream_t st) {
    const long long n = (long long)a.B * a.H;
    const int nb = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(class_hidden_kernel, dim3(nb), dim3(256), 0, st, a);
}

// ---- class_head_update_kernel: grid (ceil(H / 64) + 1, C).  A column workgroup owns 64 hidden units of class c: its four waves
// take the rows j = w, w + 4, ... in ascending order, the four partial sums meet as (s0 + s1) + (s2 + s3) - an order that depends
// on B alone; S = sigmoid(t + U[c]) is recomputed from the OLD U, which every thread reads before any thread writes.  The last
// workgroup of a class reduces coef[:, c] (lane-strided sums + butterfly) and applies the bias rule to yb[c]
__global__ __launch_bounds__(256) void class_head_update_kernel(ClassHeadArgs a) {
    __shared__ float s_part[4][64];
    const int c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {          // the class bias
        if (w != 0) return;
        float s = 0.f;
        for (int j = lane; j < a.B; j += 64) s = __fadd_rn(s, a.coef[(size_t)j * a.C + c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
        if (lane == 0) {
            const float g = s / a.N;
            const float d = a.lr * (a.mom * a.dyb[c] + g);      // rbm_bias_kernel's rule
            a.dyb[c] = d;
            a.yb[c] = a.yb[c] + d;
        }
        return;
    }
    const int i = blockIdx.x * 64 + lane;
    const bool in = i < a.H;
    const float u = in ? a.U[(size_t)c * a.ldu + i] : 0.f;
    float s = 0.f;
    if (in)
        for (int j = w; j < a.B; j += 4)
            s = __fmaf_rn(a.coef[(size_t)j * a.C + c], sigmoid(__fadd_rn(a.T[(size_t)j * a.ldt + i], u)), s);
    s_part[w][lane] = s;
    __syncthreads();
    if (w == 0 && in) {
        const float tot = __fadd_rn(__fadd_rn(s_part[0][lane], s_part[1][lane]), __fadd_rn(s_part[2][lane], s_part[3][lane]));
        float wv = u, dv = a.dU[(size_t)c * a.ldu + i];
        apply_w_update(__fdiv_rn(tot, a.N), 0.f, a.l2, a.lr, a.mom, wv, dv);
        a.U[(size_t)c * a.ldu + i] = wv;
        a.dU[(size_t)c * a.ldu + i] = dv;
    }
}
void launch_class_head_update(const ClassHeadArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_head_update_kernel, dim3((a.H + 63) / 64 + 1, a.C), dim3(256), 0, st, a);
}

// ---- class_sum_kernel: one workgroup; thread-strided double sums, then an LDS tree
__global__ __launch_bounds__(256) void class_sum_kernel(const float *rowlp, const float *rowhit, int B, double *acc) {
    __shared__ double s0[256], s1[256];
    double a0 = 0.0, a1 = 0.0;
    for (int j = threadIdx.x; j < B; j += 256) { a0 += (double)rowlp[j]; a1 += (double)rowhit[j]; }
    s0[threadIdx.x] = a0; s1[threadIdx.x] = a1;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) { s0[threadIdx.x] += s0[threadIdx.x + n]; s1[threadIdx.x] += s1[threadIdx.x + n]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { acc[0] += s0[0]; acc[1] += s1[0]; }
}
void launch_class_sum(const float *rowlp, const float *rowhit, int B, double *acc, hipStream_t st) {
    hipLaunchKernelGGL(class_sum_kernel, dim3(1), dim3(256), 0, st, rowlp, rowhit, B, acc);
}

}  // namespace bm
