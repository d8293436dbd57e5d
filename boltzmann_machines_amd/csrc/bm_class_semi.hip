// bm_class_semi.hip - semi-supervised training of the classification RBM: the three small fixed-order kernels of
// the update on unlabelled rows (bm_class.h lists the launches).  No act_kernel flavour lives here: the passes are the CR and CB
// passes of bm_class.hip / bm_class_joint.hip as they are.  A translation unit of its own so that the modules of the plain, CR
// and CB kernels hold exactly the kernels they held (profiles/class_semi_resources.md).  Compiled into libbm355.so next to
// bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_class.h"

namespace bm {

// ---- class_posterior_kernel: one thread per row, so every sum is one serial chain over the classes in ascending order, whatever
// C is.  The row's prob values are widened to double: total, then the prefix sums; one float32 uniform at flat index row0 + j;
// y0 = the lowest c with u * total < prefix_c, C - 1 if there is none (class_draw_kernel's rule).  The same pass forms the
// entropy -sum_c p_c log p_c in double (a zero p_c adds nothing), rounded to float once, and max_c p_c
__global__ __launch_bounds__(64) void class_posterior_kernel(ClassPosteriorArgs a) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= a.B) return;
    const float *p = a.prob + (size_t)row * a.C;
    double total = 0.0;
    for (int c = 0; c < a.C; ++c) total += (double)p[c];
    const double thr = (double)philox_uniform_at(a.key, (uint64_t)(a.row0 + row)) * total;
    double pre = 0.0, ent = 0.0;
    float mx = p[0];
    int y = a.C - 1;
    bool found = false;
    for (int c = 0; c < a.C; ++c) {
        const float pf = p[c];
        const double pc = (double)pf;
        pre += pc;
        if (!found && thr < pre) { y = c; found = true; }
        if (pc > 0.0) ent -= pc * log(pc);
        mx = pf > mx ? pf : mx;
    }
    a.y0[row] = y;
    a.ent[row] = (float)ent;
    a.conf[row] = mx;
}
void launch_class_posterior(const ClassPosteriorArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_posterior_kernel, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
}

// ---- class_marginal_kernel: elementwise over [B][H].  em = sum_c p_c sigmoid(t + U[c]) = E[h | x] with y summed out, the classes
// in ascending order as one fma chain from 0: the exact negation of class_hidden_kernel's negm
__global__ __launch_bounds__(256) void class_marginal_kernel(ClassMarginalArgs a) {
    const long long n = (long long)a.B * a.H;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / a.H), i = (int)(e - (long long)j * a.H);
        const float x = a.T[(size_t)j * a.ldt + i];
        float em = 0.f;
        for (int c = 0; c < a.C; ++c)
            em = __fmaf_rn(a.prob[(size_t)j * a.C + c], sigmoid(__fadd_rn(x, a.U[(size_t)c * a.ldu + i])), em);
        a.em[(size_t)j * a.ld + i] = em;
    }
}
void launch_class_marginal(const ClassMarginalArgs &a, hipStream_t st) {
    const long long n = (long long)a.B * a.H;
    hipLaunchKernelGGL(class_marginal_kernel, dim3((int)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, a);
}

// ---- class_unsup_update_kernel: the grid, the wave layout and the row order of class_joint_update_kernel.  A column workgroup
// owns 64 hidden units of class c: wave w takes the rows j = w, w + 4, ... in ascending order as one chain - per row
// fma(p_jc, sigmoid(t_ji + U[c][i]), .), then + (-hk_ji) where yk_j == c - and the four partial sums meet as (s0 + s1) + (s2 + s3);
// the sigmoid is that of the OLD U, which every thread reads before any thread writes.  The last workgroup of a class sums
// p_jc - 1[yk_j == c] lane-strided, a butterfly, and applies the bias rule to yb[c]
__global__ __launch_bounds__(256) void class_unsup_update_kernel(ClassUnsupArgs a) {
    __shared__ float s_part[4][64];
    const int c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {          // the class bias
        if (w != 0) return;
        float s = 0.f;
        for (int j = lane; j < a.B; j += 64)
            s = __fadd_rn(s, __fsub_rn(a.prob[(size_t)j * a.C + c], a.yk[j] == c ? 1.f : 0.f));
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
        for (int j0 = w; j0 < a.B; j0 += 32) {            // eight of the wave's rows at a time: their operands are requested together
            float p[8], t[8];
            int k[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j = j0 + 4 * q;
                const bool ok = j < a.B;
                p[q] = ok ? a.prob[(size_t)j * a.C + c] : 0.f;
                t[q] = ok ? a.T[(size_t)j * a.ldt + i] : 0.f;
                k[q] = ok ? a.yk[j] : -1;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {                     // ... the chain itself in ascending row order
                const int j = j0 + 4 * q;
                if (j >= a.B) break;
                s = __fmaf_rn(p[q], sigmoid(__fadd_rn(t[q], u)), s);
                if (k[q] == c) s = __fadd_rn(s, a.hkneg[(size_t)j * a.ldhk + i]);
            }
        }
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
void launch_class_unsup_update(const ClassUnsupArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_unsup_update_kernel, dim3((a.H + 63) / 64 + 1, a.C), dim3(256), 0, st, a);
}

}  // namespace bm
