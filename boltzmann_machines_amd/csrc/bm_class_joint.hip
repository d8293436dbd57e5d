// bm_class_joint.hip - joint training of the classification RBM and sampling by class: the instantiations of
// act_kernel's CB flavour, and the small fixed-order kernels of the chain and the update (bm_class.h lists them).  A
// translation unit of its own, as bm_grad_cen.hip and bm_class.hip are: beside the CB instantiations the compiler allocates the
// registers of some CR instantiations differently, and the kernels that exist are to stay exactly what they were
// (profiles/class_joint_resources.md).  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_class.h"

namespace bm {

void launch_act_cb_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_as<FL_CB>(geo, a, st); }      // (bm_launch.h)

// ---- class_draw_kernel: y ~ p(y | h), one wave per row.  logit_c = yb_c + sum_i h_i U[c][i] in double: lane l adds the products
// of i = l, l + 64, ... in ascending order, the 64 partial sums meet in a butterfly (offsets 32 .. 1: every lane holds the same
// bits), yb_c is added last - an order that depends on H alone.  Maximum, sum of exp(logit - max) and the prefix sums run over
// the classes in ascending order, in double, in every lane alike.  One float32 uniform per row at flat index row0 + j:
// y = the lowest c with u * total < prefix_c, C - 1 if there is none.  Up to CLASS_DRAW_KEEP logits stay in LDS between the
// three passes over the classes; a larger head recomputes them (the same bits)
constexpr int CLASS_DRAW_KEEP = 512;
__device__ __forceinline__ double class_logit(const ClassDrawArgs &a, const float *hrow, int c, int lane) {
    const float *u = a.U + (size_t)c * a.ldu;
    double s = 0.0;
    for (int i = lane; i < a.H; i += 64) s += (double)hrow[i] * (double)u[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return (double)a.yb[c] + s;
}
__global__ __launch_bounds__(256) void class_draw_kernel(ClassDrawArgs a) {
    __shared__ double s_logit[4][CLASS_DRAW_KEEP];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * 4 + w;
    if (row >= a.B) return;                                    // (no workgroup barrier below: a wave works alone)
    const float *hrow = a.h + (size_t)row * a.ldh;
    const bool keep = a.C <= CLASS_DRAW_KEEP;
    double mx = 0.0;
    // four classes at a time share the loads of h (each class's sum keeps the order of class_logit: the same bits)
    for (int c0 = 0; c0 < a.C; c0 += 4) {
        const float *u[4];
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { u[q] = a.U + (size_t)(c0 + q < a.C ? c0 + q : a.C - 1) * a.ldu; s[q] = 0.0; }
#pragma unroll 2
        for (int i = lane; i < a.H; i += 64) {
            const double hv = (double)hrow[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += hv * (double)u[q][i];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], off);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + q;
            if (c >= a.C) break;
            const double l = (double)a.yb[c] + s[q];
            if (keep) s_logit[w][c] = l;                       // every lane stores the same value and reads back its own store
            mx = (c == 0 || l > mx) ? l : mx;
        }
    }
    double total = 0.0;
    for (int c = 0; c < a.C; ++c) total += exp((keep ? s_logit[w][c] : class_logit(a, hrow, c, lane)) - mx);
    const double thr = (double)philox_uniform_at(a.key, (uint64_t)(a.row0 + row)) * total;
    double pre = 0.0;
    int y = a.C - 1;
    for (int c = 0; c < a.C; ++c) {                            // (wave-uniform: every lane holds the same numbers)
        pre += exp((keep ? s_logit[w][c] : class_logit(a, hrow, c, lane)) - mx);
        if (thr < pre) { y = c; break; }
    }
    if (lane == 0) a.y[row] = y;
}
void launch_class_draw(const ClassDrawArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_draw_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
}

// ---- class_joint_update_kernel: the grid, the wave layout and the order of class_head_update_kernel.  A column workgroup owns
// 64 hidden units of class c: wave w takes the rows j = w, w + 4, ... in ascending order as one chain - per row + h0m where
// y_j == c, - hk where yk_j == c, then fma(gamma * coef_jc, sigmoid(t_ji + U[c][i]), .) - and the four partial sums meet as
// (s0 + s1) + (s2 + s3); the sigmoid is that of the OLD U, which every thread reads before any thread writes.  gamma == 0: coef
// and T are not read.  hk_neg: the buffer holds -hk and is added (exact).  A label outside [0, C) takes its row out of every
// sum.  The last workgroup of a class sums 1[y_j == c] - 1[yk_j == c] (+ fma(gamma, coef_jc, .)) lane-strided, a butterfly,
// and applies the bias rule to yb[c]
__global__ __launch_bounds__(256) void class_joint_update_kernel(ClassJointArgs a) {
    __shared__ float s_part[4][64];
    const int c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool disc = a.gamma > 0.f;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {          // the class bias
        if (w != 0) return;
        float s = 0.f;
        for (int j = lane; j < a.B; j += 64) {
            const int t = a.y[j];
            if ((unsigned)t >= (unsigned)a.C) continue;
            s = __fadd_rn(s, __fsub_rn(t == c ? 1.f : 0.f, a.yk[j] == c ? 1.f : 0.f));
            if (disc) s = __fmaf_rn(a.gamma, a.coef[(size_t)j * a.C + c], s);
        }
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
        for (int j0 = w; j0 < a.B; j0 += 32) {            // eight of the wave's rows at a time: their labels are requested together
            int t[8], k[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j = j0 + 4 * q;
                t[q] = j < a.B ? a.y[j] : -1;
                k[q] = j < a.B ? a.yk[j] : -1;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {                     // ... the chain itself in ascending row order
                const int j = j0 + 4 * q;
                if ((unsigned)t[q] >= (unsigned)a.C) continue;
                const bool p = t[q] == c, n = k[q] == c;
                const float hp = p ? a.h0m[(size_t)j * a.ldh0 + i] : 0.f, hn = n ? a.hk[(size_t)j * a.ldhk + i] : 0.f;
                if (p) s = __fadd_rn(s, hp);
                if (n) s = a.hk_neg ? __fadd_rn(s, hn) : __fsub_rn(s, hn);
                if (disc) s = __fmaf_rn(__fmul_rn(a.gamma, a.coef[(size_t)j * a.C + c]), sigmoid(__fadd_rn(a.T[(size_t)j * a.ldt + i], u)), s);
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
void launch_class_joint_update(const ClassJointArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(class_joint_update_kernel, dim3((a.H + 63) / 64 + 1, a.C), dim3(256), 0, st, a);
}

// ---- class_mix_kernel: the hybrid objective's positive-phase operand h0m := fma(gamma, pos + negm, h0m), elementwise
__global__ __launch_bounds__(256) void class_mix_kernel(float *h0m, const float *pos, const float *negm, int ld, int B, int H, float gamma) {
    const long long n = (long long)B * H;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / H), i = (int)(e - (long long)j * H);
        const size_t o = (size_t)j * ld + i;
        h0m[o] = __fmaf_rn(gamma, __fadd_rn(pos[o], negm[o]), h0m[o]);
    }
}
void launch_class_mix(float *h0m, const float *pos, const float *negm, int ld, int B, int H, float gamma, hipStream_t st) {
    const long long n = (long long)B * H;
    hipLaunchKernelGGL(class_mix_kernel, dim3((int)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, h0m, pos, negm, ld, B, H, gamma);
}

// ---- class_v0_kernel: the Ber(1/2) start of bm_rbm_class_gibbs, every entry at its flat index of the global row
__global__ __launch_bounds__(256) void class_v0_kernel(float *v, int ld, int B, int V, PhiloxKey key, unsigned long long row0) {
    const long long n = (long long)B * V;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / V), i = (int)(e - (long long)j * V);
        v[(size_t)j * ld + i] = philox_uniform_at(key, (row0 + (unsigned long long)j) * (unsigned long long)V + i) < 0.5f ? 1.f : 0.f;
    }
}
void launch_class_v0(float *v, int ld, int B, int V, const PhiloxKey &key, long long row0, hipStream_t st) {
    const long long n = (long long)B * V;
    hipLaunchKernelGGL(class_v0_kernel, dim3((int)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, v, ld, B, V, key,
                       (unsigned long long)row0);
}

}  // namespace bm
