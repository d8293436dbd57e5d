// bm_class.h — the class head of a Bernoulli RBM (Larochelle & Bengio 2008, "Classification using discriminative
// restricted Boltzmann machines"): the arguments and launchers of its kernels.  The kernels themselves, and the CR flavour of
// act_kernel that feeds them, are compiled in bm_class.hip.  Host code only.
//
//   z_i        = (x W)_i + hb_i
//   s_c        = yb_c + sum_i softplus(z_i + U[c][i])
//   log p(c|x) = s_c - logsumexp_c' s_c'
//
// One discriminative update (ascent of the batch mean of log p(t|x)), in stream order:
//   1. act_kernel, CR flavour      t = z + hb as [B][H]; per class the slot partials of sum_i softplus(t_i + U[c][i])
//   2. class_row_kernel            s_c, logsumexp, log p, p, coef = 1[c == t] - p; the row's log p(t|x) and hit      (double sums)
//   3. class_hidden_kernel         pos = sigmoid(t + U[t_j]),  negm = -sum_c p_c sigmoid(t + U[c])  ->  the h0 / -h_k buffers
//   4. class_head_update_kernel    dU, dyb from coef and the recomputed sigmoids; the U and yb update rules
//   5. grad_kernel form 0 + bias tail, unchanged, with the input as its negative-phase visible operand: W, W^T, hb, vb
#pragma once
#include <hip/hip_runtime.h>
#include "bm_rng.h"

namespace bm {

struct ClassRowArgs {
    const float *part;        // [C][nslots][ldp] slot partials (ActArgs::cr_part)
    int ldp, nslots, C, B;
    const float *yb;          // [C]
    const int *y;             // [B] labels or null (prediction: logp / prob only)
    float *logp, *prob;       // [B][C] dense
    float *coef;              // [B][C]: 1[c == t] - p(c|x); a row whose label is outside [0, C): zeros
    int *tl;                  // [B]: the label, -1 where it is outside [0, C)
    float *rowlp, *rowhit;    // [B]: log p(t|x) and 1[argmax == t] (0 for a bad label)
    int *bad;                 // device flag raised by a label outside [0, C)
};
struct ClassHiddenArgs {
    const float *T;           // [B][H] pitch ldt: t = z + hb
    const float *U;           // [C][H] pitch ldu
    const float *prob;        // [B][C]
    const int *tl;            // [B]
    float *pos, *negm;        // [B][H] pitch ld
    int ldt, ldu, ld, B, H, C;
};
struct ClassHeadArgs {
    const float *T;           // [B][H] pitch ldt
    const float *coef;        // [B][C]
    float *U, *dU;            // [C][H] pitch ldu
    float *yb, *dyb;          // [C]
    int ldt, ldu, B, H, C;
    float N, l2, lr, mom;
};

// ---- joint training of p(x, y): the CD-k chain on (x, y) and the U / yb update behind it; these kernels and
// the CB flavour of act_kernel are compiled in bm_class_joint.hip
//   p(h_i = 1 | x, y) = sigmoid((x W)_i + hb_i + U[y][i])      act_kernel, CB flavour (LayerPass::class_bias)
//   p(y = c | h)      = softmax_c(yb_c + sum_i h_i U[c][i])     class_draw_kernel
//   dU[c][i] = (1/B) sum_j (1[y_j = c] h0m_ji - 1[yk_j = c] hk_ji + gamma coef_jc sigmoid(t_ji + U[c][i])),  dyb alike
struct ClassDrawArgs {
    const float *h;           // [B][H] pitch ldh: what the chain feeds downward (states or means)
    const float *U;           // [C][H] pitch ldu
    const float *yb;          // [C]
    int *y;                   // [B] out
    int ldh, ldu, B, H, C;
    PhiloxKey key;            // one uniform per row, at flat index row0 + j
    long long row0;
};
struct ClassJointArgs {
    const int *y, *yk;        // [B] the labels (outside [0, C): the row is out of every sum) and the chain's last class draws
    const float *h0m;         // [B][H] pitch ldh0: E[h | x, y]
    const float *hk;          // [B][H] pitch ldhk: E[h | v_k, y_k], or its negation (hk_neg)
    int ldh0, ldhk, hk_neg;
    float gamma;              // the discriminative weight; 0: coef and T are not read
    const float *coef;        // [B][C]
    const float *T;           // [B][H] pitch ldt: t = x W + hb
    float *U, *dU;            // [C][H] pitch ldu
    float *yb, *dyb;          // [C]
    int ldt, ldu, B, H, C;
    float N, l2, lr, mom;
};
void launch_class_draw(const ClassDrawArgs &a, hipStream_t st);
void launch_class_joint_update(const ClassJointArgs &a, hipStream_t st);
// h0m := fma(gamma, pos + negm, h0m), elementwise over [B][H] (pitch ld each)
void launch_class_mix(float *h0m, const float *pos, const float *negm, int ld, int B, int H, float gamma, hipStream_t st);
// v [B][V] (pitch ld) := Ber(1/2), u < 0.5 at flat index (row0 + j) V + i
void launch_class_v0(float *v, int ld, int B, int V, const PhiloxKey &key, long long row0, hipStream_t st);

void launch_class_row(const ClassRowArgs &a, hipStream_t st);
void launch_class_hidden(const ClassHiddenArgs &a, hipStream_t st);
void launch_class_head_update(const ClassHeadArgs &a, hipStream_t st);
// acc[0] += sum_j rowlp[j], acc[1] += sum_j rowhit[j], in double, in an order that depends on B alone
void launch_class_sum(const float *rowlp, const float *rowhit, int B, double *acc, hipStream_t st);

}  // namespace bm
