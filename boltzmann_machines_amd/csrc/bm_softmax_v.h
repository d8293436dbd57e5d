// bm_softmax_v.h — softmax (categorical) visible units: the launchers of softmax_groups_kernel,
// group_missing_mask_kernel and group_scores_kernel, compiled in bm_softmax_v.hip.  Host code only.
//
// A visible layer of G = V / K groups of K mutually exclusive units, one-hot per group.  Groups of 2, 4, 8 or 16 in a layer of
// V % 4 == 0 are served by the SM flavour of act_kernel in one launch (ActArgs::sm_k; ActFlavour<FL_SM>, bm_launch.h).  For every
// other shape the prop-down is a pair of launches, as the Multinomial hidden layer's prop-up is: a kind-3 pass of act_kernel leaves
// the logits l = h W^T + vb, then softmax_groups_kernel turns every group of a row into its means and its one-hot state, in place.
// Both produce the same bits.
//
// Clamped groups: a clamp mask that is constant within every group (the caller's guarantee, not checked on the
// device) holds whole groups at clamp_val - an observed group at its one-hot value, a missing group at zeros.  Fused path: the
// SM + CL flavour (the CL block of act_epilogue behind the SM block); generic path: the clamp fields of SgArgs.  Means, states
// and uniforms of the free groups are those of the unclamped pass; a clamped group's uniform is consumed by position, not used.
#pragma once
#include <hip/hip_runtime.h>
#include "bm_rng.h"

namespace bm {

// Per row j and group g, sequentially left to right in float32 - the operation sequence of softmax_multinomial_kernel (and of
// the oracle's softmax_multinomial_row) at width K with M = 1 and one draw:
//   mx = max_k l[k];  e[k] = exp_neg(min(mx - l[k], 80));  c[k] = c[k-1] + e[k], c[-1] = 0;  S = c[K-1];  mean[k] = e[k] / S
//   u = the uniform at flat index (row0 + j) * V + g K on `key` (the layer's per-element stream, read at the group's first unit)
//   t = u * S;  state[k] = (c[k] > t) && !(c[k-1] > t)          - the first k with c[k] > t; it exists: t < S
// sample == 0: state = mean.
struct SgArgs {
    float *L; int ld;                // [J][V] logits in, means out (in place)
    float *states; int ld_states;    // [J][V], may be null
    int V, K, J, sample;             // V % K == 0, K >= 2
    PhiloxKey key; long long row0;
    // clamped groups: a unit with clamp_mask != 0 stores clamp_val as its mean and its state ([J][V], one pitch); null: none
    const float *clamp_val, *clamp_mask; int ld_clamp;
};
void launch_softmax_groups(const SgArgs &a, hipStream_t st);

// M[b][i] = 1 where the group of unit i is empty (all zeros) in X[b], else 0: the clamp mask of a row with missing groups
// (bm_rbm_groups_set_missing).  X [B][V] pitch ldx, M [B][V] pitch ldm
void launch_group_missing_mask(const float *X, int ldx, float *M, int ldm, int B, int V, int K, hipStream_t st);

// Exact group conditionals (bm_rbm_groups_scores).  For row b, whose groups are each one-hot or empty, group g
// with current unit c (none: empty) and category k:
//   a_j = z[b][j] - W[c][j] (one rounded float32 subtraction; empty: a_j = z[b][j]);  t_j = softplus_hw(a_j + W[gK+k][j]) in float32
//   S[b][gK+k] = vb[gK+k] + sum_j t_j, accumulated in double in ascending j
// so that log p(v_g = k | v_-g) = S[g][k] - logsumexp_k' S[g][k'].  z [B][H] = x W + hb in float32 (a kind-3 prop-up).
struct GsArgs {
    const float *X; int ldx;         // [B][V] rows
    const float *Z; int ldz;         // [B][H] pre-activations
    const float *W; int ldw;         // [V][H]
    const float *vb;                 // [V]
    double *S;                       // [B][V] dense
    int B, V, H, K;
};
void launch_group_scores(const GsArgs &a, hipStream_t st);

}  // namespace bm
