// bm_softmax_v.h — softmax (categorical) visible units: the launcher of softmax_groups_kernel, compiled in
// bm_softmax_v.hip.  Host code only.
//
// A visible layer of G = V / K groups of K mutually exclusive units, one-hot per group.  Groups of 2, 4, 8 or 16 in a layer of
// V % 4 == 0 are served by the SM flavour of act_kernel in one launch (ActArgs::sm_k; ActFlavour<FL_SM>, bm_launch.h).  For every
// other shape the prop-down is a pair of launches, as the Multinomial hidden layer's prop-up is: a kind-3 pass of act_kernel leaves
// the logits l = h W^T + vb, then softmax_groups_kernel turns every group of a row into its means and its one-hot state, in place.
// Both produce the same bits.
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
};
void launch_softmax_groups(const SgArgs &a, hipStream_t st);

}  // namespace bm
