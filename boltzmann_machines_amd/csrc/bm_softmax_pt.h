// bm_softmax_pt.h — parallel tempering over softmax visible units (bm_rbm_groups_pt_*): the launchers of the start
// kernel and of the generic route's tempered groups kernel, compiled in bm_softmax_pt.hip next to the SM + SA + RT instantiations of
// act_kernel (launch_act_sm_pt, bm_launch.h).  Host code only.
//
// An ensemble row is a COMPLETE one-hot row: every group is there (no pattern of absent groups).  Row j carries its own temperature
// beta_j = row_mult[j]; the logits of its prop-down are l = fl(fl(beta_j z) + fl(beta_j b)) - two rounded multiplies and one rounded
// add, never an FMA - so that beta_j == 1 gives l = z + b, the plain softmax pass, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "bm_rng.h"

namespace bm {

// Start of the ensemble.  Row j < rows = M R (chain j / R, slot j % R):
//   V0 null: per group g one uniform category by the softmax-group rule of bm_softmax_v.h with zero logits - e = 1, c[k] = k + 1,
//            S = K, t = u K, the first k with c[k] > t - u the uniform at flat index (row0 + j) * V + g K on `key`;
//   V0 [M][V] (dense): the row of chain j / R, for all its R replicas (complete one-hot rows: the caller's guarantee).
// It leaves the slot partials of v_0 . vb in the order of pt_vb_slot (bm_pt.h) and sets row_mult[j] = beta[j % R], idx[j] = j % R -
// the contract of pt_init_kernel.  v [rows][ld]; part [ceil(V / 16)][ld_part], ld_part >= rows
struct SpStartArgs {
    float *v; int ld;
    int rows, R, V, K;
    const float *V0, *vb, *beta;             // [M][V] or null, [V], [R]
    PhiloxKey key; unsigned long long row0;
    float *part; int ld_part;
    float *row_mult; int *idx;               // [rows], [rows]
};
void launch_softmax_pt_init(const SpStartArgs &a, hipStream_t st);

// The generic route's groups step, behind a raw pass that left Z = h W^T [J][V] (kind 2, mult 1): per row j and group g the logits
// l[k] = fl(fl(beta_j Z[j][gK+k]) + fl(beta_j bias[gK+k])), beta_j = row_mult[j], then the operation sequence of
// softmax_groups_kernel (mx, e, sequential c, S, t = u S, the first k with c[k] > t; u at flat index (row0 + j) * V + g K on `key`)
// and the one-hot state into states [J][V].  Always samples; stores no means.  Any width K >= 2, any V % K == 0
struct SpGroupsArgs {
    const float *Z; int ldz;
    float *states; int ld_states;
    int V, K, J;
    const float *bias, *row_mult;            // [V], [J]
    PhiloxKey key; long long row0;
};
void launch_softmax_pt_groups(const SpGroupsArgs &a, hipStream_t st);

}  // namespace bm
