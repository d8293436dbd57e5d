// bm_softmax_ais.h — AIS over softmax visible units (bm_rbm_groups_ais): the launchers of the start kernel and of
// the generic route's row-dot kernel, compiled in bm_softmax_ais.hip next to the SM + SA instantiations of act_kernel
// (launch_act_sm_ais, bm_launch.h).  Host code only.
//
// A run has ONE pattern of observed groups, the same for every chain: `absent` [V] floats, non-zero on every unit of a group that
// is not part of the model (constant within a group), or null - every group is there.  Absent groups are stored as zeros; their
// uniforms are consumed by position, not used.
#pragma once
#include <hip/hip_runtime.h>
#include "bm_rng.h"

namespace bm {

// v_0: per row j < rows and group g, one categorical draw from the logits a_g by the softmax-group rule of bm_softmax_v.h (mx, e,
// sequential c, S, the first k with c[k] > u S), u the uniform at flat index (row0 + j) * V + g K on `key`; and the slot partials
// of v_0 . dvec for the first score: the whole dot product in slot 0 (a lane's groups in ascending order, then a butterfly over the
// 64 lanes: a fixed order that depends on nothing but V and K), zeros in the slots 1 .. nslot - 1 - the contract of
// rbm_ais_init_kernel.  v [rows][ld]; part [nslot][ld_part], ld_part >= rows
struct SaStartArgs {
    float *v; int ld;
    int rows, V, K;
    const float *abase, *dvec, *absent;     // [V], [V], [V] or null
    PhiloxKey key; unsigned long long row0;
    float *part; int ld_part, nslot;
};
void launch_softmax_ais_start(const SaStartArgs &a, hipStream_t st);

// part[s * ld_part + j] = the partial of x_j . dvec over the 16-column slot s, for every j < rows and s < ceil(V / 16): quads of 4
// consecutive columns left to right, then (q0 + q1) + (q2 + q3) - the order act_kernel's epilogue leaves (pt_vb_slot in bm_pt.h is
// the same order).  The generic route's third launch, behind the logits pass and softmax_groups_kernel
void launch_softmax_ais_dot(const float *x, int ldx, int rows, int V, const float *dvec, float *part, int ld_part, hipStream_t st);

}  // namespace bm
