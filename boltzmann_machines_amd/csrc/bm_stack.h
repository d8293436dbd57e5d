// bm_stack.h — fine-tuning a stack of sigmoid layers below a class head by back-propagation: the launchers of
// the kernels compiled in bm_stack.hip.  Host code only.
//
//   a_0 = x,  a_l = sigmoid(a_{l-1} W_l + hb_l)  (l = 1..D),  log p(c|x) = the head's exact posterior (3.18) of the top RBM on a_D
//
// One update (ascent of the batch mean of log p(t|x)); ' marks pre-update values, g = pos + negm of the top handle:
//   delta_D = (g W_top'^T)             .* a_D .* (1 - a_D)
//   delta_l = (delta_{l+1} W_{l+1}'^T) .* a_l .* (1 - a_l)
//   layer l: the handle's fused update on (a_{l-1}, delta_l) against (a_{l-1}, 0);  top: the update of 3.18 on the input a_D
// The launches of one update are listed in bm_rbm.hip (stack_update).
#pragma once
#include <hip/hip_runtime.h>

namespace bm {

// g[j][i] = __fadd_rn(pos[j][i], negm[j][i]), elementwise over [B][H] (pitch ld each); pos and negm keep their bits
void launch_stack_g(const float *pos, const float *negm, float *g, int ld, int B, int H, hipStream_t st);

}  // namespace bm
