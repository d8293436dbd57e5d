// bm_fast.h - fast-weights PCD (FPCD, Tieleman & Hinton 2009): what the RBM engine and bm_grad_fast.hip share.
// The fast set Wf, vbf, hbf decays quickly and learns from the update's own gradient; the tempered ensemble runs under the
// effective set We = W + Wf, vbe = vb + vbf, hbe = hb + hbf.  The weight part of the update is grad_kernel's fast-weights
// flavour (bm_kernels.h: GradFast); the two kernels described here are fixed order, one thread per element.  Host code only.
#pragma once
#include "bm_common.h"
#include "bm_kernels.h"

namespace bm {

// The fast bias update, behind the regular update in stream order: g0 = s / N from the raw column sums the update published
// (raw_tail: sv [V] | sh [H]), the IEEE division of rbm_bias_apply and no penalty term;
//   bf <- decay * bf + fast_lr * g0;  be <- b_new + bf      (every product and sum rounded once)
struct FastBiasArgs {
    const float *sv, *sh;             // raw column sums
    const float *vb, *hb;             // the regular biases AFTER their update
    float *vbf, *hbf, *vbe, *hbe;
    int V, H;
    float N, fast_lr, fast_decay;
};
// The refresh: the effective copies from the regular and the fast set (the effective transpose where Wet is not null)
struct FastRefreshArgs {
    const float *W, *Wf; float *We, *Wet;
    int V, H, ldw, ldf, ldet;
    const float *vb, *vbf, *hb, *hbf; float *vbe, *hbe;
};

// (bm_grad_fast.hip)
// geo: 4 | 8 waves, as launch_grad_cen; fused only; the bias tail (g.nbias) and a penalty (g.pen) are both legal
void launch_grad_fast(int geo, const GradArgs &g, const GradFast &f, hipStream_t st);
void launch_fast_bias(const FastBiasArgs &a, hipStream_t st);
void launch_fast_refresh(const FastRefreshArgs &a, hipStream_t st);

}  // namespace bm
