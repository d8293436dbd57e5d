// bm_softmax_v.hip - softmax (categorical) visible units: the instantiations of act_kernel's SM flavour (groups
// of 2, 4, 8 or 16 units in a layer of V % 4 == 0), and softmax_groups_kernel, the generic path behind a logits pass for every
// other shape.  A translation unit of its own, as bm_stack.hip and bm_nrelu.hip are: the kernels of the other units are compiled
// exactly as before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_softmax_v.h"

namespace bm {

// An SM pass is a prop-down from W itself (x-major P): only those kernels are instantiated, as for the BP flavour (bm_launch.h:
// ActFlavour<FL_SM>::xm_only) - one quad per lane, which the epilogue's group logic is written for
void launch_act_sm_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_SM>(geo, a, st); }

// ---- softmax_groups_kernel: every width the SM flavour does not cover (3, 5, 10, 26, ...) and every layer with V % 4 != 0.
// One wave per row (four rows per workgroup), a lane per group in turn; the K units of a group are walked three times in the
// same order - maximum, S, then means and state - and nothing is kept between the walks but mx, S and the running c: e[k] is
// recomputed (exp_neg of the same d gives the same bits), so there is no array per lane, no LDS and no limit on K.  In place:
// walk 3 reads l[k] before it stores mean[k].
__global__ __launch_bounds__(256) void softmax_groups_kernel(SgArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.J) return;
    float *l = a.L + (size_t)row * a.ld;
    float *s = a.states ? a.states + (size_t)row * a.ld_states : nullptr;
    const int G = a.V / a.K;
    for (int g = lane; g < G; g += 64) {
        const int i0 = g * a.K;
        float mx = -3.402823466e38f;
        for (int k = 0; k < a.K; ++k) mx = fmaxf(mx, l[i0 + k]);
        float S = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - l[i0 + k];
            if (d > 80.0f) d = 80.0f;
            S = S + exp_neg(d);
        }
        float t = 0.0f;
        if (s && a.sample) {
            const float u = philox_uniform_at(a.key, (unsigned long long)(a.row0 + row) * (unsigned long long)a.V + (unsigned long long)i0);
            t = u * S;
        }
        float c = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - l[i0 + k];
            if (d > 80.0f) d = 80.0f;
            const float e = exp_neg(d);
            const float cp = c;
            c = c + e;
            const float m = e / S;
            l[i0 + k] = m;
            if (s) s[i0 + k] = a.sample ? ((c > t && !(cp > t)) ? 1.0f : 0.0f) : m;
        }
    }
}

void launch_softmax_groups(const SgArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(softmax_groups_kernel, dim3((a.J + 3) / 4), dim3(256), 0, st, a);
}

}  // namespace bm
