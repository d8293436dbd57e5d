// bm_softmax_pt.hip - parallel tempering over softmax visible units (bm_rbm_groups_pt_*): the instantiations of
// act_kernel's SM + SA + RT flavour - the softmax-group prop-down with a temperature per row that leaves the slot partials of
// state . dot_vec and hands the beta = 1 rows to the update, for exactly the geometries SM has - the start kernel and the tempered
// groups kernel of the generic route.  A translation unit of its own, as bm_softmax_ais.hip is beside bm_softmax_v.hip: the kernels
// of every other unit are compiled exactly as before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_pt.h"
#include "bm_softmax_pt.h"

namespace bm {

void launch_act_smpt_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_SM | FL_SA | FL_RT>(geo, a, st); }

// ---- softmax_pt_init_kernel (SpStartArgs).  One wave per row (four rows per workgroup).  First a lane per group in turn: the
// group's category and its K stores; then a lane per 16-column slot in turn: the slot's partial of v_0 . vb through pt_vb_slot, whose
// x_at(c) forms the state of unit c again from the group's uniform (or reads V0) - the same bits as the stores, and no lane reads what
// another lane wrote.  With zero logits e[k] = 1 and c[k] = k + 1 exactly (K < 2^24), S = K.  Every store is bounded by rows, V
// (g K + k < V: V % K == 0) and the slot count
__global__ __launch_bounds__(256) void softmax_pt_init_kernel(SpStartArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;                    // wave-uniform
    float *v = a.v + (size_t)row * a.ld;
    const float *v0 = a.V0 ? a.V0 + (size_t)(row / a.R) * a.V : nullptr;
    const int K = a.K, G = a.V / K;
    const unsigned long long base = (a.row0 + (unsigned long long)row) * (unsigned long long)a.V;
    const float S = (float)K;
    // the state of unit c of this row
    const auto unit = [&](int c) -> float {
        if (v0) return v0[c];
        const int g = c / K, k = c - g * K;
        const float t = __fmul_rn(philox_uniform_at(a.key, base + (unsigned long long)(g * K)), S);
        return ((float)(k + 1) > t && !((float)k > t)) ? 1.0f : 0.0f;
    };
    for (int g = lane; g < G; g += 64) {
        const int i0 = g * K;
        if (v0) {
            for (int k = 0; k < K; ++k) v[i0 + k] = v0[i0 + k];
            continue;
        }
        const float t = __fmul_rn(philox_uniform_at(a.key, base + (unsigned long long)i0), S);
        for (int k = 0; k < K; ++k) v[i0 + k] = ((float)(k + 1) > t && !((float)k > t)) ? 1.0f : 0.0f;
    }
    const int nslot = (a.V + 15) / 16;
    for (int slot = lane; slot < nslot; slot += 64) a.part[(size_t)slot * a.ld_part + row] = pt_vb_slot(slot, a.V, a.vb, unit);
    if (lane == 0) { a.row_mult[row] = a.beta[row % a.R]; a.idx[row] = row % a.R; }
}

void launch_softmax_pt_init(const SpStartArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(softmax_pt_init_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
}

// ---- softmax_pt_groups_kernel (SpGroupsArgs): softmax_groups_kernel's layout and three walks - maximum, S, then the draw - over
// logits that every walk forms again from the raw z, the bias and the row's temperature (the same three rounded operations give the
// same bits): nothing is kept between the walks but mx, S and the running c, no array per lane, no limit on K
__global__ __launch_bounds__(256) void softmax_pt_groups_kernel(SpGroupsArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.J) return;                       // wave-uniform
    const float *z = a.Z + (size_t)row * a.ldz;
    float *s = a.states + (size_t)row * a.ld_states;
    const float beta = a.row_mult[row];
    const int G = a.V / a.K;
    const auto logit = [&](int i) -> float { return __fadd_rn(__fmul_rn(beta, z[i]), __fmul_rn(beta, a.bias[i])); };
    for (int g = lane; g < G; g += 64) {
        const int i0 = g * a.K;
        float mx = -3.402823466e38f;
        for (int k = 0; k < a.K; ++k) mx = fmaxf(mx, logit(i0 + k));
        float S = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - logit(i0 + k);
            if (d > 80.0f) d = 80.0f;
            S = S + exp_neg(d);
        }
        const float u = philox_uniform_at(a.key, (unsigned long long)(a.row0 + row) * (unsigned long long)a.V + (unsigned long long)i0);
        const float t = u * S;
        float c = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            float d = mx - logit(i0 + k);
            if (d > 80.0f) d = 80.0f;
            const float cp = c;
            c = c + exp_neg(d);
            s[i0 + k] = (c > t && !(cp > t)) ? 1.0f : 0.0f;
        }
    }
}

void launch_softmax_pt_groups(const SpGroupsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(softmax_pt_groups_kernel, dim3((a.J + 3) / 4), dim3(256), 0, st, a);
}

}  // namespace bm
