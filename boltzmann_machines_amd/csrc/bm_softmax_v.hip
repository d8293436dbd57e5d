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
            float m = e / S;
            float sv = a.sample ? ((c > t && !(cp > t)) ? 1.0f : 0.0f) : m;
            if (a.clamp_mask) {              // a clamped unit (the mask is constant within the group): both are the clamp value
                const size_t oc = (size_t)row * a.ld_clamp + i0 + k;
                if (a.clamp_mask[oc] != 0.f) { m = a.clamp_val[oc]; sv = m; }
            }
            l[i0 + k] = m;
            if (s) s[i0 + k] = sv;
        }
    }
}

void launch_softmax_groups(const SgArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(softmax_groups_kernel, dim3((a.J + 3) / 4), dim3(256), 0, st, a);
}

// ---- group_missing_mask_kernel: a thread per (row, group) in turn; an empty group marks its K units
__global__ __launch_bounds__(256) void group_missing_mask_kernel(const float *X, int ldx, float *M, int ldm, int B, int V, int K) {
    const int G = V / K;
    const long long n = (long long)B * G;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const int b = (int)(t / G), g = (int)(t % G);
        const float *x = X + (size_t)b * ldx + (size_t)g * K;
        bool any = false;
        for (int k = 0; k < K; ++k) any = any || (x[k] != 0.f);
        float *m = M + (size_t)b * ldm + (size_t)g * K;
        for (int k = 0; k < K; ++k) m[k] = any ? 0.f : 1.f;
    }
}

void launch_group_missing_mask(const float *X, int ldx, float *M, int ldm, int B, int V, int K, hipStream_t st) {
    const long long n = (long long)B * (V / K);
    const int nb = (int)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(group_missing_mask_kernel, dim3(nb), dim3(256), 0, st, X, ldx, M, ldm, B, V, K);
}

// ---- group_scores_kernel (bm_softmax_v.h: GsArgs).  A wave takes 64 / NS rows of ONE group and a chunk of at most KC <= 16 of its
// categories: the lane's row is lane % (64 / NS), its share of the j range the segment lane / (64 / NS) - contiguous, a multiple of
// 4 long, a function of H and NS alone.  With NS == 1 every address of W is wave-uniform (the compiler keeps those loads uniform);
// the lane reads its own row of z in 16-byte pieces.  GATHER == false (K <= 16, one chunk): W[c] is one of the chunk's own KC values,
// picked by the lane's c; GATHER == true (wider groups, chunks of 16, each re-walking j): W[c][j] is loaded per lane.  KC double
// accumulators per lane, fully unrolled (no scratch); the NS partial sums are added in double in the order of the segments, through
// lane reads (no LDS).  Rows past B run on row B - 1 and store nothing.
template <int KC, int NS, bool GATHER>
__global__ __launch_bounds__(256) void group_scores_kernel(GsArgs a, int nchunk) {
    constexpr int RW = 64 / NS;
    const int lane = threadIdx.x & 63;
    const int G = a.V / a.K;
    const long long units = (long long)((a.B + RW - 1) / RW) * G * nchunk;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= units) return;                     // wave-uniform
    const int ch = (int)(wave % nchunk);
    const long long t = wave / nchunk;
    const int g = (int)(t % G), rb = (int)(t / G);
    const int r = lane % RW, seg = lane / RW;
    const int b = rb * RW + r;
    const bool live = b < a.B;
    const int bb = live ? b : a.B - 1;
    const int k0 = ch * 16;
    const int kn = (a.K - k0 < KC) ? a.K - k0 : KC;
    int c = -1;                                    // the group's current unit: the first non-zero entry; none: the group is empty
    {
        const float *x = a.X + (size_t)bb * a.ldx + (size_t)g * a.K;
        for (int k = a.K - 1; k >= 0; --k) if (x[k] != 0.f) c = k;
    }
    const int H = a.H;
    const int seg_len = (((H + NS - 1) / NS) + 3) & ~3;
    const int j0 = seg * seg_len, j1 = (j0 + seg_len < H) ? j0 + seg_len : H;
    const float *zrow = a.Z + (size_t)bb * a.ldz;
    const float *wg = a.W + ((size_t)g * a.K + k0) * a.ldw;
    const float *wcrow = a.W + ((size_t)g * a.K + (c < 0 ? 0 : c)) * a.ldw;
    double acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = (seg == 0 && k < kn) ? (double)a.vb[g * a.K + k0 + k] : 0.0;
    for (int j = j0; j < j1; j += 4) {             // (ldz % 4 == 0 and a 16-byte base: the workspace is the engine's own)
        const float4 zq = *reinterpret_cast<const float4 *>(zrow + j);
        const float zv[4] = {zq.x, zq.y, zq.z, zq.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (j + q >= j1) break;
            float w[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) w[k] = (k < kn) ? wg[(size_t)k * a.ldw + j + q] : 0.f;
            float wc = 0.f;                        // empty group: a = z - 0 = z, bit for bit
            if constexpr (GATHER) { if (c >= 0) wc = wcrow[j + q]; }
            else {
#pragma unroll
                for (int k = 0; k < KC; ++k) if (c == k) wc = w[k];
            }
            const float av = __fsub_rn(zv[q], wc);
#pragma unroll
            for (int k = 0; k < KC; ++k)
                if (k < kn) acc[k] += (double)softplus_hw(__fadd_rn(av, w[k]));
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        double tot = acc[k];
        if constexpr (NS > 1) {
            tot = __shfl(acc[k], r);
#pragma unroll
            for (int s = 1; s < NS; ++s) tot += __shfl(acc[k], r + s * RW);
        }
        if (live && seg == 0 && k < kn) a.S[(size_t)b * a.V + (size_t)g * a.K + k0 + k] = tot;
    }
}

template <int KC, bool GATHER>
static void launch_group_scores_kc(const GsArgs &a, int nchunk, hipStream_t st) {
    // the split of the j range is a function of the shape alone: four segments unless whole waves of 64 rows already make 4096
    // waves (four per SIMD of 256 CUs) or H is too short to split (profiles/softmax_missing_bench.md has the measurement)
    const int G = a.V / a.K;
    const long long u1 = (long long)((a.B + 63) / 64) * G * nchunk;
#ifdef BM_GS_FORCE_NS             // (experiments only: a build that forces the split, for the A/B of profiles/softmax_missing_bench.md)
    static_assert(BM_GS_FORCE_NS == 1 || BM_GS_FORCE_NS == 4, "group_scores_kernel is instantiated for 1 and 4 segments");
    const int ns = BM_GS_FORCE_NS;
#else
    const int ns = (u1 >= 4096 || a.H < 16) ? 1 : 4;
#endif
    const int rw = 64 / ns;
    const long long units = (long long)((a.B + rw - 1) / rw) * G * nchunk;
    const dim3 grid((unsigned)((units + 3) / 4)), blk(256);
    if (ns == 1) hipLaunchKernelGGL((group_scores_kernel<KC, 1, GATHER>), grid, blk, 0, st, a, nchunk);
    else         hipLaunchKernelGGL((group_scores_kernel<KC, 4, GATHER>), grid, blk, 0, st, a, nchunk);
}

void launch_group_scores(const GsArgs &a, hipStream_t st) {
    if (a.K > 16)      launch_group_scores_kc<16, true>(a, (a.K + 15) / 16, st);
    else if (a.K > 8)  launch_group_scores_kc<16, false>(a, 1, st);
    else if (a.K > 4)  launch_group_scores_kc<8, false>(a, 1, st);
    else if (a.K > 2)  launch_group_scores_kc<4, false>(a, 1, st);
    else               launch_group_scores_kc<2, false>(a, 1, st);
}

}  // namespace bm
