// bm_grad_fast.hip - fast-weights PCD: the fast-weights flavour of grad_kernel, its instantiations and their
// launcher, and the two small kernels of the mode (fast bias update, refresh of the effective copies), in a translation unit of
// their own as bm_grad_cen.hip is (bm_launch.h says why).  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_fast.h"

namespace bm {

template <class G>
static inline void launch_grad_fast_geo(const GradArgs &g, const GradFast &f, hipStream_t st) {
    const double kt = (double)g.Kpos + (double)g.Kneg;
    const TileMap tmap = make_tile_map((g.I + G::TI - 1) / G::TI, (g.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, g.map_xi);
    const bool fast = operand_fast(g.Ppos, KM, g.Kpos) && operand_fast(g.Qpos, KM, g.Kpos) &&
                      operand_fast(g.Pneg, KM, g.Kneg) && operand_fast(g.Qneg, KM, g.Kneg);
    static_assert(G::SMEM_FLOATS >= CS_SMEM_FLOATS, "the bias tail reuses the tile LDS");
    const dim3 grid(((g.I + G::TI - 1) / G::TI) * ((g.J + G::TJ - 1) / G::TJ) + g.nbias), blk(G::NT);
    if (fast) hipLaunchKernelGGL((grad_kernel<G, true, 0, STG_DMA, 1, GradFast>), grid, blk, 0, st, g, tmap, f);
    else      hipLaunchKernelGGL((grad_kernel<G, false, 0, STG_DMA, 1, GradFast>), grid, blk, 0, st, g, tmap, f);
}

void launch_grad_fast(int geo, const GradArgs &g, const GradFast &f, hipStream_t st) {
    if (geo == 8) launch_grad_fast_geo<GeoGrad8>(g, f, st);
    else          launch_grad_fast_geo<GeoGrad>(g, f, st);
}

// one thread per bias: visible units first, then hidden ones
static __global__ __launch_bounds__(256) void fast_bias_kernel(FastBiasArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.V + a.H) return;
    const bool vis = c < a.V;
    const int u = vis ? c : c - a.V;
    const float g0 = __fdiv_rn(vis ? a.sv[u] : a.sh[u], a.N);
    float *bf = vis ? a.vbf : a.hbf, *be = vis ? a.vbe : a.hbe;
    const float f = __fadd_rn(__fmul_rn(a.fast_decay, bf[u]), __fmul_rn(a.fast_lr, g0));
    bf[u] = f;
    be[u] = __fadd_rn((vis ? a.vb : a.hb)[u], f);
}

void launch_fast_bias(const FastBiasArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(fast_bias_kernel, dim3((a.V + a.H + 255) / 256), dim3(256), 0, st, a);
}

// one thread per weight (h fastest: coalesced along the rows of W); the first V + H threads also take one bias each
static __global__ __launch_bounds__(256) void fast_refresh_kernel(FastRefreshArgs a) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < a.V) a.vbe[e] = __fadd_rn(a.vb[e], a.vbf[e]);
    else if (e < a.V + a.H) a.hbe[e - a.V] = __fadd_rn(a.hb[e - a.V], a.hbf[e - a.V]);
    if (e >= (long long)a.V * a.H) return;
    const int v = (int)(e / a.H), h = (int)(e % a.H);
    a.We[(size_t)v * a.ldf + h] = __fadd_rn(a.W[(size_t)v * a.ldw + h], a.Wf[(size_t)v * a.ldf + h]);
}

void launch_fast_refresh(const FastRefreshArgs &a, hipStream_t st) {
    // (V * H >= V + H fails only for a 1 x n model: cover the biases as well)
    const long long n = std::max((long long)a.V * a.H, (long long)a.V + a.H);
    hipLaunchKernelGGL(fast_refresh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    if (a.Wet) {
        const int nt = ((a.V + 31) / 32) * ((a.H + 31) / 32);
        hipLaunchKernelGGL(transpose_kernel, dim3(nt), dim3(256), 0, st, (const float *)a.We, a.ldf, a.Wet, a.ldet, a.V, a.H);
    }
}

}  // namespace bm
