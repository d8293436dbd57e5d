// bm_stack.hip - back-propagation below a class head: the BP flavour of act_kernel with its launcher, and the
// elementwise kernel that forms g = pos + negm of the top handle.  A translation unit of its own, as bm_class.hip is: the kernels
// of the other units are compiled exactly as before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_stack.h"

namespace bm {

// A BP pass is a prop-down from W itself (x-major P): only those kernels are instantiated.  The tile map and the 16-byte / generic
// choice are dispatch_act's
template <class G, int MINB, int STG>
static inline void launch_act_bp_geo(const ActArgs &a, hipStream_t st) {
    const double kt = (double)a.K1;
    const TileMap tmap = make_tile_map((a.I + G::TI - 1) / G::TI, (a.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, a.map_xi);
    const bool fast = operand_fast(a.P1, XM, a.K1) && operand_fast(a.Q1, XM, a.K1);
    launch_act_kernel<G, MINB, STG, FL_BP, false, XM>(fast, 0, st, a, tmap);
}
// geo: the codes of launch_act_as, resolved as that ladder resolves them for an x-major P (6, 9, 4 -> 8; 5, 7 -> 3): every code
// lands on a geometry with MI == 1, none of them uses scratch (profiles/stack_resources.md)
void launch_act_bp_as(int geo, const ActArgs &a, hipStream_t st) {
    if (geo == 208) { launch_act_bp_geo<GeoAct8, 1, STG_DMAH>(a, st); return; }
    if (geo == 6 || geo == 9) geo = 8;
    if (geo == 5 || geo == 7) geo = 3;
    const bool reg = geo >= 100;
    geo %= 100;
    if (reg) {
        if (geo == 1)      launch_act_bp_geo<GeoActS, 2, STG_REG>(a, st);
        else if (geo == 3) launch_act_bp_geo<GeoActS32, 4, STG_REG>(a, st);
        else               launch_act_bp_geo<GeoAct8, 1, STG_REG>(a, st);
    } else {
        if (geo == 1)      launch_act_bp_geo<GeoActS, 2, STG_DMA>(a, st);
        else if (geo == 3) launch_act_bp_geo<GeoActS32, 4, STG_DMA>(a, st);
        else               launch_act_bp_geo<GeoAct8, 1, STG_DMA>(a, st);
    }
}

// ---- stack_g_kernel: elementwise over [B][H], one rounded add
__global__ __launch_bounds__(256) void stack_g_kernel(const float *pos, const float *negm, float *g, int ld, int B, int H) {
    const long long n = (long long)B * H;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / H), i = (int)(e - (long long)j * H);
        const size_t o = (size_t)j * ld + i;
        g[o] = __fadd_rn(pos[o], negm[o]);
    }
}
void launch_stack_g(const float *pos, const float *negm, float *g, int ld, int B, int H, hipStream_t st) {
    const long long n = (long long)B * H;
    const int nb = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(stack_g_kernel, dim3(nb), dim3(256), 0, st, pos, negm, g, ld, B, H);
}

}  // namespace bm
