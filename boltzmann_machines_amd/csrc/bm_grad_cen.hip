// bm_grad_cen.hip - the centred flavour of grad_kernel: its instantiations and their launcher, in a translation
// unit of their own (bm_launch.h says why).  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"

namespace bm {

void launch_grad_cen(int geo, const GradArgs &g, const GradCen &cen, hipStream_t st);      // (bm_launch.h)

template <class G>
static inline void launch_grad_cen_geo(const GradArgs &g, const GradCen &cen, hipStream_t st) {
    const double kt = (double)g.Kpos + (double)g.Kneg;
    const TileMap tmap = make_tile_map((g.I + G::TI - 1) / G::TI, (g.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, g.map_xi);
    const bool fast = operand_fast(g.Ppos, KM, g.Kpos) && operand_fast(g.Qpos, KM, g.Kpos) &&
                      operand_fast(g.Pneg, KM, g.Kneg) && operand_fast(g.Qneg, KM, g.Kneg);
    const dim3 grid(((g.I + G::TI - 1) / G::TI) * ((g.J + G::TJ - 1) / G::TJ)), blk(G::NT);
    if (fast) hipLaunchKernelGGL((grad_kernel<G, true, 0, STG_DMA, 1, GradCen>), grid, blk, 0, st, g, tmap, cen);
    else      hipLaunchKernelGGL((grad_kernel<G, false, 0, STG_DMA, 1, GradCen>), grid, blk, 0, st, g, tmap, cen);
}

void launch_grad_cen(int geo, const GradArgs &g, const GradCen &cen, hipStream_t st) {
    if (geo == 8) launch_grad_cen_geo<GeoGrad8>(g, cen, st);
    else          launch_grad_cen_geo<GeoGrad>(g, cen, st);
}

}  // namespace bm
