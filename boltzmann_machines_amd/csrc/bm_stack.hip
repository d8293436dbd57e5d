// bm_stack.hip - back-propagation below a class head: the instantiations of act_kernel's BP flavour, and the
// elementwise kernel that forms g = pos + negm of the top handle.  A translation unit of its own, as bm_class.hip is: the kernels
// of the other units are compiled exactly as before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_stack.h"

namespace bm {

// A BP pass is a prop-down from W itself (x-major P): only those kernels are instantiated (bm_launch.h: ActFlavour<FL_BP>::xm_only)
void launch_act_bp_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_BP>(geo, a, st); }

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
