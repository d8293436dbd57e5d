// bm_nrelu.hip - noisy rectified-linear hidden units: the instantiations of act_kernel's NR flavour.  A
// translation unit of its own, as bm_class.hip and bm_stack.hip are: the kernels of the other units are compiled exactly as
// before.  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"

namespace bm {

// geo: the codes of launch_act_as.  An NR pass is a single-segment prop-up in either operand layout: the ladder resolves the
// k-major-only tiles for an x-major P (W^T) as it does for the plain flavour
void launch_act_nr_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_as<FL_NR>(geo, a, st); }      // (bm_launch.h)

}  // namespace bm
