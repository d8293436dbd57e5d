// bm_softmax_cl.hip - clamped groups of softmax visible units: the instantiations of act_kernel's SM + CL
// flavour - the SM epilogue with the CL block behind it, for exactly the geometries SM has.  A translation unit of its own, as
// bm_class_joint.hip is beside bm_class.hip: with these instantiations in bm_softmax_v.hip the compiler allocates the registers
// of three of the SM instantiations differently (1 VGPR), and those are to stay exactly what they were
// (profiles/softmax_missing_resources.md).  Compiled into libbm355.so next to bm355.hip.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"

namespace bm {

void launch_act_smcl_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_xm_as<FL_SM | FL_CL>(geo, a, st); }

}  // namespace bm
