// bm355.hip — the main translation unit of libbm355.so (bm_grad_cen.hip, the centred flavour of grad_kernel, is the only other one).  The kernels live in headers
// (bm_kernels.h; their launchers and the launch tuner in bm_launch.h, included at its end) shared by the RBM and DBM entry
// points, so both are compiled together; bm_rbm64.hip / bm_dbm64.hip are the float64 paths (own small kernels).
#include "bm_rbm.hip"
#include "bm_rbm_pt.hip"      // (the tempered entries of the RBM handle: part of this unit, it uses bm_rbm.hip's statics)
#include "bm_dbm.hip"
#include "bm_rbm64.hip"
#include "bm_dbm64.hip"
#include "bm_comm.hip"
#include "bm_xchg.hip"
