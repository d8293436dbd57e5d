// bm_gauss.h — Gaussian visible units as one joint model (bm_rbm_gauss_ais, bm_rbm_gauss_free_energy_rows, bm_rbm_gauss_pt_*;
// DESIGN.md 3.30): the launchers of the small kernels, compiled in bm_gauss.hip next to the RT + GT instantiations of act_kernel
// (launch_act_gauss_pt, bm_launch.h).  Host code only.
//
// Everything runs on the SCALED variable u = x / sigma, with unit variance and centre c_i = fl32(vb_i / sigma_i):
//   E(u, h) = 1/2 |u - c|^2 - u W h - hb.h,    h | u ~ Ber(sigmoid(u W + hb)),    u | h ~ N(c + W h, I).
// Data units appear at the boundary only: u = fl32(x / sigma) on the way in, x = fl32(u sigma) on the way out.
#pragma once
#include <hip/hip_runtime.h>
#include "bm_rng.h"

namespace bm {

// c[i] = vb[i] / sigma[i] (one correctly rounded division: what div_cols_kernel does to a batch) and ones[i] = 1, i < V
void launch_gauss_prep(const float *vb, const float *sigma, int V, float *c, float *ones, hipStream_t st);

// AIS start: u_0 = a + n per row j < rows and unit i, n the standard normal at flat index (row0 + j) * V + i on `key` (the Gaussian
// layer's word-to-draw mapping, draw4), and the slot partials of u_0 . dvec for the first score: the whole dot product in slot 0 (a
// lane's units in ascending order, then a butterfly over the 64 lanes), zeros in the slots 1 .. nslot - 1 - the contract of
// rbm_ais_init_kernel.  v [rows][ld]; part [nslot][ld_part], ld_part >= rows
struct GaStartArgs {
    float *v; int ld;
    int rows, V;
    const float *abase, *dvec;               // [V], [V]
    PhiloxKey key; unsigned long long row0;
    float *part; int ld_part, nslot;
};
void launch_gauss_ais_start(const GaStartArgs &a, hipStream_t st);

// F(u_j) = 1/2 |u_j - c|^2 - sum_i softplus((u_j W + hb)_i) per row j < rows, from the slot partials of the softplus terms a prop-up
// left (ActArgs::rowacc_single) and the row itself, in double, in a fixed order: one wave per row, a lane's units then its slots in
// ascending order, then a butterfly over the 64 lanes.  U [rows][ldu]; part [nslot][ld_part]; out [rows] double
void launch_gauss_fe_rows(const float *U, int ldu, int rows, int V, const float *c, const float *part, int ld_part, int nslot, double *out,
                          hipStream_t st);

// Start of the tempered ensemble.  Row j < rows = M R (chain j / R, slot r = j % R):
//   V0 null: u_0 = __fadd_rn(c, __fmul_rn(n, sd[r])), n the standard normal at flat index (row0 + j) * V + i on `key`;
//   V0 [M][V] (dense, data units): u_0 = __fdiv_rn(V0[j / R][i], sigma[i]) for all R replicas of the chain.
// It leaves the slot partials of -1/2 (u_0 - c)^2 - d = __fsub_rn(u, c), term __fmul_rn(__fmul_rn(-0.5f, d), d), quads left to right,
// then (q0 + q1) + (q2 + q3): the arithmetic of the GT flavour - and sets row_mult[j] = beta[r], idx[j] = r.
// v [rows][ld]; part [ceil(V / 16)][ld_part], ld_part >= rows
struct GpStartArgs {
    float *v; int ld;
    int rows, R, V;
    const float *V0, *c, *sigma, *beta, *sd; // [M][V] or null, [V], [V], [R], [R]
    PhiloxKey key; unsigned long long row0;
    float *part; int ld_part;
    float *row_mult; int *idx;               // [rows], [rows]
};
void launch_gauss_pt_init(const GpStartArgs &a, hipStream_t st);

// The generic route's second launch, behind a raw pass that left Z = h W^T [J][V] (kind 2, mult 1): states and slot partials of the GT
// flavour, operation by operation (m = z + c, s = m + n sd[idx[j]], -1/2 (s - c)^2 by slots), n at flat index (row0 + j) * V + i
struct GpRowsArgs {
    const float *Z; int ldz;
    float *states; int ld_states;
    int V, J;
    const float *c, *sd; const int *idx;     // [V], [R], [J]
    PhiloxKey key; long long row0;
    float *part; int ld_part;
};
void launch_gauss_pt_rows(const GpRowsArgs &a, hipStream_t st);

// x[j][i] = __fmul_rn(x[j][i], sigma[i]) in place, dense [rows][V]: the read-out of the beta = 1 rows in data units
void launch_gauss_scale_rows(float *x, int rows, int V, const float *sigma, hipStream_t st);

}  // namespace bm
