// bm_rsm.h — replicated softmax visible units (Salakhutdinov & Hinton 2009): the launchers of the kernels
// compiled in bm_rsm.hip.  Host code only.
//
// The visible layer is ONE softmax over the whole vocabulary of V units, sampled D_j times for row j and summed into a count
// vector; the hidden bias is scaled by the document length D_j.  The prop-up is the DB flavour of act_kernel (ActArgs::row_bmult;
// ActFlavour<FL_DB>, bm_launch.h).  The prop-down is a pair of launches: a kind-3 pass of act_kernel leaves the logits
// l = h W^T + vb, then multinomial_counts_kernel turns every row into its expected counts and its drawn counts, in place.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "bm_rng.h"

namespace bm {

constexpr int RSM_MAX_V = 16384;        // a row's prefix sums and counts live in LDS: 2 x 64 KiB of the CU's 160 KiB

// ---- row_lengths_kernel: D[j] = sum_i X[j][i], one wave per row, lane-strided partial sums and a butterfly.  The entries are
// integers and the sum is below 2^24 for every row that passes the checks, so every partial sum is an integer below 2^24, exact
// in float32: THE SUM IS EXACT IN ANY ORDER, and the order of this kernel is no part of the contract.  *bad (a device flag in the
// style of cb_bad) is OR-ed with RSM_BAD_NEGATIVE for a row with a negative entry, RSM_BAD_FRACTION for one with a non-integer
// entry (NaN and infinities included), RSM_BAD_EMPTY for D == 0 and RSM_BAD_LONG for D > max_length; the host turns it into an
// error that names the kind (bm_rbm_sync and every entry that waits for the stream anyway).
enum : int { RSM_BAD_NEGATIVE = 1, RSM_BAD_FRACTION = 2, RSM_BAD_EMPTY = 4, RSM_BAD_LONG = 8 };
struct RowLenArgs {
    const float *X; int ld, V, J;
    float *D;                        // [J]
    int max_length;
    int *bad;
};
void launch_row_lengths(const RowLenArgs &a, hipStream_t st);

// ---- multinomial_counts_kernel: one workgroup of 256 threads (four waves) per row j of the logits, everything in float32.
//   mx   = max_i l[i]
//   e[i] = exp_neg(min(mx - l[i], 80))                                   (bm_numerics.h; e = 0 for the padding i >= V)
//   c[i] = prefix sums of e in THE PREFIX ORDER below;  S = c[V-1]
//   mean[i] = __fmul_rn(D_j, e[i] / S)                                    - the expected counts, two rounded steps
//   draw d = 0 .. D_j - 1:  u = philox_uniform_at(key, (row0 + j) * max_length + d);  t = u * S;
//        category = the smallest i with c[i] > t, found by bisection - lo = 0, hi = V - 1; while lo < hi: mid = (lo + hi) >> 1;
//        c[mid] > t ? hi = mid : lo = mid + 1 - whose start hi = V - 1 is the clamp (t < S = c[V-1] in exact arithmetic, and
//        u S < S in float32 as well since u <= 1 - 2^-23); c is non-decreasing, so every probe sequence that is a correct search
//        returns the same i
//   state[i] = the number of draws that fell on i (integer LDS atomics: order-free);  sample == 0: state = mean
// THE PREFIX ORDER - parallel, monotone and a function of V alone (not of the launch geometry, J, or how a caller slices rows):
//   level 0  within each aligned run of 16 units [16 r, 16 r + 16): r_k = r_{k-1} + e[16 r + k], r_{-1} = 0, sequentially
//   level 1  within each aligned block of 256 units = 16 runs q = 0..15 with totals T_q = r_15 of run q: O_0 = 0,
//            O_q = O_{q-1} + T_{q-1} sequentially;  local[q][k] = O_q + r_k    (local of run 0 is r_k itself: 0 + x == x)
//   level 2  over the blocks b in ascending order: base_0 = 0, base_b = base_{b-1} + local_{b-1}[15][15] sequentially;
//            c[256 b + 16 q + k] = base_b + local_b[q][k]
// Every c is a sum of non-negative terms in which a later unit's c is reached from an earlier one's by rounded additions of
// non-negative numbers, and the carry into a run / block equals the last c of the run / block before it bit for bit: c is
// non-decreasing (DESIGN.md 3.27 has the proof).  A unit with e[i] == 0 exactly, or whose e[i] is absorbed (c[i] == c[i-1]),
// is never drawn.  tests/rsm_twin.py restates the order.
// Limits: 2 <= V <= RSM_MAX_V (launch_multinomial_counts refuses anything else with a message and returns non-zero); D_j is read
// per row from `lengths`; max_length is a property of the handle, so a row's draws do not depend on the batch it arrives in.
struct McArgs {
    float *L; int ld;                // [J][V] logits in, expected counts out (in place)
    float *states; int ld_states;    // [J][V] counts, may be null
    const float *lengths;            // [J] document lengths D_j (integers in float32)
    int V, J, sample, max_length;
    PhiloxKey key; long long row0;
};
int launch_multinomial_counts(const McArgs &a, hipStream_t st);

// ---- the AIS flavour of multinomial_counts_kernel (a template parameter: the instantiations above carry none of it; bm_rbm_rsm_ais,
// DESIGN.md 3.28).  Everything above, with sample == 1 and states; behind the draws the row also leaves its state . dvec for the
// next AIS score, from the counts in LDS (nothing is read back from memory):
//   s = sum_i (double)count[i] * (double)dvec[i]  - every product exact (counts are integers below 2^24, dvec is float32) - summed
//       in double by the three levels of the prefix order: within each aligned run of 16 units sequentially from 0; within each
//       aligned block of 16 runs the run totals sequentially from 0; the block totals in ascending order from 0.  The padding
//       past V adds exact zeros: the order is a function of V alone
//   part[row] = hi = (float)s;   part[ld_part + row] = lo = (float)(s - (double)hi)
// A float32 pair in two "slots" of pitch ld_part: ais_score_kernel adds slots in double, hi + lo, which is s to 2^-48 |s| (s - hi
// is exact in double, |s - hi| <= 2^-24 |s|, and lo rounds it to 2^-24 of that).  The tempered hidden pass that goes with it is the
// DB flavour at mult == bmult == beta (bm_kernels.h: ActArgs::row_bmult).
struct McAisArgs : McArgs {
    const float *dvec;               // [V]
    float *part; int ld_part;        // [2][ld_part], ld_part >= J
};
int launch_multinomial_counts_ais(const McAisArgs &a, hipStream_t st);

// ---- the PT flavour of multinomial_counts_kernel (a second template parameter on top of AIS: the plain and the AIS instantiations
// carry none of it; bm_rbm_rsm_pt_*).  The prop-down of a tempered ensemble, behind a raw pass (kind 2, mult 1) that
// left Z = h W^T in L:
//   l[i] = __fadd_rn(__fmul_rn(beta_j, Z[j][i]), __fmul_rn(beta_j, bias[i])),  beta_j = row_mult[j]   - formed on load, never stored;
//          RT's two rounded multiplies and one rounded add, so that beta_j == 1 gives l = z + b, the plain prop-down's logits
//          (a null L / a null bias read as zeros: the uniform start of an ensemble)
//   mx .. the draws: the operation sequence above (the prefix order, the bisection, the index (row0 + j) * max_length + d)
//   no means are stored (L is read only); it always samples
//   part: state . dvec as the AIS flavour leaves it (dvec = vb: the visible half of the swap energy, a float32 pair in TWO slots)
//   sel_out non-null: a row with row_mult[j] == 1.0f and j / sel_R < sel_rows stores its counts a second time at
//          sel_out + (j / sel_R) * sel_ld (the hand-over of a tempered update: what pt_gather_kernel would copy, bit for bit)
// A tempered prop-down moves 8 V bytes per row (Z in, counts out) where the plain route moves 12 V (logits in, means and counts out).
struct McPtArgs : McAisArgs {
    const float *bias;               // [V] or null
    const float *row_mult;           // [J]
    float *sel_out; int sel_ld, sel_R, sel_rows;
};
int launch_multinomial_counts_pt(const McPtArgs &a, hipStream_t st);

// ---- the kernels of bm_rsm_pt.hip
// rsm_pt_start_kernel: row j < rows = M R (chain j / R, slot j % R) gets row_mult[j] = beta[j % R], idx[j] = j % R,
// len[j] = chain_len[j / R] and, with a V0 [M][V] (dense), the count row of its chain.  V0_len [M] (row_lengths_kernel's sums of
// V0; null without V0): a chain whose sum is not its length raises RSM_BAD_MISMATCH in *bad
enum : int { RSM_BAD_MISMATCH = 16 };
struct RsmPtStartArgs {
    float *v; int ld;
    int rows, R, V;
    const float *V0, *V0_len, *chain_len, *beta;     // [M][V] or null, [M] or null, [M], [R]
    float *row_mult, *len; int *idx;                 // [rows] each
    int *bad;
};
void launch_rsm_pt_start(const RsmPtStartArgs &a, hipStream_t st);
// rsm_pt_rescore_kernel: part[row] / part[ld_part + row] = the float32 pair of sum_i (double)x[row][i] * (double)vb[i] in the double
// three-level order of the count kernel's AIS block (runs of 16, blocks of 16 runs, the blocks ascending; the padding adds exact
// zeros) from the counts IN MEMORY: the bits the count kernel leaves under the same vb
void launch_rsm_pt_rescore(const float *x, int ld, int rows, int V, const float *vb, float *part, int ld_part, hipStream_t st);

// ---- rsm_fill_rows_kernel: L[j][i] = a[i] for j < J, i < V - the logits rows of the AIS start, v_0 ~ Multinomial(D_j, softmax(a))
void launch_rsm_fill_rows(float *L, int ld, int J, int V, const float *a, hipStream_t st);

// ---- rsm_bias_kernel: the bias block of the update with the hidden-bias sums weighted by the document lengths; launched in
// front of the unchanged grad_kernel (which then runs without its bias tail, as it does for a handle with a sparsity penalty).
// The visible half and the q_means sums are rbm_bias_fused_block's own code and order (block_colsum).  The hidden-bias sum of
// column h is, sequentially over the rows b = 0 .. B-1 in ascending order,
//   s = __fadd_rn(s, __fmul_rn(D_b, __fsub_rn(h0[b][h], hk[b][h]))),  s = 0 at the start
// (hk read from the negated store where the chain left only -h_k: h0 + (-hk) is the same rounded number); it takes the place of
// the plain column sum in the update of hb / dhb and in the published raw tail.
struct RbmBiasFusedArgs;
void launch_rsm_bias(const RbmBiasFusedArgs &a, const float *lengths, hipStream_t st);
// the two-length flavour (the tempered update): the negative rows are chains with lengths of their own, lengths_neg
// [B]; the term of row b is __fsub_rn(__fmul_rn(D_b, h0[b][h]), __fmul_rn(Dn_b, hk[b][h])) (from the negated store:
// __fadd_rn(__fmul_rn(D_b, h0), __fmul_rn(Dn_b, -hk)), the same bits), summed as above.  A kernel of its own (rsm_bias2_kernel)
void launch_rsm_bias2(const RbmBiasFusedArgs &a, const float *lengths, const float *lengths_neg, hipStream_t st);

}  // namespace bm
