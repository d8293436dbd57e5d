// bm_pt.h — the small kernels of parallel tempering that the RBM and the DBM engine share: the slot
// partial of a state . bias product in the epilogue's order, the re-scoring of those partials under moved biases, the replica
// exchange, the gather of the beta = 1 rows.
#pragma once
#include "bm_rng.h"

namespace bm {

// The partial of x.vb over the 16-column slot `slot`, in the order of ActArgs::rowdot_out (quads of 4 columns left
// to right, then (q0 + q1) + (q2 + q3)); x_at(c) supplies column c of the row (and may store it)
template <class F>
__device__ __forceinline__ float pt_vb_slot(int slot, int V, const float *vb, F x_at) {
    float q[4];
    for (int g = 0; g < 4; ++g) {
        float acc = 0.f;
        for (int r = 0; r < 4; ++r) {
            const int c = slot * 16 + 4 * g + r;
            if (c >= V) break;
            acc += x_at(c) * vb[c];
        }
        q[g] = acc;
    }
    return (q[0] + q[1]) + (q[2] + q[3]);
}

// Replica exchange: one thread per chain c and candidate ladder pair (p, p + 1) with p % 2 == parity; the pairs of one step are
// disjoint.  a / b = the chain's rows that hold ladder index p / p + 1 (found by scanning the chain's R index entries: the
// entries another thread of this step may change hold neither p nor p + 1 before or after).  E = -(sum of the row's v.vb slots +
// sum of its `part_m` slots + sum of its h.(z + b) slots), each array ascending, in that order, in double; accepted iff
// delta = (beta_a - beta_b)(E_a - E_b) >= 0 or u < exp(delta).  part_m is the DBM's h2.b2 (nslot_m == 0: absent - the RBM, whose
// sums then are the two-array sums they always were).
// An accepted swap exchanges the rows' temperatures and ladder indices; the states stay where they are.
__global__ __launch_bounds__(256) void pt_swap_kernel(int M, int R, int parity, const float *part_v, int nslot_v, const float *part_m,
                                                      int nslot_m, const float *part_h, int nslot_h, int ld_part, float *row_mult,
                                                      int *idx, unsigned long long *cnt, PhiloxKey key, unsigned long long chain0) {
    const int npair = (R - parity) / 2;                  // pairs p = parity, parity + 2, ... <= R - 2
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)M * npair) return;
    const int c = (int)(e / npair), p = parity + 2 * (int)(e % npair);
    int ra = -1, rb = -1;
    for (int r = 0; r < R; ++r) {
        const int k = idx[(size_t)c * R + r];
        if (k == p) ra = c * R + r;
        if (k == p + 1) rb = c * R + r;
    }
    if (ra < 0 || rb < 0) return;                        // (cannot happen: the index entries of a chain are a permutation)
    double sa = 0.0, sb = 0.0;
    for (int q = 0; q < nslot_v; ++q) { sa += (double)part_v[(size_t)q * ld_part + ra]; sb += (double)part_v[(size_t)q * ld_part + rb]; }
    for (int q = 0; q < nslot_m; ++q) { sa += (double)part_m[(size_t)q * ld_part + ra]; sb += (double)part_m[(size_t)q * ld_part + rb]; }
    for (int q = 0; q < nslot_h; ++q) { sa += (double)part_h[(size_t)q * ld_part + ra]; sb += (double)part_h[(size_t)q * ld_part + rb]; }
    const float ba = row_mult[ra], bb = row_mult[rb];
    const double delta = ((double)ba - (double)bb) * ((-sa) - (-sb));
    const float u = philox_uniform_at(key, (chain0 + (unsigned long long)c) * (unsigned long long)(R - 1) + (unsigned long long)p);
    const bool accept = delta >= 0.0 || (double)u < exp(delta);
    atomicAdd(cnt + p, 1ull);
    if (accept) {
        atomicAdd(cnt + (R - 1) + p, 1ull);
        row_mult[ra] = bb; row_mult[rb] = ba;
        idx[ra] = p + 1; idx[rb] = p;
    }
}

// Re-scoring at the start of a tempered update: the state . bias slot partials of every row from its stored
// state and the CURRENT bias - the previous update changed the bias after the pass that left them.  Up to two jobs in one launch
// (the RBM: v.vb; the DBM: v.vb and, at two hidden layers, h2.b2; n == 0: absent), one thread per row and slot of either, the
// computation of the init kernels': with an unchanged bias it rewrites the bits that are there.
struct PtRescoreJob { const float *x; int ld, n; const float *bias; float *part; };
__global__ __launch_bounds__(256) void pt_rescore_kernel(int rows, int ld_part, PtRescoreJob a, PtRescoreJob b) {
    const int nsa = (a.n + 15) / 16, ns = nsa + (b.n + 15) / 16;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)rows * ns) return;
    const int row = (int)(e / ns), s = (int)(e % ns);
    const PtRescoreJob &j = s < nsa ? a : b;
    const int slot = s < nsa ? s : s - nsa;
    j.part[(size_t)slot * ld_part + row] = pt_vb_slot(slot, j.n, j.bias, [&](int c) { return j.x[(size_t)row * j.ld + c]; });
}

// the beta = 1 row of every chain c < M (ladder index R - 1: exactly one) -> row c of up to three matrices (src [.][n] pitch lds ->
// dst [M][n] pitch ldd; dst null: absent): bm_*_pt_read, the gather form of the RBM's hand-over, the DBM's hand-over of
// (v, h1, h2) to its dense particle matrices.  One workgroup per chain.
struct PtGatherJob { const float *src; int lds, n; float *dst; int ldd; };
struct PtGatherJobs { PtGatherJob j[3]; };
__global__ __launch_bounds__(256) void pt_gather_kernel(int M, int R, const int *idx, PtGatherJobs g) {
    const int c = blockIdx.x;
    if (c >= M) return;
    int src = -1;
    for (int r = 0; r < R; ++r) if (idx[(size_t)c * R + r] == R - 1) src = c * R + r;
    if (src < 0) return;
    for (int m = 0; m < 3; ++m) {
        const PtGatherJob &j = g.j[m];
        if (!j.dst) continue;
        for (int i = threadIdx.x; i < j.n; i += blockDim.x) j.dst[(size_t)c * j.ldd + i] = j.src[(size_t)src * j.lds + i];
    }
}

}  // namespace bm
