// bm_pt.h — parallel tempering, everything that does not depend on the model: the tempered ensemble as a type
// (PtEnsemble: up to three layers of states and slot partials, the rows' temperatures and ladder indices, the ladder, the swap
// counters), the checks of a ladder, the start of an ensemble, and the small kernels with their launches - the slot partial of a
// state . bias product in the epilogue's order, the start, the replica exchange, the re-scoring of the partials under moved
// biases, the gather of the beta = 1 rows, the read-out of counters and ladder indices, the sweep loop and the read tail.  An
// engine adds its model's check, its row-tempered passes and their order within a step, and its Philox sites (bm_rbm_pt.hip,
// bm_dbm.hip).
#pragma once
#include "bm_common.h"
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

#ifndef BM_KERNELS_ONLY      // (a unit that only needs the slot order above - bm_softmax_pt.hip - compiles none of the kernels below)
// Start of the ensemble: one thread per row and 16-column slot of the visible layer, then of h2 (nH2 == 0: the model has none - an
// RBM, a one-layer stack - and every thread is a visible slot).  v_0 ~ Ber(1/2) at its flat index of the global row (V0 null) or
// the chain's row of V0 [M][V] for all its R replicas; h2_0 ~ Ber(1/2) always (key_h2); the slot's partial of v_0.vb / h2_0.b2
// (pt_vb_slot); row c * R + r starts at ladder index r, temperature beta[r]
__global__ __launch_bounds__(256) void pt_init_kernel(float *v, int ldv, int rows, int R, int V, const float *V0, const float *vb,
                                                      float *h2, int ldh2, int nH2, const float *b2, const float *beta,
                                                      PhiloxKey key_v, PhiloxKey key_h2, unsigned long long row0, float *part_v,
                                                      float *part_h2, int ld_part, float *row_mult, int *idx) {
    const int nsv = (V + 15) / 16, ns = nsv + (nH2 + 15) / 16;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)rows * ns) return;
    const int row = (int)(e / ns), slot = (int)(e % ns);
    if (slot < nsv) {
        part_v[(size_t)slot * ld_part + row] = pt_vb_slot(slot, V, vb, [&](int c) {
            const float x = V0 ? V0[(size_t)(row / R) * V + c]
                               : (philox_uniform_at(key_v, (row0 + row) * (unsigned long long)V + c) < 0.5f ? 1.f : 0.f);
            v[(size_t)row * ldv + c] = x;
            return x;
        });
    } else {
        const int s2 = slot - nsv;
        part_h2[(size_t)s2 * ld_part + row] = pt_vb_slot(s2, nH2, b2, [&](int c) {
            const float x = philox_uniform_at(key_h2, (row0 + row) * (unsigned long long)nH2 + c) < 0.5f ? 1.f : 0.f;
            h2[(size_t)row * ldh2 + c] = x;
            return x;
        });
    }
    if (slot == 0) { row_mult[row] = beta[row % R]; idx[row] = row % R; }
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
// computation of the init kernel's: with an unchanged bias it rewrites the bits that are there.
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

// ---- the ensemble and its launches (host)

// one layer of the ensemble: its states, the slot partials the swap energy sums, its width (0: the model has no such layer)
struct PtLayer {
    Mat x;                                         // [rows][n]
    DevBuf part;                                   // [nslot()][rows]
    int n = 0;
    // the slot count of `part`: nslots(n), the 16-column slots of the epilogue's order, unless the engine's passes leave another
    // number (ns > 0; replicated softmax, DESIGN.md 3.31: the float32 pair of a double sum, two slots whatever n is)
    int ns = 0;
    int nslot() const { return ns > 0 ? ns : nslots(n); }
};

// The tempered ensemble of M chains x R replicas, chain-major rows (row c * R + r), allocated on demand for `rows` rows; the
// handle that holds one frees it member by member.  The partials are those of v.vb, of h1.(its whole input + b1) and of h2.b2.
struct PtEnsemble {
    PtLayer v, h1, h2;
    DevBuf mult, beta;                             // the temperature of every row [rows] (ActArgs::row_mult), the ladder [R]
    DevArray<int> idx;                             // the ladder index of every row [rows]
    DevArray<unsigned long long> cnt;              // [2][R - 1]: swap attempts, accepts per ladder pair
    int rows = 0, M = 0, R = 0;                    // row capacity (the pitch of the partials); M == 0: no ensemble
    int64_t chain0 = 0;                            // global index of chain 0 (Philox flat indices)
    long long step = 0;                            // steps done since the start: its parity picks the even or the odd ladder pairs

    PtLayer &layer(int i) { return i == 0 ? v : (i == 1 ? h1 : h2); }
    int nrows() const { return M * R; }
    int64_t row0() const { return chain0 * R; }    // global index of row 0 (Philox flat indices)

    // room for `want` rows of the widths {V, n1, n2} and a ladder of R_; grows only
    // v_slots > 0: the visible layer's slot count (PtLayer::ns), else nslots(V); a change of it allocates again
    int ensure(int want, int R_, const int widths[3], int v_slots = 0) {
        const size_t ncnt = (size_t)2 * std::max(R_ - 1, 1);
        if (cnt.n < ncnt) BM_TRY(cnt.alloc(ncnt));
        if (beta.n < (size_t)R_) BM_TRY(beta.alloc(R_));
        if (want <= rows && v.ns == v_slots) return 0;
        want = std::max(want, rows);
        rows = 0;                                  // (set again once every buffer exists: a failure leaves none counted)
        v.ns = v_slots;
        for (int i = 0; i < 3; ++i) {
            PtLayer &l = layer(i);
            l.n = widths[i];
            if (!l.n) continue;
            BM_TRY(l.x.alloc(want, l.n)); BM_TRY(l.part.alloc((size_t)l.nslot() * want));
        }
        BM_TRY(mult.alloc(want)); BM_TRY(idx.alloc(want));
        rows = want;
        return 0;
    }
};

// the arguments of a *_pt_init that do not depend on the model
static inline int pt_check_ladder(int32_t n_chains, int32_t n_temps, const float *betas_host, int64_t chain0) {
    BM_CHECK(n_temps >= 1, "n_temps must be >= 1 (got %d)", (int)n_temps);
    BM_CHECK(betas_host, "null argument");
    BM_CHECK(n_chains >= 1 && chain0 >= 0, "bad ensemble (n_chains %d >= 1, chain0 %lld >= 0)", (int)n_chains, (long long)chain0);
    BM_CHECK((long long)n_chains * n_temps <= (1ll << 24), "n_chains * n_temps = %lld rows exceed 2^24",
             (long long)n_chains * n_temps);
    for (int r = 0; r < n_temps; ++r)
        BM_CHECK(betas_host[r] > 0.f && betas_host[r] <= 1.f && (r == 0 || betas_host[r] > betas_host[r - 1]),
                 "betas must increase strictly inside (0, 1] (betas[%d] = %g)", r, (double)betas_host[r]);
    BM_CHECK(betas_host[n_temps - 1] == 1.0f, "the last beta must be 1 (got %g)", (double)betas_host[n_temps - 1]);
    return 0;
}

// Start an ensemble of M chains x R replicas of the widths {V, n1, n2} (n2 == 0: no h2) from a checked ladder; start(e, rows): the
// engine's own start launch on `stream` - it fills e.v.x (and e.h2.x), the first v.vb (h2.b2) partials, e.mult from e.beta and e.idx
template <class StartFn>
static inline int pt_begin_with(PtEnsemble &e, hipStream_t stream, const int widths[3], int M, int R, int64_t chain0,
                                const float *betas_host, StartFn &&start, int v_slots = 0) {
    const int rows = M * R;
    e.M = 0;                                       // (an ensemble exists once everything below went through)
    BM_TRY(e.ensure(rows, R, widths, v_slots));
    BM_HIP(hipStreamSynchronize(stream));
    BM_HIP(hipMemcpy(e.beta.p, betas_host, (size_t)R * sizeof(float), hipMemcpyHostToDevice));
    BM_HIP(hipMemsetAsync(e.cnt.p, 0, (size_t)2 * std::max(R - 1, 1) * sizeof(unsigned long long), stream));
    start(e, rows);
    BM_HIP(hipGetLastError());
    e.M = M; e.R = R; e.chain0 = chain0; e.step = 0;
    return 0;
}
// ... with pt_init_kernel as the start: v_0 from V0_dev (null: Ber(1/2) under key_v), h2_0 ~ Ber(1/2) under key_h2; vb / b2: the
// biases the first partials are scored with.
static inline int pt_begin(PtEnsemble &e, hipStream_t stream, const int widths[3], int M, int R, int64_t chain0,
                           const float *betas_host, const float *V0_dev, const float *vb, const float *b2, PhiloxKey key_v,
                           PhiloxKey key_h2) {
    return pt_begin_with(e, stream, widths, M, R, chain0, betas_host, [&](PtEnsemble &en, int rows) {
        const long long nthr = (long long)rows * (nslots(en.v.n) + nslots(en.h2.n));
        hipLaunchKernelGGL(pt_init_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, en.v.x.p, en.v.x.ld, rows, R, en.v.n,
                           V0_dev, vb, en.h2.x.p, en.h2.x.ld, en.h2.n, b2, (const float *)en.beta.p, key_v, key_h2,
                           (unsigned long long)chain0 * (unsigned long long)R, en.v.part.p, en.h2.part.p, en.rows, en.mult.p, en.idx.p);
    });
}

// The replica exchange of step t of a call (parity of the global step number e.step + t); nothing to launch at R == 1 or where
// the parity has no pair.  The partial arrays go to the kernel as v, then h2 (its part_m; absent: no slots), then h1: that is the
// order of the double additions in the swap energy, so changing it changes accept decisions.
static inline void pt_launch_swap(PtEnsemble &e, hipStream_t stream, int t, PhiloxKey key) {
    const int parity = (int)((e.step + t) & 1);
    const int npair = (e.R - parity) / 2;
    if (npair <= 0) return;
    const long long nthr = (long long)e.M * npair;
    hipLaunchKernelGGL(pt_swap_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, e.M, e.R, parity,
                       (const float *)e.v.part.p, e.v.nslot(), (const float *)e.h2.part.p, nslots(e.h2.n),
                       (const float *)e.h1.part.p, nslots(e.h1.n), e.rows, e.mult.p, e.idx.p, e.cnt.p, key,
                       (unsigned long long)e.chain0);
}

// the v.vb and (where there is an h2) h2.b2 partials of every row under the biases of NOW, one launch
static inline void pt_launch_rescore(PtEnsemble &e, hipStream_t stream, const float *vb, const float *b2) {
    const PtRescoreJob jv{e.v.x.p, e.v.x.ld, e.v.n, vb, e.v.part.p};
    const PtRescoreJob jh{e.h2.x.p, e.h2.x.ld, e.h2.n, b2, e.h2.part.p};
    const long long nthr = (long long)e.nrows() * (nslots(e.v.n) + nslots(e.h2.n));
    hipLaunchKernelGGL(pt_rescore_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, e.nrows(), e.rows, jv, jh);
}

// the beta = 1 rows of the chains [0, n_chains) of the layers v, h1, h2 -> dst[i] with pitch ldd[i] (null: not wanted), one
// launch; none where nothing is wanted
static inline void pt_launch_gather(PtEnsemble &e, hipStream_t stream, int n_chains, float *const dst[3], const int ldd[3]) {
    if (!dst[0] && !dst[1] && !dst[2]) return;
    PtGatherJobs g{};
    for (int i = 0; i < 3; ++i) {
        const PtLayer &l = e.layer(i);
        if (dst[i]) g.j[i] = {l.x.p, l.x.ld, l.n, dst[i], ldd[i]};
    }
    hipLaunchKernelGGL(pt_gather_kernel, dim3(n_chains), dim3(256), 0, stream, n_chains, e.R, (const int *)e.idx.p, g);
}

// the end of a *_pt_read: wait for the stream, then the swap counters [2][R - 1] and the ladder indices [M][R] (either null:
// skipped)
static inline int pt_read_host(PtEnsemble &e, hipStream_t stream, int64_t *swaps_host, int32_t *ladder_idx_host) {
    BM_HIP(hipGetLastError());
    BM_HIP(hipStreamSynchronize(stream));
    if (swaps_host && e.R > 1) {
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
        BM_HIP(hipMemcpy(swaps_host, e.cnt.p, (size_t)2 * (e.R - 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    if (ladder_idx_host) BM_HIP(hipMemcpy(ladder_idx_host, e.idx.p, (size_t)e.nrows() * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// the body of a *_pt_sweep: step(t) for the n_steps steps of the call, then the global step number moves on (the caller's checks
// come before it, its call counter and hipGetLastError after it)
template <class StepFn>
static inline void pt_sweep_with(PtEnsemble &e, int n_steps, StepFn &&step) {
    for (int t = 0; t < n_steps; ++t) step(t);
    e.step += n_steps;
}

// the body of a *_pt_read: the gather of every chain's beta = 1 row, what the engine does to the gathered rows in stream order
// (after_gather; the Gaussian unit scales them), pt_read_host
template <class AfterFn>
static inline int pt_read_with(PtEnsemble &e, hipStream_t stream, float *const dst[3], const int ldd[3], int64_t *swaps_host,
                               int32_t *ladder_idx_host, AfterFn &&after_gather) {
    pt_launch_gather(e, stream, e.M, dst, ldd);
    after_gather();
    return pt_read_host(e, stream, swaps_host, ladder_idx_host);
}
static inline int pt_read_with(PtEnsemble &e, hipStream_t stream, float *const dst[3], const int ldd[3], int64_t *swaps_host,
                               int32_t *ladder_idx_host) {
    return pt_read_with(e, stream, dst, ldd, swaps_host, ladder_idx_host, [] {});
}

#endif  // BM_KERNELS_ONLY

}  // namespace bm
