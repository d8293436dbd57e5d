// bm_xchg.hip — one-shot exchange over peer-mapped device memory (bm_xchg_* of include/bm355.h).
//
// SURVEY §5 ("Distributed communication backend") / §8e: the exchange step of data-parallel training is ONE
// all-reduce(sum) of the fused `grad` buffer (3.3 MB at 784 x 1024) per update, on the critical path.  A ring
// all-reduce over the point-to-point xGMI links of an 8-GPU node serialises 2 (N - 1) hops; at this size it is
// latency bound.  Here every rank maps every peer's buffer (hipIpcGetMemHandle / hipIpcOpenMemHandle: one process
// per GPU) and ONE kernel per rank does reduce-scatter + all-gather directly:
//
//   READY   rank r tells every peer "my buffer holds step e" (the producing kernel precedes this one in stream
//           order, so its writes have left the L2s), and waits for the same word from every peer;
//   reduce  rank r owns slice r (count / N floats): it reads slice r of EVERY rank's buffer - all 7 links at once,
//           16-byte system-scope loads that bypass the caches - adds them in RANK ORDER 0 .. N-1 (each element
//           is summed by exactly one rank, so all replicas receive the same bits; the order is the oracle's
//           shard algebra), and leaves the sum in its own buffer and in a staging slice `red` (write-through);
//   DONE    after a system-scope release, the last workgroup of rank r publishes "slice r is reduced";
//   gather  every rank pulls the other N - 1 reduced slices out of their owners' staging slices into its buffer.
//
// Two flag round trips and 2 (N - 1) / N of the buffer over each rank's links, in one launch.  Only LOADS cross
// the fabric (and 4-byte flag stores into fine-grained memory): what a rank's later kernels read was written by
// the rank itself, so no assumption is made about when a peer's store becomes visible to the home GPU's caches.
// The staging slice decouples the epochs: a rank overwrites `red` only after READY(e + 1) from every peer, i.e.
// after every peer has left epoch e.  Every wait is bounded (BM_XCHG_TIMEOUT_S, default 20 s): on expiry the
// kernel records an error in the status word and runs on without waiting - a lost rank shows up as an error from
// bm_xchg_status(), not as a hung GPU.
//
// bm_xchg_allreduce_max1: the same idea for ONE float (the mean-field residual of a data-parallel DBM,
// dbm.py:449-452 over the global minibatch): every rank stores {value, epoch} as one 8-byte word into every
// peer's slot and takes the max of the N words it receives - one fabric hop instead of a ring of 4-byte messages.
#include "../../include/bm355.h"
#include "bm_common.h"

#include <unistd.h>

namespace bmx {

constexpr int MAXR = 8;
constexpr int NTX = 256;
enum : int { F_READY = 0, F_DONE = MAXR, F_STATUS = 2 * MAXR, F_WORDS = 2 * MAXR + 8 };

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct Blob {                       // what one rank publishes to the others (bm_xchg_export), 256 bytes
    hipIpcMemHandle_t h_buf, h_red, h_flags;       // 3 x 64 bytes
    uint64_t off_buf;                              // the registered buffer need not start its allocation
    int32_t pid, device, rank, pad;
    uint64_t count;
    char fill[256 - 3 * 64 - 8 - 16 - 8];
};
static_assert(sizeof(Blob) == 256, "blob layout");

struct Args {
    float *buf, *red;
    unsigned long long count, chunk;               // floats; chunk % 4 == 0
    unsigned long long red_cap;                    // floats of every rank's staging slice (>= chunk)
    int rank, n;
    unsigned epoch;
    const float *pbuf[MAXR], *pred[MAXR];          // rank r's buffer / staging slice (own entries = local pointers)
    unsigned *pflags[MAXR];                        // rank r's flag words
    unsigned *flags;                               // this rank's flag words (fine-grained memory)
    unsigned *ctr;                                 // workgroup completion counter (local)
    int grid;
    long long timeout_ticks;                       // wall_clock64 ticks (100 MHz)
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p, unsigned long long bytes) {
    const unsigned n = bytes > 0xfffffff0ull ? 0xfffffff0u : (unsigned)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)n, 0x00020000);
}
// 16-byte load that bypasses L1 / L2 (sc0 sc1): peer memory is read at its home, never from a stale line
__device__ __forceinline__ f32x4 load_sys(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 17));
}
__device__ __forceinline__ void store_sys(__amdgpu_buffer_rsrc_t r, unsigned byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_off, 0, 17);
}

// wait until flags[base + r] >= epoch for every r < n (one lane per rank), bounded.  Returns false - for the WHOLE
// workgroup - when a wait expired: the status word then names the phase and the rank, it is STICKY (never cleared; the
// engines' sync entry points report it as an error, round-3 advisor), and the caller writes NaN instead of sums so
// that a lost rank can never pass for a result.
__device__ __forceinline__ bool wait_all(const Args &a, int base, int code) {
    const int tid = threadIdx.x;
    int bad = 0;
    if (tid < a.n) {
        const long long t0 = wall_clock64();
        while ((int)(__hip_atomic_load(a.flags + base + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - a.epoch) < 0) {
            __builtin_amdgcn_s_sleep(4);
            if (wall_clock64() - t0 > a.timeout_ticks) { bad = 1; break; }
        }
        if (bad) __hip_atomic_store(a.flags + F_STATUS, (unsigned)(code * 16 + tid + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    bad = __syncthreads_or(bad);
    if (!bad && __hip_atomic_load(a.flags + F_STATUS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) bad = 1;   // an earlier launch failed
    __atomic_thread_fence(__ATOMIC_ACQUIRE);                 // system scope: nothing cached from before the wait
    return !bad;
}

__global__ __launch_bounds__(NTX) void allreduce_kernel(Args a) {
    const int tid = threadIdx.x, me = a.rank, n = a.n;
    // READY(e): my buffer is complete (stream order) - tell every rank, myself included
    if (blockIdx.x == 0 && tid < n)
        __hip_atomic_store(a.pflags[tid] + F_READY + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const bool ok1 = wait_all(a, F_READY, 1);
    const float qnan = __builtin_nanf("");
    // ---- reduce slice `me`
    const unsigned long long base = (unsigned long long)me * a.chunk;
    const unsigned long long len = base < a.count ? (a.count - base < a.chunk ? a.count - base : a.chunk) : 0ull;
    const unsigned long long len4 = (len + 3) / 4;          // float4 (the buffer's allocation is padded to 16 bytes)
    {
        __amdgpu_buffer_rsrc_t rs[MAXR];
#pragma unroll
        for (int r = 0; r < MAXR; ++r) rs[r] = rsrc(r < n ? a.pbuf[r] + base : a.buf, r < n ? len4 * 16 : 0);
        __amdgpu_buffer_rsrc_t rred = rsrc(a.red, len4 * 16);
        for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < len4; e += (unsigned long long)a.grid * NTX) {
            const unsigned off = (unsigned)(e * 16);
            f32x4 v[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) if (r < n) v[r] = load_sys(rs[r], off);
            f32x4 s = v[0];
#pragma unroll
            for (int r = 1; r < MAXR; ++r) if (r < n) s = s + v[r];          // rank order
            if (!ok1) s = (f32x4){qnan, qnan, qnan, qnan};                  // a failed wait never passes for a sum
            *reinterpret_cast<f32x4 *>(a.buf + base + e * 4) = s;
            store_sys(rred, off, s);
        }
    }
    // DONE(e): every workgroup's stores are out; the last one to arrive publishes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == (unsigned)a.grid * a.epoch) {
            __threadfence_system();
            for (int r = 0; r < n; ++r)
                __hip_atomic_store(a.pflags[r] + F_DONE + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (n == 1) return;
    const bool ok2 = wait_all(a, F_DONE, 2);
    // ---- gather the other ranks' reduced slices (rotated start: the pulls spread over the links)
    for (int d = 1; d < n; ++d) {
        if (!ok2) {                                         // the owner never answered: its slice is NaN here, not stale
            const unsigned long long bq = (unsigned long long)((me + d) % n) * a.chunk;
            const unsigned long long lq = bq < a.count ? (a.count - bq < a.chunk ? a.count - bq : a.chunk) : 0ull;
            for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < (lq + 3) / 4; e += (unsigned long long)a.grid * NTX)
                *reinterpret_cast<f32x4 *>(a.buf + bq + e * 4) = (f32x4){qnan, qnan, qnan, qnan};
            continue;
        }
        const int q = (me + d) % n;
        const unsigned long long bq = (unsigned long long)q * a.chunk;
        const unsigned long long lq = bq < a.count ? (a.count - bq < a.chunk ? a.count - bq : a.chunk) : 0ull;
        const unsigned long long lq4 = (lq + 3) / 4;
        __amdgpu_buffer_rsrc_t rq = rsrc(a.pred[q], lq4 * 16);
        unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid;
        const unsigned long long st = (unsigned long long)a.grid * NTX;
        for (; e + st < lq4; e += 2 * st) {                  // two loads in flight per lane
            const f32x4 v0 = load_sys(rq, (unsigned)(e * 16)), v1 = load_sys(rq, (unsigned)((e + st) * 16));
            *reinterpret_cast<f32x4 *>(a.buf + bq + e * 4) = v0;
            *reinterpret_cast<f32x4 *>(a.buf + bq + (e + st) * 4) = v1;
        }
        if (e < lq4) *reinterpret_cast<f32x4 *>(a.buf + bq + e * 4) = load_sys(rq, (unsigned)(e * 16));
    }
}

// ---- fused exchange of data-parallel CD-k (round-3 verdict): reduce-scatter -> parameter update on the owned slice
// -> all-gather of the UPDATED WEIGHTS, one launch.  The buffer is the RBM's fused gradient [V * ldw | V | H | H]:
//   * the W part is cut into N slices; rank r sums slice r of all ranks in rank order (as allreduce_kernel), applies
//     g = raw / N - l2 W - pen, dW = lr (mom dW + g), W += dW to ITS slice of W / dW (apply_w_update's arithmetic:
//     the replicas' bits are those of allreduce + bm_rbm_apply_step) and leaves the new weights in its staging slice;
//     the momentum buffer of a slice is only ever read by its owner (bm_rbm_exchange_gather_dw refreshes the rest
//     when the host asks for dW);
//   * the 2.8 K floats of the tail are reduced by EVERY rank itself (rank order: same bits everywhere) and the bias /
//     q_means update is applied to every replica - by the LAST workgroup, which then publishes the sparsity penalty
//     the W update needs (an agent-scope flag; only waited for when sparsity_cost != 0);
//   * gather: every rank pulls the other N - 1 updated slices of W.
// One launch and 7/8 of the apply work less on every rank's critical path than allreduce + apply_step.
struct RbmApply {
    float *W, *dW;                                  // local [V][ldw]
    unsigned long long countW, chunkW;              // floats of the W part; slice length (% 4 == 0)
    int I, ldw, V, H;
    float N, l2, lr, mom, damping, cost, target;
    float *vb, *dvb, *hb, *dhb, *q, *pen;           // local vectors
    float *tail_red;                                // local [V + 2 H (+3)]: the reduced tail
    unsigned *tail_flag;                            // local word: epoch for which tail_red / pen are valid
    int dw_only;                                    // 1: no update - gather the owners' dW slices (bm_rbm_exchange_gather_dw)
};

__global__ __launch_bounds__(NTX) void exchange_apply_kernel(Args a, RbmApply p) {
    const int tid = threadIdx.x, me = a.rank, n = a.n;
    const float qnan = __builtin_nanf("");
    if (blockIdx.x == 0 && tid < n)
        __hip_atomic_store(a.pflags[tid] + F_READY + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const bool ok1 = wait_all(a, F_READY, 1);
    const unsigned long long base = (unsigned long long)me * p.chunkW;
    const unsigned long long len = base < p.countW ? (p.countW - base < p.chunkW ? p.countW - base : p.chunkW) : 0ull;
    const unsigned long long len4 = len / 4;                 // countW % 4 == 0, chunkW % 4 == 0
    __amdgpu_buffer_rsrc_t rred = rsrc(a.red, len4 * 16);
    if (!p.dw_only) {
        // ---- tail (last workgroup): reduce, update the biases / q_means of this replica, publish the penalty
        if (blockIdx.x == gridDim.x - 1) {
            const int T = p.V + 2 * p.H, T4 = (T + 3) / 4;
            __amdgpu_buffer_rsrc_t rt[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) rt[r] = rsrc(r < n ? a.pbuf[r] + p.countW : a.buf, r < n ? (unsigned long long)T4 * 16 : 0);
            for (int c4 = tid; c4 < T4; c4 += NTX) {
                f32x4 v[MAXR];
#pragma unroll
                for (int r = 0; r < MAXR; ++r) if (r < n) v[r] = load_sys(rt[r], (unsigned)c4 * 16u);
                f32x4 s = v[0];
#pragma unroll
                for (int r = 1; r < MAXR; ++r) if (r < n) s = s + v[r];      // rank order
                if (!ok1) s = (f32x4){qnan, qnan, qnan, qnan};
                *reinterpret_cast<f32x4 *>(p.tail_red + 4 * c4) = s;
            }
            __syncthreads();
            const float *sv = p.tail_red, *sh = p.tail_red + p.V, *sq = p.tail_red + p.V + p.H;
            for (int c = tid; c < p.V + p.H; c += NTX) {          // rbm_bias_update (bm_kernels.h), same operations
                if (c < p.V) {
                    const float g = sv[c] / p.N;
                    const float d = p.lr * (p.mom * p.dvb[c] + g);
                    p.dvb[c] = d;
                    p.vb[c] = p.vb[c] + d;
                } else {
                    const int h = c - p.V;
                    const float qn = p.damping * p.q[h] + (1.0f - p.damping) * sq[h];
                    p.q[h] = qn;
                    const float pen = p.cost * (qn - p.target);
                    p.pen[h] = pen;
                    float g = sh[h] / p.N;
                    g = g - pen;
                    const float d = p.lr * (p.mom * p.dhb[h] + g);
                    p.dhb[h] = d;
                    p.hb[h] = p.hb[h] + d;
                }
            }
            __threadfence();
            __syncthreads();
            if (tid == 0) __hip_atomic_store(p.tail_flag, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- W slice `me`: sum over the ranks, update, stage the new weights
        bool okp = true;
        if (p.cost != 0.f) {                                 // the penalty of this step (wave-uniform branch)
            int bad = 0;
            if (tid == 0) {
                const long long t0 = wall_clock64();
                while ((int)(__hip_atomic_load(p.tail_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - a.epoch) < 0) {
                    __builtin_amdgcn_s_sleep(2);
                    if (wall_clock64() - t0 > a.timeout_ticks) { bad = 1; break; }
                }
                if (bad) __hip_atomic_store(a.flags + F_STATUS, (unsigned)(4 * 16 + me + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            okp = !__syncthreads_or(bad);
        }
        const bool pow2 = bm::grad_pow2(p.N);
        const float invN = 1.0f / p.N;
        __amdgpu_buffer_rsrc_t rs[MAXR];
#pragma unroll
        for (int r = 0; r < MAXR; ++r) rs[r] = rsrc(r < n ? a.pbuf[r] + base : a.buf, r < n ? len4 * 16 : 0);
        for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < len4; e += (unsigned long long)a.grid * NTX) {
            const unsigned off = (unsigned)(e * 16);
            f32x4 v[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) if (r < n) v[r] = load_sys(rs[r], off);
            f32x4 s = v[0];
#pragma unroll
            for (int r = 1; r < MAXR; ++r) if (r < n) s = s + v[r];          // rank order
            const unsigned long long flat = base + e * 4;
            const int i = (int)(flat % (unsigned long long)p.ldw);
            f32x4 wv = *reinterpret_cast<const f32x4 *>(p.W + flat), dv = *reinterpret_cast<const f32x4 *>(p.dW + flat);
            if (i < p.I) {                                       // I % 4 == 0: the whole group is inside the row
                f32x4 pe = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (p.cost != 0.f) pe = *reinterpret_cast<const f32x4 *>(p.pen + i);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float g = bm::grad_norm1(s[c], p.N, invN, pow2);
                    float w = wv[c], d = dv[c];
                    bm::apply_w_update(g, pe[c], p.l2, p.lr, p.mom, w, d);
                    wv[c] = w; dv[c] = d;
                }
                if (!ok1 || !okp) wv = dv = (f32x4){qnan, qnan, qnan, qnan};
                *reinterpret_cast<f32x4 *>(p.W + flat) = wv;
                *reinterpret_cast<f32x4 *>(p.dW + flat) = dv;
            }
            store_sys(rred, off, wv);
        }
    } else {
        // ---- dW gather: stage this rank's slice of dW
        for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < len4; e += (unsigned long long)a.grid * NTX)
            store_sys(rred, (unsigned)(e * 16), *reinterpret_cast<const f32x4 *>(p.dW + base + e * 4));
    }
    // DONE(e)
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == (unsigned)a.grid * a.epoch) {
            __threadfence_system();
            for (int r = 0; r < n; ++r)
                __hip_atomic_store(a.pflags[r] + F_DONE + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (n == 1) return;
    const bool ok2 = wait_all(a, F_DONE, 2);
    // ---- gather the other ranks' slices of the new W (or of dW) into this replica
    float *dst = p.dw_only ? p.dW : p.W;
    for (int d = 1; d < n; ++d) {
        const int q = (me + d) % n;
        const unsigned long long bq = (unsigned long long)q * p.chunkW;
        const unsigned long long lq = bq < p.countW ? (p.countW - bq < p.chunkW ? p.countW - bq : p.chunkW) : 0ull;
        const unsigned long long lq4 = lq / 4;
        __amdgpu_buffer_rsrc_t rq = rsrc(a.pred[q], lq4 * 16);
        const unsigned long long st = (unsigned long long)a.grid * NTX;
        unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid;
        if (!ok2) {
            for (; e < lq4; e += st) *reinterpret_cast<f32x4 *>(dst + bq + e * 4) = (f32x4){qnan, qnan, qnan, qnan};
            continue;
        }
        for (; e + st < lq4; e += 2 * st) {                  // two loads in flight per lane
            const f32x4 v0 = load_sys(rq, (unsigned)(e * 16)), v1 = load_sys(rq, (unsigned)((e + st) * 16));
            *reinterpret_cast<f32x4 *>(dst + bq + e * 4) = v0;
            *reinterpret_cast<f32x4 *>(dst + bq + (e + st) * 4) = v1;
        }
        if (e < lq4) *reinterpret_cast<f32x4 *>(dst + bq + e * 4) = load_sys(rq, (unsigned)(e * 16));
    }
}

// ---- fused exchange of the data-parallel DBM update (round-4 verdict 4a): COLUMN-sliced ownership.  The DBM rescales every
// column of W_i to the max-norm after the update (dbm.py:511-513, 603-606), and a column norm is a canonical chain over the
// whole column (maxnorm_kernel): rank r therefore owns columns [r sw_i, (r + 1) sw_i) of every W_i (sw_i a multiple of 32),
// i.e. a strided slice of W_i / dW_i / the raw outer products and a contiguous row block of the maintained transpose.
//   launch A  dbm_exchange_apply_kernel: READY, sums of the owned columns of pos_i / neg_i over the ranks in rank order,
//             g = pos / N - neg / M - l2 W - pen, dW = lr (mom dW + g), W += dW on the owned columns; the column sums
//             (tail) are reduced by every rank itself and the bias / running-mean / penalty update (dbm_bias_update) applied
//             to every replica by the last workgroup, which publishes the penalties the W update needs;
//   then      maxnorm_kernel + maxnorm_scale_kernel on the owned columns (the kernels of the one-GPU update, same bits;
//             they also write the owned rows of W_i^T and the owned column norms);
//   launch B  dbm_exchange_gather_kernel: stage the owned columns (and norms), DONE, pull the other ranks' columns in
//             32 x 32 tiles that are written to W_i and, transposed through LDS, to W_i^T.
// Replaces bm_dbm_allreduce_grads_direct + bm_dbm_apply_step with the same bits; the gather moves W (half of the two raw
// buffers) and 1 / N of the update and max-norm work is on a rank's critical path.  dW_i stays with the owners
// (bm_dbm_exchange_gather_dw = launch B in dW mode with its own READY round).
struct DbmLayerX {
    float *W, *dW, *Wt, *wnorm;
    const float *pen;
    unsigned long long off_pos, off_neg;           // floats into the exchanged buffer, pitch ldw
    unsigned long long red_off;                    // floats into the staging slice: [J][sw] values, then [sw] column norms
    int I, J, ldw, ldwt, sw;
};
struct DbmApply {
    int L, mode, do_ready;                         // mode 0: weights, 1: dW (launch B)
    DbmLayerX lay[BM_DBM_MAX_LAYERS];
    bm::DbmBiasArgs bias[BM_DBM_MAX_LAYERS + 1];       // [0] visible, [1 + i] hidden layer i; s_pos / s_neg point into tail_red
    unsigned long long off_sums; int n_sums;
    float N, M, l2, lr, mom;
    float *tail_red; unsigned *tail_flag;
};

__global__ __launch_bounds__(NTX) void dbm_exchange_apply_kernel(Args a, DbmApply p) {
    const int tid = threadIdx.x, me = a.rank, n = a.n;
    const float qnan = __builtin_nanf("");
    if (blockIdx.x == 0 && tid < n)
        __hip_atomic_store(a.pflags[tid] + F_READY + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const bool ok1 = wait_all(a, F_READY, 1);
    __amdgpu_buffer_rsrc_t rs[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) rs[r] = rsrc(r < n ? a.pbuf[r] : a.buf, r < n ? ((a.count + 3) & ~3ull) * 4 : 0);
    // ---- tail (last workgroup): column sums over the ranks, biases / running means / penalties of this replica
    if (blockIdx.x == gridDim.x - 1) {
        const int T4 = (p.n_sums + 3) / 4;
        for (int c4 = tid; c4 < T4; c4 += NTX) {
            const unsigned off = (unsigned)((p.off_sums + 4ull * c4) * 4);
            f32x4 v[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) if (r < n) v[r] = load_sys(rs[r], off);
            f32x4 s = v[0];
#pragma unroll
            for (int r = 1; r < MAXR; ++r) if (r < n) s = s + v[r];          // rank order
            if (!ok1) s = (f32x4){qnan, qnan, qnan, qnan};
            *reinterpret_cast<f32x4 *>(p.tail_red + 4 * c4) = s;
        }
        __syncthreads();
        for (int v = 0; v <= p.L; ++v)
            for (int c = tid; c < p.bias[v].n; c += NTX) bm::dbm_bias_update(p.bias[v], c);
        __threadfence();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(p.tail_flag, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the penalties of this step (always read, as bm_dbm_apply_step does: pen = cost * (..) may be -0)
    bool okp = true;
    {
        int bad = 0;
        if (tid == 0) {
            const long long t0 = wall_clock64();
            while ((int)(__hip_atomic_load(p.tail_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - a.epoch) < 0) {
                __builtin_amdgcn_s_sleep(2);
                if (wall_clock64() - t0 > a.timeout_ticks) { bad = 1; break; }
            }
            if (bad) __hip_atomic_store(a.flags + F_STATUS, (unsigned)(4 * 16 + me + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        okp = !__syncthreads_or(bad);
    }
    const bool pow2 = bm::grad_pow2(p.N) && bm::grad_pow2(p.M);            // apply_w_tiled_kernel's rule
    const float invN = 1.0f / p.N, invM = 1.0f / p.M;
    for (int i = 0; i < p.L; ++i) {
        const DbmLayerX &y = p.lay[i];
        const int c0 = me * y.sw, c1 = (c0 + y.sw < y.I) ? c0 + y.sw : y.I;
        if (c1 <= c0) continue;
        const unsigned w4 = (unsigned)(c1 - c0) / 4u;                       // I % 4 == 0
        const unsigned long long n4 = (unsigned long long)y.J * w4;
        for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < n4; e += (unsigned long long)a.grid * NTX) {
            const int j = (int)(e / w4), c = c0 + 4 * (int)(e % w4);
            const unsigned long long o = (unsigned long long)j * y.ldw + c;
            const unsigned bp = (unsigned)((y.off_pos + o) * 4), bn = (unsigned)((y.off_neg + o) * 4);
            f32x4 vp[MAXR], vn[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) if (r < n) { vp[r] = load_sys(rs[r], bp); vn[r] = load_sys(rs[r], bn); }
            f32x4 sp = vp[0], sn = vn[0];
#pragma unroll
            for (int r = 1; r < MAXR; ++r) if (r < n) { sp = sp + vp[r]; sn = sn + vn[r]; }      // rank order
            f32x4 wv = *reinterpret_cast<const f32x4 *>(y.W + o), dv = *reinterpret_cast<const f32x4 *>(y.dW + o);
            const f32x4 pe = *reinterpret_cast<const f32x4 *>(y.pen + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float g = bm::grad_norm2(sp[q], sn[q], p.N, p.M, invN, invM, pow2);
                float w = wv[q], d = dv[q];
                bm::apply_w_update(g, pe[q], p.l2, p.lr, p.mom, w, d);
                wv[q] = w; dv[q] = d;
            }
            if (!ok1 || !okp) wv = dv = (f32x4){qnan, qnan, qnan, qnan};
            *reinterpret_cast<f32x4 *>(y.W + o) = wv;
            *reinterpret_cast<f32x4 *>(y.dW + o) = dv;
        }
    }
}

__global__ __launch_bounds__(NTX) void dbm_exchange_gather_kernel(Args a, DbmApply p) {
    __shared__ float t[32][33];
    const int tid = threadIdx.x, me = a.rank, n = a.n;
    const float qnan = __builtin_nanf("");
    if (p.do_ready) {                                      // the dW gather is an exchange of its own: nobody stages into a
        if (blockIdx.x == 0 && tid < n)                    // slice a peer may still be pulling from
            __hip_atomic_store(a.pflags[tid] + F_READY + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        (void)wait_all(a, F_READY, 1);
    }
    // ---- stage the owned columns (after the max-norm pass) and their norms
    __amdgpu_buffer_rsrc_t rred = rsrc(a.red, a.red_cap * 4);
    for (int i = 0; i < p.L; ++i) {
        const DbmLayerX &y = p.lay[i];
        const int c0 = me * y.sw, c1 = (c0 + y.sw < y.I) ? c0 + y.sw : y.I;
        if (c1 <= c0) continue;
        const float *src = p.mode ? y.dW : y.W;
        const unsigned w4 = (unsigned)(c1 - c0) / 4u;
        const unsigned long long n4 = (unsigned long long)y.J * w4;
        for (unsigned long long e = (unsigned long long)blockIdx.x * NTX + tid; e < n4; e += (unsigned long long)a.grid * NTX) {
            const int j = (int)(e / w4), cc = 4 * (int)(e % w4);
            store_sys(rred, (unsigned)((y.red_off + (unsigned long long)j * y.sw + cc) * 4),
                      *reinterpret_cast<const f32x4 *>(src + (unsigned long long)j * y.ldw + c0 + cc));
        }
        if (!p.mode && blockIdx.x == 0)
            for (unsigned e = tid; e < w4; e += NTX)
                store_sys(rred, (unsigned)((y.red_off + (unsigned long long)y.J * y.sw + 4 * e) * 4),
                          *reinterpret_cast<const f32x4 *>(y.wnorm + c0 + 4 * e));
    }
    // DONE(e)
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == (unsigned)a.grid * a.epoch) {
            __threadfence_system();
            for (int r = 0; r < n; ++r)
                __hip_atomic_store(a.pflags[r] + F_DONE + me, a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (n == 1) return;
    const bool ok2 = wait_all(a, F_DONE, 2);
    // ---- pull the other ranks' columns: 32 x 32 tiles -> W_i (or dW_i) and, transposed, W_i^T
    for (int i = 0; i < p.L; ++i) {
        const DbmLayerX &y = p.lay[i];
        float *dst = p.mode ? y.dW : y.W;
        for (int d = 1; d < n; ++d) {
            const int q = (me + d) % n;
            const int q0 = q * y.sw, q1 = (q0 + y.sw < y.I) ? q0 + y.sw : y.I;
            if (q1 <= q0) continue;
            __amdgpu_buffer_rsrc_t rq = rsrc(a.pred[q], a.red_cap * 4);
            const int tiles_c = (q1 - q0 + 31) / 32, tiles_j = (y.J + 31) / 32;
            for (int tile = blockIdx.x; tile < tiles_c * tiles_j; tile += a.grid) {
                const int cb = (tile % tiles_c) * 32, j0 = (tile / tiles_c) * 32;
                const int r = tid >> 3, c4 = tid & 7;
                const int j = j0 + r, c = q0 + cb + 4 * c4;
                f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (j < y.J && c < q1) {                                   // I % 4 == 0: the whole group is inside
                    v = ok2 ? load_sys(rq, (unsigned)((y.red_off + (unsigned long long)j * y.sw + cb + 4 * c4) * 4))
                            : (f32x4){qnan, qnan, qnan, qnan};
                    *reinterpret_cast<f32x4 *>(dst + (unsigned long long)j * y.ldw + c) = v;
                }
                if (!p.mode) {
                    t[r][4 * c4] = v[0]; t[r][4 * c4 + 1] = v[1]; t[r][4 * c4 + 2] = v[2]; t[r][4 * c4 + 3] = v[3];
                    __syncthreads();
                    const int cc = q0 + cb + r, jq = j0 + 4 * c4;          // row cc of the transpose, 4 consecutive j
                    if (cc < q1 && jq < y.J) {
                        float *wt = y.Wt + (unsigned long long)cc * y.ldwt + jq;
                        if (jq + 3 < y.J) *reinterpret_cast<f32x4 *>(wt) = (f32x4){t[4 * c4][r], t[4 * c4 + 1][r], t[4 * c4 + 2][r], t[4 * c4 + 3][r]};
                        else for (int e = 0; e < 4; ++e) if (jq + e < y.J) wt[e] = t[4 * c4 + e][r];
                    }
                    __syncthreads();
                }
            }
            if (!p.mode && blockIdx.x == 0)
                for (int e = tid; e < (q1 - q0) / 4; e += NTX)
                    *reinterpret_cast<f32x4 *>(y.wnorm + q0 + 4 * e) =
                        ok2 ? load_sys(rq, (unsigned)((y.red_off + (unsigned long long)y.J * y.sw + 4 * e) * 4)) : (f32x4){qnan, qnan, qnan, qnan};
        }
    }
}

// ---- all-reduce(max) of one float.  slots [2][MAXR] of {value bits, epoch} (one 8-byte store each), by epoch parity
struct MaxArgs {
    float *val;                                    // in / out (device, local)
    unsigned long long *slots;                     // this rank's slots (fine-grained)
    unsigned long long *pslots[MAXR];              // rank r's slots
    unsigned *flags;                               // status word lives here
    int rank, n;
    unsigned epoch;
    long long timeout_ticks;
};
__global__ __launch_bounds__(64) void max1_kernel(MaxArgs a) {
    const int tid = threadIdx.x;
    const unsigned par = a.epoch & 1u;
    const float mine = *a.val;
    float got = 0.f;
    if (tid < a.n) {
        const unsigned long long word = ((unsigned long long)a.epoch << 32) | (unsigned long long)__float_as_uint(mine);
        __hip_atomic_store(a.pslots[tid] + par * MAXR + a.rank, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const long long t0 = wall_clock64();
        unsigned long long w;
        bool ok = true;
        while ((unsigned)((w = __hip_atomic_load(a.slots + par * MAXR + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) >> 32) != a.epoch) {
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > a.timeout_ticks) { ok = false; break; }
        }
        if (ok) got = __uint_as_float((unsigned)w);
        else __hip_atomic_store(a.flags + F_STATUS, (unsigned)(3 * 16 + tid + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) got = fmaxf(got, __shfl_xor(got, off));
    if (tid == 0) *a.val = got;                    // residuals are >= 0
}

// mean-field loop control of a data-parallel DBM in ONE launch: mf_resid_kernel (local residual from the per-workgroup
// slots and the atomic cell, both reset), max1_kernel (max over the ranks) and mf_latch_kernel (counter / `done`), same
// operations in the same order.  The exchange runs whether or not `done` is latched: every rank issues the same sequence.
__global__ __launch_bounds__(256) void mf_ctl_max1_kernel(MaxArgs a, bm::MfCtl *c, float *blk, int nblk, float tol, int init) {
    __shared__ float s_m[4];
    __shared__ float s_resid;
    const int tid = threadIdx.x;
    float m = 0.f;
    for (int e = tid; e < nblk; e += 256) { m = fmaxf(m, blk[e]); blk[e] = 0.f; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        s_resid = fmaxf(fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])), __uint_as_float(c->maxdiff));
        c->maxdiff = 0u;
    }
    __syncthreads();
    if (tid >= 64) return;
    const unsigned par = a.epoch & 1u;
    const float mine = s_resid;
    float got = 0.f;
    if (tid < a.n) {
        const unsigned long long word = ((unsigned long long)a.epoch << 32) | (unsigned long long)__float_as_uint(mine);
        __hip_atomic_store(a.pslots[tid] + par * MAXR + a.rank, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const long long t0 = wall_clock64();
        unsigned long long w;
        bool ok = true;
        while ((unsigned)((w = __hip_atomic_load(a.slots + par * MAXR + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) >> 32) != a.epoch) {
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > a.timeout_ticks) { ok = false; break; }
        }
        if (ok) got = __uint_as_float((unsigned)w);
        else __hip_atomic_store(a.flags + F_STATUS, (unsigned)(3 * 16 + tid + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) got = fmaxf(got, __shfl_xor(got, off));
    if (tid != 0) return;
    c->resid = got;
    if (init) {
        c->steps = 0;
        c->done = !(got > tol);
    } else if (!c->done) {
        c->steps += 1;
        c->done = !(got > tol);
    }
}

}  // namespace bmx

struct bm_xchg {
    int rank = 0, nranks = 1, device = 0;
    float *buf = nullptr, *red = nullptr;
    size_t count = 0, chunk = 0, red_cap = 0;      // red_cap: floats of the staging slice (>= chunk; the same on every rank)
    unsigned *flags = nullptr, *ctr = nullptr;     // flags: F_WORDS words + the max slots behind them
    unsigned long long *slots = nullptr;
    const float *pbuf[bmx::MAXR], *pred[bmx::MAXR];
    unsigned *pflags[bmx::MAXR];
    void *opened[3 * bmx::MAXR];
    int n_opened = 0;
    bool attached = false;
    unsigned epoch = 0, epoch_max = 0;
    int grid = 1;
    long long timeout_ticks = 0;
    // fused exchange + update (bm_rbm_exchange_apply_direct): the reduced tail and the flag that publishes the penalty
    float *tail_red = nullptr;
    unsigned *tail_flag = nullptr;
    size_t tail_n = 0;
    bool dw_stale = false;          // the owners' slices of dW moved since the replicas were last refreshed
    bm_xchg **user = nullptr;       // the engine field that points at this exchange (cleared when it is destroyed)
};

static int xchg_alloc_flags(bm_xchg *x) {
    const size_t bytes = bmx::F_WORDS * sizeof(unsigned) + 2 * bmx::MAXR * sizeof(unsigned long long);
    void *p = nullptr;
    // fine-grained, uncached device memory: written by the peers, polled here
    hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained); }
    BM_HIP(e);
    BM_HIP(hipMemset(p, 0, bytes));
    x->flags = (unsigned *)p;
    x->slots = (unsigned long long *)((char *)p + bmx::F_WORDS * sizeof(unsigned));
    return 0;
}

// 0 when no wait of this exchange has ever expired; otherwise an error (the status word is sticky).  Reads 4 bytes
// of fine-grained memory; the caller has synchronised the stream.
static int xchg_check_status(bm_xchg *x) {
    if (!x) return 0;
    unsigned s = 0;
    BM_HIP(hipMemcpy(&s, x->flags + bmx::F_STATUS, sizeof(s), hipMemcpyDeviceToHost));
    BM_CHECK(s == 0, "bm_xchg: a wait for rank %u expired in phase %u (1 READY, 2 DONE, 3 max, 4 penalty): the results of "
                     "this exchange are NaN-poisoned, the job is lost", (s & 15u) - 1u, s >> 4);
    return 0;
}

static void xchg_bind_user(bm_xchg *x, bm_xchg **slot) { if (x) x->user = slot; }
static void xchg_dw_replaced(bm_xchg *x) { if (x) x->dw_stale = false; }

static int xchg_mf_ctl_step(bm_xchg *x, bm::MfCtl *ctl, float *blk, int nblk, float tol, int init, hipStream_t stream) {
    BM_CHECK(x && x->attached && ctl, "exchange not attached / null argument");
    bmx::MaxArgs a;
    memset(&a, 0, sizeof(a));
    a.val = &ctl->resid; a.slots = x->slots; a.flags = x->flags; a.rank = x->rank; a.n = x->nranks;
    a.epoch = ++x->epoch_max; a.timeout_ticks = x->timeout_ticks;
    for (int r = 0; r < bmx::MAXR; ++r)
        a.pslots[r] = (unsigned long long *)((char *)x->pflags[r] + bmx::F_WORDS * sizeof(unsigned));
    hipLaunchKernelGGL(bmx::mf_ctl_max1_kernel, dim3(1), dim3(256), 0, stream, a, ctl, blk, nblk, tol, init);
    BM_HIP(hipGetLastError());
    return 0;
}

extern "C" {

static int xchg_create(int32_t rank, int32_t nranks, float *buf_dev, size_t count, size_t min_red, bm_xchg **out) {
    BM_CHECK(out && buf_dev, "null argument");
    BM_CHECK(nranks >= 1 && nranks <= bmx::MAXR && rank >= 0 && rank < nranks, "bad rank %d of %d (at most %d ranks)", rank, nranks, bmx::MAXR);
    BM_CHECK(((uintptr_t)buf_dev & 15u) == 0, "the exchanged buffer must be 16-byte aligned");
    bm_xchg *x = new bm_xchg();
    x->rank = rank; x->nranks = nranks; x->buf = buf_dev; x->count = count;
    x->chunk = (((count + nranks - 1) / nranks) + 3) & ~(size_t)3;
    x->red_cap = ((x->chunk > min_red ? x->chunk : min_red) + 3) & ~(size_t)3;
    // (an early return below must not leak what was allocated so far: round-3 advisor)
    auto fail = [&]() { if (x->red) (void)hipFree(x->red); if (x->ctr) (void)hipFree(x->ctr); if (x->flags) (void)hipFree(x->flags); delete x; return 1; };
    if (hipGetDevice(&x->device) != hipSuccess ||
        hipMalloc((void **)&x->red, (x->red_cap ? x->red_cap : 4) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&x->ctr, 64) != hipSuccess || hipMemset(x->ctr, 0, 64) != hipSuccess) {
        bm::set_error("bm_xchg_create: device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return fail();
    }
    if (xchg_alloc_flags(x)) return fail();
    // Launch width: every workgroup of an exchange launch must be CO-RESIDENT (the last one publishes DONE while the others
    // already wait for the peers), so the bound is what the device can hold at once - one workgroup per CU, checked against
    // the occupancy of the heaviest exchange kernel - not a constant (round-5 advisor).
    int ncu = 0, per_cu = 0;
    {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, x->device) == hipSuccess) ncu = pr.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmx::dbm_exchange_gather_kernel, bmx::NTX, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    }
    if (ncu < 1 || per_cu < 1) { bm::set_error("bm_xchg_create: cannot establish a co-resident launch width (CUs %d, workgroups per CU %d)", ncu, per_cu); return fail(); }
    const size_t f4 = (x->chunk / 4 + bmx::NTX - 1) / bmx::NTX;
    x->grid = (int)(f4 < 1 ? 1 : (f4 > (size_t)ncu ? (size_t)ncu : f4));
    const char *t = getenv("BM_XCHG_TIMEOUT_S");
    x->timeout_ticks = (long long)((t ? atof(t) : 20.0) * 1e8);
    for (int r = 0; r < bmx::MAXR; ++r) { x->pbuf[r] = x->buf; x->pred[r] = x->red; x->pflags[r] = x->flags; }
    x->attached = nranks == 1;
    *out = x;
    return 0;
}

int bm_xchg_create(int32_t rank, int32_t nranks, float *buf_dev, size_t count, bm_xchg **out) {
    return xchg_create(rank, nranks, buf_dev, count, 0, out);
}

int bm_xchg_blob_bytes(void) { return (int)sizeof(bmx::Blob); }

int bm_xchg_export(bm_xchg *x, void *out_blob256) {
    BM_CHECK(x && out_blob256, "null argument");
    bmx::Blob b;
    memset(&b, 0, sizeof(b));
    void *base = nullptr; size_t sz = 0;
    BM_HIP(hipMemGetAddressRange((hipDeviceptr_t *)&base, &sz, (hipDeviceptr_t)x->buf));
    // the whole reduced range must be readable by the peers, including the 16-byte round-up of the last slice
    BM_CHECK((char *)x->buf + ((x->count + 3) & ~(size_t)3) * sizeof(float) <= (char *)base + sz,
             "the exchanged buffer's allocation must cover its length rounded up to 16 bytes");
    b.off_buf = (uint64_t)((char *)x->buf - (char *)base);
    BM_HIP(hipIpcGetMemHandle(&b.h_buf, base));
    BM_HIP(hipIpcGetMemHandle(&b.h_red, x->red));
    BM_HIP(hipIpcGetMemHandle(&b.h_flags, x->flags));
    b.pid = (int32_t)getpid(); b.device = x->device; b.rank = x->rank; b.count = x->count;
    memcpy(out_blob256, &b, sizeof(b));
    return 0;
}

int bm_xchg_attach(bm_xchg *x, const void *all_blobs) {
    BM_CHECK(x && all_blobs, "null argument");
    BM_CHECK(!x->attached || x->nranks == 1, "already attached");
    const bmx::Blob *bl = (const bmx::Blob *)all_blobs;
    for (int r = 0; r < x->nranks; ++r) {
        BM_CHECK(bl[r].rank == r, "blob %d carries rank %d: the blobs must be ordered by rank", r, bl[r].rank);
        BM_CHECK(bl[r].count == x->count, "rank %d exchanges %llu floats, this rank %zu", r, (unsigned long long)bl[r].count, x->count);
        if (r == x->rank) continue;
        BM_CHECK(bl[r].pid != (int32_t)getpid(), "rank %d lives in this process: one process per rank", r);
        void *pb = nullptr, *pr = nullptr, *pf = nullptr;
        BM_HIP(hipIpcOpenMemHandle(&pb, bl[r].h_buf, hipIpcMemLazyEnablePeerAccess));
        x->opened[x->n_opened++] = pb;
        BM_HIP(hipIpcOpenMemHandle(&pr, bl[r].h_red, hipIpcMemLazyEnablePeerAccess));
        x->opened[x->n_opened++] = pr;
        BM_HIP(hipIpcOpenMemHandle(&pf, bl[r].h_flags, hipIpcMemLazyEnablePeerAccess));
        x->opened[x->n_opened++] = pf;
        x->pbuf[r] = (const float *)((char *)pb + bl[r].off_buf);
        x->pred[r] = (const float *)pr;
        x->pflags[r] = (unsigned *)pf;
    }
    x->attached = true;
    return 0;
}

// Teardown is COLLECTIVE in one respect: a rank's kernel ends when every peer has published DONE, not when every peer
// has finished pulling this rank's staging slice - so a rank must not free `red` / `flags` while a slower peer may still
// be reading them.  The caller therefore places a host barrier over all ranks between the last exchange and
// bm_xchg_destroy (parallel.DirectExchange.close() does: one more gather of the rendezvous channel); the library
// cannot do it itself without a host channel.
int bm_xchg_destroy(bm_xchg *x) {
    if (!x) return 0;
    (void)hipDeviceSynchronize();
    if (x->user) *x->user = nullptr;
    for (int i = 0; i < x->n_opened; ++i) (void)hipIpcCloseMemHandle(x->opened[i]);
    if (x->red) (void)hipFree(x->red);
    if (x->tail_red) (void)hipFree(x->tail_red);
    if (x->tail_flag) (void)hipFree(x->tail_flag);
    if (x->ctr) (void)hipFree(x->ctr);
    if (x->flags) (void)hipFree(x->flags);
    delete x;
    return 0;
}

// in-place all-reduce(sum) of the registered buffer, enqueued on `stream`; every rank must call it in the same order
int bm_xchg_allreduce_sum(bm_xchg *x, void *stream) {
    BM_CHECK(x && x->attached, "exchange not attached (bm_xchg_export -> gather the blobs -> bm_xchg_attach)");
    bmx::Args a;
    memset(&a, 0, sizeof(a));
    a.buf = x->buf; a.red = x->red; a.count = x->count; a.chunk = x->chunk;
    a.rank = x->rank; a.n = x->nranks; a.epoch = ++x->epoch;
    for (int r = 0; r < bmx::MAXR; ++r) { a.pbuf[r] = x->pbuf[r]; a.pred[r] = x->pred[r]; a.pflags[r] = x->pflags[r]; }
    a.flags = x->flags; a.ctr = x->ctr; a.grid = x->grid; a.timeout_ticks = x->timeout_ticks;
    hipLaunchKernelGGL(bmx::allreduce_kernel, dim3(x->grid), dim3(bmx::NTX), 0, (hipStream_t)stream, a);
    BM_HIP(hipGetLastError());
    return 0;
}

// in-place all-reduce(max) of ONE non-negative float at val_dev (device memory of this rank), enqueued on `stream`
int bm_xchg_allreduce_max1(bm_xchg *x, float *val_dev, void *stream) {
    BM_CHECK(x && x->attached && val_dev, "exchange not attached / null argument");
    bmx::MaxArgs a;
    memset(&a, 0, sizeof(a));
    a.val = val_dev; a.slots = x->slots; a.flags = x->flags; a.rank = x->rank; a.n = x->nranks;
    a.epoch = ++x->epoch_max; a.timeout_ticks = x->timeout_ticks;
    for (int r = 0; r < bmx::MAXR; ++r)
        a.pslots[r] = (unsigned long long *)((char *)x->pflags[r] + bmx::F_WORDS * sizeof(unsigned));
    hipLaunchKernelGGL(bmx::max1_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    BM_HIP(hipGetLastError());
    return 0;
}

// 0 = every wait so far was answered; otherwise 16 * phase (1 READY, 2 DONE, 3 max) + rank waited for + 1.
// Synchronises the device.
int bm_xchg_status(bm_xchg *x, int32_t *out_status) {
    BM_CHECK(x && out_status, "null argument");
    BM_HIP(hipDeviceSynchronize());
    unsigned s = 0;
    BM_HIP(hipMemcpy(&s, x->flags + bmx::F_STATUS, sizeof(s), hipMemcpyDeviceToHost));
    *out_status = (int32_t)s;
    if (s) bm::set_error("bm_xchg: wait for rank %u timed out in phase %u (1 READY, 2 DONE, 3 max)", (s & 15u) - 1u, s >> 4);
    return 0;
}

// bound of every in-kernel wait of later launches (seconds; the default is BM_XCHG_TIMEOUT_S or 20 s)
int bm_xchg_set_timeout(bm_xchg *x, double seconds) {
    BM_CHECK(x && seconds > 0.0, "bad argument");
    x->timeout_ticks = (long long)(seconds * 1e8);
    return 0;
}

// Upper bound of the workgroups of every later exchange launch (default: up to 256, one per CU).  For ranks that SHARE a
// device (dry runs of the multi-rank path on one GPU): a launch whose workgroups sit on every CU and spin for a peer can
// keep that peer's own kernels - same device, another process - from ever being placed (observed: intermittent READY
// time-outs at 784 x 1024 with two ranks on one MI355X, never with small shapes); with a bound well below the CU count the
// peer always finds free CUs.  One rank per GPU needs no bound.  Before the first exchange only (the completion counter
// counts whole launches).
int bm_xchg_set_max_workgroups(bm_xchg *x, int32_t n) {
    BM_CHECK(x && n >= 1, "bad argument");
    BM_CHECK(x->epoch == 0, "bm_xchg_set_max_workgroups: call it before the first exchange");
    if (x->grid > n) x->grid = n;
    return 0;
}

int bm_xchg_info(bm_xchg *x, int32_t *out_rank, int32_t *out_nranks, size_t *out_count) {
    BM_CHECK(x, "null argument");
    if (out_rank) *out_rank = x->rank;
    if (out_nranks) *out_nranks = x->nranks;
    if (out_count) *out_count = x->count;
    return 0;
}

static int xchg_launch_apply(bm_rbm *h, bm_xchg *x, float N_global, float lr, float mom, int dw_only) {
    void *p = nullptr; size_t n = 0;
    BM_TRY(bm_rbm_dev_ptr(h, "grad", &p, &n));
    BM_CHECK(x->attached && p == (void *)x->buf && n == x->count, "the exchange was created for another buffer (gradient slots are not supported)");
    BM_CHECK(h->H % 4 == 0 && h->W.ld % 4 == 0 && h->W.ld == h->dW.ld, "the fused exchange needs n_hidden % 4 == 0");
    const size_t tail = (size_t)h->V + 2 * (size_t)h->H;
    if (!x->tail_red || x->tail_n < tail) {
        if (x->tail_red) (void)hipFree(x->tail_red);
        BM_HIP(hipMalloc((void **)&x->tail_red, (tail + 4) * sizeof(float)));
        x->tail_n = tail;
    }
    if (!x->tail_flag) {
        BM_HIP(hipMalloc((void **)&x->tail_flag, 64));
        BM_HIP(hipMemsetAsync(x->tail_flag, 0, 64, h->stream));
    }
    bmx::Args a;
    memset(&a, 0, sizeof(a));
    a.buf = x->buf; a.red = x->red; a.count = x->count; a.chunk = x->chunk;
    a.rank = x->rank; a.n = x->nranks; a.epoch = ++x->epoch;
    for (int r = 0; r < bmx::MAXR; ++r) { a.pbuf[r] = x->pbuf[r]; a.pred[r] = x->pred[r]; a.pflags[r] = x->pflags[r]; }
    a.flags = x->flags; a.ctr = x->ctr; a.grid = x->grid; a.timeout_ticks = x->timeout_ticks;
    bmx::RbmApply q;
    memset(&q, 0, sizeof(q));
    q.W = h->W.p; q.dW = h->dW.p;
    h->wt_valid = false;
    h->eff_valid = false;
    q.countW = (unsigned long long)h->V * h->W.ld;
    q.chunkW = (((q.countW + x->nranks - 1) / x->nranks) + 3) & ~3ull;
    BM_CHECK(q.chunkW <= x->chunk, "staging slice too small");       // chunk covers count / N >= countW / N
    q.I = h->H; q.ldw = h->W.ld; q.V = h->V; q.H = h->H;
    q.N = N_global; q.l2 = h->cfg.l2; q.lr = lr; q.mom = mom;
    q.damping = h->cfg.sparsity_damping; q.cost = h->cfg.sparsity_cost; q.target = h->cfg.sparsity_target;
    q.vb = h->vb.p; q.dvb = h->dvb.p; q.hb = h->hb.p; q.dhb = h->dhb.p; q.q = h->q.p; q.pen = h->pen.p;
    q.tail_red = x->tail_red; q.tail_flag = x->tail_flag; q.dw_only = dw_only;
    hipLaunchKernelGGL(bmx::exchange_apply_kernel, dim3(x->grid), dim3(bmx::NTX), 0, h->stream, a, q);
    BM_HIP(hipGetLastError());
    h->xchg_used = x; x->user = &h->xchg_used;
    return 0;
}

// data-parallel CD-k, the exchange and the update in ONE launch: replaces bm_rbm_allreduce_grads_direct +
// bm_rbm_apply_step (same bits).  After it every replica holds the new W, vb, hb, dvb, dhb, q_means; of dW every rank
// holds ITS slice (bm_rbm_exchange_gather_dw completes the replicas, e.g. before a checkpoint).
int bm_rbm_exchange_apply_direct(bm_rbm *h, bm_xchg *x, int32_t B_global, float lr, float mom) {
    BM_CHECK(!h || !h->cen_on, "bm_rbm_exchange_apply_direct: the exchange's fused apply has no centred form; switch centering off");
    BM_TRY(refuse_nrelu(h, "bm_rbm_exchange_apply_direct"));
    BM_CHECK(h && x, "null argument");
    BM_CHECK(B_global > 0, "bm_rbm_exchange_apply_direct: B_global = %d must be positive", B_global);
    BM_TRY(xchg_launch_apply(h, x, (float)B_global, lr, mom, 0));
    x->dw_stale = x->nranks > 1;
    h->dw_sharded = x->dw_stale;       // readers of dW fail until bm_rbm_exchange_gather_dw (check_dw, bm_rbm.hip)
    return 0;
}
// COLLECTIVE wherever the fused exchange can serve this engine (a property every rank shares), whether or not THIS rank's
// copy is stale: a rank that replaced dW itself (bm_rbm_set_param clears its flag) still enters the READY round its peers
// wait in - skipping on the local flag left them to their time-out (round-5 advisor).  bm_*_set_param(dW) on a
// data-parallel job must be made on every rank: the gather keeps each OWNER's slice.
int bm_rbm_exchange_gather_dw(bm_rbm *h, bm_xchg *x) {
    BM_CHECK(h && x, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_exchange_gather_dw"));
    if (x->nranks == 1 || (!x->dw_stale && !(h->H % 4 == 0 && h->W.ld % 4 == 0 && h->W.ld == h->dW.ld))) {
        x->dw_stale = false; h->dw_sharded = false; return 0;
    }
    BM_TRY(xchg_launch_apply(h, x, 1.f, 0.f, 0.f, 1));
    x->dw_stale = false;
    h->dw_sharded = false;
    return 0;
}

// the exchange step of data-parallel training over the direct path (bm_*_allreduce_grads over RCCL is the other)
int bm_rbm_xchg_create(bm_rbm *h, int32_t rank, int32_t nranks, bm_xchg **out) {
    BM_CHECK(h && out, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_xchg_create"));
    void *p = nullptr; size_t n = 0;
    BM_TRY(bm_rbm_dev_ptr(h, "grad", &p, &n));
    return bm_xchg_create(rank, nranks, (float *)p, n, out);
}
// columns of W_i a rank owns in the fused DBM exchange: a multiple of 32 (the tiles of maxnorm_scale_kernel and of the pull)
static int dbm_slice_width(int I, int nranks) { return 32 * ((I + 32 * nranks - 1) / (32 * nranks)); }
static size_t dbm_staging_floats(const bm_dbm *h, int nranks) {
    size_t need = 0;
    for (int i = 0; i < h->L; ++i) need += ((size_t)h->n[i] + 1) * (size_t)dbm_slice_width(h->n[i + 1], nranks);
    return need;
}
int bm_dbm_xchg_create(bm_dbm *h, int32_t rank, int32_t nranks, bm_xchg **out) {
    BM_CHECK(h && out, "null argument");
    void *p = nullptr; size_t n = 0;
    BM_TRY(bm_dbm_dev_ptr(h, "grad", &p, &n));
    return xchg_create(rank, nranks, (float *)p, n, nranks >= 1 ? dbm_staging_floats(h, nranks) : 0, out);
}

// 1 when bm_dbm_exchange_apply_direct can serve this engine (every layer width a multiple of 4, offsets within 4 GiB)
static bool dbm_fused_ok(const bm_dbm *h, const bm_xchg *x) {
    if (!x->attached || x->buf != h->grad.p || x->count != h->grad.n) return false;
    if (((x->count + 3) & ~(size_t)3) * sizeof(float) >= 0xfffffff0ull || x->red_cap * sizeof(float) >= 0xfffffff0ull) return false;
    if (dbm_staging_floats(h, x->nranks) > x->red_cap) return false;
    for (int i = 0; i < h->L; ++i)
        if (h->n[i + 1] % 4 != 0 || h->W[i].ld % 4 != 0 || h->Wt[i].ld % 4 != 0 || h->W[i].ld != h->dW[i].ld) return false;
    return true;
}
int bm_dbm_exchange_apply_ok(bm_dbm *h, bm_xchg *x, int32_t *out_ok) {
    BM_CHECK(h && x && out_ok, "null argument");
    *out_ok = dbm_fused_ok(h, x) ? 1 : 0;
    return 0;
}

static int dbm_fill_exchange(bm_dbm *h, bm_xchg *x, bmx::Args &a, bmx::DbmApply &q, bool new_epoch) {
    memset(&a, 0, sizeof(a));
    a.buf = x->buf; a.red = x->red; a.count = x->count; a.chunk = x->chunk; a.red_cap = x->red_cap;
    a.rank = x->rank; a.n = x->nranks; a.epoch = new_epoch ? ++x->epoch : x->epoch;
    for (int r = 0; r < bmx::MAXR; ++r) { a.pbuf[r] = x->pbuf[r]; a.pred[r] = x->pred[r]; a.pflags[r] = x->pflags[r]; }
    a.flags = x->flags; a.ctr = x->ctr; a.grid = x->grid; a.timeout_ticks = x->timeout_ticks;
    memset(&q, 0, sizeof(q));
    q.L = h->L;
    size_t roff = 0;
    for (int i = 0; i < h->L; ++i) {
        bmx::DbmLayerX &y = q.lay[i];
        y.W = h->W[i].p; y.dW = h->dW[i].p; y.Wt = h->Wt[i].p; y.wnorm = h->wnorm[i].p; y.pen = h->pen[i].p;
        y.off_pos = h->raw_off[i][0]; y.off_neg = h->raw_off[i][1];
        y.I = h->n[i + 1]; y.J = h->n[i]; y.ldw = h->W[i].ld; y.ldwt = h->Wt[i].ld;
        y.sw = dbm_slice_width(y.I, x->nranks);
        y.red_off = roff;
        roff += ((size_t)y.J + 1) * (size_t)y.sw;
    }
    return 0;
}

// Data-parallel DBM update, exchange and update fused (see dbm_exchange_apply_kernel): replaces
// bm_dbm_allreduce_grads_direct + bm_dbm_apply_step, same bits.  Afterwards every replica holds the new W_i, W_i^T, column
// norms, biases, running means; of the momentum buffers dW_i a rank holds its columns (bm_dbm_exchange_gather_dw).
int bm_dbm_exchange_apply_direct(bm_dbm *h, bm_xchg *x, int32_t N_global, int32_t M_global, float lr, float mom) {
    BM_CHECK(!h || !h->cen_on, "bm_dbm_exchange_apply_direct: the exchange's fused apply has no centred form; switch centering off");
    BM_CHECK(h && x, "null argument");
    BM_CHECK(N_global > 0 && M_global > 0, "bm_dbm_exchange_apply_direct: N_global = %d and M_global = %d must be positive", N_global, M_global);
    BM_CHECK(!h->failed, "an earlier launch of this engine failed");
    BM_CHECK(dbm_fused_ok(h, x), "the fused DBM exchange needs an attached exchange created by bm_dbm_xchg_create for this "
                                 "engine and layer widths that are multiples of 4 (bm_dbm_exchange_apply_ok)");
    const size_t nsums = h->grad.n - (size_t)(h->sums_p - h->grad.p);
    if (!x->tail_red || x->tail_n < nsums) {
        if (x->tail_red) (void)hipFree(x->tail_red);
        BM_HIP(hipMalloc((void **)&x->tail_red, (nsums + 4) * sizeof(float)));
        x->tail_n = nsums;
    }
    if (!x->tail_flag) {
        BM_HIP(hipMalloc((void **)&x->tail_flag, 64));
        BM_HIP(hipMemsetAsync(x->tail_flag, 0, 64, h->stream));
    }
    bmx::Args a; bmx::DbmApply q;
    BM_TRY(dbm_fill_exchange(h, x, a, q, true));
    q.off_sums = (unsigned long long)(h->sums_p - h->grad.p); q.n_sums = (int)nsums;
    q.N = (float)N_global; q.M = (float)M_global; q.l2 = h->cfg.l2; q.lr = lr; q.mom = mom;
    q.tail_red = x->tail_red; q.tail_flag = x->tail_flag;
    {   // launch_dbm_biases' arguments with the column sums read from the reduced tail
        DbmBiasArgs &b = q.bias[0];
        b.s_pos = x->tail_red + sums_off(h, 0); b.s_neg = x->tail_red + sums_off(h, 1);
        b.b = h->vb.p; b.db = h->dvb.p; b.n = h->V; b.N = q.N; b.M = q.M; b.lr = lr; b.mom = mom;
        for (int i = 0; i < h->L; ++i) {
            DbmBiasArgs &c = q.bias[1 + i];
            c.s_pos = x->tail_red + sums_off(h, 2 + 2 * i); c.s_neg = x->tail_red + sums_off(h, 3 + 2 * i);
            c.b = h->hb[i].p; c.db = h->dhb[i].p; c.q = h->q[i].p; c.mm = h->mm[i].p; c.pen = h->pen[i].p;
            c.n = h->n[i + 1]; c.layer = i; c.N = q.N; c.M = q.M; c.lr = lr; c.mom = mom;
            c.damping = h->cfg.sparsity_damping; c.cost = h->cfg.sparsity_cost[i]; c.target = h->cfg.sparsity_target[i];
        }
    }
    hipLaunchKernelGGL(bmx::dbm_exchange_apply_kernel, dim3(x->grid), dim3(bmx::NTX), 0, h->stream, a, q);
    for (int i = 0; i < h->L; ++i) {
        const int c0 = x->rank * q.lay[i].sw;
        const int c1 = c0 + q.lay[i].sw < q.lay[i].I ? c0 + q.lay[i].sw : q.lay[i].I;
        launch_dbm_maxnorm(h, i, c0, c1 > c0 ? c1 : c0);            // the owned columns (none: no launch)
    }
    hipLaunchKernelGGL(bmx::dbm_exchange_gather_kernel, dim3(x->grid), dim3(bmx::NTX), 0, h->stream, a, q);
    BM_HIP(hipGetLastError());
    h->xchg_used = x; x->user = &h->xchg_used;
    x->dw_stale = x->nranks > 1;
    h->dw_sharded = x->dw_stale;
    h->dw_set_mask = 0;
    BM_CHECK(!h->failed, "a launch helper of this update could not allocate");       // bm_dbm_apply_step's post-condition
    return 0;
}
int bm_dbm_exchange_gather_dw(bm_dbm *h, bm_xchg *x) {          // collective like bm_rbm_exchange_gather_dw, see there
    BM_CHECK(h && x, "null argument");
    if (x->nranks == 1 || (!x->dw_stale && !dbm_fused_ok(h, x))) { x->dw_stale = false; h->dw_sharded = false; return 0; }
    BM_CHECK(dbm_fused_ok(h, x), "the exchange does not belong to this engine");
    bmx::Args a; bmx::DbmApply q;
    BM_TRY(dbm_fill_exchange(h, x, a, q, true));
    q.mode = 1; q.do_ready = 1;
    hipLaunchKernelGGL(bmx::dbm_exchange_gather_kernel, dim3(x->grid), dim3(bmx::NTX), 0, h->stream, a, q);
    BM_HIP(hipGetLastError());
    h->xchg_used = x; x->user = &h->xchg_used;
    x->dw_stale = false;
    h->dw_sharded = false;
    return 0;
}
// ---- chain-sharded AIS over the direct exchange (dbm.py:922-939 returns every chain's value)
// The all-gather of the per-chain values as an all-reduce(sum) of a window of the registered buffer in which every rank has
// written ITS chains at their global index and zeros everywhere else: x + 0 + ... + 0 is x exactly, so every rank receives
// the bits the owner computed, through the one exchange kernel that the gradient path uses (READY / reduce / DONE / gather,
// bounded waits, NaN poison on a lost rank).  `n` floats of the buffer take part (chunk = ceil(n / ranks), like a buffer of
// that length); the launch width stays the exchange's own - its completion counter counts whole launches.
static int xchg_allreduce_prefix(bm_xchg *x, size_t n, hipStream_t stream) {
    BM_CHECK(x && x->attached && n >= 1 && n <= x->count, "exchange not attached / bad prefix length");
    bmx::Args a;
    memset(&a, 0, sizeof(a));
    a.buf = x->buf; a.red = x->red; a.count = n;
    a.chunk = (((n + x->nranks - 1) / x->nranks) + 3) & ~(size_t)3;
    BM_CHECK(a.chunk <= x->red_cap, "staging slice too small");
    a.rank = x->rank; a.n = x->nranks; a.epoch = ++x->epoch;
    for (int r = 0; r < bmx::MAXR; ++r) { a.pbuf[r] = x->pbuf[r]; a.pred[r] = x->pred[r]; a.pflags[r] = x->pflags[r]; }
    a.flags = x->flags; a.ctr = x->ctr; a.grid = x->grid; a.timeout_ticks = x->timeout_ticks;
    hipLaunchKernelGGL(bmx::allreduce_kernel, dim3(x->grid), dim3(bmx::NTX), 0, stream, a);
    BM_HIP(hipGetLastError());
    return 0;
}

// window[e] = value of global chain lo + e when this rank owns it (chains [a, b)), else 0; `fail`: NaN instead of the values
__global__ void ais_window_kernel(const double *logw, float *win, int lo, int n_win, int a, int b, double logZ0, int literal, int fail) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_win) return;
    const int c = lo + e;
    float v = 0.f;
    if (c >= a && c < b) v = fail ? __builtin_nanf("") : (literal ? (float)logw[c - a] + (float)logZ0 : (float)(logw[c - a] + logZ0));
    win[e] = v;
}

// Like bm_dbm_ais_sharded, with the direct exchange in the place of the RCCL communicator: this rank runs chains [a, b) of
// n_runs_total (the same contiguous slices), no communication during the sweep, then the values travel through the
// exchange's registered buffer (the engine's gradient payload: overwritten, it is recomputed by every update) in windows
// of at most its length - one window, one launch, for any realistic n_runs.  Every rank returns all n_runs_total values.
int bm_dbm_ais_sharded_direct(bm_dbm *h, bm_xchg *x, int32_t n_betas, int32_t n_runs_total, int32_t k, uint64_t seed,
                              float *values_host) {
    BM_CHECK(h && x && values_host, "null argument");
    BM_CHECK(x->attached, "exchange not attached");
    BM_CHECK(n_runs_total >= 1, "bad AIS arguments");
    void *gp = nullptr; size_t gn = 0;
    BM_TRY(bm_dbm_dev_ptr(h, "grad", &gp, &gn));
    BM_CHECK(gp == (void *)x->buf && gn == x->count, "the exchange was created for another buffer");
    BM_CHECK(!h->dw_sharded, "the momentum buffers are sharded (bm_dbm_exchange_gather_dw first)");
    const int rank = x->rank, world = x->nranks;
    const int q = n_runs_total / world, rem = n_runs_total % world;
    const int a = rank * q + (rank < rem ? rank : rem), b = a + q + (rank < rem ? 1 : 0);
    // A rank whose sweep fails must still enter the exchange - the others would wait for it until their time-out - so the
    // failure is made collective: the failing rank contributes NaNs and every rank reports the error.
    std::string first_err;
    int rc = 0;
    if (b > a) rc = ais_core(h, n_betas, b - a, k, seed, a);
    if (rc) { first_err = bm_last_error(); (void)hipGetLastError(); }
    const double z0 = ais_log_Z0(h, h->ais_literal != 0);
    h->xchg_used = x; x->user = &h->xchg_used;
    int rc_x = 0, rc_m = 0;
    for (size_t lo = 0; lo < (size_t)n_runs_total && !rc_x && !rc_m; lo += x->count) {
        const size_t nw = (size_t)n_runs_total - lo < x->count ? (size_t)n_runs_total - lo : x->count;
        hipLaunchKernelGGL(ais_window_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream,
                           (const double *)h->alogw.p, x->buf, (int)lo, (int)nw, a, b, z0, h->ais_literal, rc ? 1 : 0);
        rc_x = xchg_allreduce_prefix(x, nw, h->stream);
        if (rc_x) { if (first_err.empty()) first_err = bm_last_error(); break; }
        if (hipMemcpyAsync(values_host + lo, x->buf, nw * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc_m = 1;
        if (hipStreamSynchronize(h->stream) != hipSuccess) rc_m = 1;       // the window is reused by the next round
    }
    if (rc || rc_x) { bm::set_error("bm_dbm_ais_sharded_direct (rank %d): %s", rank, first_err.c_str()); return rc ? rc : rc_x; }
    if (rc_m) { bm::set_error("bm_dbm_ais_sharded_direct: device copy / synchronisation failed"); return 1; }
    BM_TRY(xchg_check_status(x));                    // a wait that expired (a lost rank): sticky, the values are NaN
    for (int e = 0; e < n_runs_total; ++e)
        BM_CHECK(values_host[e] == values_host[e], "bm_dbm_ais_sharded_direct: another rank's AIS sweep failed (chain %d arrived as NaN)", e);
    return 0;
}

int bm_rbm_allreduce_grads_direct(bm_rbm *h, bm_xchg *x) {
    BM_CHECK(h && x, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_allreduce_grads_direct"));
    void *p = nullptr, *st = nullptr; size_t n = 0;
    BM_TRY(bm_rbm_dev_ptr(h, "grad", &p, &n));
    BM_CHECK(p == (void *)x->buf && n == x->count, "the exchange was created for another buffer (gradient slots are not supported)");
    BM_TRY(bm_rbm_stream(h, &st));
    h->xchg_used = x; x->user = &h->xchg_used;
    return bm_xchg_allreduce_sum(x, st);
}
int bm_dbm_allreduce_grads_direct(bm_dbm *h, bm_xchg *x) {
    BM_CHECK(h && x, "null argument");
    void *p = nullptr, *st = nullptr; size_t n = 0;
    BM_TRY(bm_dbm_dev_ptr(h, "grad", &p, &n));
    BM_CHECK(p == (void *)x->buf && n == x->count, "the exchange was created for another buffer");
    BM_TRY(bm_dbm_stream(h, &st));
    h->xchg_used = x; x->user = &h->xchg_used;
    return bm_xchg_allreduce_sum(x, st);
}

}  // extern "C"
