// bm_rsm.hip - replicated softmax visible units: the instantiations of act_kernel's DB flavour (the prop-up
// with a length-scaled bias), row_lengths_kernel, multinomial_counts_kernel (the prop-down's count sampler for vocabulary-wide
// rows, and its AIS flavour with rsm_fill_rows_kernel: DESIGN.md 3.28) and rsm_bias_kernel (the bias block with length-weighted
// hidden sums).  A translation unit of its own, as bm_nrelu.hip
// and bm_softmax_v.hip are: the kernels of the other units are compiled exactly as before.  Compiled into libbm355.so next to
// bm355.hip.  bm_rsm.h fixes the operation sequences.
#define BM_KERNELS_ONLY
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_rsm.h"

namespace bm {

// geo: the codes of launch_act_as.  A DB pass is a single-segment Bernoulli prop-up in either operand layout
void launch_act_db_as(int geo, const ActArgs &a, hipStream_t st) { launch_act_as<FL_DB>(geo, a, st); }      // (bm_launch.h)

// ---- row_lengths_kernel (bm_rsm.h): one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void row_lengths_kernel(RowLenArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.J) return;
    const float *x = a.X + (size_t)row * a.ld;
    float s = 0.f;
    int flags = 0;
    for (int i = lane; i < a.V; i += 64) {
        const float v = x[i];
        if (v < 0.f) flags |= RSM_BAD_NEGATIVE;
        if (!(fabsf(v) < 16777216.0f) || v != truncf(v)) flags |= RSM_BAD_FRACTION;
        s += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); flags |= __shfl_xor(flags, off); }
    if (lane == 0) {
        if (s == 0.f) flags |= RSM_BAD_EMPTY;
        if (s > (float)a.max_length) flags |= RSM_BAD_LONG;
        a.D[row] = s;
        if (flags) atomicOr(a.bad, flags);
    }
}
void launch_row_lengths(const RowLenArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(row_lengths_kernel, dim3((a.J + 3) / 4), dim3(256), 0, st, a);
}

// ---- multinomial_counts_kernel (bm_rsm.h).  RPT runs of 16 units per thread: thread tid owns the runs p * 256 + tid, p < RPT -
// its e values stay in registers from the load to the stores, c and the counts of the row live in LDS (CAP = RPT * 4096 units).
// A run is four 16-byte loads where the row is 16-byte aligned and the run lies inside it; scalar loads at the ragged end and
// for unaligned rows.  Level 1 of the prefix order runs in the 16-lane groups of a wave (15 dependent shuffle steps, every group
// of the workgroup at once), level 2 in thread 0 over at most 64 block totals.
// AIS (bm_rsm.h: McAisArgs): behind the draws the row's state . dvec from the counts in LDS, in double, as a float32 pair.
// PT (bm_rsm.h: McPtArgs; on top of AIS): the logits are formed on load from the raw z, the bias and the row's temperature and never
// stored, no means are stored, the beta = 1 row of a chain repeats its counts in the dense particle store.
template <int RPT, bool AIS = false, bool PT = false>
__global__ __launch_bounds__(256) void multinomial_counts_kernel(std::conditional_t<PT, McPtArgs, std::conditional_t<AIS, McAisArgs, McArgs>> a) {
    static_assert(AIS || !PT, "the PT flavour sits on top of the AIS flavour");
    constexpr int CAP = RPT * 4096;
    __shared__ __attribute__((aligned(16))) float s_c[CAP];
    __shared__ __attribute__((aligned(16))) int s_cnt[CAP];
    __shared__ float s_blk[RPT * 16], s_base[RPT * 16], s_red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, l16 = tid & 15;
    float *l = a.L + (size_t)row * a.ld;
    const int V = a.V;
    const bool al = (((uintptr_t)l) & 15u) == 0;
    constexpr float NEG = -3.402823466e38f;
    float v[RPT][16];
    float mx = NEG;
    float beta = 1.0f;
    (void)beta;
    if constexpr (PT) beta = a.row_mult[row];
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int i0 = (p * 256 + tid) * 16;
        if constexpr (PT) {
            // l = fl(fl(beta z) + fl(beta b)): RT's two rounded multiplies and one rounded add (a null L / bias reads as zeros)
            if (i0 < V) {
                if (a.L && al && i0 + 16 <= V) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 t = *reinterpret_cast<const float4 *>(l + i0 + 4 * q);
                        v[p][4 * q] = t.x; v[p][4 * q + 1] = t.y; v[p][4 * q + 2] = t.z; v[p][4 * q + 3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[p][k] = (a.L && i0 + k < V) ? l[i0 + k] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float b = (a.bias && i0 + k < V) ? a.bias[i0 + k] : 0.0f;
                    v[p][k] = (i0 + k < V) ? __fadd_rn(__fmul_rn(beta, v[p][k]), __fmul_rn(beta, b)) : NEG;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) v[p][k] = NEG;
            }
        } else if (al && i0 + 16 <= V) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 t = *reinterpret_cast<const float4 *>(l + i0 + 4 * q);
                v[p][4 * q] = t.x; v[p][4 * q + 1] = t.y; v[p][4 * q + 2] = t.z; v[p][4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) v[p][k] = (i0 + k < V) ? l[i0 + k] : NEG;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) mx = fmaxf(mx, v[p][k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    // e (zero past the row's end), level 0 totals, level 1 offsets
    float O[RPT];
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int i0 = (p * 256 + tid) * 16;
        float T = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float d = mx - v[p][k];
            if (d > 80.0f) d = 80.0f;
            const float e = (i0 + k < V) ? exp_neg(d) : 0.0f;
            v[p][k] = e;
            T = T + e;
        }
        float incl = T, off = 0.f;
        for (int q = 1; q < 16; ++q) {                  // O_q = O_{q-1} + T_{q-1}, one step per run of the block
            const float prev = __shfl(incl, (lane & 48) + q - 1);
            if (l16 == q) { off = prev; incl = prev + T; }
        }
        O[p] = off;
        if (l16 == 15) s_blk[p * 16 + (tid >> 4)] = incl;      // local[15][15], the block's total
    }
    __syncthreads();
    if (tid == 0) {                                     // level 2: the blocks in ascending order
        float base = 0.f;
        for (int b = 0; b < RPT * 16; ++b) { s_base[b] = base; base = base + s_blk[b]; }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int i0 = (p * 256 + tid) * 16;
        const float base = s_base[p * 16 + (tid >> 4)];
        float r = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 t;
            r = r + v[p][4 * q];     t.x = base + (O[p] + r);
            r = r + v[p][4 * q + 1]; t.y = base + (O[p] + r);
            r = r + v[p][4 * q + 2]; t.z = base + (O[p] + r);
            r = r + v[p][4 * q + 3]; t.w = base + (O[p] + r);
            *reinterpret_cast<float4 *>(s_c + i0 + 4 * q) = t;
            if (a.sample && a.states) *reinterpret_cast<int4 *>(s_cnt + i0 + 4 * q) = make_int4(0, 0, 0, 0);
        }
    }
    __syncthreads();
    const float S = s_c[V - 1], D = a.lengths[row];
    float *st = a.states ? a.states + (size_t)row * a.ld_states : nullptr;
    const bool al_st = st && (((uintptr_t)st) & 15u) == 0;
    const bool counts = st && a.sample;
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        if constexpr (PT) break;                        // no means: the logits of a tempered row do not touch memory
        const int i0 = (p * 256 + tid) * 16;
        if (i0 >= V) continue;
#pragma unroll
        for (int k = 0; k < 16; ++k) v[p][k] = __fmul_rn(D, v[p][k] / S);
        if (al && i0 + 16 <= V) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4 *>(l + i0 + 4 * q) = make_float4(v[p][4 * q], v[p][4 * q + 1], v[p][4 * q + 2], v[p][4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) if (i0 + k < V) l[i0 + k] = v[p][k];
        }
        if (st && !counts) {
#pragma unroll
            for (int k = 0; k < 16; ++k) if (i0 + k < V) st[i0 + k] = v[p][k];
        }
    }
    if (!counts) return;                                // (uniform over the workgroup)
    // the row's draws: Philox block by block, the words whose flat index lies in [idx0, idx0 + Dn) - philox_uniform_at of that index
    // (a length outside [0, max_length] belongs to a row that row_lengths_kernel has flagged: clamped, so that nothing runs away)
    const int Dn = (D >= 0.f) ? ((D < (float)a.max_length) ? (int)D : a.max_length) : 0;
    const unsigned long long idx0 = (unsigned long long)(a.row0 + row) * (unsigned long long)a.max_length, idx1 = idx0 + (unsigned long long)Dn;
    if (Dn > 0) {
        const unsigned long long blk_last = (idx1 - 1) >> 2;
        for (unsigned long long blk = (idx0 >> 2) + (unsigned long long)tid; blk <= blk_last; blk += 256) {
            uint32_t w[4];
            philox_block(a.key, blk, w);
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                const unsigned long long flat = 4 * blk + (unsigned long long)wd;
                if (flat < idx0 || flat >= idx1) continue;
                const float t = u32_to_uniform(w[wd]) * S;
                int lo = 0, hi = V - 1;                  // smallest i with c[i] > t; hi = V - 1 is the clamp
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_c[mid] > t) hi = mid; else lo = mid + 1;
                }
                atomicAdd(s_cnt + lo, 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RPT; ++p) {
        const int i0 = (p * 256 + tid) * 16;
        if (i0 >= V) continue;
        if (al_st && i0 + 16 <= V) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 t = *reinterpret_cast<const int4 *>(s_cnt + i0 + 4 * q);
                *reinterpret_cast<float4 *>(st + i0 + 4 * q) = make_float4((float)t.x, (float)t.y, (float)t.z, (float)t.w);
            }
        } else {
            for (int k = 0; k < 16; ++k) if (i0 + k < V) st[i0 + k] = (float)s_cnt[i0 + k];
        }
    }
    if constexpr (PT) {                                 // the hand-over: the chain's beta = 1 row, chains c < sel_rows (uniform over the workgroup)
        if (a.sel_out && beta == 1.0f && row / a.sel_R < a.sel_rows) {
            float *so = a.sel_out + (size_t)(row / a.sel_R) * a.sel_ld;
            for (int i = tid; i < V; i += 256) so[i] = (float)s_cnt[i];
        }
    }
    if constexpr (AIS) {
        // state . dvec in double, by the three levels of the prefix order (bm_rsm.h): every product is exact, the padding adds zeros
        __shared__ double s_dr[RPT * 256], s_db[RPT * 16];
#pragma unroll
        for (int p = 0; p < RPT; ++p) {
            const int i0 = (p * 256 + tid) * 16;
            double r = 0.0;
            if (i0 < V) {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (i0 + k < V) r = r + (double)s_cnt[i0 + k] * (double)a.dvec[i0 + k];
            }
            s_dr[p * 256 + tid] = r;
        }
        __syncthreads();
        if (tid < RPT * 16) {                           // level 1: the 16 runs of block `tid` in ascending order
            double b = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) b = b + s_dr[tid * 16 + q];
            s_db[tid] = b;
        }
        __syncthreads();
        if (tid == 0) {                                 // level 2: the blocks in ascending order
            double s = 0.0;
            for (int b = 0; b < RPT * 16; ++b) s = s + s_db[b];
            const float hi = (float)s, lo = (float)(s - (double)hi);
            a.part[row] = hi;
            a.part[(size_t)a.ld_part + row] = lo;
        }
    }
}

int launch_multinomial_counts_ais(const McAisArgs &a, hipStream_t st) {
    if (a.V < 2 || a.V > RSM_MAX_V || !a.sample || !a.states || !a.dvec || !a.part || a.ld_part < a.J) {
        fprintf(stderr, "bm355: the AIS flavour of multinomial_counts_kernel draws the counts of rows of 2 to %d units (got %d) and leaves "
                "their state . dvec: it needs states, dvec and partials of pitch >= J\n", RSM_MAX_V, a.V);
        return 1;
    }
    if (a.J < 1) return 0;
    if (a.V <= 4096) hipLaunchKernelGGL((multinomial_counts_kernel<1, true>), dim3(a.J), dim3(256), 0, st, a);
    else             hipLaunchKernelGGL((multinomial_counts_kernel<4, true>), dim3(a.J), dim3(256), 0, st, a);
    return 0;
}

int launch_multinomial_counts_pt(const McPtArgs &a, hipStream_t st) {
    if (a.V < 2 || a.V > RSM_MAX_V || !a.sample || !a.states || !a.dvec || !a.part || a.ld_part < a.J || !a.row_mult ||
        (a.sel_out && (a.sel_R < 1 || a.sel_rows < 0 || a.sel_ld < a.V))) {
        fprintf(stderr, "bm355: the PT flavour of multinomial_counts_kernel draws the counts of rows of 2 to %d units (got %d) under a temperature "
                "per row and leaves their state . dvec: it needs states, dvec, row_mult and partials of pitch >= J\n", RSM_MAX_V, a.V);
        return 1;
    }
    if (a.J < 1) return 0;
    if (a.V <= 4096) hipLaunchKernelGGL((multinomial_counts_kernel<1, true, true>), dim3(a.J), dim3(256), 0, st, a);
    else             hipLaunchKernelGGL((multinomial_counts_kernel<4, true, true>), dim3(a.J), dim3(256), 0, st, a);
    return 0;
}

// ---- rsm_fill_rows_kernel (bm_rsm.h): L[j][i] = a[i]
__global__ __launch_bounds__(256) void rsm_fill_rows_kernel(float *L, int ld, int J, int V, const float *a) {
    const size_t n = (size_t)J * (size_t)V;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t j = e / (size_t)V, i = e % (size_t)V;
        L[j * (size_t)ld + i] = a[i];
    }
}
void launch_rsm_fill_rows(float *L, int ld, int J, int V, const float *a, hipStream_t st) {
    if (J < 1) return;
    const size_t n = (size_t)J * (size_t)V;
    const unsigned grid = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(rsm_fill_rows_kernel, dim3(grid), dim3(256), 0, st, L, ld, J, V, a);
}

int launch_multinomial_counts(const McArgs &a, hipStream_t st) {
    if (a.V < 2 || a.V > RSM_MAX_V) {
        fprintf(stderr, "bm355: multinomial_counts_kernel serves rows of 2 to %d units (got %d): a row's prefix sums and counts live in LDS\n",
                RSM_MAX_V, a.V);
        return 1;
    }
    if (a.J < 1) return 0;
    if (a.V <= 4096) hipLaunchKernelGGL(multinomial_counts_kernel<1>, dim3(a.J), dim3(256), 0, st, a);
    else             hipLaunchKernelGGL(multinomial_counts_kernel<4>, dim3(a.J), dim3(256), 0, st, a);
    return 0;
}

// ---- rsm_bias_kernel (bm_rsm.h): the grid of rbm_bias_fused_kernel; a visible group is rbm_bias_fused_block itself
// TWO (the tempered update): the negative rows have lengths of their own, lengths_neg [B] - the term of row b is
// __fsub_rn(__fmul_rn(D_b, h0), __fmul_rn(Dn_b, hk)), from the negated store __fadd_rn(__fmul_rn(D_b, h0), __fmul_rn(Dn_b, -hk)): the
// same bits.  A compile-time flavour: the kernel of the CD path carries none of it
template <bool TWO>
__device__ __forceinline__ void rsm_bias_body(const RbmBiasFusedArgs &a, const float *lengths, const float *lengths_neg) {
    __shared__ __attribute__((aligned(16))) float smem[CS_SMEM_FLOATS];
    __shared__ float s_w[64];
    float *s_t = smem;                                  // [64][64] terms of a chunk of rows, ahead of block_colsum's use of smem
    const int wv = blockIdx.x, nv = (a.u.V + 63) / 64;
    if (wv < nv) { rbm_bias_fused_block(a, wv, smem); return; }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int c0 = (wv - nv) * 64;
    {
        // the length-weighted sum of column c0 + (tid & 63), rows in ascending order: the terms D_b (h0 - hk) of 64 rows at a time
        // are formed by the whole workgroup into LDS (the loads of a chunk are independent: one memory round trip per chunk, not
        // one per row), then the first wave adds them row by row
        const int col = tid & 63, rq = tid >> 6, h = c0 + col;
        float s = 0.f;
        for (int b0 = 0; b0 < a.B; b0 += 64) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = rq + 4 * i, b = b0 + r;
                float t = 0.f;
                if (b < a.B && h < a.u.H) {
                    const float p = a.h0m[(size_t)b * a.ldh0 + h], n = a.hm[(size_t)b * a.ldh + h];
                    if constexpr (TWO) {
                        const float tp = __fmul_rn(lengths[b], p), tn = __fmul_rn(lengths_neg[b], n);
                        t = a.hm_negated ? __fadd_rn(tp, tn) : __fsub_rn(tp, tn);
                    } else {
                        const float d = a.hm_negated ? __fadd_rn(p, n) : __fsub_rn(p, n);
                        t = __fmul_rn(lengths[b], d);
                    }
                }
                s_t[r * 64 + col] = t;
            }
            __syncthreads();
            if (tid < 64) {
                const int nr = (a.B - b0 < 64) ? a.B - b0 : 64;
#pragma unroll 8
                for (int r = 0; r < nr; ++r) s = __fadd_rn(s, s_t[r * 64 + tid]);
            }
            __syncthreads();
        }
        if (tid < 64) s_w[tid] = s;
    }
    f32x4 s1, s2;
    block_colsum(a.h0m, a.ldh0, a.hm, a.ldh, c0, a.u.H, a.B, true, smem, s1, s2, a.hm_negated != 0);      // (s2: sum(h_k), as the plain block forms it)
    __syncthreads();
    if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cl = w * 16 + g * 4 + r, h = c0 + cl;
            if (h < a.u.H) {
                const float sh = s_w[cl], sq = s2[r];
                a.raw_tail[a.u.V + h] = sh;
                a.raw_tail[a.u.V + a.u.H + h] = sq;
                const float qn = a.u.damping * a.u.q[h] + (1.0f - a.u.damping) * sq;
                a.u.q[h] = qn;
                const float pen = a.u.cost * (qn - a.u.target);
                a.u.pen[h] = pen;
                float gr = sh / a.u.N;
                gr = gr - pen;
                const float d = a.u.lr * (a.u.mom * a.u.dhb[h] + gr);
                a.u.dhb[h] = d;
                a.u.hb[h] = a.u.hb[h] + d;
            }
        }
    }
}
__global__ __launch_bounds__(NT) void rsm_bias_kernel(RbmBiasFusedArgs a, const float *lengths) { rsm_bias_body<false>(a, lengths, nullptr); }
__global__ __launch_bounds__(NT) void rsm_bias2_kernel(RbmBiasFusedArgs a, const float *lengths, const float *lengths_neg) {
    rsm_bias_body<true>(a, lengths, lengths_neg);
}
void launch_rsm_bias2(const RbmBiasFusedArgs &a, const float *lengths, const float *lengths_neg, hipStream_t st) {
    hipLaunchKernelGGL(rsm_bias2_kernel, dim3((a.u.V + 63) / 64 + (a.u.H + 63) / 64), dim3(NT), 0, st, a, lengths, lengths_neg);
}
void launch_rsm_bias(const RbmBiasFusedArgs &a, const float *lengths, hipStream_t st) {
    hipLaunchKernelGGL(rsm_bias_kernel, dim3((a.u.V + 63) / 64 + (a.u.H + 63) / 64), dim3(NT), 0, st, a, lengths);
}

}  // namespace bm
