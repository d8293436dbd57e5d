// bm_dbm.hip — C-ABI entry points for the DBM path (include/bm355.h): block-Gibbs
// sweep, mean-field, PCD particles, train op, sample_v, reconstruction, AIS, ELBO.
//
// Reference graph restated: boltzmann_machines/dbm.py:385-427 (Gibbs sweep),
// :429-478 (mean-field), :480-509 (particles), :511-639 (train op + max-norm),
// :641-648 (sample_v), :650-736 (AIS), :738-759 (ELBO).  Every layer update is one
// act_kernel launch (two-sided inputs = two K segments of one MFMA pipeline).
#include "../../include/bm355.h"
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_pass.h"
#include "bm_pt.h"
#include "bm_center.h"

#include <math.h>
#include <memory>

using namespace bm;

struct bm_xchg;
// bm_xchg.hip: mf_resid_kernel + bm_xchg_allreduce_max1 + mf_latch_kernel as one launch (the per-sweep loop control of a
// data-parallel mean-field over the direct exchange)
static int xchg_mf_ctl_step(bm_xchg *x, MfCtl *ctl, float *blk, int nblk, float tol, int init, hipStream_t stream);

namespace {
// RNG sites (counter word 2 = site + 16 * sweep index); DESIGN.md "RNG"
enum : uint32_t { SITE_DBM_H = 8 /* + layer */, SITE_DBM_V = 12, SITE_AIS_X0 = 13 };
// bm_dbm_pt_* (bm355.h): the swap uniforms (flat index = global chain * (R - 1) + ladder pair) and the random start (v_0 at
// t = 0, h2_0 at t = 1 of the site)
enum : uint32_t { SITE_DBM_PT_SWAP = 14, SITE_DBM_PT_START = 15 };
constexpr int MAXL = BM_DBM_MAX_LAYERS;
}  // namespace

struct bm_dbm {
    bm_dbm_config cfg;
    bm_xchg *xchg_used = nullptr;          // the direct exchange this engine last used (bm_dbm_sync checks its status word)
    // after bm_dbm_exchange_apply_direct (bm_xchg.hip) a rank holds only ITS column slices of the momentum buffers dW_i:
    // every reader - get_param, the single-GPU update, apply_step - fails until bm_dbm_exchange_gather_dw (check_dw)
    bool dw_sharded = false;
    unsigned dw_set_mask = 0;              // layers whose dW the host has replaced since the buffers became sharded
    int L, V, N, M;
    int n[MAXL + 1];                       // n[0] = V, n[i+1] = hidden layer i
    Stream stream;                         // (streams first: members are destroyed in reverse order)
    Event ev0, ev1;
    // The fantasy-particle sweeps (PCD) read only the parameters and the particles, the mean-field only the
    // parameters, X and mu: within one update they are independent, so the particle sweeps run on a second stream
    // (fork at the start of the update, join before the gradients) and fill the launch / fill / tail gaps of the
    // small mean-field kernels.  `cur` is the stream issue() / gibbs_sweep enqueue on.
    Stream stream2;
    hipStream_t cur = nullptr;
    Event ev_fork, ev_join;
    int pcd_geo = 0;                               // tile of the particle passes while they share the chip with the mean-field
                                                   // loop (ActArgs::geo_hint; BM355_DEBUG=dbm_pcd_geo=N, 0 = the tuner's choice):
                                                   // 3 (32 x 32, 32 KiB) where there IS a loop of small latency-bound passes to
                                                   // share CUs with - two or more layers of <= 2M weights, <= 1024 rows: 1.388 ->
                                                   // 1.353 ms per update at 784-512-1024 x 512 - and the tuner's pick elsewhere
                                                   // (3072 x 5000, one layer: 1.21 -> 1.29 .. 1.51 ms with the small tile;
                                                   // profiles/r6_dbm_ab.txt)
    int pcd_geo_now = 0;                           // ... and only while the loop is not SHORT: the small tile makes the particle
                                                   // chain itself slower (228 against 190 us for PCD-5), and that chain is the
                                                   // critical path under a loop of 3 sweeps (0.384 against 0.364 ms per update
                                                   // with the hint; from ~6 sweeps on the hint wins: 0.409 against 0.437 ms at 7).
                                                   // Decided per update from the previous trip count: MORE than one loop sweep per
                                                   // particle sweep (BM355_DEBUG=dbm_pcd_ratio=N; the crossover measured at
                                                   // 784-512-1024 x 512, PCD-5 lies between 5 and 6 sweeps).
    int updates_seen = 0;                          // the first updates run on one stream (launch tuning measures alone)
    // mean-field loop control mirror: pinned host copies of `ctl`, one per enqueued group of sweeps, so that the next
    // group is enqueued BEFORE the previous group's result is read (the GPU never waits for the host)
    static constexpr int MF_RING = 4;
    Pinned<MfCtl> ctl_host;
    Event ctl_ev[MF_RING];
    int mf_pred = 0;                               // trip count of the previous mean-field call (size of the first group)
    // variables
    Mat W[MAXL], Wt[MAXL], dW[MAXL];       // W[i]: [n[i]][n[i+1]]
    DevBuf vb, dvb, sigma;
    DevBuf hb[MAXL], dhb[MAXL], q[MAXL], mm[MAXL], pen[MAXL];
    Mat mu[MAXL], mu_alt[MAXL], mu_new[MAXL];      // [N][n[i+1]]: result, ping-pong partner, approx-inference init
    Mat v, v_new, H[MAXL], H_new[MAXL];            // particles [M][*]
    Mat recon;                                     // [N][V]
    DevBuf grad;                                   // data-parallel payload: [pos_i | neg_i per layer | sums]
    float *sums_p = nullptr;                       // column sums inside `grad`: [V | V | (n_i | n_i) per layer]
    size_t raw_off[MAXL][2];                       // offsets of the raw pos / neg outer products of layer i
    float (*mf_reduce)(float, void *) = nullptr;   // max over ranks of the mean-field residual through a HOST callback
    void *mf_ctx = nullptr;                        // (bm_dbm_set_mf_allreduce: collectives the library does not own)
    bm_comm *comm = nullptr;                       // bm_dbm_set_comm: the residual is all-reduced (max) ON DEVICE, on the
                                                   // engine stream, by the library's own RCCL communicator
    bm_xchg *xchg = nullptr;                       // bm_dbm_set_xchg: the same through the direct peer-memory exchange
    DevBuf wnorm[MAXL];
    // centred update (bm_dbm_set_centering), by layer 0 = v, l = hidden layer l - 1: the offsets are variables
    // ("ov", "oh", "oh_1", ...; zero until set), the rest is workspace allocated when the mode is first switched on
    bool cen_on = false;
    float cen_nu[MAXL + 1] = {0.f, 0.f, 0.f, 0.f, 0.f};
    DevBuf cen_o[MAXL + 1], cen_g[MAXL + 1];       // [n_l] offsets, plain bias gradients of the running update
    DevBuf cen_a;                                  // [L + 1][N + M] row scalars: positive rows, then negative rows
    DevBuf mn_fac[MAXL];                           // max-norm column factors [2][n_{i+1}]: min(norm, c) | max(norm, 1e-8)
    Mat logits[MAXL];                              // Multinomial layers: row store of the logits / means [rows][n_i], on demand
    int logit_rows[MAXL] = {0, 0, 0, 0};
    bool failed = false;                           // a launch helper could not allocate (sticky; reported by the entry points)
    bool multinomial(int layer) const { return layer >= 0 && cfg.h_unit[layer] == BM_UNIT_MULTINOMIAL; }
    unsigned *flag = nullptr;                      // mean-field residual cell (= &ctl->maxdiff)
    DevArray<MfCtl> ctl;                           // device-side loop control
    DevBuf mfblk;                                  // [2][MAXL * BM_MF_SLOTS] per-workgroup residual slots of the mean-field
                                                   // sweeps, double-buffered by sweep parity (ActArgs::chk_ctl)
    Mat xw0;                                       // [N][n1] hoisted X.W0 of the current minibatch
    DevArray<double> scal;
    // AIS / ELBO workspaces (allocated on demand).  AIS state by depth (depth 0 = v, depth i + 1 = hidden layer i): the
    // odd-depth layers {h1, h3} are the chain x, the even-depth layers {v, h2, h4} are summed out analytically
    int ais_rows = 0;
    Mat ae[3];                                     // even-depth states (v, h2, h4)
    Mat ao[2][2];                                  // odd-depth states (h1, h3), ping-pong pairs
    DevBuf apart_e[3];                             // per-16-column slot partial sums (ActArgs::rowacc): softplus terms of the
                                                   // even-depth layers (AIS) / the layers' sum((mu_{l-1} W_l) * mu_l) (ELBO)
    DevBuf apart_o[2][2];                          // x.hb of the odd-depth layers, current / next (ActArgs::rowdot_out)
    DevBuf rowtmp;
    DevArray<double> alogw;                        // [ais_rows] log-weights, accumulated in double in a fixed order
    DevBuf ais_send, ais_recv;                     // bm_dbm_ais_sharded: this rank's values / the all-gathered values
    Mat sv_v[2], sv_H[2][MAXL];                    // bm_dbm_sample_v: ping-pong states of its mean sweeps [M][*]
    // bm_dbm_pt_*: the tempered ensemble (bm_pt.h; layers v, h1 and, at L == 2, h2), allocated on demand; nothing else in the
    // handle reads or writes it (L <= 2)
    PtEnsemble pt;
    // fast-binary mode (bm_bf3.h, bm_dbm_set_fast_binary): bf16 planes of W_l (x = below unit, k = above unit) and of
    // W_l^T, bf16 shadows of the AIS state matrices; `fast_now` is set while a sweep with all-binary states runs
    int ais_literal = 0;                           // bm_dbm_set_ais_literal: float32 accumulation in the reference's order
    int sigmoid_literal = 0;                       // bm_dbm_set_sigmoid_literal: every Bernoulli activation as float32 1 / (1 + exp(-x))
    int fast = 0;
    bool fast_now = false;
    bool fast_ais = false;                         // the running fast sweep is AIS (fp32 copies of v / h2 are not needed)
    Mat16 W3[MAXL], W3t[MAXL];
    Mat16 ax16, ax2_16, av16, ah2_16;
    // PCD particles: one shadow per physical buffer (the Mat structs swap, the buffers keep their shadows)
    Mat16 pv16[2], pH16[MAXL][2];
    // the one table of shadows: state buffer -> its bf16 image, filled where the images are allocated (the fast AIS set-up,
    // fast_pcd_begin).  An AIS shadow is always valid; a particle shadow is valid once a launch of the running call has
    // written it (the particles a call starts from may be non-binary initial values: they are read in fp32)
    struct Shadow { const float *state = nullptr; const Mat16 *m = nullptr; bool valid = false; };
    static constexpr int AIS_SHADOWS = 4, SHADOWS = AIS_SHADOWS + 2 * (1 + MAXL);
    Shadow shadow[SHADOWS];                        // [0, AIS_SHADOWS): AIS states; then per particle buffer set b: v, H_0 ..
    Shadow &particle_shadow(int b, int layer /* -1 = v */) { return shadow[AIS_SHADOWS + b * (1 + MAXL) + 1 + layer]; }
    uint64_t seed = 0;
    uint32_t call = 0;
    int64_t row0 = 0, prow0 = 0;
};

static PhiloxKey dkey(const bm_dbm *h, uint32_t site, int t, uint64_t seed, uint32_t call) {
    PhiloxKey k;
    k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32);
    k.site = site + 16u * (uint32_t)t;
    k.call = call;
    return k;
}

// the bf16 shadow of a state matrix of the running fast-binary sweep (null: none)
static bm_dbm::Shadow *fast_shadow(bm_dbm *h, const float *p) {
    if (p) for (bm_dbm::Shadow &s : h->shadow) if (s.state == p) return &s;
    return nullptr;
}
// the shadow of an INPUT state matrix: only one whose contents are known to mirror the fp32 matrix
static const Mat16 *fast_shadow_in(bm_dbm *h, const float *p) {
    const bm_dbm::Shadow *s = fast_shadow(h, p);
    return (s && s->valid) ? s->m : nullptr;
}

// (re)build the bf16 weight planes from the current parameters (fast-binary mode; cheap next to any sweep), on stream
// `st`.  skip_t0: the planes of W_0^T are not needed (the visible layer of the sweep is not a bitmap)
static int fast_build_planes(bm_dbm *h, hipStream_t st = nullptr, bool skip_t0 = false) {
    if (!st) st = h->stream;
    for (int l = 0; l < h->L; ++l) {
        const int a = h->n[l], b = h->n[l + 1];
        if (h->W3t[l].rows != b || h->W3t[l].cols != a) { BM_TRY(h->W3[l].alloc(3, a, b)); BM_TRY(h->W3t[l].alloc(3, b, a)); }
        hipLaunchKernelGGL(split3_kernel, dim3(1024), dim3(256), 0, st, (const float *)h->W[l].p, h->W[l].ld, a, b,
                           h->W3[l].p, h->W3[l].plane_stride(), h->W3[l].ld, 0);
        if (!(skip_t0 && l == 0))
            hipLaunchKernelGGL(split3_kernel, dim3(1024), dim3(256), 0, st, (const float *)h->W[l].p, h->W[l].ld, a, b,
                               h->W3t[l].p, h->W3t[l].plane_stride(), h->W3t[l].ld, 1);
    }
    BM_HIP(hipGetLastError());
    return 0;
}

// Single-segment passes read their weights x-major ([i][k], k contiguous: one ds_read_b128 per 16 k and lane where the
// k-major image needs four ds_read_b32; 12.95 -> 12.5 us per pass at 784 x 1024, bm_rbm.hip) - the engine keeps W_l and
// W_l^T anyway, so the x-major image of either direction is the OTHER matrix.  BM355_DEBUG=dbm_xm=0: k-major as before.
static bool dbm_xm() {
    static const bool on = !(bm::dbg("dbm_xm") && atoi(bm::dbg("dbm_xm")) == 0);
    return on;
}

// ---- a layer pass as a value (bm_pass.h: layer_pass() describes it, issue() launches it): out = act(mult * (below.W_lo [+ above.W_hi^T]) + bmult * bias)
//   below [J][n_lo] (pitch ldb) with W_lo = W[lo] ([n_lo][I]);  above [J][n_hi] with Wt[lo+1] ([n_hi][I])
static LayerOut mean_out(const bm_dbm *h, float *p, int ld) { return LayerOut{0, p, nullptr, ld, dkey(h, 0, 0, h->seed, h->call), 0}; }
// the clamp of a call's visible-layer passes (null mask: none)
struct Clamp { const float *val, *mask; int ld; };

// Operands of a pass with ONE K segment, through W_l - up: below [J][n_l] -> [J][n_{l+1}], down: above [J][n_{l+1}] -> [J][n_l] -
// x-major where the kernel can read it (dbm_xm above)
static void single_segment(const bm_dbm *h, ActArgs &a, int l, bool up, LayerIn in) {
    a.K1 = up ? h->n[l] : h->n[l + 1];
    a.p_xm = (dbm_xm() && (a.K1 & 3) == 0) ? 1 : 0;
    const Mat &w = (up != (a.p_xm != 0)) ? h->W[l] : h->Wt[l];           // k-major: W_l (up), W_l^T (down); x-major: the other
    a.P1 = make_operand(w.p, w.ld, a.I); a.Q1 = make_operand(in.p, in.ld, a.J);
}

// Describes one layer update; queues nothing, allocates nothing.  `below_sum`: the below segment of the pre-activation is
// already summed there (the hoisted X.W0 of the mean-field sweeps: continuing the chain from it is bit-identical to
// recomputing it), only the top-down segment is streamed.
static LayerPass layer_pass(const bm_dbm *h, int layer, int J, LayerIn below, LayerIn above, float mult, float bmult,
                            const LayerOut &out, const Mat *below_sum = nullptr) {
    LayerPass p;
    ActArgs &a = p.a;
    memset(&a, 0, sizeof(ActArgs));
    p.layer = layer; p.below = below_sum ? nullptr : below.p; p.above = above.p;
    a.J = J; a.I = h->n[layer + 1];
    if (layer < 0) {
        single_segment(h, a, 0, false, above);                            // W[0]^T [k = h0][i = v]
        a.bias = h->vb.p; a.sigma = h->sigma.p; a.kind = h->cfg.v_unit;
    } else {
        if (below_sum) {
            a.acc_init = below_sum->p; a.ld_init = below_sum->ld;
            single_segment(h, a, layer + 1, false, above);                // W[layer+1]^T [k = above][i]
        } else if (!above.p) {
            single_segment(h, a, layer, true, below);                     // W[layer][k = below][i]
        } else {
            a.P1 = make_operand(h->W[layer].p, h->W[layer].ld, a.I); a.Q1 = make_operand(below.p, below.ld, J); a.K1 = h->n[layer];
            a.P2 = make_operand(h->Wt[layer + 1].p, h->Wt[layer + 1].ld, a.I); a.Q2 = make_operand(above.p, above.ld, J); a.K2 = h->n[layer + 2];
        }
        a.bias = h->hb[layer].p; a.kind = BM_UNIT_BERNOULLI;
    }
    a.mult = mult; a.bmult = bmult; a.lit = h->sigmoid_literal;
    a.sample = out.sample; a.means = out.means; a.states = out.states; a.ldo = out.ld; a.key = out.key; a.row0 = out.row0;
    return p;
}

// fast-binary: the same contraction from the bf16 weight planes and the bf16 shadows of the {0,1} inputs (a state matrix
// without a valid shadow - real-valued visibles, the first PCD sweep - keeps the fp32 path), and the shadow of the output
static void fast_substitute(bm_dbm *h, LayerPass &p) {
    ActArgs &a = p.a;
    const Mat16 *sb = fast_shadow_in(h, p.below), *sa = fast_shadow_in(h, p.above);
    auto opnd = [](const Mat16 &m, int nx) { Bf3Operand o; o.p = m.p; o.plane_stride = m.plane_stride(); o.ld = m.ld; o.nx = nx; return o; };
    bool ok = false;
    Bf3Range r;
    memset(&r, 0, sizeof(r));
    if (p.layer >= 0 && sb && (!p.above || sa)) {
        r.P1 = opnd(h->W3t[p.layer], a.I); r.Q1 = opnd(*sb, a.J); r.K1 = sb->ld;          // W_layer^T: [i][k = below]
        if (p.above) { r.P2 = opnd(h->W3[p.layer + 1], a.I); r.Q2 = opnd(*sa, a.J); r.K2 = sa->ld; }   // W_{layer+1}: [i][k = above]
        ok = true;
    } else if (p.layer < 0 && sa) {
        r.P1 = opnd(h->W3[0], a.I); r.Q1 = opnd(*sa, a.J); r.K1 = sa->ld;                 // W_0: [i = v][k = h0]
        ok = true;
    }
    if (ok) a.b3 = r;
    // the shadow of what this launch writes, when that is a sampled bitmap (written by either path's epilogue)
    bm_dbm::Shadow *so = (a.states && a.sample && a.kind == BM_UNIT_BERNOULLI) ? fast_shadow(h, a.states) : nullptr;
    if (so) {
        a.states16 = so->m->p; a.ld16 = so->m->ld;
        so->valid = true;
        // AIS: the fp32 copy of a state matrix that only fast-binary launches read is not written at all (visible /
        // top-layer states: 145 MB per beta); x keeps it for the x.hb0 partial sums of the epilogue
        if (ok && h->fast_ais && !a.rowdot_out) a.states = nullptr;
    }
}

// MultinomialLayer inside the stack (layers.py:54-70): the GEMM writes the logits mult*z + bmult*b, then one
// wave per row does the softmax (activation = n_samples * softmax) and, when sampling, the n_samples
// categorical draws (counts); same two kernels as the MultinomialRBM hidden layer (bm_rbm.hip issue)
static void issue_multinomial(bm_dbm *h, ActArgs a, int layer) {
    float *lg = a.means; int ldl = a.ldo;
    if (!lg) {                                 // sampled sweep: the means are not kept, they pass through a row store
        if (h->logit_rows[layer] < a.J) {
            // (bm_dbm_create preallocates max(N, M) rows: this only grows the store for an unusual row count)
            if (h->logits[layer].alloc(a.J, a.I)) { h->failed = true; h->logit_rows[layer] = 0; return; }
            h->logit_rows[layer] = a.J;
        }
        lg = h->logits[layer].p; ldl = h->logits[layer].ld;
    }
    SmArgs m;
    memset(&m, 0, sizeof(m));
    m.L = lg; m.ld = ldl; m.ld_states = a.ldo; m.I = a.I; m.J = a.J; m.M = h->cfg.n_samples[layer]; m.sample = a.sample;
    m.states = (a.states && (a.sample || a.states != lg)) ? a.states : nullptr;
    m.key = a.key; m.row0 = a.row0; m.prev = a.prev; m.ld_prev = a.ldo; m.maxdiff = a.maxdiff; m.skip = a.skip;
    a.kind = 3; a.sample = 0; a.means = lg; a.ldo = ldl; a.states = nullptr; a.negmeans = nullptr;
    a.prev = nullptr; a.maxdiff = nullptr; a.maxdiff_blk = nullptr;
    launch_act(a, h->cur);
    hipLaunchKernelGGL(softmax_multinomial_kernel, dim3(a.J), dim3(64), 2 * (size_t)a.I * sizeof(float), h->cur, m);
}

// everything that is about launching a pass, on h->cur
static void issue(bm_dbm *h, LayerPass p) {
    const bool tempered = p.a.row_mult != nullptr;      // a plain fp32 launch, always (the RT launcher has no other flavour)
    if (h->cur == h->stream2 && h->pcd_geo_now && !tempered) p.a.geo_hint = h->pcd_geo_now;   // a pass that runs beside the mean-field loop
    const bool act = p.a.kind != 2, multinomial = h->multinomial(p.layer);
    if (h->fast_now && act && !multinomial && !p.a.clamp_mask && !tempered) fast_substitute(h, p);      // (a clamped pass is fp32, always)
    if (act && multinomial) issue_multinomial(h, p.a, p.layer);
    else launch_act(p.a, h->cur);
}

// `_make_gibbs_step` (dbm.py:385-427): bottom-up Gauss-Seidel sweep.
//   vin / Hin  : current states (Hin[i] may alias mu)      vout / Hout : new states
//   out_means  : Hout receives means (sample == 0) or samples (per-layer flags)
// A mean-field sweep (null: a plain one) also leaves its residual against Hin in the atomic cell `maxdiff` and the slots
// `slots_mine` (null: the cell alone), starts the first layer from the hoisted `xw0` (null: recomputes it), returns at once when
// `*skip`, and its first kernel evaluates the loop control of the sweep before it from `slots_prev` (null: no check)
struct MfSweep { unsigned *maxdiff; const Mat *xw0; const int *skip; float *slots_mine; const float *slots_prev; };
static void gibbs_sweep(bm_dbm *h, int J, LayerIn vin, const Mat *Hin, Mat *vout, Mat *Hout,
                        bool update_v, bool sample, int t, int64_t row0, const MfSweep *mf = nullptr, const Clamp *cl = nullptr) {
    const int L = h->L;
    for (int i = 0; i < L; ++i) {
        const LayerIn below = (i == 0) ? vin : in_of(Hout[i - 1]);                        // NEW below   :400-402
        const LayerIn above = (i + 1 < L) ? in_of(Hin[i + 1]) : NO_IN;                   // OLD above
        const int smp = sample && h->cfg.sample_h_states[i];
        const LayerOut out = value_out(smp, Hout[i].p, Hout[i].ld, dkey(h, SITE_DBM_H + i, t, h->seed, h->call), row0);
        // mean-field: X.W0 is loop invariant - start the chain from the hoisted partial sum
        const Mat *xw0 = (i == 0 && mf && mf->xw0 && above.p && !h->multinomial(0)) ? mf->xw0 : nullptr;
        LayerPass p = layer_pass(h, i, J, below, above, 1.f, 1.f, out, xw0);
        if (mf) {
            p.residual(Hin[i].p, mf->maxdiff, mf->slots_mine ? mf->slots_mine + (size_t)i * BM_MF_SLOTS : nullptr).skip_if(mf->skip);
            if (i == 0 && mf->slots_prev) p.check(h->ctl.p, mf->slots_prev, L * BM_MF_SLOTS, h->cfg.mf_tol);
        }
        issue(h, p);
    }
    if (update_v) {                                                                       // :419-425
        const int smp = sample && h->cfg.sample_v_states;
        LayerPass p = layer_pass(h, -1, J, NO_IN, in_of(Hout[0]), 1.f, 1.f,
                                 value_out(smp, vout->p, vout->ld, dkey(h, SITE_DBM_V, t, h->seed, h->call), row0));
        if (cl) p.clamp(cl->val, cl->mask, cl->ld);
        issue(h, p);
    }
}

static int read_flag(bm_dbm *h, float *out) {
    unsigned bits = 0;
    BM_HIP(hipMemcpyAsync(&bits, h->flag, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    memcpy(out, &bits, sizeof(float));
    // data-parallel: the loop condition (dbm.py:449-452) is over ALL rows, i.e. the max over ranks
    if (h->mf_reduce) *out = h->mf_reduce(*out, h->mf_ctx);
    return 0;
}

// `_make_mf` (dbm.py:429-478).  Leaves the result in h->mu; returns executed sweeps.
// The loop trip count is data dependent (residual > tol).  The sweeps are enqueued in groups without host
// round trips — a device-side control word (MfCtl) latches `done` and every later launch returns at once.
// The first group is as long as the previous call's trip count + 1, the host reads the control word of a
// group from a pinned mirror while the next group is already queued.  With the library's communicator
// installed (bm_dbm_set_comm) the residual is all-reduced (max) on the device, in stream order, per sweep;
// only the host-callback hook (bm_dbm_set_mf_allreduce) costs a host round trip per sweep.
static bool mf_self_ctl(const bm_dbm *h) {
    // Self-controlled sweeps (single GPU, Bernoulli layers, grids that fit the residual slots), see MfRing
    bool ok = !h->comm && !h->xchg && !h->mf_reduce;
    for (int i = 0; i < h->L; ++i)
        ok = ok && !h->multinomial(i) && ((h->n[i + 1] + 31) / 32) * ((h->N + 31) / 32) <= BM_MF_SLOTS;
    return ok;
}
// the part of `_make_mf` in front of the loop: approximate-inference init, the hoisted X.W0, the step-0 condition
static int mf_prologue(bm_dbm *h, const float *X_dev, bool &hoist) {
    const int L = h->L, N = h->N;
    static const bool fold = !(bm::dbg("mf_fold") && atoi(bm::dbg("mf_fold")) == 0);   // =0: the separate residual kernels (A/B)
    // cond at step 0 compares the persistent mu with the init values (:449-452): every init pass leaves max |mu_new - mu| of
    // its tile in its residual slot (or, where there are no slots, in the atomic cell) - the mean-field passes' own epilogue
    // path - instead of two more kernels reading both matrices again
    BM_HIP(hipMemsetAsync(h->flag, 0, sizeof(unsigned), h->stream));
    // the residual slots of self-controlled sweeps start from zero: in front of the init passes that write them, else behind them
    const bool self_ctl = mf_self_ctl(h);
    const size_t slot_bytes = 2 * (size_t)MAXL * BM_MF_SLOTS * sizeof(float);
    if (self_ctl && fold) BM_HIP(hipMemsetAsync(h->mfblk.p, 0, slot_bytes, h->stream));
    const bool slots = fold && !h->mf_reduce;                  // (the host-callback path reads the atomic cell alone)
    // hoisted loop invariant of the sweeps: z0 = X.W0 (raw chain, no activation)
    hoist = L >= 2 && !h->multinomial(0);
    if (hoist) issue(h, layer_pass(h, 0, N, LayerIn{X_dev, h->V}, NO_IN, 1.f, 1.f, mean_out(h, h->xw0.p, h->xw0.ld)).raw());
    // approximate-inference init into the mu_new VARIABLES (:434-446): doubled bottom-up pass
    for (int i = 0; i < L; ++i) {
        const LayerIn below = (i == 0) ? LayerIn{X_dev, h->V} : in_of(h->mu_new[i - 1]);
        const float mult = (i == 0 || i < L - 1) ? 2.f : 1.f;
        float *blk = slots ? h->mfblk.p + (size_t)i * BM_MF_SLOTS : nullptr;
        if (i == 0 && hoist && fold) {
            // the first layer's init is the activation of the chain just stored: sigmoid(2 z0 + hb) elementwise, same bits
            hipLaunchKernelGGL(mf_init0_kernel, dim3(N < 256 ? N : 256), dim3(256), 0, h->stream, (const float *)h->xw0.p, h->xw0.ld,
                               (const float *)h->hb[0].p, (const float *)h->mu[0].p, h->mu[0].ld, h->mu_new[0].p, h->mu_new[0].ld,
                               N, h->n[1], mult, 1.f, h->sigmoid_literal ? 1 : 0, h->flag, blk);
            continue;
        }
        LayerPass p = layer_pass(h, i, N, below, NO_IN, mult, 1.f, mean_out(h, h->mu_new[i].p, h->mu_new[i].ld));
        if (fold) p.residual(h->mu[i].p, h->flag, blk);
        issue(h, p);
    }
    if (!fold) {
        for (int i = 0; i < L; ++i)
            hipLaunchKernelGGL(maxabsdiff_kernel, dim3(N < 256 ? N : 256), dim3(256), 0, h->stream, (const float *)h->mu[i].p, h->mu[i].ld,
                               (const float *)h->mu_new[i].p, h->mu_new[i].ld, N, h->n[i + 1], h->flag);
        if (self_ctl) BM_HIP(hipMemsetAsync(h->mfblk.p, 0, slot_bytes, h->stream));
    }
    return 0;
}

// `mid` (optional) is called ONCE, after the part in front of the loop is in the queue and before the first sweep: work for a
// second stream (the particle sweeps of a training update) is enqueued there - behind the few launches the critical chain starts
// with, in front of the (up to 2 x max_mf_updates) launches of the loop, so that neither a slow host nor a long loop decides
// when the second stream starts.
struct MfMid { int (*fn)(bm_dbm *, void *); void *ctx; bool called; };
static int mf_mid(bm_dbm *h, MfMid *m) {
    if (!m || m->called) return 0;
    m->called = true;
    return m->fn(h, m->ctx);
}

// loop driver 1, the host-callback hook: a host round trip per sweep.  Returns the executed sweeps in *steps
static int mf_loop_host(bm_dbm *h, const float *X_dev, bool hoist, int *steps) {
    Mat *cur = h->mu, *alt = h->mu_alt;
    const MfSweep mf{h->flag, hoist ? &h->xw0 : nullptr, nullptr, nullptr, nullptr};
    float diff = 0.f;
    BM_TRY(read_flag(h, &diff));
    // body (:454-457): mu_new = sweep(X, mu) (values, not the mu_new variables), then swap
    for (*steps = 0; *steps < h->cfg.max_mf_updates && diff > h->cfg.mf_tol; ++*steps) {
        BM_HIP(hipMemsetAsync(h->flag, 0, sizeof(unsigned), h->stream));
        gibbs_sweep(h, h->N, LayerIn{X_dev, h->V}, cur, nullptr, alt, false, false, 0, 0, &mf);
        BM_TRY(read_flag(h, &diff));
        std::swap(cur, alt);
    }
    return 0;
}

// loop control of one sweep: local (one kernel) or global (residual all-reduced over the ranks in stream order: every rank
// enqueues the same sequence and latches the same `done`, so no host round trip is needed and the ranks stay in lockstep)
typedef int (*MfCtlStep)(bm_dbm *h, int init);
static int mf_ctl_local(bm_dbm *h, int init) {
    hipLaunchKernelGGL(mf_ctl_kernel, dim3(1), dim3(256), 0, h->stream, h->ctl.p, h->cfg.mf_tol, init, h->mfblk.p, h->L * BM_MF_SLOTS);
    return 0;
}
static int mf_ctl_xchg(bm_dbm *h, int init) {     // ONE launch (three per sweep were 0.4 ms of a 1.8 ms data-parallel update at 45 sweeps)
    return xchg_mf_ctl_step(h->xchg, h->ctl.p, h->mfblk.p, h->L * BM_MF_SLOTS, h->cfg.mf_tol, init, h->stream);
}
static int mf_ctl_rccl(bm_dbm *h, int init) {
    hipLaunchKernelGGL(mf_resid_kernel, dim3(1), dim3(256), 0, h->stream, h->ctl.p, h->mfblk.p, h->L * BM_MF_SLOTS);
    BM_TRY(bm_comm_allreduce_max(h->comm, &h->ctl.p->resid, 1, (void *)h->stream));
    hipLaunchKernelGGL(mf_latch_kernel, dim3(1), dim3(64), 0, h->stream, h->ctl.p, h->cfg.mf_tol, init);
    return 0;
}

// The groups of sweeps in flight: the loop-control record is copied to a pinned mirror after each group and READ ONE GROUP
// LATE, so the GPU never idles waiting for the host (sweeps enqueued past the end of the loop return at once).
// Self-controlled sweeps (single GPU, Bernoulli layers, grids that fit the residual slots): the loop-control update of
// sweep s-1 is evaluated by the first kernel of sweep s (ActArgs::chk_ctl) from the slot set of the other parity; only the
// LAST sweep of a group needs the one-workgroup control kernel.  Otherwise (communicator installed, Multinomial layers,
// > BM_MF_SLOTS workgroups possible) one control step per sweep.
struct MfRing {
    bm_dbm *h; const float *X_dev; bool hoist, self_ctl; MfCtlStep ctl_step;
    int enq = 0, g_enq = 0, g_read = 0;       // sweeps enqueued; groups enqueued / read
    MfCtl host{0, 0, 0, 0.f};                 // the newest record read
    static constexpr int R = bm_dbm::MF_RING;

    int enqueue_group(int g) {
        const size_t set_sz = (size_t)MAXL * BM_MF_SLOTS;
        for (int s = 0; s < g; ++s) {
            // sweep number enq+s runs only if all before it ran, so its ping-pong parity is static
            const int sw = enq + s;
            Mat *src = (sw & 1) ? h->mu_alt : h->mu, *dst = (sw & 1) ? h->mu : h->mu_alt;
            MfSweep mf{h->flag, hoist ? &h->xw0 : nullptr, &h->ctl.p->done, h->mfblk.p, nullptr};
            if (self_ctl) {
                mf.slots_mine = h->mfblk.p + (size_t)(sw & 1) * set_sz;
                if (s > 0) mf.slots_prev = h->mfblk.p + (size_t)((sw & 1) ^ 1) * set_sz;
            }
            gibbs_sweep(h, h->N, LayerIn{X_dev, h->V}, src, nullptr, dst, false, false, 0, 0, &mf);
            if (!self_ctl) BM_TRY(ctl_step(h, 0));
            else if (s == g - 1)      // Check(last sweep of the group); it also clears the slots it read
                hipLaunchKernelGGL(mf_ctl_kernel, dim3(1), dim3(256), 0, h->stream, h->ctl.p, h->cfg.mf_tol, 0,
                                   mf.slots_mine, h->L * BM_MF_SLOTS);
        }
        enq += g;
        BM_HIP(hipMemcpyAsync(&h->ctl_host[g_enq % R], h->ctl.p, sizeof(MfCtl), hipMemcpyDeviceToHost, h->stream));
        BM_HIP(hipEventRecord(h->ctl_ev[g_enq % R], h->stream));
        ++g_enq;
        return 0;
    }
    int read_oldest() {
        BM_HIP(hipEventSynchronize(h->ctl_ev[g_read % R]));
        host = h->ctl_host[g_read++ % R];
        return 0;
    }
    int drain() {                      // groups enqueued past the end of the loop do nothing; free their ring slots
        if (g_read < g_enq) BM_HIP(hipEventSynchronize(h->ctl_ev[(g_enq - 1) % R]));
        g_read = g_enq;
        return 0;
    }
};

// loop driver 2, device-controlled: the first group is as long as the previous call's trip count - for a training run the
// count barely moves from one minibatch to the next - so a typical call costs one or two reads
static int mf_loop_device(bm_dbm *h, const float *X_dev, bool hoist, int *steps) {
    constexpr int MF_GROUP = 8;
    MfRing ring{h, X_dev, hoist, mf_self_ctl(h), h->xchg ? mf_ctl_xchg : h->comm ? mf_ctl_rccl : mf_ctl_local};
    BM_TRY(ring.ctl_step(h, 1));
    const int max_it = h->cfg.max_mf_updates;
    if (max_it <= 0) {                 // no sweeps: fetch the step-0 record
        BM_HIP(hipMemcpyAsync(&h->ctl_host[0], h->ctl.p, sizeof(MfCtl), hipMemcpyDeviceToHost, h->stream));
        BM_HIP(hipStreamSynchronize(h->stream));
        ring.host = h->ctl_host[0];
    } else {
        // first group: the previous trip count + 1 (a sweep too many costs two kernels that return at once,
        // a sweep too few costs a host round trip), read before anything else is enqueued
        BM_TRY(ring.enqueue_group(std::min(max_it, h->mf_pred > 0 ? h->mf_pred + 1 : MF_GROUP)));
        BM_TRY(ring.read_oldest());
        // not converged yet: short groups, one of them always queued behind the one being read
        while (!ring.host.done && (ring.enq < max_it || ring.g_read < ring.g_enq)) {
            while (ring.enq < max_it && ring.g_enq - ring.g_read < 2)
                BM_TRY(ring.enqueue_group(std::min(max_it - ring.enq, MF_GROUP / 2)));
            BM_TRY(ring.read_oldest());
        }
        BM_TRY(ring.drain());
    }
    h->mf_pred = ring.host.steps > 0 ? ring.host.steps : 0;
    *steps = ring.host.steps;
    return 0;
}

static int mean_field(bm_dbm *h, const float *X_dev, int *out_n, MfMid *mid = nullptr) {
    bool hoist = false;
    int steps = 0;                     // executed sweeps
    BM_TRY(mf_prologue(h, X_dev, hoist));                                                  // in front of the loop
    BM_TRY(mf_mid(h, mid));                                                                // work for the second stream
    BM_TRY((h->mf_reduce ? mf_loop_host : mf_loop_device)(h, X_dev, hoist, &steps));       // the loop, by its driver
    if (steps & 1)                     // `self._mu[i].assign(mu[i])` (:477): keep the handle's mu as the result
        for (int i = 0; i < h->L; ++i) std::swap(h->mu[i], h->mu_alt[i]);
    if (out_n) *out_n = steps;
    return 0;
}

// `_make_particles_update` (dbm.py:480-509)
// fast-binary PCD: the hidden layers are sampled Bernoulli layers (bitmaps from the second sweep on), the visible one
// may be real valued (then only the top-down half of each sweep runs on the bf16 cores)
static bool fast_pcd_ok(const bm_dbm *h, bool sample) {
    // (level 1: only where the particle sweeps gain - from 8M weights in the bottom layer upwards; at 784-512-1024 they lose,
    //  profiles/r5_dbm_summary.md.  Level 2: wherever legal)
    if (!h->fast || !sample) return false;
    if (h->fast < 2 && (long long)h->V * h->n[1] < (8ll << 20)) return false;
    for (int i = 0; i < h->L; ++i) if (h->multinomial(i) || !h->cfg.sample_h_states[i]) return false;
    return true;
}
// fast_now lasts as long as the sweeps of one call (AIS run, particle update)
struct FastScope { bm_dbm *h; ~FastScope() { h->fast_now = false; } void begin(bool ais) { h->fast_now = true; h->fast_ais = ais; } };
static int fast_pcd_begin(bm_dbm *h) {
    const bool vbits = h->cfg.v_unit == BM_UNIT_BERNOULLI && h->cfg.sample_v_states;
    if (!h->particle_shadow(0, 0).state) {        // one shadow per physical particle buffer (entered once all exist)
        for (int b = 0; b < 2; ++b) {
            if (vbits) BM_TRY(h->pv16[b].alloc(1, h->M, h->V));
            for (int i = 0; i < h->L; ++i) BM_TRY(h->pH16[i][b].alloc(1, h->M, h->n[i + 1]));
        }
        for (int b = 0; b < 2; ++b) {
            if (vbits) h->particle_shadow(b, -1) = {(b ? h->v_new : h->v).p, &h->pv16[b], false};
            for (int i = 0; i < h->L; ++i) h->particle_shadow(b, i) = {(b ? h->H_new[i] : h->H[i]).p, &h->pH16[i][b], false};
        }
    }
    for (int s = bm_dbm::AIS_SHADOWS; s < bm_dbm::SHADOWS; ++s) h->shadow[s].valid = false;
    return fast_build_planes(h, h->cur, !vbits);  // the parameters changed since the last update
}

static void particles_update(bm_dbm *h, int k, bool sample, const Clamp *cl = nullptr) {
    FastScope scope{h};
    if (!cl && fast_pcd_ok(h, sample)) {           // (clamp values may be grey levels: a clamped call keeps the fp32 path)
        if (fast_pcd_begin(h) == 0) scope.begin(false);
        else h->failed = true;
    }
    for (int t = 0; t < k; ++t) {
        // (fast-binary: sweep 0 reads the particles it starts from in fp32 and leaves shadows of what it samples; from
        // then on every sampled Bernoulli input is a bitmap with a valid shadow)
        gibbs_sweep(h, h->M, in_of(h->v), h->H, &h->v_new, h->H_new, true, sample, t, h->prow0, nullptr, cl);
        std::swap(h->v, h->v_new);                                        // swap particles (:493)
        for (int i = 0; i < h->L; ++i) std::swap(h->H[i], h->H_new[i]);
    }
}


// mean-field on the data rows and PCD sweeps on the particles of one update, concurrently (see bm_dbm::stream2).
// The particle sweeps go to the second stream, between a fork event (recorded before anything of this update is enqueued: the
// previous parameter update) and a join event the main stream waits for before anything reads the particles; the host enqueues
// them from mean_field()'s `mid` hook - after the launches in front of the mean-field loop, before the loop's own.  Same kernels,
// same RNG streams: results do not change.
static bool pcd_overlap_ok(const bm_dbm *h) {
    static const bool off = bm::dbg("dbm_overlap") && atoi(bm::dbg("dbm_overlap")) == 0;
    if (off || h->updates_seen < 2) return false;          // the first updates tune their launches undisturbed
    for (int i = 0; i < h->L; ++i) if (h->multinomial(i)) return false;     // one logits row store per layer
    return true;
}
static int enqueue_particles_stream2(bm_dbm *h, void *ctx) {
    const int k = *(const int *)ctx;
    BM_HIP(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    static const int min_ratio = bm::dbg("dbm_pcd_ratio") ? atoi(bm::dbg("dbm_pcd_ratio")) : 1;
    h->pcd_geo_now = (h->pcd_geo && h->mf_pred > min_ratio * k) ? h->pcd_geo : 0;
    h->cur = h->stream2;
    particles_update(h, k, true);                                 // :521
    h->cur = h->stream;
    h->pcd_geo_now = 0;
    BM_HIP(hipEventRecord(h->ev_join, h->stream2));
    return 0;
}
static int mean_field_and_particles(bm_dbm *h, const float *X_dev, int k, int *out_n) {
    const bool ov = pcd_overlap_ok(h);
    // where the host enqueues the particle sweeps: behind the mean-field's prologue (default) or in front of it (=0); same time
    // per update on a fast host (profiles/r6_dbm_ab.txt)
    static const bool late = !(bm::dbg("dbm_pcd_late") && atoi(bm::dbg("dbm_pcd_late")) == 0);
    MfMid mid{enqueue_particles_stream2, &k, false};
    if (ov) {
        BM_HIP(hipEventRecord(h->ev_fork, h->stream));            // = the previous parameter update
        if (!late) BM_TRY(mf_mid(h, &mid));
    }
    int rc = mean_field(h, X_dev, out_n, ov ? &mid : nullptr);    // :517
    if (ov && !mid.called) {                                      // the mean-field failed before its hook ran
        if (mf_mid(h, &mid) && !rc) rc = 1;
    }
    // (the join is enqueued even when the mean-field failed: later calls on the main stream must not race the
    //  particle sweeps still running on the second one)
    if (ov) { if (hipStreamWaitEvent(h->stream, h->ev_join, 0) != hipSuccess && !rc) { set_error("hipStreamWaitEvent(join) failed"); return 1; } }
    else if (!rc) particles_update(h, k, true);
    h->updates_seen++;
    return rc;
}

static void xchg_dw_replaced(bm_xchg *x);
static int check_dw(const bm_dbm *h, const char *what) {
    BM_CHECK(!h->dw_sharded, "%s: after bm_dbm_exchange_apply_direct this rank holds only its column slices of the momentum "
                             "buffers dW; call bm_dbm_exchange_gather_dw (DirectExchange.gather_dw) on every rank first", what);
    return 0;
}

static size_t sums_off(const bm_dbm *h, int which /* 0: X, 1: v, 2+2i: mu_i, 3+2i: H_i */) {
    size_t o = 0;
    if (which == 0) return 0;
    o += h->V;
    if (which == 1) return o;
    o += h->V;
    for (int i = 0; i < h->L; ++i) {
        if (which == 2 + 2 * i) return o;
        o += h->n[i + 1];
        if (which == 3 + 2 * i) return o;
        o += h->n[i + 1];
    }
    return o;
}

// raw column sums of X, v, mu_i, H_i (dbm.py:553, :573-576, :581-586)
static void launch_dbm_colsums(bm_dbm *h, const float *X_dev) {
    const int L = h->L;
    ColSumArgs c;
    memset(&c, 0, sizeof(c));
    int nj = 0;
    c.job[nj++] = ColSumJob{X_dev, nullptr, h->V, 0, h->V, h->N, h->sums_p + sums_off(h, 0)};
    c.job[nj++] = ColSumJob{h->v.p, nullptr, h->v.ld, 0, h->V, h->M, h->sums_p + sums_off(h, 1)};
    for (int i = 0; i < L; ++i) {
        c.job[nj++] = ColSumJob{h->mu[i].p, nullptr, h->mu[i].ld, 0, h->n[i + 1], h->N, h->sums_p + sums_off(h, 2 + 2 * i)};
        c.job[nj++] = ColSumJob{h->H[i].p, nullptr, h->H[i].ld, 0, h->n[i + 1], h->M, h->sums_p + sums_off(h, 3 + 2 * i)};
    }
    c.njobs = nj;
    c.first_wave[0] = 0;
    for (int j = 0; j < nj; ++j) c.first_wave[j + 1] = c.first_wave[j] + (c.job[j].ncols + 63) / 64;
    hipLaunchKernelGGL(colsum_kernel, dim3(c.first_wave[nj]), dim3(NT), 0, h->stream, c);
}

// bias / running-mean / sparsity updates from the (possibly all-reduced) column sums
static void launch_dbm_biases(bm_dbm *h, float N, float M, float lr, float mom) {
    static_assert(DBM_BIAS_JOBS == 1 + MAXL, "one job per layer + the visible one");
    DbmBiasMulti m;
    memset(&m, 0, sizeof(m));
    int nmax = h->V;
    {
        DbmBiasArgs &b = m.job[0];
        b.s_pos = h->sums_p + sums_off(h, 0); b.s_neg = h->sums_p + sums_off(h, 1);
        b.b = h->vb.p; b.db = h->dvb.p; b.n = h->V; b.N = N; b.M = M; b.lr = lr; b.mom = mom;
    }
    for (int i = 0; i < h->L; ++i) {
        DbmBiasArgs &b = m.job[1 + i];
        b.s_pos = h->sums_p + sums_off(h, 2 + 2 * i); b.s_neg = h->sums_p + sums_off(h, 3 + 2 * i);
        b.b = h->hb[i].p; b.db = h->dhb[i].p; b.q = h->q[i].p; b.mm = h->mm[i].p; b.pen = h->pen[i].p;
        b.n = h->n[i + 1]; b.layer = i;
        b.N = N; b.M = M; b.lr = lr; b.mom = mom;
        b.damping = h->cfg.sparsity_damping; b.cost = h->cfg.sparsity_cost[i]; b.target = h->cfg.sparsity_target[i];
        if (b.n > nmax) nmax = b.n;
    }
    hipLaunchKernelGGL(dbm_bias_multi_kernel, dim3((nmax + 255) / 256, 1 + h->L), dim3(256), 0, h->stream, m);
}

// outer products of layer i: fused (update in the epilogue) or raw pos / neg into `grad`
static void launch_dbm_grad(bm_dbm *h, const float *X_dev, int i, int fused, float N, float M, float lr, float mom, hipStream_t st = nullptr) {
    GradArgs g;
    memset(&g, 0, sizeof(g));
    const float *below_pos = (i == 0) ? X_dev : h->mu[i - 1].p;
    const int ld_bp = (i == 0) ? h->V : h->mu[i - 1].ld;
    const Mat &below_neg = (i == 0) ? h->v : h->H[i - 1];
    g.Ppos = make_operand(h->mu[i].p, h->mu[i].ld, h->n[i + 1]);      // mu_i         [k = b][i]
    g.Qpos = make_operand(below_pos, ld_bp, h->n[i]);                  // X / mu_{i-1} [k = b][j]
    g.Kpos = h->N;
    g.Pneg = make_operand(h->H[i].p, h->H[i].ld, h->n[i + 1]);
    g.Qneg = make_operand(below_neg.p, below_neg.ld, h->n[i]);
    g.Kneg = h->M;
    g.I = h->n[i + 1]; g.J = h->n[i];
    g.form = 1; g.fused = fused;
    g.raw = h->grad.p + h->raw_off[i][0]; g.raw2 = h->grad.p + h->raw_off[i][1];
    g.W = h->W[i].p; g.dW = h->dW[i].p; g.Wt = nullptr;                // Wt is rewritten by the max-norm pass
    g.ldw = h->W[i].ld; g.ldwt = h->Wt[i].ld;
    g.pen = h->pen[i].p;
    g.N = N; g.M = M; g.l2 = h->cfg.l2; g.lr = lr; g.mom = mom;
    if (h->cen_on && fused) {
        const GradCen cen{h->cen_o[i].p, h->cen_g[i].p, h->cen_o[i + 1].p, h->cen_g[i + 1].p};
        launch_grad(g, st ? st : h->stream, &cen);
    } else launch_grad(g, st ? st : h->stream);
}

// The centred form of launch_dbm_biases, three launches behind the column sums, all on the main stream and
// in front of the fork of apply_update:
//   1. offsets o_l and plain bias gradients g_l of every layer from the column sums   (cen_ema_kernel)
//   2. row scalars a = (x - o).o of every layer's positive and negative rows         (cen_rowscal_kernel)
//   3. bias corrections r_l + the bias / running-mean / penalty updates               (cen_bias_kernel)
static void launch_dbm_center(bm_dbm *h, const float *X_dev, float lr, float mom) {
    const int L = h->L, N = h->N, M = h->M;
    const float *pos[MAXL + 1], *neg[MAXL + 1]; int ldp[MAXL + 1], ldn[MAXL + 1];
    pos[0] = X_dev; ldp[0] = h->V; neg[0] = h->v.p; ldn[0] = h->v.ld;
    for (int i = 0; i < L; ++i) { pos[i + 1] = h->mu[i].p; ldp[i + 1] = h->mu[i].ld; neg[i + 1] = h->H[i].p; ldn[i + 1] = h->H[i].ld; }
    auto a_pos = [&](int l) { return h->cen_a.p + (size_t)l * (N + M); };
    auto a_neg = [&](int l) { return h->cen_a.p + (size_t)l * (N + M) + N; };
    CenEmaArgs e;
    memset(&e, 0, sizeof(e));
    CenRowArgs r;
    memset(&r, 0, sizeof(r));
    CenBiasArgs b;
    memset(&b, 0, sizeof(b));
    e.N = (float)N; e.M = (float)M; b.N = N; b.M = M;
    int nmax = 0;
    for (int l = 0; l <= L; ++l) {
        const int n = h->n[l];
        if (n > nmax) nmax = n;
        const float *sp = h->sums_p + sums_off(h, 2 * l), *sn = h->sums_p + sums_off(h, 2 * l + 1);
        e.job[l] = CenEmaJob{sp, sn, h->cen_o[l].p, h->cen_g[l].p, n, h->cen_nu[l]};
        r.job[r.njobs++] = CenRowJob{pos[l], h->cen_o[l].p, a_pos(l), ldp[l], N, n, 0};
        r.job[r.njobs++] = CenRowJob{neg[l], h->cen_o[l].p, a_neg(l), ldn[l], M, n, 0};
        CenBiasJob &j = b.job[b.njobs++];
        j.pos = pos[l]; j.ldp = ldp[l]; j.neg = neg[l]; j.ldn = ldn[l]; j.n = n;
        if (l > 0) { j.wp0 = a_pos(l - 1); j.wn0 = a_neg(l - 1); }
        if (l < L) { j.wp1 = a_pos(l + 1); j.wn1 = a_neg(l + 1); }
        j.o = h->cen_o[l].p; j.g = h->cen_g[l].p;
        DbmBiasArgs &d = j.d;
        d.s_pos = sp; d.s_neg = sn; d.n = n; d.N = (float)N; d.M = (float)M; d.lr = lr; d.mom = mom;
        if (l == 0) { d.b = h->vb.p; d.db = h->dvb.p; }
        else {
            const int i = l - 1;
            d.b = h->hb[i].p; d.db = h->dhb[i].p; d.q = h->q[i].p; d.mm = h->mm[i].p; d.pen = h->pen[i].p; d.layer = i;
            d.damping = h->cfg.sparsity_damping; d.cost = h->cfg.sparsity_cost[i]; d.target = h->cfg.sparsity_target[i];
        }
    }
    hipLaunchKernelGGL(cen_ema_kernel, dim3((nmax + 255) / 256, L + 1), dim3(256), 0, h->stream, e);
    launch_cen_rowscal(r, h->stream);
    launch_cen_bias(b, h->stream);
}

static int recon_msre(bm_dbm *h, const float *X_dev, float *out_msre);

static void launch_dbm_maxnorm(bm_dbm *h, int i, int c_first = 0, int c_end = -1, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    MaxNormArgs m;
    m.c_first = c_first; m.c_end = c_end < 0 ? h->n[i + 1] : c_end;
    if (m.c_end <= m.c_first) return;
    m.W = h->W[i].p; m.Wt = h->Wt[i].p; m.I = h->n[i + 1]; m.J = h->n[i]; m.ldw = h->W[i].ld; m.ldwt = h->Wt[i].ld;
    m.max_norm = h->cfg.max_norm; m.norm_out = h->wnorm[i].p;
    m.num = h->mn_fac[i].p; m.den = h->mn_fac[i].p + m.I;
    const int nc = m.c_end - m.c_first;
    hipLaunchKernelGGL(maxnorm_kernel, dim3((nc + MN_COLS - 1) / MN_COLS), dim3(NT), 0, st, m);
    hipLaunchKernelGGL(maxnorm_scale_kernel, dim3(((nc + 31) / 32) * ((m.J + 31) / 32)), dim3(256), 0, st, m);
}

// gradients + sparsity + momentum + max-norm (dbm.py:550-621) from the current mu / particles
static int apply_update(bm_dbm *h, const float *X_dev, float lr, float mom) {
    const float N = (float)h->N, M = (float)h->M;
    launch_dbm_colsums(h, X_dev);
    if (h->cen_on) launch_dbm_center(h, X_dev, lr, mom);
    else launch_dbm_biases(h, N, M, lr, mom);
    // The layers' outer products + max-norm passes are independent of each other (each reads mu / particles and its own
    // penalty vector, writes its own W / dW / W^T): odd layers go to the second stream, between a fork and a join event, so
    // that the 104 + 128 tiles of a 784-512-1024 stack share the chip instead of taking turns (once the launches are tuned).
    static const bool split_off = bm::dbg("dbm_tail_split") && atoi(bm::dbg("dbm_tail_split")) == 0;
    const bool split = !split_off && h->L >= 2 && h->updates_seen >= 3;
    if (split) {
        BM_HIP(hipEventRecord(h->ev_fork, h->stream));
        BM_HIP(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    }
    for (int i = 0; i < h->L; ++i) {
        hipStream_t st = (split && (i & 1)) ? h->stream2 : h->stream;
        launch_dbm_grad(h, X_dev, i, 1, N, M, lr, mom, st);
        launch_dbm_maxnorm(h, i, 0, -1, st);
    }
    if (split) {
        BM_HIP(hipEventRecord(h->ev_join, h->stream2));
        BM_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    }
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

// reconstruction sigma(mu0 W0^T + vb) (dbm.py:625-628) into R (pitch ldr)
static void reconstruct_from_mu(bm_dbm *h, float *R, int ldr) {
    issue(h, layer_pass(h, -1, h->N, NO_IN, in_of(h->mu[0]), 1.f, 1.f, mean_out(h, R, ldr)));
}

// AIS at any depth (dbm.py:650-736 for L = 2, extended): the odd-depth layers are the chain x, the even-depth layers are
// conditionally independent given x and summed out analytically.  `ev`: layer_pass index of the even-depth layers in
// ascending depth (-1 = v, then hidden 1, 3); `od`: hidden index of the odd-depth layers (0, 2)
struct AisLayers { int ne, no; int ev[3]; int od[2]; };
static AisLayers ais_layers(const bm_dbm *h) {
    AisLayers s;
    s.ne = 0; s.no = 0;
    s.ev[s.ne++] = -1;
    for (int i = 0; i < h->L; ++i) {                 // hidden layer i has depth i + 1
        if (i & 1) s.ev[s.ne++] = i;
        else s.od[s.no++] = i;
    }
    return s;
}

// log Z_0 = (V + sum_i n_i) log 2 (dbm.py:731-734); `literal`: the reference's float32 node
static double ais_log_Z0(const bm_dbm *h, bool literal) {
    int units = h->V;
    for (int i = 1; i <= h->L; ++i) units += h->n[i];
    return literal ? (double)((float)units * logf(2.0f)) : (double)units * (double)logf(2.0f);
}

extern "C" {

int bm_dbm_create(const bm_dbm_config *cfg, bm_dbm **out) {
    BM_CHECK(cfg && out, "null argument");
    BM_CHECK(cfg->n_layers >= 1 && cfg->n_layers <= MAXL, "n_layers %d outside [1, %d]", cfg->n_layers, MAXL);
    BM_CHECK(cfg->n_visible >= 1 && cfg->n_particles >= 1 && cfg->batch_size >= 1, "bad sizes");
    BM_CHECK(bm_device_count() > 0, "no HIP device visible: libbm355 has no CPU fallback");
    auto h = std::make_unique<bm_dbm>();
    h->cfg = *cfg;
    h->L = cfg->n_layers; h->V = cfg->n_visible; h->N = cfg->batch_size; h->M = cfg->n_particles;
    h->n[0] = h->V;
    for (int i = 0; i < h->L; ++i) {
        BM_CHECK(cfg->n_hiddens[i] >= 1, "bad hidden size");
        BM_CHECK(cfg->n_hiddens[i] > i, "layer %d needs more than %d units (sparsity index, dbm.py:583)", i, i);
        BM_CHECK(cfg->h_unit[i] == BM_UNIT_BERNOULLI || cfg->h_unit[i] == BM_UNIT_MULTINOMIAL, "unknown unit %d of hidden layer %d",
                 cfg->h_unit[i], i);
        if (cfg->h_unit[i] == BM_UNIT_MULTINOMIAL) {
            BM_CHECK(cfg->n_samples[i] >= 1, "Multinomial layer %d: n_samples must be >= 1 (got %d)", i, cfg->n_samples[i]);
            int64_t q[4];
            BM_TRY(bm_rbm_multinomial_limit(q));
            BM_CHECK(cfg->n_hiddens[i] <= q[3], "Multinomial layer %d: %d units > %lld (softmax row staged in LDS: 8 bytes per unit, the "
                     "runtime allows a workgroup %lld bytes of dynamic LDS; at most 8192 units)", i, cfg->n_hiddens[i], (long long)q[3], (long long)q[2]);
        }
        h->n[i + 1] = cfg->n_hiddens[i];
    }
    BM_TRY(create(h->stream)); BM_TRY(create(h->stream2));
    {
        bool small = h->L >= 2 && h->N <= 1024 && h->M <= 1024 && cfg->max_mf_updates >= 2;
        for (int i = 0; i < h->L; ++i) small = small && (long long)h->n[i] * h->n[i + 1] <= (2ll << 20);
        h->pcd_geo = small ? 3 : 0;
        if (bm::dbg("dbm_pcd_geo")) h->pcd_geo = atoi(bm::dbg("dbm_pcd_geo"));
    }
    h->cur = h->stream;
    BM_TRY(create(h->ev0)); BM_TRY(create(h->ev1));
    BM_TRY(create(h->ev_fork, hipEventDisableTiming)); BM_TRY(create(h->ev_join, hipEventDisableTiming));
    BM_TRY(create(h->ctl_host, bm_dbm::MF_RING));
    for (int i = 0; i < bm_dbm::MF_RING; ++i) BM_TRY(create(h->ctl_ev[i], hipEventDisableTiming));
    size_t nsums = 2 * (size_t)h->V;
    for (int i = 0; i < h->L; ++i) {
        const int a = h->n[i], b = h->n[i + 1];
        BM_TRY(h->W[i].alloc(a, b)); BM_TRY(h->Wt[i].alloc(b, a)); BM_TRY(h->dW[i].alloc(a, b));
        BM_TRY(h->hb[i].alloc(b)); BM_TRY(h->dhb[i].alloc(b)); BM_TRY(h->q[i].alloc(b)); BM_TRY(h->mm[i].alloc(b));
        BM_TRY(h->pen[i].alloc(b)); BM_TRY(h->wnorm[i].alloc(b)); BM_TRY(h->mn_fac[i].alloc(2 * (size_t)b));
        BM_TRY(h->mu[i].alloc(h->N, b)); BM_TRY(h->mu_alt[i].alloc(h->N, b)); BM_TRY(h->mu_new[i].alloc(h->N, b));
        BM_TRY(h->H[i].alloc(h->M, b)); BM_TRY(h->H_new[i].alloc(h->M, b));
        if (h->multinomial(i)) {                   // row store of the logits: the sweeps cannot fail on an allocation
            const int rows = h->N > h->M ? h->N : h->M;
            BM_TRY(h->logits[i].alloc(rows, b));
            h->logit_rows[i] = rows;
        }
        nsums += 2 * (size_t)b;
    }
    BM_TRY(h->vb.alloc(h->V)); BM_TRY(h->dvb.alloc(h->V)); BM_TRY(h->sigma.alloc(h->V));
    for (int l = 0; l <= h->L; ++l) BM_TRY(h->cen_o[l].alloc(h->n[l]));
    BM_TRY(h->v.alloc(h->M, h->V)); BM_TRY(h->v_new.alloc(h->M, h->V));
    BM_TRY(h->recon.alloc(h->N, h->V));
    {   // one contiguous buffer so that data-parallel training needs ONE all-reduce
        size_t off = 0;
        for (int i = 0; i < h->L; ++i)
            for (int s = 0; s < 2; ++s) { h->raw_off[i][s] = off; off += h->W[i].count(); }
        BM_TRY(h->grad.alloc(off + nsums));
        h->sums_p = h->grad.p + off;
    }
    BM_TRY(h->mfblk.alloc(2 * (size_t)BM_DBM_MAX_LAYERS * BM_MF_SLOTS));
    BM_TRY(h->ctl.alloc(1));
    h->flag = &h->ctl.p->maxdiff;
    BM_TRY(h->xw0.alloc(h->N, h->n[1]));
    BM_TRY(h->scal.alloc(4));
    {
        std::vector<float> ones(h->V, 1.0f);
        BM_HIP(hipMemcpy(h->sigma.p, ones.data(), h->V * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = h.release();
    return 0;
}

int bm_dbm_destroy(bm_dbm *h) {
    if (!h) return 0;
    for (hipStream_t st : {h->stream.h, h->stream2.h}) if (st) (void)hipStreamSynchronize(st);
    if (h->xchg_used) xchg_bind_user(h->xchg_used, nullptr);
    delete h;
    return 0;
}

int bm_dbm_sync(bm_dbm *h) {
    BM_HIP(hipStreamSynchronize(h->stream));
    if (h->xchg_used) BM_TRY(xchg_check_status(h->xchg_used));      // a lost rank is an ERROR here, never a silent wrong sum
    return 0;
}
int bm_dbm_seed(bm_dbm *h, uint64_t seed) { h->seed = seed; h->call = 0; return 0; }
int bm_dbm_set_row_offset(bm_dbm *h, int64_t row0, int64_t particle0) { h->row0 = row0; h->prow0 = particle0; return 0; }

// "W", "W_1", "hb_2" ... -> (base, layer)
static bool split_name(const std::string &nm, std::string &base, int &idx) {
    const size_t u = nm.rfind('_');
    base = nm; idx = 0;
    if (u != std::string::npos && u + 1 < nm.size() && isdigit((unsigned char)nm[u + 1])) {
        bool digits = true;
        for (size_t i = u + 1; i < nm.size(); ++i) digits = digits && isdigit((unsigned char)nm[i]);
        if (digits) { base = nm.substr(0, u); idx = atoi(nm.c_str() + u + 1); }
    }
    return true;
}

static int resolve(bm_dbm *h, const char *name, Mat **mat, DevBuf **vec, bool *is_W) {
    std::string base; int idx;
    split_name(std::string(name ? name : ""), base, idx);
    *mat = nullptr; *vec = nullptr; *is_W = false;
    BM_CHECK(idx >= 0 && idx < h->L, "layer index %d out of range in '%s'", idx, name ? name : "(null)");
    if (base == "W") { *mat = &h->W[idx]; *is_W = true; }
    else if (base == "dW") *mat = &h->dW[idx];
    else if (base == "mu") *mat = &h->mu[idx];
    else if (base == "mu_new") *mat = &h->mu_new[idx];
    else if (base == "h") *mat = &h->H[idx];
    else if (base == "h_new") *mat = &h->H_new[idx];
    else if (base == "v" && idx == 0) *mat = &h->v;
    else if (base == "v_new" && idx == 0) *mat = &h->v_new;
    else if (base == "hb") *vec = &h->hb[idx];
    else if (base == "dhb") *vec = &h->dhb[idx];
    else if (base == "q_means") *vec = &h->q[idx];
    else if (base == "mu_means") *vec = &h->mm[idx];
    else if (base == "W_norm") *vec = &h->wnorm[idx];
    else if (base == "vb" && idx == 0) *vec = &h->vb;
    else if (base == "dvb" && idx == 0) *vec = &h->dvb;
    else if (base == "sigma" && idx == 0) *vec = &h->sigma;
    else if (base == "ov" && idx == 0) *vec = &h->cen_o[0];      // centering offsets (bm_dbm_set_centering)
    else if (base == "oh") *vec = &h->cen_o[idx + 1];
    BM_CHECK(*mat || *vec, "unknown DBM variable '%s'", name ? name : "(null)");
    return 0;
}

// Centred update (bm355.h).  A property of the handle: while it is on, bm_dbm_train_step and
// bm_dbm_train_step_pt take the centred update.  nu [n_layers + 1]: the sliding factors of v, h_1, ... (read when `on`).
int bm_dbm_set_centering(bm_dbm *h, int32_t on, const float *nu) {
    BM_CHECK(h, "null argument");
    if (!on) { h->cen_on = false; return 0; }
    BM_CHECK(nu, "centering: null sliding factors");
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "centering needs Bernoulli visible units (this handle's are Gaussian)");
    for (int i = 0; i < h->L; ++i) BM_CHECK(!h->multinomial(i), "centering needs Bernoulli hidden units (layer %d of this handle is Multinomial)", i);
    for (int l = 0; l <= h->L; ++l) BM_CHECK(nu[l] >= 0.f && nu[l] <= 1.f, "centering: sliding factor %g of layer %d outside [0, 1]", (double)nu[l], l);
    if (!h->cen_a.p) {
        for (int l = 0; l <= h->L; ++l) BM_TRY(h->cen_g[l].alloc(h->n[l]));
        BM_TRY(h->cen_a.alloc((size_t)(h->L + 1) * (h->N + h->M)));      // last: the workspace is complete once it exists
    }
    for (int l = 0; l <= h->L; ++l) h->cen_nu[l] = nu[l];
    h->cen_on = true;
    return 0;
}

int bm_dbm_set_param(bm_dbm *h, const char *name, const float *host, size_t n) {
    Mat *m; DevBuf *v; bool isW;
    BM_TRY(resolve(h, name, &m, &v, &isW));
    BM_HIP(hipStreamSynchronize(h->stream));
    if (m) {
        BM_CHECK(n == (size_t)m->rows * m->cols, "variable '%s' has %zu elements, got %zu", name, (size_t)m->rows * m->cols, n);
        BM_TRY(m->upload(host));
        if (m >= h->dW && m < h->dW + MAXL && h->dw_sharded) {
            // the host replaces a momentum buffer whole: with every layer's buffer replaced the replicas are complete again
            h->dw_set_mask |= 1u << (unsigned)(m - h->dW);
            if (h->dw_set_mask == (1u << (unsigned)h->L) - 1u) { h->dw_sharded = false; if (h->xchg_used) xchg_dw_replaced(h->xchg_used); }
        }
        if (isW) {
            std::vector<float> t(n);
            for (int r = 0; r < m->rows; ++r)
                for (int c = 0; c < m->cols; ++c) t[(size_t)c * m->rows + r] = host[(size_t)r * m->cols + c];
            Mat *wt = &h->Wt[m - h->W];
            BM_TRY(wt->upload(t.data()));
        }
        return 0;
    }
    BM_CHECK(n == v->n, "variable '%s' has %zu elements, got %zu", name, v->n, n);
    BM_HIP(hipMemcpy(v->p, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int bm_dbm_get_param(bm_dbm *h, const char *name, float *host, size_t n) {
    Mat *m; DevBuf *v; bool isW;
    BM_TRY(resolve(h, name, &m, &v, &isW));
    BM_HIP(hipStreamSynchronize(h->stream));
    if (m) {
        BM_CHECK(n == (size_t)m->rows * m->cols, "variable '%s' has %zu elements, got %zu", name, (size_t)m->rows * m->cols, n);
        if (m >= h->dW && m < h->dW + MAXL) BM_TRY(check_dw(h, "bm_dbm_get_param(dW)"));
        return m->download(host);
    }
    BM_CHECK(n == v->n, "variable '%s' has %zu elements, got %zu", name, v->n, n);
    BM_HIP(hipMemcpy(host, v->p, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int bm_dbm_dev_ptr(bm_dbm *h, const char *name, void **out_dev, size_t *out_n) {
    if (name && std::string(name) == "grad") {
        *out_dev = h->grad.p;
        if (out_n) *out_n = h->grad.n;
        return 0;
    }
    Mat *m; DevBuf *v; bool isW;
    BM_TRY(resolve(h, name, &m, &v, &isW));
    BM_CHECK(v, "no device view for '%s' (matrices are pitched; use get/set_param)", name);
    *out_dev = v->p;
    if (out_n) *out_n = v->n;
    return 0;
}

int bm_dbm_train_step(bm_dbm *h, const float *X_dev, float lr, float mom, int32_t k,
                      int32_t *out_n_mf, float *out_msre) {
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", k);
    BM_TRY(check_dw(h, "bm_dbm_train_step"));
    int nmf = 0;
    BM_TRY(mean_field_and_particles(h, X_dev, k, &nmf));      // :517, :521
    if (out_msre) BM_TRY(recon_msre(h, X_dev, out_msre));     // :625-630 (W before the update)
    BM_TRY(apply_update(h, X_dev, lr, mom));
    if (out_n_mf) *out_n_mf = nmf;
    h->call++;
    return 0;
}

// msre of sigma(mu0 W0^T + vb) against X (dbm.py:625-630), mu from the last mean_field()
static int recon_msre(bm_dbm *h, const float *X_dev, float *out_msre) {
    reconstruct_from_mu(h, h->recon.p, h->recon.ld);
    BM_HIP(hipMemsetAsync(h->scal.p, 0, sizeof(double), h->stream));
    hipLaunchKernelGGL(sqdiff_kernel, dim3(128), dim3(256), 0, h->stream, X_dev, h->V, (const float *)h->recon.p,
                       h->recon.ld, h->N, h->V, h->scal.p);
    double s = 0.0;
    BM_HIP(hipMemcpyAsync(&s, h->scal.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    *out_msre = (float)(s / ((double)h->N * h->V));
    return 0;
}

// session.run([msre, n_mf_updates]) of _run_val_metrics (dbm.py:813): both tensors are built under
// tf.control_dependencies([v_update, v_new_update] + H_updates + H_new_updates + mu_updates) (:521-523),
// so the fetch runs the mean-field on X AND advances the fantasy particles by n_gibbs_steps; no parameter update.
int bm_dbm_metrics(bm_dbm *h, const float *X_dev, int32_t k, int32_t *out_n_mf, float *out_msre) {
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", k);
    int nmf = 0;
    BM_TRY(mean_field_and_particles(h, X_dev, k, &nmf));
    if (out_msre) BM_TRY(recon_msre(h, X_dev, out_msre));
    if (out_n_mf) *out_n_mf = nmf;
    h->call++;
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_set_comm(bm_dbm *h, bm_comm *c) {
    BM_CHECK(h, "null argument");
    h->comm = c;
    return 0;
}

// Opt-in fast-binary mode (bm_bf3.h): contractions whose input states are {0,1} bitmaps run as exact-product
// bf16 x 3 on the bf16 matrix cores (AIS with all layers sampled).  Results then agree with the default fp32 chain to
// fp32 round-off, not bit for bit.  0 restores the default.  1 = where it pays: AIS (0.82 -> 0.42 s per 1000-beta run of
// 20 000 chains) and the particle sweeps of stacks with >= 8M weights in the bottom layer (3072 x 5000: +4 %); 2 = wherever
// legal (tests, measurements: the particle sweeps of the 784-512-1024 stack are SLOWER in this mode).
int bm_dbm_set_fast_binary(bm_dbm *h, int32_t on) {
    BM_CHECK(h, "null argument");
    BM_CHECK(!(on && h->sigmoid_literal), "fast-binary mode and the literal sigmoid exclude each other");
    h->fast = on >= 2 ? 2 : (on ? 1 : 0);
    return 0;
}

// 1: the AIS log-weights are accumulated as the reference's graph does it - every log p*_beta(x) formed and added /
// subtracted in float32, in the order of dbm.py:708-728 (two extra score-only passes per beta); 0 (default): the
// difference of the two softplus terms per element, summed in double (deterministic, closer to the exactly
// enumerable log Z; the reference's README admits the nats its float32 loop loses at many betas)
int bm_dbm_set_ais_literal(bm_dbm *h, int32_t on) {
    BM_CHECK(h, "null argument");
    h->ais_literal = on ? 1 : 0;
    return 0;
}

// 1: every Bernoulli activation of this engine - mean-field, particle sweeps, AIS transitions, reconstruction - is the literal
// float32 `1 / (1 + exp(-x))` of tf.nn.sigmoid (layers.py:47-48; bm_numerics.h sigmoid_literal) instead of the engine's own
// one-division form.  The values agree to float32 round-off; what changes is the mean-field trip count at an mf_tol near
// that round-off (dbm.py:449-452 at the default 1e-7 is decided in the last bits of the means): with the literal form the
// engine executes the sweeps the reference's graph executes.  Turns the fast-binary mode off for this engine (its epilogue
// is the hardware sigmoid).
int bm_dbm_set_sigmoid_literal(bm_dbm *h, int32_t on) {
    BM_CHECK(h, "null argument");
    h->sigmoid_literal = on ? 1 : 0;
    if (on) h->fast = 0;
    return 0;
}

int bm_dbm_set_xchg(bm_dbm *h, bm_xchg *x) {
    BM_CHECK(h, "null argument");
    h->xchg = x;
    if (x) { h->xchg_used = x; xchg_bind_user(x, &h->xchg_used); }
    return 0;
}

int bm_dbm_set_mf_allreduce(bm_dbm *h, float (*fn)(float, void *), void *ctx) {
    h->mf_reduce = fn; h->mf_ctx = ctx;
    return 0;
}

// data-parallel halves: phase 1 leaves the raw local sums in "grad", the caller
// all-reduces that buffer, phase 2 normalises with the GLOBAL N and M and applies the update.
int bm_dbm_grad_step(bm_dbm *h, const float *X_dev, int32_t k, int32_t *out_n_mf) {
    BM_CHECK(!h->cen_on, "bm_dbm_grad_step: the split step has no centred form; switch centering off (bm_dbm_set_centering)");
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", k);
    int nmf = 0;
    BM_TRY(mean_field_and_particles(h, X_dev, k, &nmf));
    launch_dbm_colsums(h, X_dev);
    for (int i = 0; i < h->L; ++i) launch_dbm_grad(h, X_dev, i, 0, 1.f, 1.f, 0.f, 0.f);
    if (out_n_mf) *out_n_mf = nmf;
    h->call++;
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_apply_step(bm_dbm *h, int32_t N_global, int32_t M_global, float lr, float mom) {
    BM_CHECK(!h->cen_on, "bm_dbm_apply_step: the split step has no centred form; switch centering off (bm_dbm_set_centering)");
    const float N = (float)N_global, M = (float)M_global;
    BM_TRY(check_dw(h, "bm_dbm_apply_step"));
    launch_dbm_biases(h, N, M, lr, mom);
    for (int i = 0; i < h->L; ++i) {
        ApplyWArgs a;
        memset(&a, 0, sizeof(a));
        a.raw = h->grad.p + h->raw_off[i][0]; a.raw2 = h->grad.p + h->raw_off[i][1];
        a.W = h->W[i].p; a.dW = h->dW[i].p; a.Wt = nullptr; a.pen = h->pen[i].p;
        a.I = h->n[i + 1]; a.J = h->n[i]; a.ldw = h->W[i].ld; a.ldwt = h->Wt[i].ld; a.form = 1;
        a.N = N; a.M = M; a.l2 = h->cfg.l2; a.lr = lr; a.mom = mom;
        launch_apply_w(a, nullptr, h->stream);
        launch_dbm_maxnorm(h, i);
    }
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_stream(bm_dbm *h, void **out_stream) { *out_stream = (void *)h->stream; return 0; }

int bm_dbm_mean_field(bm_dbm *h, const float *X_dev, float *MU_top_dev, int32_t *out_n_mf) {
    int nmf = 0;
    BM_TRY(mean_field(h, X_dev, &nmf));
    if (MU_top_dev) {
        const Mat &t = h->mu[h->L - 1];
        hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)t.p, t.ld, MU_top_dev, t.cols,
                           t.rows, t.cols);
    }
    if (out_n_mf) *out_n_mf = nmf;
    h->call++;
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_reconstruct(bm_dbm *h, const float *X_dev, float *R_dev) {
    BM_CHECK(R_dev, "null output");
    BM_TRY(mean_field(h, X_dev, nullptr));
    reconstruct_from_mu(h, R_dev, h->V);
    h->call++;
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

// cl: the visible units held at observed values (bm_dbm_sample_v_clamped), null: none
static int sample_v(bm_dbm *h, int32_t k, float *V_dev, const Clamp *cl) {
    BM_CHECK(k >= 0, "n_gibbs_steps must be >= 0");
    if (cl) hipLaunchKernelGGL(clamp_apply_kernel, dim3(256), dim3(256), 0, h->stream, h->v.p, h->v.ld, cl->val, cl->mask, cl->ld, h->M, h->V);
    particles_update(h, k, true, cl);                         // :643-644
    // `_make_particles_update(sample=False)` whose v assign is the only one fetched (:646-647):
    // k mean sweeps from the sampled state; only v takes the result, H / *_new keep theirs.
    // scratch: the mu buffers do not fit (M != N); the handle's own, allocated at the first call (sv_v[1] last)
    if (!h->sv_v[1].p) {
        for (int b = 0; b < 2; ++b) for (int i = 0; i < h->L; ++i) BM_TRY(h->sv_H[b][i].alloc(h->M, h->n[i + 1]));
        BM_TRY(h->sv_v[0].alloc(h->M, h->V)); BM_TRY(h->sv_v[1].alloc(h->M, h->V));
    }
    const Mat *Hin = h->H; LayerIn vin = in_of(h->v);
    Mat *Hout = h->sv_H[0], *Hout2 = h->sv_H[1]; Mat *vout = &h->sv_v[0], *vout2 = &h->sv_v[1];
    for (int t = 0; t < k; ++t) {
        gibbs_sweep(h, h->M, vin, Hin, vout, Hout, true, false, k + t, h->prow0, nullptr, cl);
        vin = in_of(*vout); Hin = Hout;
        Mat *x = Hout; Hout = Hout2; Hout2 = x;
        Mat *y = vout; vout = vout2; vout2 = y;
    }
    // v <- v_means (the last vout is now vout2 after the swap).  k == 0: no sweep ran, v keeps its value
    // (the reference's op list is empty then, dbm.py:641-648; oracle: orc_dbm_sample_v)
    if (k > 0)
        hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)vout2->p, vout2->ld, h->v.p, h->v.ld,
                           h->M, h->V);
    if (V_dev)
        hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)h->v.p, h->v.ld, V_dev, h->V,
                           h->M, h->V);
    BM_HIP(hipStreamSynchronize(h->stream));
    h->call++;
    return 0;
}
int bm_dbm_sample_v(bm_dbm *h, int32_t k, float *V_dev) { return sample_v(h, k, V_dev, nullptr); }

// bm_dbm_sample_v with the visible units of the particles held at observed values where the mask is non-zero (DESIGN.md
// 3.12): the clamp is applied to the particles' visible layer first, then in the epilogue of EVERY visible-layer pass of the
// call (LayerPass::clamp; the CL flavour of act_kernel), the mean sweeps included
int bm_dbm_sample_v_clamped(bm_dbm *h, int32_t k, const float *clamp_val_dev, const float *clamp_mask_dev, float *V_dev) {
    BM_CHECK(h && clamp_val_dev && clamp_mask_dev, "null argument");
    for (int i = 0; i < h->L; ++i)
        BM_CHECK(!h->multinomial(i), "bm_dbm_sample_v_clamped: a Multinomial hidden layer (layer %d) is not supported", i);
    const Clamp cl{clamp_val_dev, clamp_mask_dev, h->V};
    return sample_v(h, k, V_dev, &cl);
}

// ---- parallel tempering (bm355.h: bm_dbm_pt_init / _sweep / _read)

// (the ensemble, its start, the replica exchange, the rescore and the gather: bm_pt.h, shared with bm_rbm_pt_*)

// what the tempered family is defined for (the messages name the reason; bm355.h)
static int check_pt_model(const bm_dbm *h, const char *what) {
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "%s: Gaussian visible units are not supported (their tempered noise scale differs; "
             "Bernoulli visible units only)", what);
    for (int i = 0; i < h->L; ++i)
        BM_CHECK(!h->multinomial(i), "%s: a Multinomial hidden layer (layer %d) is not supported (Bernoulli hidden layers only)", what, i);
    BM_CHECK(h->L <= 2, "%s: %d hidden layers are not supported (at most 2): from three layers on a pass reads the OLD layer above, "
             "so at no point of the sweep do the slot partials hold every interaction term of ONE consistent state and the swap "
             "energy would have to be recomputed", what, h->L);
    BM_CHECK(!h->sigmoid_literal, "%s: the handle is in literal-sigmoid mode (bm_dbm_set_sigmoid_literal); the row-tempered kernels "
             "have no literal flavour", what);
    return 0;
}

// one row-tempered pass of the ensemble (the RT flavour of act_kernel), always a per-pass fp32 launch on the main stream:
//   layer 0: h1 ~ Ber(sigmoid(beta_row (v W0 + h2 W1^T + b1))) from (pt.v, pt.h2) - two K segments at L == 2 - leaving the slot
//            partials of h1.(v W0 + h2 W1^T + b1);  layer 1: h2 from pt.h1, leaving those of h2.b2;  layer -1: v from pt.h1,
//            leaving those of v.vb
static void pt_pass(bm_dbm *h, int layer, int t) {
    PtEnsemble &e = h->pt;
    const LayerIn below = layer == 0 ? in_of(e.v.x) : (layer == 1 ? in_of(e.h1.x) : NO_IN);
    const LayerIn above = layer == 0 ? (h->L == 2 ? in_of(e.h2.x) : NO_IN) : (layer == 1 ? NO_IN : in_of(e.h1.x));
    PtLayer &out = e.layer(layer + 1);
    const PhiloxKey key = dkey(h, layer < 0 ? SITE_DBM_V : SITE_DBM_H + layer, t, h->seed, h->call);
    LayerPass p = layer_pass(h, layer, e.nrows(), below, above, 1.f, 1.f,
                             value_out(1, out.x.p, out.x.ld, key, e.row0()));   // (mult: not read)
    if (layer == 0) p.energy_rows(out.part.p, e.rows);
    else p.statedot_rows(out.part.p, e.rows, layer == 1 ? h->hb[1].p : h->vb.p);
    issue(h, p.row_tempered(e.mult.p));     // (h->cur is the main stream here: only enqueue_particles_stream2 moves it, and back)
}

// step t of a tempered call, in gibbs_sweep's order with every layer sampled: h1 from (v, OLD h2); the swap of the parity of the
// global step number - the state is (v_t, h1_{t+1}, h2_t) and the three partial arrays are exactly its -E; h2; v
static void pt_step(bm_dbm *h, int t) {
    pt_pass(h, 0, t);
    pt_launch_swap(h->pt, h->stream, t, dkey(h, SITE_DBM_PT_SWAP, t, h->seed, h->call));
    if (h->L == 2) pt_pass(h, 1, t);
    pt_pass(h, -1, t);
}

// Parallel tempering of a DBM (replica exchange).  The ensemble lives in the handle; see bm355.h for the contract.
int bm_dbm_pt_init(bm_dbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0) {
    BM_CHECK(h, "null argument");
    BM_TRY(check_pt_model(h, "bm_dbm_pt_init"));
    BM_TRY(pt_check_ladder(n_chains, n_temps, betas_host, chain0));
    const int widths[3] = {h->V, h->n[1], h->L == 2 ? h->n[2] : 0};
    return pt_begin(h->pt, h->stream, widths, n_chains, n_temps, chain0, betas_host, V0_dev, h->vb.p, h->hb[1].p,
                    dkey(h, SITE_DBM_PT_START, 0, h->seed, h->call), dkey(h, SITE_DBM_PT_START, 1, h->seed, h->call));
}

int bm_dbm_pt_sweep(bm_dbm *h, int32_t n_steps) {
    BM_CHECK(h, "null argument");
    BM_CHECK(h->pt.M > 0, "bm_dbm_pt_sweep: no ensemble (call bm_dbm_pt_init first)");
    BM_TRY(check_pt_model(h, "bm_dbm_pt_sweep"));  // (the literal-sigmoid mode may have been switched on since the init)
    BM_CHECK(n_steps >= 1, "n_steps must be >= 1 (got %d)", (int)n_steps);
    pt_sweep_with(h->pt, n_steps, [&](int t) { pt_step(h, t); });
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_pt_read(bm_dbm *h, float *V_dev, float *H1_dev, float *H2_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    BM_CHECK(h, "null argument");
    BM_CHECK(h->pt.M > 0, "bm_dbm_pt_read: no ensemble (call bm_dbm_pt_init first)");
    BM_CHECK(!H2_dev || h->L == 2, "bm_dbm_pt_read: H2_dev for a stack of one hidden layer");
    BM_CHECK(V_dev || !H1_dev, "bm_dbm_pt_read: H1_dev without V_dev");
    float *const dst[3] = {V_dev, H1_dev, H2_dev};
    const int ldd[3] = {h->V, h->n[1], h->L == 2 ? h->n[2] : 0};
    return pt_read_with(h->pt, h->stream, dst, ldd, swaps_host, ladder_idx_host);        // (one gather launch for the up to three matrices)
}

// One update whose negative particles are the beta = 1 rows of the tempered ensemble (bm355.h): bm_dbm_train_step
// with another source for h->v / h->H[i].  Everything on the main stream, no host synchronisation of its own.
int bm_dbm_train_step_pt(bm_dbm *h, const float *X_dev, float lr, float mom, int32_t k, int32_t *out_n_mf, float *out_msre) {
    BM_CHECK(h && X_dev, "null argument");
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", (int)k);
    BM_TRY(check_dw(h, "bm_dbm_train_step_pt"));
    BM_CHECK(h->pt.M > 0, "bm_dbm_train_step_pt: no ensemble (call bm_dbm_pt_init first)");
    BM_CHECK(h->pt.M >= h->M, "bm_dbm_train_step_pt: the ensemble has %d chains, fewer than n_particles = %d (every particle is the "
             "beta = 1 row of a chain of its own)", h->pt.M, h->M);
    BM_TRY(check_pt_model(h, "bm_dbm_train_step_pt"));
    BM_CHECK(!h->comm && !h->xchg && !h->mf_reduce, "bm_dbm_train_step_pt: the handle has a communicator or a direct exchange attached "
             "(data-parallel job); the chains of the ensemble are not sharded over ranks");
    // 1. the v.vb and h2.b2 partials of the swap energy under the biases of NOW (the previous update moved them)
    pt_launch_rescore(h->pt, h->stream, h->vb.p, h->hb[1].p);
    // 2. positive phase
    int nmf = 0;
    BM_TRY(mean_field(h, X_dev, &nmf));
    // 3. the tempered steps of all rows: a sweep at the handle's call
    for (int t = 0; t < k; ++t) pt_step(h, t);
    // 4. hand-over: the beta = 1 rows of the chains [0, n_particles) become the dense particles the update reads (a launch of
    //    its own: h1 is stored BEFORE the swap that settles which row is at beta = 1)
    {
        float *const dst[3] = {h->v.p, h->H[0].p, h->L == 2 ? h->H[1].p : nullptr};
        const int ldd[3] = {h->v.ld, h->H[0].ld, h->L == 2 ? h->H[1].ld : 0};
        pt_launch_gather(h->pt, h->stream, h->M, dst, ldd);
    }
    h->updates_seen++;
    h->pt.step += k;
    BM_HIP(hipGetLastError());
    // 5. + 6. as bm_dbm_train_step
    if (out_msre) BM_TRY(recon_msre(h, X_dev, out_msre));
    BM_TRY(apply_update(h, X_dev, lr, mom));
    if (out_n_mf) *out_n_mf = nmf;
    h->call++;
    return 0;
}

static int ensure_ais(bm_dbm *h, int rows) {
    if (rows <= h->ais_rows) return 0;
    h->ais_rows = 0;                               // (set again once every buffer exists: a failure leaves none counted)
    const AisLayers s = ais_layers(h);
    int nmax = 1;
    for (int l = 0; l <= h->L; ++l) nmax = h->n[l] > nmax ? h->n[l] : nmax;
    // every partial buffer holds the slots of the widest layer: AIS and ELBO use them for different layers
    const size_t part = (size_t)nslots(nmax) * rows;
    for (int e = 0; e < s.ne; ++e) {
        BM_TRY(h->ae[e].alloc(rows, s.ev[e] < 0 ? h->V : h->n[s.ev[e] + 1]));
        BM_TRY(h->apart_e[e].alloc(part));
    }
    for (int o = 0; o < s.no; ++o)
        for (int b = 0; b < 2; ++b) {
            BM_TRY(h->ao[o][b].alloc(rows, h->n[s.od[o] + 1]));
            BM_TRY(h->apart_o[o][b].alloc(part));
        }
    BM_TRY(h->rowtmp.alloc(rows));
    BM_TRY(h->alogw.alloc(rows));
    h->ais_rows = rows;
    return 0;
}

// x0 ~ Bernoulli(1/2): Bernoulli(logits=0).sample(seed) (dbm.py:699-702)
__global__ void ais_init_kernel(float *X, int ld, int rows, int cols, PhiloxKey key, unsigned long long row0) {
    const size_t n = (size_t)rows * cols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / (size_t)cols, c = e % (size_t)cols;
        X[r * ld + c] = (philox_uniform_at(key, (row0 + r) * (unsigned long long)cols + c) < 0.5f) ? 1.f : 0.f;
    }
}

// rowdot[j] = sum_i X[j][i] * vec[i]  (one wave per row; fixed lane-strided order + butterfly: deterministic)
__global__ __launch_bounds__(256) void rowdot_kernel(const float *X, int ld, int rows, int cols, const float *vec, float *out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane; c < cols; c += 64) s += X[(size_t)row * ld + c] * vec[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = s;
}

// (AisScoreArgs / ais_score_kernel, the default accumulation: bm_kernels.h, shared with bm_rbm_ais)
// LITERAL accumulation (bm_dbm_set_ais_literal; the reference's arithmetic, dbm.py:650-660 and :708-728): one call
// adds or subtracts ONE log p*_beta(x) to the running log-weight, everything in float32 - for L = 2
//   lp = (x.hb0 * beta + sum_i softplus(beta (x W0^T + vb)_i)) + sum_k softplus(beta (x W1 + hb1)_k);   lz = lz -/+ lp
// (`T1 *= beta; log_p = T1; log_p += reduce_sum(..); log_p += reduce_sum(..)`; `log_Z += / -= ...`); at other depths
// the odd-depth x.hb terms times beta in ascending depth, then the even-depth softplus sums in ascending depth.  The row
// sums are the slot partials added in ascending order in float32.  logw holds the float value (exactly) in its double.
__global__ __launch_bounds__(256) void ais_score_literal_kernel(double *logw, int J, int ld, AisScoreArgs p, float beta, int sign) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    float lp = 0.f;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        if (o >= p.no) break;
        float dot = 0.f;
        for (int q = 0; q < p.no_slots[o]; ++q) dot = dot + p.po[o][(size_t)q * ld + j];
        lp = (o == 0) ? dot * beta : lp + dot * beta;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (e >= p.ne) break;
        float sv = 0.f;
        for (int q = 0; q < p.ne_slots[e]; ++q) sv = sv + p.pe[e][(size_t)q * ld + j];
        lp = lp + sv;
    }
    const float lz = (float)logw[j];
    logw[j] = (double)(sign > 0 ? lz + lp : lz - lp);
}

// the AIS run itself: leaves the per-chain log-weights (without log Z_0) in h->alogw [n_runs] (device, double).
// Any depth: the chain is x = the odd-depth layers, log p*_beta(x) = beta sum_odd b_l.x_l + sum_even sum_i
// softplus(beta a_{l,i}); one transition step updates the even-depth layers given x, then the odd-depth layers given
// them, both in ascending depth.  For L = 2 this is the reference's construction (dbm.py:650-736) launch for launch.
static int ais_core(bm_dbm *h, int32_t n_betas, int32_t n_runs, int32_t k, uint64_t seed, int64_t chain0) {
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "AIS needs Bernoulli visible units (dbm.py:926-927)");
    for (int i = 0; i < h->L; ++i) BM_CHECK(!h->multinomial(i), "AIS needs Bernoulli hidden layers (dbm.py:926-927)");
    BM_CHECK(n_betas >= 2 && n_runs >= 1 && k >= 1, "bad AIS arguments");
    BM_TRY(ensure_ais(h, n_runs));
    const AisLayers S = ais_layers(h);
    const int R = n_runs, V = h->V, H1 = h->n[1];
    const float db = 1.0f / (float)n_betas;                               // delta_beta (dbm.py:929)
    // x.hb of the current / next state as slot partials (pitch ldp); x0's comes from rowdot_kernel as ONE slot
    const int ldp = h->ais_rows;
    Mat *x[2], *xn[2];                                                    // odd-depth states: current / next
    float *rdot_cur[2], *rdot_next[2];
    int nd_cur[2];
    for (int o = 0; o < S.no; ++o) {
        x[o] = &h->ao[o][0]; xn[o] = &h->ao[o][1];
        rdot_cur[o] = h->apart_o[o][0].p; rdot_next[o] = h->apart_o[o][1].p;
        nd_cur[o] = 1;
    }
    BM_HIP(hipMemsetAsync(h->alogw.p, 0, (size_t)R * sizeof(double), h->stream));
    for (int o = 0; o < S.no; ++o)                                        // odd-depth layer o: site SITE_AIS_X0 + 16 o
        hipLaunchKernelGGL(ais_init_kernel, dim3(512), dim3(256), 0, h->stream, x[o]->p, x[o]->ld, R, h->n[S.od[o] + 1],
                           dkey(h, SITE_AIS_X0, o, seed, 0), (unsigned long long)chain0);
    // fast-binary mode: every state of the run is a {0,1} bitmap when all three layers are sampled (the default).
    // 2-layer DBMs only: at other depths the run takes the fp32 path (bm355.h)
    FastScope fast_scope{h};
    if (h->fast && h->L == 2 && h->cfg.sample_v_states && h->cfg.sample_h_states[0] && h->cfg.sample_h_states[1]) {
        const int H2 = h->n[2];
        BM_TRY(fast_build_planes(h));
        if (h->ah2_16.rows != h->ais_rows) {      // (ah2_16 is allocated last)
            BM_TRY(h->ax16.alloc(1, h->ais_rows, H1)); BM_TRY(h->ax2_16.alloc(1, h->ais_rows, H1));
            BM_TRY(h->av16.alloc(1, h->ais_rows, V)); BM_TRY(h->ah2_16.alloc(1, h->ais_rows, H2));
        }
        // (entered on every run: ensure_ais may have moved the state matrices since the last one)
        h->shadow[0] = {h->ao[0][0].p, &h->ax16, true}; h->shadow[1] = {h->ao[0][1].p, &h->ax2_16, true};
        h->shadow[2] = {h->ae[0].p, &h->av16, true};    h->shadow[3] = {h->ae[1].p, &h->ah2_16, true};
        hipLaunchKernelGGL(shadow16_kernel, dim3(512), dim3(256), 0, h->stream, (const float *)x[0]->p, x[0]->ld, R, H1, h->ax16.p, h->ax16.ld);
        fast_scope.begin(true);
    }
    for (int o = 0; o < S.no; ++o)
        hipLaunchKernelGGL(rowdot_kernel, dim3((R + 3) / 4), dim3(256), 0, h->stream, (const float *)x[o]->p, x[o]->ld, R,
                           h->n[S.od[o] + 1], (const float *)h->hb[S.od[o]].p, rdot_cur[o]);

    // the inputs of a layer update from the AIS states: an even-depth layer reads the odd-depth states x, an odd-depth
    // layer the even-depth states (its neighbours in depth; the top layer has no `above`)
    auto state_of = [&](int hidden) -> LayerIn {                          // state of hidden layer `hidden` (-1: v)
        const int d = hidden + 1;
        return in_of((d & 1) ? *x[d >> 1] : h->ae[d >> 1]);
    };
    auto below_of = [&](int li) { return li < 0 ? NO_IN : state_of(li - 1); };
    auto above_of = [&](int li) { return li + 1 < h->L ? state_of(li + 1) : NO_IN; };
    auto site_of = [](int li) -> uint32_t { return li < 0 ? SITE_DBM_V : SITE_DBM_H + (uint32_t)li; };
    auto width_of = [&](int li) { return li < 0 ? V : h->n[li + 1]; };
    auto score_args = [&]() {
        AisScoreArgs p;
        memset(&p, 0, sizeof(p));
        p.ne = S.ne; p.no = S.no;
        for (int e = 0; e < S.ne; ++e) { p.pe[e] = h->apart_e[e].p; p.ne_slots[e] = nslots(width_of(S.ev[e])); }
        for (int o = 0; o < S.no; ++o) { p.po[o] = rdot_cur[o]; p.no_slots[o] = nd_cur[o]; }
        return p;
    };

    // visit(x; beta_a, beta_b, beta_c): logw += log p*_{beta_b}(x) - log p*_{beta_a}(x) (score != 0),
    // then k transitions T_{beta_c} (dbm.py:662-694).  `step` feeds the RNG call counter.
    const bool literal = h->ais_literal != 0;
    // literal mode: -log p*_{ba}(x) as its own score-only launches (the default path shares the pre-activations
    // of the transition and accumulates the DIFFERENCE of the two softplus terms per element, in double)
    auto score_only = [&](float bscore, int sign) -> int {
        for (int e = 0; e < S.ne; ++e) {
            const int li = S.ev[e];
            const LayerOut none{0, nullptr, nullptr, h->ae[e].ld, dkey(h, site_of(li), 0, seed, 0), chain0};
            issue(h, layer_pass(h, li, R, below_of(li), above_of(li), bscore, bscore, none)
                         .softplus_rows(h->apart_e[e].p, ldp, 0.f, bscore, 1));
        }
        hipLaunchKernelGGL(ais_score_literal_kernel, dim3((R + 255) / 256), dim3(256), 0, h->stream, h->alogw.p, R, ldp,
                           score_args(), bscore, sign);
        return 0;
    };
    auto visit = [&](bool score, float ba, float bb, bool transit, float bc, uint32_t step) -> int {
        if (literal && score) {                 // log_Z -= log p*_{ba}(x); log_Z += log p*_{bb}(x)   (:708, :714, :718, :728)
            BM_TRY(score_only(ba, -1));
            BM_TRY(score_only(bb, +1));
            score = false;
        }
        for (int t = 0; t < (transit ? k : 1); ++t) {
            const bool sc = score && t == 0;
            // even-depth layers given x: v~ <- sigma(beta*x W0^T + beta*vb), h2~ <- sigma(beta*(x1 W1 + x3 W2^T) + beta*hb1),
            // ... - and each layer's softplus term of log p*
            for (int e = 0; e < S.ne; ++e) {
                const int li = S.ev[e];
                const int smp = transit && (li < 0 ? h->cfg.sample_v_states : h->cfg.sample_h_states[li]);
                LayerPass p = layer_pass(h, li, R, below_of(li), above_of(li), bc, bc,
                                         value_out(smp, transit ? h->ae[e].p : nullptr, h->ae[e].ld, dkey(h, site_of(li), t, seed, step), chain0));
                if (sc) p.softplus_rows(h->apart_e[e].p, ldp, ba, bb, 0);
                issue(h, p);
            }
            if (sc)     // the softplus terms + (bb - ba) * x.hb, slots in fixed order, into the double log-weights
                hipLaunchKernelGGL(ais_score_kernel, dim3((R + 31) / 32), dim3(256), 0, h->stream, h->alogw.p, R, ldp,
                                   score_args(), bb - ba);
            if (!transit) break;
            // odd-depth layers given the new even-depth ones: x^ <- sigma(beta*(v W0 + h2 W1^T) + beta*hb0), ...; also
            // x^.hb for the next score
            for (int o = 0; o < S.no; ++o) {
                const int li = S.od[o];
                const LayerOut out{h->cfg.sample_h_states[li], nullptr, xn[o]->p, xn[o]->ld, dkey(h, site_of(li), t, seed, step), chain0};
                issue(h, layer_pass(h, li, R, below_of(li), above_of(li), bc, bc, out).statedot_rows(rdot_next[o], ldp, h->hb[li].p));
            }
            for (int o = 0; o < S.no; ++o) {
                Mat *tm = x[o]; x[o] = xn[o]; xn[o] = tm;
                float *tr = rdot_cur[o]; rdot_cur[o] = rdot_next[o]; rdot_next[o] = tr;
                nd_cur[o] = nslots(h->n[S.od[o] + 1]);
            }
        }
        return 0;
    };
    // x_1 ~ T_{db}(x_0)                                                     (:704-705)
    BM_TRY(visit(false, 0.f, 0.f, true, db, 0));
    // -log p_0(x_1), then the loop over beta = db, 2db, ... (fp32 accumulation, :710-726)
    float beta = db, prev = 0.f;
    uint32_t step = 1;
    while (beta < 1.0f - db + 1e-5f) {
        BM_TRY(visit(true, prev, beta, true, beta + db, step++));            // +log p_beta(x) -log p_prev(x); x' ~ T_{beta+db}
        prev = beta;
        beta = beta + db;
    }
    BM_TRY(visit(true, prev, 1.0f, false, 0.f, step++));                     // +log p_1(x_M) - log p_prev(x_M)  (:728)
    BM_CHECK(!h->failed, "bm_dbm: a device allocation failed inside a sweep (row store of a Multinomial layer)");
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_dbm_ais(bm_dbm *h, int32_t n_betas, int32_t n_runs, int32_t k, uint64_t seed, int64_t chain0,
               float *values_host) {
    BM_CHECK(values_host, "null output");
    BM_TRY(ais_core(h, n_betas, n_runs, k, seed, chain0));
    const int R = n_runs;
    std::vector<double> w(R);
    BM_HIP(hipMemcpyAsync(w.data(), h->alogw.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    const double logZ0 = ais_log_Z0(h, h->ais_literal != 0);
    if (h->ais_literal) {                        // log_Z += log_Z0 in float32 (:731-734)
        const float z0 = (float)logZ0;
        for (int r = 0; r < R; ++r) values_host[r] = (float)w[r] + z0;
    } else {
        for (int r = 0; r < R; ++r) values_host[r] = (float)(w[r] + logZ0);
    }
    return 0;
}

// values[r] = (float)(logw[r] + log Z_0) for r < n, 0 in the padding up to npad
__global__ void ais_finish_kernel(const double *logw, float *out, int n, int npad, double logZ0, int literal) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < npad) out[r] = (r < n) ? (literal ? (float)logw[r] + (float)logZ0 : (float)(logw[r] + logZ0)) : 0.f;
}

// Chain-sharded AIS: this rank runs chains [start, stop) of n_runs_total (contiguous slices, the
// remainder spread over the first ranks), no communication during the sweep, then ONE all-gather of the
// per-chain values over the library's communicator; every rank returns all n_runs_total values.
int bm_dbm_ais_sharded(bm_dbm *h, bm_comm *c, int32_t n_betas, int32_t n_runs_total, int32_t k, uint64_t seed,
                       float *values_host) {
    BM_CHECK(h && c && values_host, "null argument");
    int32_t rank = 0, world = 1;
    BM_TRY(bm_comm_rank(c, &rank, &world));
    BM_CHECK(n_runs_total >= 1, "bad AIS arguments");
    auto shard = [&](int r, int &a, int &b) {
        const int q = n_runs_total / world, rem = n_runs_total % world;
        a = r * q + (r < rem ? r : rem);
        b = a + q + (r < rem ? 1 : 0);
    };
    int a = 0, b = 0;
    shard(rank, a, b);
    const int n = b - a, npad = (n_runs_total + world - 1) / world;
    // send / receive buffers live in the handle (grown on demand, never on the steady path)
    if (h->ais_send.n < (size_t)npad) BM_TRY(h->ais_send.alloc((size_t)npad));
    if (h->ais_recv.n < (size_t)npad * world) BM_TRY(h->ais_recv.alloc((size_t)npad * world));
    float *send = h->ais_send.p, *recv = h->ais_recv.p;
    // A rank whose sweep fails must still enter the collective - the other ranks would block in it forever - so the
    // failure is made collective: the failing rank contributes NaNs and every rank reports the error.
    std::string first_err;
    int rc = 0;
    if (n > 0) rc = ais_core(h, n_betas, n, k, seed, a);
    if (rc) {
        first_err = bm_last_error();
        (void)hipGetLastError();
        std::vector<float> nan((size_t)npad, __builtin_nanf(""));
        (void)hipMemcpyAsync(send, nan.data(), nan.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
        (void)hipStreamSynchronize(h->stream);
    } else {
        const double z0 = ais_log_Z0(h, h->ais_literal != 0);
        hipLaunchKernelGGL(ais_finish_kernel, dim3((npad + 255) / 256), dim3(256), 0, h->stream, (const double *)h->alogw.p, send,
                           n, npad, z0, h->ais_literal);
    }
    const int rc_c = bm_comm_allgather(c, send, recv, (size_t)npad, (void *)h->stream);
    if (rc_c && first_err.empty()) first_err = bm_last_error();
    std::vector<float> all((size_t)npad * world);
    int rc_m = 0;
    if (!rc_c && hipMemcpyAsync(all.data(), recv, all.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc_m = 1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) rc_m = 1;
    if (rc || rc_c) { bm::set_error("bm_dbm_ais_sharded (rank %d): %s", rank, first_err.c_str()); return rc ? rc : rc_c; }
    if (rc_m) { bm::set_error("bm_dbm_ais_sharded: device copy / synchronisation failed"); return 1; }
    bool peer_failed = false;
    for (int r = 0; r < world; ++r) {
        int ra, rb;
        shard(r, ra, rb);
        memcpy(values_host + ra, all.data() + (size_t)r * npad, (size_t)(rb - ra) * sizeof(float));
        for (int e = ra; e < rb; ++e) if (values_host[e] != values_host[e]) { peer_failed = true; break; }
    }
    BM_CHECK(!peer_failed, "bm_dbm_ais_sharded: another rank's AIS sweep failed (its slice arrived as NaN)");
    return 0;
}

// the per-layer inputs of elbo_row_kernel: mu_l (pitch ld), its width, its bias, and the slot partials of
// sum((mu_{l-1} W_l) * mu_l) (mu_{-1} = X) from layer l's propagation
struct ElboLayers {
    const float *mu[MAXL]; int ld[MAXL], n[MAXL]; const float *hb[MAXL];
    const float *part[MAXL]; int nslot[MAXL];
    int L;
};

// per-row bias terms and entropies of the ELBO (dbm.py:746-756, every layer), one wave per row; the slot partials of
// the propagations (pitch ldp) are added layer after layer in slot order
__global__ __launch_bounds__(256) void elbo_row_kernel(const float *X, int ldx, int V, const float *vb, ElboLayers m,
                                                       int rows, int ldp, float *out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane; c < V; c += 64) s += X[(size_t)row * ldx + c] * vb[c];
#pragma unroll
    for (int l = 0; l < MAXL; ++l) {
        if (l >= m.L) break;
        for (int c = lane; c < m.n[l]; c += 64) {
            const float u = m.mu[l][(size_t)row * m.ld[l] + c];
            s += u * m.hb[l][c];
            const float q = fminf(fmaxf(u, 1e-7f), 1.f - 1e-7f);
            s += -q * logf(q) - (1.f - q) * logf(1.f - q);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        double e = 0.0;
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            if (l >= m.L) break;
            for (int q = 0; q < m.nslot[l]; ++q) e += (double)m.part[l][(size_t)q * ldp + row];
        }
        out[row] = (float)(e + (double)s);
    }
}

int bm_dbm_log_proba(bm_dbm *h, const float *X_dev, float *out_host) {
    for (int i = 0; i < h->L; ++i) BM_CHECK(!h->multinomial(i), "log_proba needs Bernoulli hidden layers (dbm.py:947-948)");
    BM_CHECK(out_host, "null output");
    BM_TRY(mean_field(h, X_dev, nullptr));
    BM_TRY(ensure_ais(h, h->N));
    // sum((X W0) * mu0), sum((mu0 W1) * mu1), ... as dot-epilogues of the layers' propagations (slot partials; the
    // AIS partial buffers, of which ensure_ais allocates at least L)
    const int ldp = h->ais_rows;
    DevBuf *parts[MAXL] = {&h->apart_e[0], &h->apart_e[1], &h->apart_o[0][0], &h->apart_o[0][1]};
    ElboLayers m;
    memset(&m, 0, sizeof(m));
    m.L = h->L;
    for (int l = 0; l < h->L; ++l) {
        const LayerIn below = l == 0 ? LayerIn{X_dev, h->V} : in_of(h->mu[l - 1]);
        issue(h, layer_pass(h, l, h->N, below, NO_IN, 1.f, 1.f, mean_out(h, nullptr, h->mu[l].ld)).zdot_rows(parts[l]->p, ldp, h->mu[l]));
        m.mu[l] = h->mu[l].p; m.ld[l] = h->mu[l].ld; m.n[l] = h->n[l + 1]; m.hb[l] = h->hb[l].p;
        m.part[l] = parts[l]->p; m.nslot[l] = nslots(h->n[l + 1]);
    }
    hipLaunchKernelGGL(elbo_row_kernel, dim3((h->N + 3) / 4), dim3(256), 0, h->stream, X_dev, h->V, h->V,
                       (const float *)h->vb.p, m, h->N, ldp, h->rowtmp.p);
    BM_HIP(hipMemcpyAsync(out_host, h->rowtmp.p, (size_t)h->N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    h->call++;
    return 0;
}

int bm_dbm_timer_start(bm_dbm *h) { BM_HIP(hipEventRecord(h->ev0, h->stream)); return 0; }
// the two halves of timer_stop: the mark is enqueued inside a timed region, the read (a host wait) after it
int bm_dbm_timer_mark(bm_dbm *h) { BM_HIP(hipEventRecord(h->ev1, h->stream)); return 0; }
int bm_dbm_timer_elapsed(bm_dbm *h, float *out_ms) {
    BM_HIP(hipEventSynchronize(h->ev1));
    BM_HIP(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return 0;
}
int bm_dbm_timer_stop(bm_dbm *h, float *out_ms) {
    BM_HIP(hipEventRecord(h->ev1, h->stream));
    BM_HIP(hipEventSynchronize(h->ev1));
    BM_HIP(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return 0;
}

}  // extern "C"
