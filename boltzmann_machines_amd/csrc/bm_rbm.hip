// bm_rbm.hip — C-ABI entry points for the RBM path (include/bm355.h) and the
// host-side sequencing of the fused kernels for one CD-k update.
//
// Reference graph restated: boltzmann_machines/rbm/base_rbm.py:415-525
// (train op + metrics), :329-413 (propagations, Gibbs chain), rbm/rbm.py:17-22,
// :101-116 (free energies, Gaussian input scaling), layers.py:39-51,73-89.
#include "../../include/bm355.h"
#include <cmath>
#include "bm_common.h"
#include "bm_kernels.h"
#include "bm_chain.h"
#include "bm_pass.h"
#include "bm_pt.h"
#include "bm_center.h"
#include "bm_fast.h"
#include "bm_class.h"
#include "bm_stack.h"
#include "bm_softmax_v.h"
#include "bm_rsm.h"
#include "bm_softmax_ais.h"
#include "bm_softmax_pt.h"
#include "bm_gauss.h"

#include <math.h>
#include <atomic>
#include <functional>
#include <memory>

namespace bm {

static thread_local char g_err[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// RNG site ids (counter word 2 = site + 16 * gibbs_step); DESIGN.md "RNG"
enum : uint32_t { SITE_DROPOUT = 1, SITE_H0 = 2, SITE_V = 3, SITE_H = 4, SITE_PLL = 5, SITE_FE = 6 };
// bm_rbm_ais (bm355.h): streams of their own, call = beta step, row offset = global chain index
enum : uint32_t { SITE_AIS_V0 = 7, SITE_AIS_V = 8, SITE_AIS_H = 9 };
// bm_rbm_pt_* (bm355.h): the swap uniforms (flat index = global chain * (R - 1) + ladder pair) and the random start v_0
enum : uint32_t { SITE_PT_SWAP = 10, SITE_PT_V0 = 11 };
// joint training of the classification RBM: the class draw of a Gibbs step (one uniform per global row), the
// Ber(1/2) start of bm_rbm_class_gibbs
enum : uint32_t { SITE_CLASS_Y = 12, SITE_CLASS_V0 = 13 };
// semi-supervised training: the start class y0 ~ p(y | x) of an unlabelled row's chain (one uniform per global row)
enum : uint32_t { SITE_CLASS_Y0 = 14 };

}  // namespace bm

using namespace bm;

struct bm_xchg;
// (bm_xchg.hip, later in this translation unit)
static int xchg_check_status(bm_xchg *x);                    // error when a wait of the exchange ever expired
static void xchg_bind_user(bm_xchg *x, bm_xchg **slot);      // the engine field that points at x (cleared by bm_xchg_destroy)
static void xchg_dw_replaced(bm_xchg *x);                    // every replica's dW was overwritten whole (set_param)

// the visible unit whose entries built the handle's tempered ensemble (bm_rbm::pt_unit)
enum PtUnit { PT_NONE = 0, PT_BERNOULLI, PT_GROUPS, PT_COUNTS, PT_GAUSS };

struct bm_rbm {
    bm_rbm_config cfg;
    bm_xchg *xchg_used = nullptr;     // the direct exchange this engine's gradients last went through (bm_rbm_sync checks it)
    // set by bm_rbm_exchange_apply_direct on more than one rank: every rank then holds only ITS slice of the momentum
    // buffer dW.  Cleared by bm_rbm_exchange_gather_dw (collective) and by a set_param of dW.  While it is set every
    // reader of dW - get_param, stage (checkpoints), apply_step and the single-GPU fused update - fails (check_dw)
    bool dw_sharded = false;
    int V, H, maxB;
    // (streams first: members are destroyed in reverse order, the buffers that run on a stream before it)
    Stream stream;
    Stream comm_stream;                // delayed data parallelism: the all-reduces (ensure_delayed)
    Stream stage_stream;               // bm_rbm_get_staged: the snapshot read-backs
    Event ev0, ev1;
    // variables (padded pitch, see pad_ld).  The prop-down reads W itself as an x-major operand (ActArgs::p_xm).
    Mat W, dW;                         // [V][H], [V][H]
    // the transpose [H][V], written by the fused update next to W: the prop-up then reads its weights x-major as well
    // (one ds_read_b128 per 16 k and lane instead of four ds_read_b32): 12.95 -> 12.5 us per prop-up, +0.45 us in the
    // update's epilogue (3.2 MB more stores): 64.1 -> 63.7 us per CD-1 update, same box, alternating runs
    // (tools/upxm_ab.sh; BM355_DEBUG=up_xm=0 switches it off).  Valid only while every write of W went through that kernel
    // (wt_valid: cleared by set_param, apply_step and the exchange); otherwise the prop-up reads W k-major as before.
    Mat Wt;
    bool use_wt = false, wt_valid = false;
    DevBuf vb, hb, dvb, dhb, q, sigma;
    // chain workspaces
    Mat h0m, h0s, hm, hs, hneg;        // [maxB][H]; hneg = -hm (negative-phase operand of the outer products)
    Mat vm, vs, Xs, Xd;                // [maxB][V]
    DevBuf grad;      // [V*ldH | V | H | H] raw sums (the data-parallel all-reduce buffer): the ACTIVE one of two
    // delayed-gradient data parallelism (bm_rbm_set_grad_slot / _allreduce_grads_async / _wait_grads): the buffer of
    // the other slot, the stream the reductions run on and their events; allocated at the first use of slot 1
    DevBuf grad_alt;
    int grad_slot = 0;
    Event ev_ready[2], ev_reduced[2];
    DevBuf pen;       // [H]
    // centred update (bm_rbm_set_centering): the offsets are variables ("ov", "oh", zero until set), the rest
    // is workspace allocated when the mode is first switched on
    bool cen_on = false;
    float cen_nu_v = 0.f, cen_nu_h = 0.f;
    DevBuf ov, oh;            // [V], [H]
    DevBuf cen_gv, cen_gh;    // [V], [H] plain bias gradients of the running update
    DevBuf cen_a;             // [4][maxB] row scalars: X, v_k, h0, h_k
    // fast-weights PCD (bm_rbm_set_fast_weights; bm_fast.h): the fast set and the effective copies We = W + Wf,
    // We^T (where the handle keeps W^T), vbe, hbe, allocated when the mode is first switched on and released when it goes off.
    // eff_valid is to the effective copies what wt_valid is to W^T: set by the fast-weights update, cleared by every other
    // writer of W, vb or hb; ensure_eff rebuilds them.  eff_now: the passes described and issued now read the effective set
    // (EffScope: bm_rbm_train_step_pt's tempered steps and negative means; nothing else ever does)
    bool fw_on = false, eff_valid = false, eff_now = false;
    float fw_lr = 0.f, fw_decay = 0.f;
    Mat Wf, We, Wet;
    DevBuf vbf, hbf, vbe, hbe;
    DevBuf rowacc;    // [3*maxB]
    DevBuf hhat;      // [3*H] MultinomialRBM free-energy h_hat vectors (rbm.py:58)
    DevArray<int> flip;
    DevArray<double> scal;    // [6] device accumulators: msre, l2, F(x), F(x~), F'(x) (multinomial), spare
    bool multinomial() const { return cfg.h_unit == BM_UNIT_MULTINOMIAL; }
    bool nrelu() const { return cfg.h_unit == BM_UNIT_NRELU; }      // noisy rectified-linear hidden units
    // softmax visible units (bm_rbm_set_visible_groups): the visible layer is V / v_groups one-hot groups of
    // v_groups units each; 0: off (Bernoulli visible units)
    int v_groups = 0;
    // incomplete rows (bm_rbm_groups_set_missing): run_chain() holds the empty groups of its input at zero.  gmask:
    // the clamp mask of the running chain, dense [maxB][V], allocated when the mode is first used
    bool groups_missing = false;
    DevBuf gmask;
    // bm_rbm_groups_scores: pre-activations [maxB][pad_ld(H)] and scores [maxB][V] of a slice, allocated at the first call;
    // nothing else in the handle reads or writes them
    Mat gs_z;
    DevArray<double> gs_out;
    // replicated softmax visible units (bm_rbm_set_replicated_softmax; bm_rsm.h): the visible layer is one softmax
    // over the V units drawn D_j times for row j; rsm_len = max_length, 0: off.  rsm_cur: the lengths [J] of the rows the passes
    // described now run on (issue() reads it) - rsm_D (computed from a batch by row_lengths_kernel), rsm_user (the caller's,
    // bm_rbm_set_row_lengths; rsm_user_n of them) or fer_len (bm_rbm_free_energy_rows).  rsm_bad: row_lengths_kernel's flag
    int rsm_len = 0, rsm_user_n = 0;
    const float *rsm_cur = nullptr;
    DevBuf rsm_D, rsm_user, fer_len;
    DevArray<int> rsm_bad;
    uint64_t seed = 0;
    uint32_t call = 0;
    int64_t row0 = 0;
    // input of the last run_chain() (after prep_input: /sigma and dropout) and its pitch
    const float *Xin = nullptr;
    int Xin_ld = 0;
    bool hm_is_neg = false;    // the last run_chain() wrote -h_k (hneg) instead of h_k (hm)
    bool fe_in_chain = false;  // the last run_chain() left the free-energy slot partials of its input in fe_part (metric fetch)
    DevBuf fe_part;            // [2][ceil(H/16)][maxB]: slot partials of sum softplus for x and for its PLL partner
    // bm_rbm_ais / bm_rbm_free_energy_rows: workspaces for `ais_rows` chains (rows), allocated on demand - max_batch does not
    // bound them
    int ais_rows = 0;
    Mat av, ah;                        // chain states [ais_rows][V], [ais_rows][H]
    DevBuf apart_h, apart_v;           // slot partials (ActArgs::rowacc / rowdot_out): [ceil(H/16)][ais_rows], [ceil(V/16)][ais_rows]
    DevArray<double> alogw;            // [ais_rows] log-weights, accumulated in double in a fixed order
    DevBuf abase, adot, abeta, atable; // a [V], vb - a [V], beta [n_betas], the mixed biases a + beta_k (vb - a) [n_betas][V]
    // bm_rbm_groups_ais, allocated at the first call: the run's pattern of absent groups and a row of zeros [V]
    // each, and - the generic route only - the logits / means [ga_rows][V] of its prop-down; nothing else reads or writes them
    DevBuf ga_absent, ga_zero;
    int ga_rows = 0;
    Mat ga_l;
    // bm_rbm_rsm_ais, allocated with the AIS workspaces at ra_rows == ais_rows rows: the logits of the run's
    // prop-downs [ra_rows][V], the chains' lengths [ra_rows] and the float32 pair of v.dvec [2][ra_rows]; nothing else reads or
    // writes them
    int ra_rows = 0;
    Mat ra_l;
    DevBuf ra_len, ra_dot;
    // The tempered ensemble of the handle (bm_pt.h; layers v and h1; bm_rbm_pt.hip), allocated on demand - max_batch
    // does not bound it; nothing else in the handle reads or writes it.  A handle holds at most one, and pt_unit says which visible
    // unit's entries built it (bm_rbm_pt_*, bm_rbm_groups_pt_*, bm_rbm_rsm_pt_*, bm_rbm_gauss_pt_*): PT_NONE while pt.M == 0 (pt_drop),
    // the family's tag once its *_pt_init went through; every other tempered entry asks for an ensemble of its own unit
    PtEnsemble pt;
    PtUnit pt_unit = PT_NONE;
    // the raw z = h W^T [ptz_rows][V] of the ensemble's prop-down where it takes more than one launch (the generic routes of the
    // groups and of the Gaussian unit, the count unit always), allocated with the ensemble; grows only (ensure_pt_z)
    int ptz_rows = 0;
    Mat pt_z;
    // bm_rbm_rsm_pt_* (DESIGN.md 3.31): the ensemble has a two-slot visible partial array; rp_len [rp_rows]: the document length of
    // every ensemble row (len[c R + r] = D_c); rp_clen [rp_rows]: the chains' lengths D_c, dense; rp_v0len: the row sums of a V0
    int rp_rows = 0;
    DevBuf rp_len, rp_clen, rp_v0len, rp_probe;      // (rp_probe: the row_mult of bm_debug_rsm_up)
    // Gaussian visible units as one joint model over u = x / sigma (bm_rbm_gauss_*; bm_gauss.h), allocated at the
    // first such call; nothing else in the handle reads or writes them.  gc / gones: the centre c = vb / sigma and a vector of ones
    // [V], formed again by every call (the parameters may have moved).  gfe_*: the scaled rows [gfe_rows][V], the softplus slot
    // partials [ceil(H/16)][gfe_rows] and F [gfe_rows] of bm_rbm_gauss_free_energy_rows.  gpt_sd [R]: the standard deviations of the
    // ladder of bm_rbm_gauss_pt_* (its ensemble is `pt` under the tag PT_GAUSS: bm_rbm_pt_* never see it)
    DevBuf gc, gones;
    int gfe_rows = 0;
    Mat gfe_u;
    DevBuf gfe_part;
    DevArray<double> gfe_out;
    DevBuf gpt_sd;
    int fer_rows = 0;
    DevBuf fer_part, fer_out;          // bm_rbm_free_energy_rows: slot partials [ceil(H/16)][fer_rows] of sum softplus, F [fer_rows]
    // fast-binary mode (bm_bf3.h, bm_rbm_set_fast_binary): bf16 planes of W ([V][H]: the prop-down operand) and of
    // W^T ([H][V]: the prop-up operand), bf16 shadows of the state workspaces hs / vs; `fast_now` while a sweep with
    // {0,1} states on both sides runs (bm_rbm_gibbs)
    int fast = 0;
    bool fast_now = false;
    Mat16 W3, W3t, hs16, vs16;
    DevArray<int> nonbinary;   // device flag: a state handed to the fast path was not a {0,1} bitmap
    // class head (bm_rbm_set_classes; bm_class.h): U [C][H] (dense), yb [C] and their momentum buffers are
    // variables; the rest is workspace for cls_rows rows (max_batch at set_classes, grown on demand by class_log_proba)
    int n_classes = 0, cls_rows = 0;
    DevBuf U, dU, yb, dyb;
    DevBuf cls_part;                   // [C][ceil(H/16)][cls_rows] slot partials of sum softplus(t + U[c])
    DevBuf cls_logp, cls_prob, cls_coef, cls_rowlp, cls_rowhit;      // [cls_rows][C] x 3, [cls_rows] x 2
    DevArray<int> cls_tl, cls_bad;     // [cls_rows] checked labels; the device flag a label outside [0, C) raises
    DevArray<double> cls_acc;          // [2] sums of log p(t|x) and of the hits
    // joint training of p(x, y), allocated at the first joint call: the chain's class draws and - the hybrid
    // objective's discriminative launches - workspaces of their own for t, pos and negm
    DevArray<int> cj_yk;               // [maxB]
    Mat cj_T, cj_pos, cj_negm;         // [maxB][H]
    // semi-supervised training, allocated at the first unlabelled call: the chain's start classes, the rows'
    // posterior entropy and max_c p(c|x), and their sums (t lives in cj_T)
    DevArray<int> cs_y0;               // [maxB]
    DevBuf cs_ent, cs_conf;            // [maxB]
    DevArray<double> cs_acc;           // [2]
    // the negative-phase visible operand of the fused update: vs, or - the class head's update - the input itself
    const float *neg_v = nullptr;
    int neg_v_ld = 0;
    // ... and its positive-phase hidden operand: h0m, or - the update of a layer below a class head - a delta
    const float *pos_h = nullptr;
    int pos_h_ld = 0;
    Event ev_stack;                    // the hand-over of a stack's launches from this handle's stream to the next handle's
    // bm_rbm_stage / bm_rbm_get_staged: device-side copies of every variable taken in stream order (a checkpoint
    // snapshot that does not stop the stream), read back on their own stream by whoever writes the checkpoint
    struct Stage { Mat W, dW; DevBuf vb, hb, dvb, dhb, q, sigma; Event ev; bool ready = false;
                   std::atomic<int> readers{0}; } stage[2];
    int last_stage = -1;
    Pinned<float> stage_host;        // pinned bounce buffer of bm_rbm_get_staged ([V][H])
    int device = 0;
    // bm_rbm_train_step_metrics_async: pinned ring of the six device sums of every pending metrics fetch
    static constexpr int MRING = 4096;
    Pinned<double> mring;                             // pinned host ring ...
    double *mring_dev = nullptr;                      // ... and its device-side address
    std::vector<int> mring_B;
    int mring_n = 0;
    Event ev_mlast;                  // behind the last pending fetch: bm_rbm_collect_metrics waits for IT, not for the stream -
                                     // updates queued after the fetch (the next epoch's first run) keep the device busy meanwhile
    // optional per-kernel-class event timing
    bool prof = false;
    struct Rec { int cls; Event a, b; };
    std::vector<Rec> recs;
    size_t grad_tail() const { return (size_t)V * W.ld; }
    // a run of dependent propagation passes recorded by issue() and launched as ONE launch (bm_chain.h)
    ChainState chain;
};

enum { KC_UP = 0, KC_DOWN = 1, KC_GRAD = 2, KC_COLSUM = 3, KC_BIAS = 4, KC_OTHER = 5 };

// the momentum buffer is complete on this rank (see bm_rbm::dw_sharded)
static int check_dw(const bm_rbm *h, const char *what) {
    BM_CHECK(!h->dw_sharded, "%s: after bm_rbm_exchange_apply_direct this rank holds only its slice of the momentum buffer dW; "
             "every rank must call bm_rbm_exchange_gather_dw first (DirectExchange.gather_dw())", what);
    return 0;
}

// no tempered ensemble any more (the buffers stay: PtEnsemble::ensure grows only)
static void pt_drop(bm_rbm *h) { h->pt.M = 0; h->pt_unit = PT_NONE; }

// what a handle with softmax visible units does not do (DESIGN.md 3.24 says why, entry by entry)
static int refuse_softmax_v(const bm_rbm *h, const char *what) {
    // ... and, at the same entries, one with replicated softmax visible units
    BM_CHECK(!h || !h->rsm_len, "%s is not available for replicated softmax visible units (bm_rbm_set_replicated_softmax: max_length %d): "
             "not built for word-count rows; see DESIGN.md 3.27", what, h->rsm_len);
    BM_CHECK(!h || !h->v_groups, "%s is not available for softmax visible units (bm_rbm_set_visible_groups: %d groups of %d): not "
             "built for one-hot groups; see DESIGN.md 3.24", what, h->V / h->v_groups, h->v_groups);
    return 0;
}
// what a handle with noisy rectified-linear hidden units does not do (DESIGN.md 3.23 says why, entry by entry) - and, at the
// same entries but the free energies (groups_ok), one with softmax visible units
static int refuse_nrelu(const bm_rbm *h, const char *what, bool groups_ok = false) {
    if (!groups_ok) BM_TRY(refuse_softmax_v(h, what));
    BM_CHECK(!h || !h->nrelu(), "%s is not available for NReLU hidden units (noisy rectified-linear, BM_UNIT_NRELU): the unit has no "
             "closed-form free energy and real-valued hidden states; see DESIGN.md 3.23", what);
    return 0;
}

struct ProfScope {
    bm_rbm *h; hipEvent_t b = nullptr;
    ProfScope(bm_rbm *h_, int cls) : h(h_) {
        if (!h->prof) return;
        bm_rbm::Rec r{cls};
        (void)create(r.a); (void)create(r.b);
        (void)hipEventRecord(r.a, h->stream);
        b = r.b;
        h->recs.push_back(std::move(r));
    }
    ~ProfScope() { if (b) (void)hipEventRecord(b, h->stream); }
};

static PhiloxKey make_key(const bm_rbm *h, uint32_t site, int t) {
    PhiloxKey k;
    k.k0 = (uint32_t)h->seed;
    k.k1 = (uint32_t)(h->seed >> 32);
    k.site = site + 16u * (uint32_t)t;
    k.call = h->call;
    return k;
}

// a chained run (bm_chain.h): the passes issue() sees between chain_begin and chain_end are recorded and launched as one
static void chain_begin(bm_rbm *h) {
    // per-class event timing, Multinomial hidden units (a softmax launch between the passes) and the fast-binary sweep
    // keep their per-pass launches
    // (noisy rectified-linear hidden units: their prop-up is a flavour of its own, never chained)
    // (softmax visible units: a softmax launch between the passes, as for Multinomial hidden units)
    // (replicated softmax visible units: the DB flavour and the count kernel, never chained)
    h->chain.on = !h->prof && !h->multinomial() && !h->nrelu() && !h->v_groups && !h->rsm_len && !h->fast_now && chain_mode(h->chain) > 0;
}
static int chain_end(bm_rbm *h) {
    BM_CHECK(chain_flush(h->chain, h->stream, h->maxB) == 0, "chained launch: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// W^T for the x-major prop-up when W was last written by something else than the fused update (set_param, a sampling-
// only handle): one transpose, valid until the next such write.  NOT called on the split (data-parallel) step, whose
// apply / exchange rewrites W every step.
static void ensure_wt(bm_rbm *h) {
    if (!h->use_wt || h->wt_valid) return;
    const int nt = ((h->V + 31) / 32) * ((h->H + 31) / 32);
    hipLaunchKernelGGL(transpose_kernel, dim3(nt), dim3(256), 0, h->stream, (const float *)h->W.p, h->W.ld, h->Wt.p, h->Wt.ld, h->V, h->H);
    h->wt_valid = true;
}

// fast-weights PCD: the effective copies We, We^T, vbe, hbe when something else than the fast-weights update last wrote W, vb
// or hb (or the fast set): one elementwise launch and - where the handle keeps W^T - one transpose, valid until the next such write
static void ensure_eff(bm_rbm *h) {
    if (!h->fw_on || h->eff_valid) return;
    FastRefreshArgs r;
    memset(&r, 0, sizeof(r));
    r.W = h->W.p; r.Wf = h->Wf.p; r.We = h->We.p; r.Wet = h->use_wt ? h->Wet.p : nullptr;
    r.V = h->V; r.H = h->H; r.ldw = h->W.ld; r.ldf = h->Wf.ld; r.ldet = h->Wet.ld;
    r.vb = h->vb.p; r.vbf = h->vbf.p; r.hb = h->hb.p; r.hbf = h->hbf.p; r.vbe = h->vbe.p; r.hbe = h->hbe.p;
    ProfScope _ps(h, KC_OTHER);
    launch_fast_refresh(r, h->stream);
    h->eff_valid = true;
}
// while one lives, rbm_pass() describes and issue() launches passes under the effective set of a fast-weights handle
// (a handle without the mode: no effect)
struct EffScope {
    bm_rbm *h;
    explicit EffScope(bm_rbm *h_) : h(h_) { h->eff_now = h->fw_on; }
    ~EffScope() { h->eff_now = false; }
};
// the parameter set the passes of now read
static const Mat &pass_w(const bm_rbm *h) { return h->eff_now ? h->We : h->W; }
static const float *pass_vb(const bm_rbm *h) { return h->eff_now ? h->vbe.p : h->vb.p; }
static const float *pass_hb(const bm_rbm *h) { return h->eff_now ? h->hbe.p : h->hb.p; }

// ---- a propagation pass as a value (bm_pass.h): rbm_pass() describes it, issue() launches it.  The RBM is the one-layer stack:
//   up   (layer 0):  E[h|v] (+ sample), base_rbm.py:339-351, from in = v [J][V]
//   down (layer -1): E[v|h] (+ sample), base_rbm.py:353-365, from in = h [J][H]
// Queues nothing, allocates nothing.  mult multiplies z and the bias: the handle's own (below) or a temperature (AIS).
static LayerPass rbm_pass(const bm_rbm *h, bool up, int J, LayerIn in, const LayerOut &out, float mult) {
    LayerPass p;
    ActArgs &a = p.a;
    memset(&a, 0, sizeof(ActArgs));
    p.layer = up ? 0 : -1; p.below = up ? in.p : nullptr; p.above = up ? nullptr : in.p;
    if (up) {
        a.P1 = make_operand(pass_w(h).p, pass_w(h).ld, h->H);   // W[k=v][i=h], k-major (issue() reads W^T x-major where the handle keeps it)
        a.K1 = h->V; a.I = h->H;
        a.bias = pass_hb(h); a.kind = BM_UNIT_BERNOULLI;  // (Multinomial hidden units: issue() turns the pass into the logits pair)
    } else {
        a.P1 = make_operand(pass_w(h).p, pass_w(h).ld, h->V);   // W[i=v][k=h], x-major P
        a.p_xm = 1;
        a.K1 = h->H; a.I = h->V;
        a.bias = pass_vb(h); a.sigma = h->sigma.p; a.kind = h->cfg.v_unit;
    }
    a.Q1 = make_operand(in.p, in.ld, J);              // in[j=b][k], x-major
    a.J = J;
    a.mult = mult; a.bmult = mult;
    a.sample = out.states ? out.sample : 0;           // no consumer of the states: no draw
    a.means = out.means; a.states = out.states; a.ldo = out.ld; a.key = out.key; a.row0 = out.row0;
    return p;
}
// the handle's own conditionals: the doubled pre-activation of a dbm_first (up) / dbm_last (down) layer
static LayerPass rbm_pass(const bm_rbm *h, bool up, int J, LayerIn in, const LayerOut &out) {
    return rbm_pass(h, up, J, in, out, 1.0f + ((up ? h->cfg.dbm_first : h->cfg.dbm_last) ? 1.0f : 0.0f));
}
// outputs drawn at the handle's seed, call counter and row offset
static LayerOut rbm_out(const bm_rbm *h, int sample, float *means, float *states, int ld, uint32_t site, int t) {
    return LayerOut{sample, means, states, ld, make_key(h, site, t), h->row0};
}

// everything that is about launching a pass, on h->stream: the one place that launches a propagation pass or records one
// into an open chained run
static void issue(bm_rbm *h, LayerPass p) {
    const bool up = p.layer == 0;
    ProfScope _ps(h, up ? KC_UP : KC_DOWN);
    ActArgs &a = p.a;
    // fast-binary: the bf16 planes of W^T (up) / W (down) x the bf16 shadow of the input bitmap, when that is the workspace
    // that carries one; the shadow of the output when the states go to the other workspace
    const bool fast = h->fast_now && (up ? p.below == h->vs.p : p.above == h->hs.p);
    if (fast) {
        const Mat16 &w3 = up ? h->W3t : h->W3, &in16 = up ? h->vs16 : h->hs16, &out16 = up ? h->hs16 : h->vs16;
        a.b3.P1 = Bf3Operand{w3.p, w3.plane_stride(), w3.ld, a.I};
        a.b3.Q1 = Bf3Operand{in16.p, 0, in16.ld, a.J};
        a.b3.K1 = in16.ld;
        if (a.states == (up ? h->hs.p : h->vs.p)) { a.states16 = out16.p; a.ld16 = out16.ld; }
    }
    if (up && h->multinomial()) {
        // MultinomialLayer (layers.py:54-70): logits from the GEMM, then one wave per row for the
        // softmax (activation) and the multinomial counts (sample)
        if (!a.means) { a.means = h->hm.p; a.ldo = h->hm.ld; }     // pure sampling sweep: hm is the scratch row store
        SmArgs m;
        memset(&m, 0, sizeof(m));
        m.L = a.means; m.ld = a.ldo; m.I = a.I; m.J = a.J; m.M = h->cfg.n_samples; m.sample = a.sample;
        m.states = a.states; m.negmeans = a.negmeans; m.key = a.key; m.row0 = a.row0;
        a.kind = 3; a.sample = 0; a.states = nullptr; a.negmeans = nullptr;
        launch_act(a, h->stream);
        hipLaunchKernelGGL(softmax_multinomial_kernel, dim3(a.J), dim3(64), 2 * (size_t)h->H * sizeof(float), h->stream, m);
        return;
    }
    if (!up && h->v_groups) {
        // softmax visible units.  Groups of 2, 4, 8 or 16 in a layer of V % 4 == 0: the SM flavour of the
        // prop-down, one launch (BM355_DEBUG=sm_fused=0 sends these shapes down the generic path as well: the same bits)
        static const bool fused_off = bm::dbg("sm_fused") && atoi(bm::dbg("sm_fused")) == 0;
        const int K = h->v_groups;
        if (!fused_off && (K == 2 || K == 4 || K == 8 || K == 16) && (a.I & 3) == 0) {
            a.kind = 3; a.sm_k = K;
            // (clamped groups, DESIGN.md 3.25: the SM + CL kernels are asked for by name; launch_act refuses the combination)
            if (a.clamp_mask) launch_act_sm_clamped(a, h->stream);
            else              launch_act(a, h->stream);
            return;
        }
        // every other shape: logits from the GEMM, in place of the means, then a lane per group for the softmax and the
        // one-hot draw
        SgArgs g;
        memset(&g, 0, sizeof(g));
        g.states = a.states; g.ld_states = a.ldo;
        // clamped groups: the clamp moves from the logits pass to the softmax kernel
        g.clamp_val = a.clamp_val; g.clamp_mask = a.clamp_mask; g.ld_clamp = a.ld_clamp;
        a.clamp_val = a.clamp_mask = nullptr; a.ld_clamp = 0;
        if (!a.means) { a.means = h->vm.p; a.ldo = h->vm.ld; }     // pure sampling sweep: vm is the scratch row store
        g.L = a.means; g.ld = a.ldo; g.V = a.I; g.K = h->v_groups; g.J = a.J; g.sample = a.sample; g.key = a.key; g.row0 = a.row0;
        a.kind = 3; a.sample = 0; a.states = nullptr;
        launch_act(a, h->stream);
        launch_softmax_groups(g, h->stream);
        return;
    }
    if (!up && h->rsm_len) {
        // replicated softmax visible units: logits from the GEMM, in place of the means, then a workgroup per
        // row for the softmax over the whole layer and the row's D_j draws (bm_rsm.h)
        McArgs m;
        memset(&m, 0, sizeof(m));
        m.states = a.states; m.ld_states = a.ldo;
        if (!a.means) { a.means = h->vm.p; a.ldo = h->vm.ld; }     // pure sampling sweep: vm is the scratch row store
        m.L = a.means; m.ld = a.ldo; m.lengths = h->rsm_cur; m.V = a.I; m.J = a.J; m.sample = a.sample; m.max_length = h->rsm_len;
        m.key = a.key; m.row0 = a.row0;
        a.kind = 3; a.sample = 0; a.states = nullptr;
        launch_act(a, h->stream);
        if (launch_multinomial_counts(m, h->stream)) abort();      // (bm_rbm_set_replicated_softmax checked the width)
        return;
    }
    // ... and their prop-up: the DB flavour scales the bias alone by the row's length (a pass that brings lengths of its own - the
    // chains of bm_rbm_rsm_ais - keeps them)
    if (up && h->rsm_len && !a.row_bmult) a.row_bmult = h->rsm_cur;
    // noisy rectified-linear hidden units: the NR flavour rectifies t = z + b (formed as kind 3 forms it) and draws a normal
    if (up && h->nrelu()) { a.kind = 3; a.nrelu = 1; }
    // the prop-up's weights x-major: W^T where the handle keeps a valid one (ensure_wt), never beside the bf16 planes
    // (a pass under the effective set of a fast-weights handle, EffScope: We^T, valid with the effective copies)
    const bool xm = up && h->use_wt && (h->eff_now ? h->eff_valid : h->wt_valid) && !fast;
    const Mat &wtm = h->eff_now ? h->Wet : h->Wt;
    const Operand wt = xm ? make_operand(wtm.p, wtm.ld, h->H) : Operand{nullptr, 0, 0, 0};     // W^T[i=h][k=v]
    if (h->chain.on) {          // a chained run is open: recorded with W k-major, W^T as the per-pass launch's alternative
        if (a.cb_y) { fprintf(stderr, "bm355: a class-bias pass does not ride in a chained launch (no such kernel)\n"); abort(); }
        h->chain.rec.push_back(a);
        h->chain.alt_p.push_back(wt);
        return;
    }
    if (xm) { a.P1 = wt; a.p_xm = 1; }
    launch_act(a, h->stream);
}

// Gaussian visibles: X / sigma (rbm.py:107); then dropout (base_rbm.py:417-418).  *Xin / *ldx: what the passes read
static void prep_input(bm_rbm *h, const float *X_dev, int B, const float **Xin, int *ldx, bool *dropped) {
    *Xin = X_dev; *ldx = h->V; *dropped = false;
    if (h->cfg.v_unit == BM_UNIT_GAUSSIAN) {
        hipLaunchKernelGGL(div_cols_kernel, dim3(256), dim3(256), 0, h->stream, *Xin, *ldx, h->sigma.p, h->Xs.p,
                           h->Xs.ld, B, h->V);
        *Xin = h->Xs.p; *ldx = h->Xs.ld;
    }
    if (h->cfg.dropout >= 0.f) {
        hipLaunchKernelGGL(dropout_kernel, dim3(256), dim3(256), 0, h->stream, *Xin, *ldx, h->Xd.p, h->Xd.ld, B, h->V,
                           h->cfg.dropout, make_key(h, SITE_DROPOUT, 0),
                           (unsigned long long)h->row0 * (unsigned long long)h->V);
        *Xin = h->Xd.p; *ldx = h->Xd.ld;
        *dropped = true;
    }
}

// input preprocessing + h0 + k Gibbs steps (base_rbm.py:417-426). Leaves
// h0m/h0s, vm/vs (last step), hm/hs (last step) and Xin in the handle.
struct ChainOpts {
    // the last step's visible MEANS are wanted (msre metric); a plain update only consumes the
    // visible states, and nothing consumes the hidden STATES of the last step: those stores (and their
    // share of the kernel-boundary L2 writeback) are skipped.
    bool need_vm = true;
    bool split_step = false;      // the data-parallel step: W^T is not rebuilt (ensure_wt)
    bool fetch = false;           // a metrics iteration (metrics_from_chain follows)
    float *hm_out = nullptr;      // the last step's h_means are written there (dense, pitch H)
};
static bool metrics_fused_ok(const bm_rbm *h);
static void metrics_prep(bm_rbm *h, int B);
// replicated softmax: the lengths D [B] of the count rows X (pitch ldx) into `D`, which the passes issued from
// now on read; a row that is no count vector of 1 .. max_length tokens raises the handle's flag (check_row_lengths)
static void rsm_lengths_of(bm_rbm *h, const float *X, int ldx, int B, float *D) {
    RowLenArgs r{X, ldx, h->V, B, D, h->rsm_len, h->rsm_bad.p};
    launch_row_lengths(r, h->stream);
    h->rsm_cur = D;
}
static int run_chain(bm_rbm *h, const float *X_dev, int B, int k, const ChainOpts &o) {
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", k);
    if (!o.split_step) ensure_wt(h);
    const float *Xin;
    int ldx;
    bool dropped;
    prep_input(h, X_dev, B, &Xin, &ldx, &dropped);
    h->Xin = Xin; h->Xin_ld = ldx;
    // replicated softmax: the batch's lengths, once; every pass of the chain keeps them (each prop-down draws exactly D_b tokens)
    if (h->rsm_len) rsm_lengths_of(h, Xin, ldx, B, h->rsm_D.p);
    // a metrics iteration: the flip columns and the zeroed accumulators first, then the h0 pass adds the free-energy row
    // sums of x and of its PLL partner from its own pre-activations (ActArgs::fe_flip) - no GEMM of their own
    const bool fe = o.fetch && metrics_fused_ok(h);
    const int fe_rm = (((h->H + 15) / 16) + 3) & ~3;
    if (fe && !h->fe_part.p) BM_TRY(h->fe_part.alloc((size_t)2 * fe_rm * h->maxB));
    h->fe_in_chain = fe;
    if (o.fetch && !fe) metrics_prep(h, B);
    // incomplete rows: the mask of the input's empty groups; every prop-down of the chain holds them at the
    // input's own zeros (one pitch for values and mask: V, the input's).  The training and metric chains only: bm_rbm_transform
    // (hm_out) runs the plain chain
    const bool missing = h->groups_missing && h->v_groups && !o.hm_out;
    if (missing) {
        if (!h->gmask.p) BM_TRY(h->gmask.alloc((size_t)h->maxB * h->V));
        launch_group_missing_mask(Xin, ldx, h->gmask.p, h->V, B, h->V, h->v_groups, h->stream);
    }
    chain_begin(h);               // h0 and the k Gibbs steps: one launch where the shape allows it (bm_chain.h)
    LayerPass h0 = rbm_pass(h, true, B, LayerIn{Xin, ldx}, rbm_out(h, 1, h->h0m.p, h->h0s.p, h->h0m.ld, SITE_H0, 0));     // :421-422
    // the flip columns straight from their Philox stream and the zeroing of the six accumulators ride on this pass: the
    // fused fetch has no prep launch
    if (fe) h0.free_energy_fetch(h->fe_part.p, fe_rm, h->maxB, make_key(h, SITE_PLL, 0), h->scal.p, Xin, ldx, h->W.p, h->W.ld);
    issue(h, h0);
    LayerIn hstate = in_of(h->cfg.sample_h_states ? h->h0s : h->h0m);             // :423
    for (int t = 0; t < k; ++t) {                                                 // :367-378
        const bool last = t == k - 1;
        LayerPass down = rbm_pass(h, false, B, hstate, rbm_out(h, h->cfg.sample_v_states, (o.need_vm && last) ? h->vm.p : nullptr, h->vs.p,
                                                               h->vs.ld, SITE_V, t));
        if (missing) down.clamp(Xin, h->gmask.p, h->V);
        issue(h, down);
        const bool last_out = o.hm_out && last;
        // plain update, last step: only -h_k is consumed (outer products and column sums)
        const bool neg_only = last && !o.hm_out && !o.need_vm && !h->multinomial();
        h->hm_is_neg = neg_only;
        LayerPass up = rbm_pass(h, true, B, in_of(h->vs),
                                rbm_out(h, h->cfg.sample_h_states, last_out ? o.hm_out : (neg_only ? nullptr : h->hm.p),
                                        last ? nullptr : h->hs.p, last_out ? h->H : h->hm.ld, SITE_H, t));
        if (!o.hm_out && last) up.negmeans_out(h->hneg.p);
        issue(h, up);
        hstate = in_of(h->hs);
    }
    BM_TRY(chain_end(h));
    return 0;
}

static void fill_bias(bm_rbm *h, float N, float lr, float mom, RbmBiasArgs &b) {
    float *tail = h->grad.p + h->grad_tail();
    b.sv = tail; b.sh = tail + h->V; b.sq = tail + h->V + h->H;
    b.vb = h->vb.p; b.dvb = h->dvb.p; b.hb = h->hb.p; b.dhb = h->dhb.p; b.q = h->q.p; b.pen = h->pen.p;
    b.V = h->V; b.H = h->H;
    b.N = N; b.lr = lr; b.mom = mom;
    b.damping = h->cfg.sparsity_damping; b.cost = h->cfg.sparsity_cost; b.target = h->cfg.sparsity_target;
}

// single-GPU path: column sums + bias/q update in ONE launch (or inside the grad launch)
static int fill_bias_fused(bm_rbm *h, int B, float lr, float mom, RbmBiasFusedArgs &a) {
    memset(&a, 0, sizeof(a));
    a.X = h->Xin; a.ldx = h->Xin_ld;
    a.vs = h->neg_v ? h->neg_v : h->vs.p; a.ldv = h->neg_v ? h->neg_v_ld : h->vs.ld;
    a.h0m = h->pos_h ? h->pos_h : h->h0m.p; a.ldh0 = h->pos_h ? h->pos_h_ld : h->h0m.ld; a.B = B;
    // the last up-pass of a plain update leaves only -h_k behind (run_chain)
    if (h->hm_is_neg) { a.hm = h->hneg.p; a.ldh = h->hneg.ld; a.hm_negated = 1; }
    else              { a.hm = h->hm.p; a.ldh = h->hm.ld; }
    a.raw_tail = h->grad.p + h->grad_tail();
    fill_bias(h, (float)B, lr, mom, a.u);     // (sv / sh / sq are not read: the kernel forms the sums itself, into raw_tail)
    return (h->V + 63) / 64 + (h->H + 63) / 64;
}

static void launch_bias_fused(bm_rbm *h, int B, float lr, float mom) {
    ProfScope _ps(h, KC_COLSUM);
    RbmBiasFusedArgs a;
    const int nw = fill_bias_fused(h, B, lr, mom, a);
    hipLaunchKernelGGL(rbm_bias_fused_kernel, dim3(nw), dim3(NT), 0, h->stream, a);
}

static void rbm_grad(bm_rbm *h, int B, int fused, float N, float lr, float mom, bool with_bias, bool fast_weights = false);
static void launch_update_centred(bm_rbm *h, int B, float lr, float mom);
static void launch_update_fast(bm_rbm *h, int B, float lr, float mom);

// whole parameter update of the fused single-GPU step (base_rbm.py:443-478)
static void launch_update_fused(bm_rbm *h, int B, float lr, float mom) {
    if (h->cen_on) { launch_update_centred(h, B, lr, mom); return; }
    if (h->rsm_len) {
        // replicated softmax: the bias block with the hidden sums weighted by the batch's lengths in front, then
        // the unchanged grad_kernel without its bias tail - the launch order of a handle with a sparsity penalty (pen is zero)
        {
            ProfScope _ps(h, KC_COLSUM);
            RbmBiasFusedArgs a;
            fill_bias_fused(h, B, lr, mom, a);
            launch_rsm_bias(a, h->rsm_D.p, h->stream);
        }
        rbm_grad(h, B, 1, (float)B, lr, mom, false);
        return;
    }
    if (h->cfg.sparsity_cost != 0.f) {      // W update needs the penalty: bias kernel first
        launch_bias_fused(h, B, lr, mom);
        rbm_grad(h, B, 1, (float)B, lr, mom, false);
    } else {                                // penalty == 0: run both in one launch
        rbm_grad(h, B, 1, (float)B, lr, mom, true);
    }
}

// The fast-weights form of launch_update_fused: the regular update exactly as there, its grad launch in the
// fast-weights flavour (Wf, We, We^T ride on it); behind it the fast bias update from the raw column sums the update published
static void launch_update_fast(bm_rbm *h, int B, float lr, float mom) {
    if (h->cfg.sparsity_cost != 0.f) {
        launch_bias_fused(h, B, lr, mom);
        rbm_grad(h, B, 1, (float)B, lr, mom, false, true);
    } else {
        rbm_grad(h, B, 1, (float)B, lr, mom, true, true);
    }
    ProfScope _ps(h, KC_BIAS);
    FastBiasArgs b;
    memset(&b, 0, sizeof(b));
    const float *tail = h->grad.p + h->grad_tail();
    b.sv = tail; b.sh = tail + h->V;
    b.vb = h->vb.p; b.hb = h->hb.p; b.vbf = h->vbf.p; b.hbf = h->hbf.p; b.vbe = h->vbe.p; b.hbe = h->hbe.p;
    b.V = h->V; b.H = h->H; b.N = (float)B; b.fast_lr = h->fw_lr; b.fast_decay = h->fw_decay;
    launch_fast_bias(b, h->stream);
    h->eff_valid = true;
}

static void fill_grad(bm_rbm *h, int B, int fused, float N, float lr, float mom, GradArgs &g) {
    memset(&g, 0, sizeof(g));
    g.Ppos = h->pos_h ? make_operand(h->pos_h, h->pos_h_ld, h->H)      // (a layer below a class head: its delta)
                      : make_operand(h->h0m.p, h->h0m.ld, h->H);       // h0 means [k=b][i=h]           :447
    g.Qpos = make_operand(h->Xin, h->Xin_ld, h->V);     // X        [k=b][j=v]
    g.Kpos = B;
    g.Pneg = make_operand(h->hneg.p, h->hneg.ld, h->H); // -(h_k means): the chain subtracts  :448
    g.Qneg = h->neg_v ? make_operand(h->neg_v, h->neg_v_ld, h->V)      // (the class head's update: the input itself)
                      : make_operand(h->vs.p, h->vs.ld, h->V);         // v_k states
    g.Kneg = B;
    g.I = h->H; g.J = h->V;
    g.form = 0; g.fused = fused;
    g.raw = h->grad.p; g.raw2 = nullptr;
    g.W = h->W.p; g.dW = h->dW.p; g.Wt = nullptr;
    g.ldw = h->W.ld; g.ldwt = 0;
    if (h->use_wt && fused) { g.Wt = h->Wt.p; g.ldwt = h->Wt.ld; }
    g.N = N; g.M = N; g.l2 = h->cfg.l2; g.lr = lr; g.mom = mom;
}
static void rbm_grad(bm_rbm *h, int B, int fused, float N, float lr, float mom, bool with_bias, bool fast_weights) {
    ProfScope _ps(h, KC_GRAD);
    GradArgs g;
    fill_grad(h, B, fused, N, lr, mom, g);
    g.pen = with_bias ? nullptr : h->pen.p;
    if (with_bias) {
        g.nbias = fill_bias_fused(h, B, lr, mom, g.bias);
        g.bias.raw_only = fused ? 0 : 1;      // split (data-parallel) step: raw column sums only
    }
    if (fast_weights) {           // (fused, never centred: bm_rbm_set_fast_weights refuses a centred handle)
        const GradFast f{h->Wf.p, h->We.p, h->use_wt ? h->Wet.p : nullptr, h->Wf.ld, h->Wet.ld, h->fw_lr, h->fw_decay};
        bm::launch_grad(g, h->stream, nullptr, &f);
    } else if (h->cen_on && fused) {
        const GradCen cen{h->ov.p, h->cen_gv.p, h->oh.p, h->cen_gh.p};
        bm::launch_grad(g, h->stream, &cen);
    } else bm::launch_grad(g, h->stream);
    h->eff_valid = false;         // (launch_update_fast sets it once the fast bias update is queued as well)
    if (fused && h->use_wt) h->wt_valid = true;      // the fused update wrote W and W^T together (every other writer of W
                                                     // clears the flag: set_param, apply_step, the exchange)
}

// The centred form of launch_update_fused, four launches in stream order:
//   1. column sums, raw tail, plain bias gradients g_v / g_h, offsets o_v / o_h   (rbm_cen_stats_kernel)
//   2. row scalars a = (x - o).o of X, v_k, h0, h_k under the NEW offsets          (cen_rowscal_kernel)
//   3. bias corrections r_v / r_h + the bias / q_means / penalty update            (cen_bias_kernel)
//   4. outer products + centred W update                                           (grad_kernel, CEN flavour, no bias tail)
static void launch_update_centred(bm_rbm *h, int B, float lr, float mom) {
    const float *hk = h->hm_is_neg ? h->hneg.p : h->hm.p;      // the last prop-up may have left only -h_k: read negated (exact)
    const int ldhk = h->hm_is_neg ? h->hneg.ld : h->hm.ld, hk_neg = h->hm_is_neg ? 1 : 0;
    float *aX = h->cen_a.p, *av = aX + h->maxB, *ah0 = av + h->maxB, *ahk = ah0 + h->maxB;
    {
        ProfScope _ps(h, KC_COLSUM);
        RbmCenStatsArgs s;
        memset(&s, 0, sizeof(s));
        s.X = h->Xin; s.ldx = h->Xin_ld; s.vs = h->vs.p; s.ldv = h->vs.ld;
        s.h0m = h->h0m.p; s.ldh0 = h->h0m.ld; s.hm = hk; s.ldh = ldhk; s.hm_negated = hk_neg;
        s.B = B; s.V = h->V; s.H = h->H;
        s.raw_tail = h->grad.p + h->grad_tail();
        s.ov = h->ov.p; s.oh = h->oh.p; s.gv = h->cen_gv.p; s.gh = h->cen_gh.p;
        s.nu_v = h->cen_nu_v; s.nu_h = h->cen_nu_h; s.N = (float)B;
        hipLaunchKernelGGL(rbm_cen_stats_kernel, dim3((h->V + 63) / 64 + (h->H + 63) / 64), dim3(NT), 0, h->stream, s);
        CenRowArgs r;
        memset(&r, 0, sizeof(r));
        r.job[0] = CenRowJob{h->Xin, h->ov.p, aX, h->Xin_ld, B, h->V, 0};
        r.job[1] = CenRowJob{h->vs.p, h->ov.p, av, h->vs.ld, B, h->V, 0};
        r.job[2] = CenRowJob{h->h0m.p, h->oh.p, ah0, h->h0m.ld, B, h->H, 0};
        r.job[3] = CenRowJob{hk, h->oh.p, ahk, ldhk, B, h->H, hk_neg};
        r.njobs = 4;
        launch_cen_rowscal(r, h->stream);
    }
    {
        ProfScope _ps(h, KC_BIAS);
        CenBiasArgs b;
        memset(&b, 0, sizeof(b));
        b.N = B; b.M = B; b.njobs = 2;
        CenBiasJob &jv = b.job[0], &jh = b.job[1];
        jv.pos = h->Xin; jv.ldp = h->Xin_ld; jv.neg = h->vs.p; jv.ldn = h->vs.ld; jv.n = h->V;
        jv.wp1 = ah0; jv.wn1 = ahk; jv.o = h->ov.p; jv.g = h->cen_gv.p;
        jh.pos = h->h0m.p; jh.ldp = h->h0m.ld; jh.neg = hk; jh.ldn = ldhk; jh.neg_negated = hk_neg; jh.n = h->H;
        jh.wp0 = aX; jh.wn0 = av; jh.o = h->oh.p; jh.g = h->cen_gh.p;
        jv.rbm = jh.rbm = 1; jh.rbm_hidden = 1;
        fill_bias(h, (float)B, lr, mom, jv.r);
        jh.r = jv.r;
        launch_cen_bias(b, h->stream);
    }
    rbm_grad(h, B, 1, (float)B, lr, mom, false);
}

static void launch_fe(bm_rbm *h, const float *Xin, int ldx, int B, bool with_flip) {
    FeArgs f;
    memset(&f, 0, sizeof(f));
    f.P = make_operand(h->W.p, h->W.ld, h->H);
    f.Q = make_operand(Xin, ldx, B);
    f.K = h->V; f.I = h->H; f.J = B;
    f.hb = h->hb.p;
    f.rowacc = h->rowacc.p;
    if (with_flip) { f.rowacc2 = h->rowacc.p + h->maxB; f.flip_col = h->flip.p; }
    if (h->multinomial()) {                    // rbm.py:52-62: fresh h_hat draws, streams t = 0, 1, 2
        (void)hipMemsetAsync(h->hhat.p, 0, 3 * (size_t)h->H * sizeof(float), h->stream);
        const int M = h->cfg.n_samples;
        hipLaunchKernelGGL(mn_hhat_kernel, dim3((M + 255) / 256), dim3(256), 0, h->stream, h->hhat.p, h->H, M,
                           make_key(h, SITE_FE, 0), make_key(h, SITE_FE, 1), make_key(h, SITE_FE, 2));
        f.hvec = h->hhat.p;
        f.rowacc3 = h->rowacc.p + 2 * (size_t)h->maxB;
    }
    launch_fe_hidden(f, h->stream);
    FeRowArgs r;
    memset(&r, 0, sizeof(r));
    r.X = Xin; r.ld = ldx; r.V = h->V; r.B = B;
    r.vb = h->vb.p; r.sigma = (h->cfg.v_unit == BM_UNIT_GAUSSIAN) ? h->sigma.p : nullptr;
    r.rowacc = f.rowacc; r.rowacc2 = f.rowacc2; r.rowacc3 = f.rowacc3; r.flip_col = f.flip_col; r.out = h->scal.p + 2;
    hipLaunchKernelGGL(fe_row_kernel, dim3((B + FE_ROWS_PER_WG - 1) / FE_ROWS_PER_WG), dim3(256), 0, h->stream, r);
}

// -lgamma(M + K) + lgamma(M + 1) + lgamma(K)  (rbm.py:61); 0 for the other RBMs
static double mn_fe_const(const bm_rbm *h) {
    if (!h->multinomial()) return 0.0;
    const double M = h->cfg.n_samples, K = h->H;
    return -lgamma(M + K) + lgamma(M + 1.0) + lgamma(K);
}

// metrics from the chain currently in the handle (base_rbm.py:482-517)
static void metrics_to_out4(const bm_rbm *h, const double *host, int B, float *out4);
// The h0 pass can carry the free-energy sums when its pre-activation IS the free energy's (no dbm_first doubling), the hidden
// units are Bernoulli and the epilogue in use is act_kernel's (not the fast-binary strip kernel)
static bool metrics_fused_ok(const bm_rbm *h) {
    static const bool off = bm::dbg("metrics_fused") && atoi(bm::dbg("metrics_fused")) == 0;
    // (replicated softmax: the h0 pass is a DB pass, which carries no metric fetch)
    return !off && !h->multinomial() && !h->nrelu() && !h->rsm_len && !h->cfg.dbm_first && !h->fast_now && (h->W.ld & 3) == 0;
}
static void metrics_prep(bm_rbm *h, int B) {
    MetricsPrepArgs mp;
    mp.scal = h->scal.p; mp.rowacc = h->rowacc.p; mp.n_rowacc = 3 * h->maxB; mp.flip = h->flip.p; mp.B = B; mp.V = h->V;
    mp.key = make_key(h, SITE_PLL, 0); mp.row0 = (unsigned long long)h->row0;
    hipLaunchKernelGGL(metrics_prep_kernel, dim3(8), dim3(256), 0, h->stream, mp);
}
// the rest of the fetch, behind a run_chain(..., fetch = true): squared sums, the visible terms of the free energies
static int metrics_from_chain(bm_rbm *h, int B, float *out4) {
    const SqJob msre{h->Xin, h->Xin_ld, h->vm.p, h->vm.ld, B, h->V, h->scal.p + 0};                        // :486-488
    const SqJob l2{h->W.p, h->W.ld, nullptr, 0, h->V, h->H, h->scal.p + 1};                                 // :482-484
    if (h->fe_in_chain) {       // the hidden terms are in fe_part already: squared sums and the row sums as ONE launch
        FeRowArgs r;
        memset(&r, 0, sizeof(r));
        r.X = h->Xin; r.ld = h->Xin_ld; r.V = h->V; r.B = B;
        r.vb = h->vb.p; r.sigma = (h->cfg.v_unit == BM_UNIT_GAUSSIAN) ? h->sigma.p : nullptr;
        r.nslot = (h->H + 15) / 16; r.ld_part = (r.nslot + 3) & ~3;
        r.rowacc = h->fe_part.p; r.rowacc2 = h->fe_part.p + (size_t)r.ld_part * h->maxB; r.out = h->scal.p + 2;
        r.flip_col = nullptr; r.has_key = 1; r.key = make_key(h, SITE_PLL, 0); r.row0 = (unsigned long long)h->row0;
        const int nb_sq = 256, nb_fe = (B + FE_ROWS_PER_WG - 1) / FE_ROWS_PER_WG;
        hipLaunchKernelGGL(metrics_tail_kernel, dim3(nb_sq + nb_fe), dim3(256), 0, h->stream, msre, l2, r, nb_sq);
    } else {
        hipLaunchKernelGGL(sqdiff2_kernel, dim3(256), dim3(256), 0, h->stream, msre, l2);
        // (NReLU: no free energy in closed form, pll / feg are NaN; replicated softmax: fe_hidden_kernel has no length-scaled bias)
        if (!h->nrelu() && !h->rsm_len) launch_fe(h, h->Xin, h->Xin_ld, B, true);
    }
    if (!out4) return 0;                                    // asynchronous caller: the sums stay in h->scal
    double host[6];
    BM_HIP(hipMemcpyAsync(host, h->scal.p, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    metrics_to_out4(h, host, B, out4);
    return 0;
}
static void metrics_to_out4(const bm_rbm *h, const double *host, int B, float *out4) {
    // MultinomialRBM: every _free_energy() call draws its own h_hat (host[4] = F(x) of the PLL pair)
    // and carries the constant of rbm.py:61 (it cancels in the PLL difference)
    const double fe = host[2] / B + mn_fe_const(h), fe1 = h->multinomial() ? host[4] / B + mn_fe_const(h) : fe;
    const double fe2 = host[3] / B + mn_fe_const(h);
    out4[0] = (float)(host[0] / ((double)B * h->V));            // msre          :487
    const float d = (float)(fe2 - fe1);                         // pll           :511-512
    const float ls = -(fmaxf(-d, 0.f) + log1pf(expf(-fabsf(d))));
    out4[1] = (float)h->V * ls;
    out4[2] = h->cfg.l2 * (float)(0.5 * host[1]);               // l2_loss       :483
    out4[3] = (float)fe;                                        // free energy   :516
    if (h->nrelu()) out4[1] = out4[3] = nanf("");               // noisy rectified-linear hidden units: neither exists in closed form
    if (h->v_groups) out4[1] = nanf("");                        // softmax visible units: a row with one bit flipped is no state of the model
    if (h->rsm_len) out4[1] = out4[3] = nanf("");               // replicated softmax: the same; the free energy is bm_rbm_free_energy_rows'
}

// ---- AIS log Z of the RBM itself and per-row free energies (bm355.h: bm_rbm_ais, bm_rbm_free_energy_rows)

// dvec = vb - a and the mixed visible biases of every temperature, table[k][i] = a_i + beta_k (vb_i - a_i): one launch in
// front of the beta loop, so that no pass of the loop waits for the host
__global__ void rbm_ais_prep_kernel(const float *vb, const float *abase, const float *beta, int n_betas, int V, float *dvec, float *table) {
    const size_t n = (size_t)n_betas * V;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t k = e / (size_t)V, i = e % (size_t)V;
        const float d = vb[i] - abase[i];
        if (k == 0) dvec[i] = d;
        table[e] = abase[i] + beta[k] * d;
    }
}

// v_0 ~ Ber(sigmoid(a)) and the slot partials of v_0.(vb - a) for the first score: the whole dot product in slot 0 (one wave per
// row, lane-strided sums + butterfly: a fixed order), zeros in the other slots
__global__ __launch_bounds__(256) void rbm_ais_init_kernel(float *v, int ld, int rows, int V, const float *abase, const float *dvec,
                                                           PhiloxKey key, unsigned long long row0, float *part, int ld_part, int nslot) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane; c < V; c += 64) {
        const float x = (philox_uniform_at(key, (row0 + row) * (unsigned long long)V + c) < sigmoid(abase[c])) ? 1.f : 0.f;
        v[(size_t)row * ld + c] = x;
        s += x * dvec[c];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) part[row] = s;
    for (int q = 1 + lane; q < nslot; q += 64) part[(size_t)q * ld_part + row] = 0.f;
}

// F(x_j) = -x_j.vb - sum_i softplus(z_ji) from the slot partials a prop-up left (ActArgs::rowacc_single), in double: one wave
// per row, lane-strided sums + butterfly (a fixed order)
__global__ __launch_bounds__(256) void rbm_fe_rows_kernel(const float *X, int ldx, int rows, int V, const float *vb, const float *part,
                                                          int ld_part, int nslot, float *out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    double s = 0.0;
    for (int c = lane; c < V; c += 64) s += (double)(X[(size_t)row * ldx + c] * vb[c]);
    for (int q = lane; q < nslot; q += 64) s += (double)part[(size_t)q * ld_part + row];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = (float)(-s);
}

// the two entry points are about the joint p(v, h) of ONE Bernoulli-Bernoulli RBM
static int check_single_joint(const bm_rbm *h, const char *what, bool groups_ok = false) {
    BM_TRY(refuse_nrelu(h, what, groups_ok));
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "%s needs Bernoulli visible units (this handle's are Gaussian)", what);
    BM_CHECK(!h->multinomial(), "%s needs Bernoulli hidden units (this handle's are Multinomial)", what);
    BM_CHECK(!h->cfg.dbm_first && !h->cfg.dbm_last, "%s: the conditionals of a dbm_first / dbm_last handle (one of them doubled) "
             "belong to no single joint distribution", what);
    return 0;
}

static int ensure_ais_rows(bm_rbm *h, int rows) {
    if (rows <= h->ais_rows) return 0;
    h->ais_rows = 0;                               // (set again once every buffer exists: a failure leaves none counted)
    BM_TRY(h->av.alloc(rows, h->V)); BM_TRY(h->ah.alloc(rows, h->H));
    BM_TRY(h->apart_h.alloc((size_t)nslots(h->H) * rows)); BM_TRY(h->apart_v.alloc((size_t)nslots(h->V) * rows));
    BM_TRY(h->alogw.alloc(rows));
    h->ais_rows = rows;
    return 0;
}

static PhiloxKey ais_key(uint64_t seed, uint32_t site, int t, uint32_t step) {
    PhiloxKey k;
    k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32);
    k.site = site + 16u * (uint32_t)t;
    k.call = step;
    return k;
}

// h ~ Ber(sigmoid(beta z)), z = v W + hb, from the chain state av into ah; score: the same pass leaves the slot partials of
// sum_j softplus(beta z_j) - softplus(beta_a z_j) in apart_h.  sample = 0: the score alone (the last beta)
// lengths (replicated softmax, bm_rbm_rsm_ais): the chains' own document lengths [R], z = v W + D hb - the tempered DB pass
static void ais_up(bm_rbm *h, int R, float beta, int sample, const PhiloxKey &key, int64_t chain0, bool score, float beta_a,
                   const float *lengths = nullptr) {
    LayerPass p = rbm_pass(h, true, R, in_of(h->av), LayerOut{sample, nullptr, sample ? h->ah.p : nullptr, h->ah.ld, key, chain0}, beta);
    if (score) p.softplus_rows(h->apart_h.p, h->ais_rows, beta_a, beta, 0);
    p.a.row_bmult = lengths;
    issue(h, p);
}
// v ~ Ber(sigmoid(beta h W^T + a + beta (vb - a))) from ah into av, the mixed bias from row `kbeta` of the table; dot: the pass
// leaves the slot partials of v.(vb - a) in apart_v for the next score
static void ais_down(bm_rbm *h, int R, float beta, int kbeta, const PhiloxKey &key, int64_t chain0, bool dot) {
    LayerPass p = rbm_pass(h, false, R, in_of(h->ah), LayerOut{1, nullptr, h->av.p, h->av.ld, key, chain0}, beta)
                      .bias(h->atable.p + (size_t)kbeta * h->V, 1.0f);
    if (dot) p.statedot_rows(h->apart_v.p, h->ais_rows, h->adot.p);
    issue(h, p);
}

extern "C" {

const char *bm_last_error(void) { return bm::g_err; }
const char *bm_version(void) { return "bm355 0.1 gfx950"; }

int bm_rbm_multinomial_limit(int64_t *out4) {
    BM_CHECK(out4, "null argument");
    long long q[3];
    BM_TRY(bm::dyn_lds_query(reinterpret_cast<const void *>(bm::softmax_multinomial_kernel), q));
    out4[0] = q[0]; out4[1] = q[1]; out4[2] = q[2];
    out4[3] = std::min<long long>(8192, q[2] / (long long)(2 * sizeof(float)));
    return 0;
}

int bm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
// Host waits (bm_*_sync, the blocking reads of metrics) SPIN instead of sleeping on an interrupt: a training loop waits
// for the device every few hundred microseconds (metric fetches, the mean-field loop control), and the wake-up of a
// blocked host thread costs tens of microseconds per wait.  BM355_HOST_WAIT=yield|block selects the other policies.
// The flag can only be set before the device's context exists: when the host framework created it first (torch), the
// call fails harmlessly and the framework's policy stays.
int bm_set_device(int device) {
    BM_HIP(hipSetDevice(device));
    const char *w = getenv("BM355_HOST_WAIT");
    unsigned flags = hipDeviceScheduleSpin;
    if (w && !strcmp(w, "yield")) flags = hipDeviceScheduleYield;
    if (w && !strcmp(w, "block")) flags = hipDeviceScheduleBlockingSync;
    if (hipSetDeviceFlags(flags) != hipSuccess) (void)hipGetLastError();
    return 0;
}
int bm_dev_alloc(size_t bytes, void **out_dev) { BM_HIP(hipMalloc(out_dev, bytes ? bytes : 1)); return 0; }
int bm_dev_free(void *dev) { BM_HIP(hipFree(dev)); return 0; }
// Host -> device.  Large pageable sources (a training set) are pinned in place for the duration of the copy: the
// runtime otherwise stages them through its own bounce buffers at a fraction of the link rate.  BM355_DEBUG=h2d_pin=0
// keeps the plain copy; any failure of the registration falls back to it.
int bm_h2d(void *dst, const void *src, size_t bytes) {
    static const bool pin = !(bm::dbg("h2d_pin") && atoi(bm::dbg("h2d_pin")) == 0);
    if (pin && bytes >= ((size_t)32 << 20)) {
        if (hipHostRegister(const_cast<void *>(src), bytes, hipHostRegisterDefault) == hipSuccess) {
            const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
            (void)hipHostUnregister(const_cast<void *>(src));
            BM_HIP(e);
            return 0;
        }
        (void)hipGetLastError();
    }
    BM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int bm_d2h(void *dst, const void *src, size_t bytes) { BM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; }
int bm_dev_memset(void *dst, int value, size_t bytes) { BM_HIP(hipMemset(dst, value, bytes)); return 0; }

int bm_rbm_create(const bm_rbm_config *cfg, bm_rbm **out) {
    BM_CHECK(cfg && out, "null argument");
    BM_CHECK(cfg->n_visible >= 1 && cfg->n_hidden >= 1, "bad layer sizes %d x %d", cfg->n_visible, cfg->n_hidden);
    BM_CHECK(cfg->max_batch >= 1, "max_batch must be >= 1");
    BM_CHECK(cfg->v_unit == BM_UNIT_BERNOULLI || cfg->v_unit == BM_UNIT_GAUSSIAN, "unknown visible unit %d", cfg->v_unit);
    BM_CHECK(cfg->h_unit == BM_UNIT_BERNOULLI || cfg->h_unit == BM_UNIT_MULTINOMIAL || cfg->h_unit == BM_UNIT_NRELU, "unknown hidden unit %d",
             cfg->h_unit);
    if (cfg->h_unit == BM_UNIT_NRELU) {
        BM_CHECK(!cfg->dbm_first && !cfg->dbm_last, "NReLU hidden units: no dbm_first / dbm_last handle (a doubled pre-activation is not the "
                 "unit's conditional, and the DBM has no such layer)");
        BM_CHECK(cfg->sparsity_cost == 0.f, "NReLU hidden units do not combine with the sparsity penalty (sparsity_cost %g: the target is a "
                 "probability, the unit's mean is not)", (double)cfg->sparsity_cost);
        BM_CHECK(cfg->dropout < 0.f, "NReLU hidden units do not combine with dropout (this configuration's is %g)", (double)cfg->dropout);
    }
    if (cfg->h_unit == BM_UNIT_MULTINOMIAL) {
        BM_CHECK(cfg->n_samples >= 1, "MultinomialRBM: n_samples must be >= 1 (got %d)", cfg->n_samples);
    }
    BM_CHECK(bm_device_count() > 0, "no HIP device visible: libbm355 has no CPU fallback");
    if (cfg->h_unit == BM_UNIT_MULTINOMIAL) {
        int64_t q[4];
        BM_TRY(bm_rbm_multinomial_limit(q));
        BM_CHECK(cfg->n_hidden <= q[3], "MultinomialRBM: n_hidden %d > %lld (softmax row staged in LDS: 8 bytes per unit, the runtime "
                 "allows a workgroup %lld bytes of dynamic LDS; at most 8192 units)", cfg->n_hidden, (long long)q[3], (long long)q[2]);
    }
    auto h = std::make_unique<bm_rbm>();
    h->cfg = *cfg;
    h->V = cfg->n_visible; h->H = cfg->n_hidden; h->maxB = cfg->max_batch;
    const int V = h->V, H = h->H, B = h->maxB;
    BM_HIP(hipGetDevice(&h->device));
    BM_TRY(create(h->stream)); BM_TRY(create(h->ev0)); BM_TRY(create(h->ev1));
    BM_TRY(h->W.alloc(V, H)); BM_TRY(h->dW.alloc(V, H));
    {
        const char *e = bm::dbg("up_xm");          // default on; 0 keeps the k-major prop-up
        h->use_wt = !(e && atoi(e) == 0) && (V % 4 == 0) && !h->multinomial();
        if (h->use_wt) BM_TRY(h->Wt.alloc(H, V));
    }
    BM_TRY(h->vb.alloc(V)); BM_TRY(h->hb.alloc(H)); BM_TRY(h->dvb.alloc(V)); BM_TRY(h->dhb.alloc(H));
    BM_TRY(h->q.alloc(H)); BM_TRY(h->sigma.alloc(V));
    BM_TRY(h->h0m.alloc(B, H)); BM_TRY(h->h0s.alloc(B, H)); BM_TRY(h->hm.alloc(B, H)); BM_TRY(h->hs.alloc(B, H)); BM_TRY(h->hneg.alloc(B, H));
    BM_TRY(h->vm.alloc(B, V)); BM_TRY(h->vs.alloc(B, V)); BM_TRY(h->Xs.alloc(B, V)); BM_TRY(h->Xd.alloc(B, V));
    BM_TRY(h->grad.alloc(h->grad_tail() + V + 2 * (size_t)H));
    BM_TRY(h->pen.alloc(H));
    BM_TRY(h->ov.alloc(V)); BM_TRY(h->oh.alloc(H));
    BM_TRY(h->rowacc.alloc(3 * (size_t)B)); BM_TRY(h->hhat.alloc(3 * (size_t)H));
    BM_TRY(h->flip.alloc(B)); BM_TRY(h->scal.alloc(6));
    {   // sigma defaults to 1 (rbm.py:88)
        std::vector<float> ones(V, 1.0f);
        BM_HIP(hipMemcpy(h->sigma.p, ones.data(), V * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = h.release();
    return 0;
}

int bm_rbm_destroy(bm_rbm *h) {
    if (!h) return 0;
    for (hipStream_t st : {h->stream.h, h->comm_stream.h, h->stage_stream.h}) if (st) (void)hipStreamSynchronize(st);
    if (h->xchg_used) xchg_bind_user(h->xchg_used, nullptr);
    delete h;
    return 0;
}

// Status words the device leaves behind (the stream `s` is idle up to the point of interest when this is called):
// the direct exchange's time-out word and the chained launches' (bm_chain.h).  A failed chained launch is reported
// ONCE - the results since the last check are invalid - and switches chaining off for this handle: later passes run as
// per-pass launches instead of leaving the handle poisoned (round-4 advisor).
static int check_device_status(bm_rbm *h) {
    if (h->xchg_used) BM_TRY(xchg_check_status(h->xchg_used));      // a lost rank is an ERROR here, never a silent wrong sum
    if (h->chain.status) {      // chained launches (bm_chain.h): an expired wait or a tile nobody computed is an ERROR
        int st[2] = {0, 0};
        BM_HIP(hipMemcpy(st, h->chain.status, sizeof(st), hipMemcpyDeviceToHost));
        const long long expect = h->chain.tiles_expected & 0xffffffffLL;
        if (st[0] != 0 || (long long)(unsigned)st[1] != expect) {
            h->chain.mode = 0;                                   // per-pass launches from here on
            h->chain.tiles_expected = 0;
            BM_HIP(hipMemset(h->chain.status, 0, sizeof(st)));
            BM_CHECK(st[0] == 0, "chained propagation launch failed (status %d: %s); the results since the last check are "
                     "invalid, chained launches are now off for this handle", st[0],
                     st[0] == CHAIN_ERR_TIMEOUT ? "a wait for a producing tile expired" : "not an 8-XCD device");
            BM_CHECK(false, "chained propagation launches computed %u tiles, expected %lld; the results since the last check "
                     "are invalid, chained launches are now off for this handle", (unsigned)st[1], expect);
        }
    }
    return 0;
}

// the class head's label flag (class_row_kernel): reported ONCE, then cleared.  The stream is idle when this is called
static int check_class_labels(bm_rbm *h) {
    if (!h->cls_bad.p) return 0;
    int bad = 0;
    BM_HIP(hipMemcpy(&bad, h->cls_bad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) {
        BM_HIP(hipMemset(h->cls_bad.p, 0, sizeof(int)));
        BM_CHECK(false, "class head: a label outside [0, n_classes=%d) reached bm_rbm_class_train_step / _epoch; its row was left "
                 "out of the update", h->n_classes);
    }
    return 0;
}

static int check_row_lengths(bm_rbm *h);      // (replicated softmax: row_lengths_kernel's flag, below)
int bm_rbm_sync(bm_rbm *h) {
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));
    if (h->nonbinary.p) {
        int bad = 0;
        BM_HIP(hipMemcpy(&bad, h->nonbinary.p, sizeof(int), hipMemcpyDeviceToHost));
        if (bad) {
            BM_HIP(hipMemset(h->nonbinary.p, 0, sizeof(int)));
            BM_CHECK(false, "fast-binary mode: bm_rbm_gibbs was given hidden states that are not a {0,1} bitmap");
        }
    }
    BM_TRY(check_class_labels(h));
    BM_TRY(check_row_lengths(h));
    return 0;
}

// Opt-in fast-binary mode (bm_bf3.h): the sampling sweep (bm_rbm_gibbs) of a Bernoulli-Bernoulli RBM with both layers
// sampled runs its contractions as exact-product bf16 x 3 on the bf16 matrix cores; agreement with the default path
// is to fp32 round-off, not bit for bit.  0 restores the default.
// 1 = where it PAYS: at 784 x 1024 x 512 the bf16 strip kernel is slower than the fp32 path (25.9 against 25.2 us per sweep,
// profiles/r5_gibbs_summary.md: the pass is bound by its fill and epilogue, not by matrix time), so the switch only takes
// effect from 8M weights upwards (the 3072 x 5000 shape gains); 2 = wherever legal (tests, measurements).
int bm_rbm_set_fast_binary(bm_rbm *h, int32_t on) {
    BM_CHECK(h, "null argument");
    h->fast = (on >= 2 || (on == 1 && (long long)h->V * h->H >= (8ll << 20))) ? 1 : 0;
    return 0;
}

// Centred update (bm355.h).  A property of the handle: while it is on, every fused update entry - train_step,
// _metrics, _metrics_async, train_epoch, train_step_pt, train_epoch_pt - takes the centred update.
int bm_rbm_set_centering(bm_rbm *h, int32_t on, float nu_v, float nu_h) {
    BM_CHECK(h, "null argument");
    if (!on) { h->cen_on = false; return 0; }
    BM_TRY(refuse_nrelu(h, "bm_rbm_set_centering"));
    BM_CHECK(!h->fw_on, "centering is not combined with fast weights (two flavours of the update kernel; bm_rbm_set_fast_weights(off) first)");
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "centering needs Bernoulli visible units (this handle's are Gaussian)");
    BM_CHECK(!h->multinomial(), "centering needs Bernoulli hidden units (this handle's are Multinomial)");
    BM_CHECK(!h->cfg.dbm_first && !h->cfg.dbm_last, "centering: a dbm_first / dbm_last handle (one conditional doubled) is not centred");
    BM_CHECK(h->cfg.dropout < 0.f, "centering does not combine with dropout (this handle's is %g)", (double)h->cfg.dropout);
    BM_CHECK(nu_v >= 0.f && nu_v <= 1.f && nu_h >= 0.f && nu_h <= 1.f, "centering: sliding factors (%g, %g) outside [0, 1]", (double)nu_v, (double)nu_h);
    if (!h->cen_a.p) {
        BM_TRY(h->cen_gv.alloc(h->V)); BM_TRY(h->cen_gh.alloc(h->H));
        BM_TRY(h->cen_a.alloc(4 * (size_t)h->maxB));      // last: the workspace is complete once it exists
    }
    h->cen_nu_v = nu_v; h->cen_nu_h = nu_h;
    h->cen_on = true;
    return 0;
}

// Fast-weights PCD (bm355.h).  A property of the handle that only bm_rbm_train_step_pt / _train_epoch_pt read.
int bm_rbm_set_fast_weights(bm_rbm *h, int32_t on, float fast_learning_rate, float fast_decay) {
    BM_CHECK(h, "null argument");
    if (!on) {          // released: the handle is what it was before the mode was ever switched on
        h->fw_on = h->eff_valid = false;
        h->fw_lr = h->fw_decay = 0.f;
        BM_HIP(hipStreamSynchronize(h->stream));
        h->Wf = Mat(); h->We = Mat(); h->Wet = Mat();
        h->vbf = DevBuf(); h->hbf = DevBuf(); h->vbe = DevBuf(); h->hbe = DevBuf();
        return 0;
    }
    BM_TRY(check_single_joint(h, "bm_rbm_set_fast_weights"));
    BM_CHECK(h->cfg.dropout < 0.f, "fast weights: the tempered family has no dropout (this handle's is %g)", (double)h->cfg.dropout);
    BM_CHECK(!h->cen_on, "fast weights are not combined with centering (two flavours of the update kernel; bm_rbm_set_centering(off) first)");
    BM_CHECK(std::isfinite(fast_learning_rate) && fast_learning_rate >= 0.f, "fast weights: fast_learning_rate %g is not a finite number >= 0",
             (double)fast_learning_rate);
    BM_CHECK(fast_decay >= 0.f && fast_decay < 1.f, "fast weights: fast_decay %g outside [0, 1)", (double)fast_decay);
    if (!h->fw_on) {    // off -> on: a zero fast set (alloc zeroes); on -> on: the two scalars only
        BM_TRY(h->Wf.alloc(h->V, h->H)); BM_TRY(h->We.alloc(h->V, h->H));
        if (h->use_wt) BM_TRY(h->Wet.alloc(h->H, h->V));
        BM_TRY(h->vbf.alloc(h->V)); BM_TRY(h->hbf.alloc(h->H)); BM_TRY(h->vbe.alloc(h->V)); BM_TRY(h->hbe.alloc(h->H));
        h->eff_valid = false;
    }
    h->fw_lr = fast_learning_rate; h->fw_decay = fast_decay;
    h->fw_on = true;
    return 0;
}

// name -> matrix / vector of the fast-weights mode (null: no such name, or the mode is off); *ro: an effective copy (get only)
static Mat *find_fast_mat(bm_rbm *h, const std::string &n, bool *ro) {
    if (!h->fw_on) return nullptr;
    *ro = n == "W_eff";
    return n == "W_fast" ? &h->Wf : n == "W_eff" ? &h->We : nullptr;
}
static DevBuf *find_fast_vec(bm_rbm *h, const std::string &n, bool *ro) {
    if (!h->fw_on) return nullptr;
    *ro = n == "vb_eff" || n == "hb_eff";
    return n == "vb_fast" ? &h->vbf : n == "hb_fast" ? &h->hbf : n == "vb_eff" ? &h->vbe : n == "hb_eff" ? &h->hbe : nullptr;
}

// name -> vector variable
static DevBuf *find_vec(bm_rbm *h, const std::string &n) {
    if (n == "vb") return &h->vb;
    if (n == "hb") return &h->hb;
    if (n == "dvb") return &h->dvb;
    if (n == "dhb") return &h->dhb;
    if (n == "q_means") return &h->q;
    if (n == "sigma") return &h->sigma;
    if (n == "ov") return &h->ov;             // centering offsets (bm_rbm_set_centering)
    if (n == "oh") return &h->oh;
    if (h->n_classes) {                       // the class head's variables (bm_rbm_set_classes), dense [C][H] and [C]
        if (n == "U") return &h->U;
        if (n == "dU") return &h->dU;
        if (n == "yb") return &h->yb;
        if (n == "dyb") return &h->dyb;
    }
    return nullptr;
}

int bm_rbm_set_param(bm_rbm *h, const char *name, const float *host, size_t n) {
    const std::string nm(name ? name : "");
    BM_HIP(hipStreamSynchronize(h->stream));
    h->eff_valid = false;       // (whatever is written: the effective copies of a fast-weights handle are rebuilt before their next use)
    bool ro = false;
    if (Mat *fm = find_fast_mat(h, nm, &ro)) {
        BM_CHECK(!ro, "variable '%s' is a derived copy (W + W_fast): get only", name);
        BM_CHECK(n == (size_t)h->V * h->H, "variable '%s' has %zu elements, got %zu", name, (size_t)h->V * h->H, n);
        return fm->upload(host);
    }
    if (DevBuf *fb = find_fast_vec(h, nm, &ro)) {
        BM_CHECK(!ro, "variable '%s' is a derived copy (bias + fast bias): get only", name);
        BM_CHECK(n == fb->n, "variable '%s' has %zu elements, got %zu", name, fb->n, n);
        BM_HIP(hipMemcpy(fb->p, host, n * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    if (nm == "W" || nm == "dW") {
        BM_CHECK(n == (size_t)h->V * h->H, "variable '%s' has %zu elements, got %zu", name, (size_t)h->V * h->H, n);
        BM_TRY((nm == "W" ? h->W : h->dW).upload(host));
        if (nm == "W") h->wt_valid = false;
        else { h->dw_sharded = false; if (h->xchg_used) xchg_dw_replaced(h->xchg_used); }
        return 0;
    }
    DevBuf *b = find_vec(h, nm);
    BM_CHECK(b, "unknown RBM variable '%s'", name ? name : "(null)");
    BM_CHECK(n == b->n, "variable '%s' has %zu elements, got %zu", name, b->n, n);
    BM_HIP(hipMemcpy(b->p, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// set a variable from DEVICE memory (dense, row-major), asynchronously, in stream order - no host synchronisation:
// re-initialising a model between runs, or `init_from` another handle's variables, without idling the GPU
int bm_rbm_set_param_dev(bm_rbm *h, const char *name, const float *src_dev, size_t n) {
    const std::string nm(name ? name : "");
    BM_CHECK(h && src_dev, "null argument");
    h->eff_valid = false;
    if (nm == "W" || nm == "dW") {
        BM_CHECK(n == (size_t)h->V * h->H, "variable '%s' has %zu elements, got %zu", name, (size_t)h->V * h->H, n);
        Mat &m = nm == "W" ? h->W : h->dW;
        if (nm == "W") h->wt_valid = false;
        else { h->dw_sharded = false; if (h->xchg_used) xchg_dw_replaced(h->xchg_used); }
        BM_HIP(hipMemcpy2DAsync(m.p, (size_t)m.ld * sizeof(float), src_dev, (size_t)m.cols * sizeof(float),
                                (size_t)m.cols * sizeof(float), m.rows, hipMemcpyDeviceToDevice, h->stream));
        return 0;
    }
    DevBuf *b = find_vec(h, nm);
    BM_CHECK(b, "unknown RBM variable '%s'", name ? name : "(null)");
    BM_CHECK(n == b->n, "variable '%s' has %zu elements, got %zu", name, b->n, n);
    BM_HIP(hipMemcpyAsync(b->p, src_dev, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// The whole tempered ensemble, read only, dense (tests and tools; bm_rbm_pt_read / bm_rbm_groups_pt_read hand out the beta = 1 rows):
// "pt_v" [M R][V], "pt_h" [M R][H], "pt_part_v" [ceil(V/16)][M R], "pt_part_h" [ceil(H/16)][M R], "pt_mult" [M R]
// ("gpt_*": the same five of the ensemble of bm_rbm_gauss_pt_*, v in the scaled variable u, part_v the slots of -1/2 (u - c)^2: the
// names that read the ensemble while its tag is PT_GAUSS, as "pt_*" do while it is any other)
static int pt_get_param(bm_rbm *h, const std::string &full, float *host, size_t n) {
    const bool gauss = full[0] == 'g';
    const std::string nm = gauss ? full.substr(1) : full;
    PtEnsemble &e = h->pt;
    BM_CHECK(h->pt_unit != PT_NONE && gauss == (h->pt_unit == PT_GAUSS),
             "variable '%s': no ensemble (bm_rbm_pt_init / bm_rbm_groups_pt_init / bm_rbm_gauss_pt_init)", full.c_str());
    const size_t rows = (size_t)e.nrows();
    const float *src = nullptr;
    size_t pitch = 0, width = 0, height = 0;
    if (nm == "pt_v")           { src = e.v.x.p; pitch = e.v.x.ld; width = h->V; height = rows; }
    else if (nm == "pt_h")      { src = e.h1.x.p; pitch = e.h1.x.ld; width = h->H; height = rows; }
    else if (nm == "pt_part_v") { src = e.v.part.p; pitch = e.rows; width = rows; height = e.v.nslot(); }
    else if (nm == "pt_len" && h->pt_unit == PT_COUNTS) { src = h->rp_len.p; pitch = rows; width = rows; height = 1; }
    else if (nm == "pt_part_h") { src = e.h1.part.p; pitch = e.rows; width = rows; height = nslots(h->H); }
    else if (nm == "pt_mult")   { src = e.mult.p; pitch = rows; width = rows; height = 1; }
    BM_CHECK(src, "unknown RBM variable '%s'", full.c_str());
    BM_CHECK(n == width * height, "variable '%s' has %zu elements, got %zu", full.c_str(), width * height, n);
    BM_HIP(hipMemcpy2D(host, width * sizeof(float), src, pitch * sizeof(float), width * sizeof(float), height, hipMemcpyDeviceToHost));
    return 0;
}
// The chain states an AIS entry left behind, read only, dense (tests): "ais_v" [rows][V], "ais_h" [rows][H], rows = n / width of the
// first rows of the AIS workspaces
static int ais_get_param(bm_rbm *h, const std::string &nm, float *host, size_t n) {
    const bool v = nm == "ais_v";
    BM_CHECK(v || nm == "ais_h", "unknown RBM variable '%s'", nm.c_str());
    const Mat &m = v ? h->av : h->ah;
    const size_t width = v ? h->V : h->H;
    BM_CHECK(n >= width && n % width == 0 && n / width <= (size_t)h->ais_rows, "variable '%s': %zu elements are no whole rows of the %d "
             "AIS chains", nm.c_str(), n, h->ais_rows);
    BM_HIP(hipMemcpy2D(host, width * sizeof(float), m.p, (size_t)m.ld * sizeof(float), width * sizeof(float), n / width, hipMemcpyDeviceToHost));
    return 0;
}

int bm_rbm_get_param(bm_rbm *h, const char *name, float *host, size_t n) {
    const std::string nm(name ? name : "");
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));        // never hand out variables computed from invalid tiles / a lost rank's sums
    if (nm.compare(0, 3, "pt_") == 0 || nm.compare(0, 4, "gpt_") == 0) return pt_get_param(h, nm, host, n);
    if (nm.compare(0, 4, "ais_") == 0) return ais_get_param(h, nm, host, n);
    bool ro = false;
    Mat *fm = find_fast_mat(h, nm, &ro);
    DevBuf *fb = fm ? nullptr : find_fast_vec(h, nm, &ro);
    if (fm || fb) {
        if (ro) {               // a stale effective copy is rebuilt first
            ensure_eff(h);
            BM_HIP(hipStreamSynchronize(h->stream));
        }
        const size_t want = fm ? (size_t)h->V * h->H : fb->n;
        BM_CHECK(n == want, "variable '%s' has %zu elements, got %zu", name, want, n);
        if (fm) return fm->download(host);
        BM_HIP(hipMemcpy(host, fb->p, n * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (nm == "W" || nm == "dW") {
        BM_CHECK(n == (size_t)h->V * h->H, "variable '%s' has %zu elements, got %zu", name, (size_t)h->V * h->H, n);
        if (nm == "dW") BM_TRY(check_dw(h, "bm_rbm_get_param(dW)"));
        return (nm == "W" ? h->W : h->dW).download(host);
    }
    DevBuf *b = find_vec(h, nm);
    BM_CHECK(b, "unknown RBM variable '%s'", name ? name : "(null)");
    BM_CHECK(n == b->n, "variable '%s' has %zu elements, got %zu", name, b->n, n);
    BM_HIP(hipMemcpy(host, b->p, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// Snapshot without a host wait (the checkpoint of an epoch while the next one already runs): bm_rbm_stage copies
// every variable into slot `slot` (0 | 1) device-to-device in stream order and returns at once; bm_rbm_get_staged
// reads a variable of that snapshot back on its own stream (it waits for the copies only) and may be called from
// another host thread while the engine's stream keeps working.  The caller must not re-stage a slot that is still
// being read.
int bm_rbm_stage(bm_rbm *h, int32_t slot) {
    BM_CHECK(h && (slot == 0 || slot == 1), "bad stage slot %d", (int)slot);
    bm_rbm::Stage &sg = h->stage[slot];
    // a slot that another thread is reading back must not be overwritten under it (any caller of the C API, not
    // only the Python bookkeeping of base.py: round-3 advisor)
    BM_CHECK(sg.readers.load() == 0, "stage slot %d is being read by bm_rbm_get_staged: use the other slot", (int)slot);
    BM_TRY(check_dw(h, "bm_rbm_stage"));
    if (!sg.ev) {
        BM_TRY(sg.W.alloc(h->V, h->H)); BM_TRY(sg.dW.alloc(h->V, h->H));
        BM_TRY(sg.vb.alloc(h->V)); BM_TRY(sg.dvb.alloc(h->V)); BM_TRY(sg.sigma.alloc(h->V));
        BM_TRY(sg.hb.alloc(h->H)); BM_TRY(sg.dhb.alloc(h->H)); BM_TRY(sg.q.alloc(h->H));
        BM_TRY(create(sg.ev, hipEventDisableTiming));            // last: the slot is complete once it exists
    }
    if (!h->stage_stream) BM_TRY(create(h->stage_stream, hipStreamNonBlocking));
    // Bound the host's run-ahead to one snapshot interval: a training loop that never fetches anything would otherwise
    // queue every epoch of the call at once (measured: 4000 updates = 16 000 launches in flight ran 101 instead of
    // 77 us per update).  Waiting for the PREVIOUS snapshot's copies leaves the whole current epoch queued: no bubble.
    static const bool bound = !(bm::dbg("stage_ahead") && atoi(bm::dbg("stage_ahead")) == 0);
    if (bound && h->last_stage >= 0) BM_HIP(hipEventSynchronize(h->stage[h->last_stage].ev));
    BM_HIP(hipMemcpyAsync(sg.W.p, h->W.p, h->W.count() * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(sg.dW.p, h->dW.p, h->dW.count() * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    DevBuf *src[] = {&h->vb, &h->hb, &h->dvb, &h->dhb, &h->q, &h->sigma};
    DevBuf *dst[] = {&sg.vb, &sg.hb, &sg.dvb, &sg.dhb, &sg.q, &sg.sigma};
    for (int i = 0; i < 6; ++i)
        BM_HIP(hipMemcpyAsync(dst[i]->p, src[i]->p, src[i]->n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    BM_HIP(hipEventRecord(sg.ev, h->stream));
    sg.ready = true;
    h->last_stage = slot;
    return 0;
}
int bm_rbm_get_staged(bm_rbm *h, int32_t slot, const char *name, float *host, size_t n) {
    BM_CHECK(h && (slot == 0 || slot == 1) && h->stage[slot].ready, "stage slot %d holds no snapshot", (int)slot);
    BM_HIP(hipSetDevice(h->device));                 // (the calling thread may be a fresh one)
    bm_rbm::Stage &sg = h->stage[slot];
    struct Reading { std::atomic<int> &n; Reading(std::atomic<int> &r) : n(r) { ++n; } ~Reading() { --n; } } reading(sg.readers);
    const std::string nm(name ? name : "");
    // Wait for the staged copies on the HOST first, then copy through a pinned bounce buffer: a pageable
    // device-to-host copy that has to wait for an event parks inside the runtime (measured: the training thread's
    // launches stalled behind it, 101 instead of 76 us per update)
    BM_HIP(hipEventSynchronize(sg.ev));
    const size_t need = (size_t)h->V * h->H * sizeof(float);
    if (!h->stage_host) BM_TRY(create(h->stage_host, (size_t)h->V * h->H));
    if (h->chain.status) {
        // the sticky error word of the chained launches (not the tile count: the training thread may be ahead of the
        // device): a checkpoint must not be written from tiles a failed launch left invalid
        BM_HIP(hipMemcpyAsync(h->stage_host, h->chain.status, sizeof(int), hipMemcpyDeviceToHost, h->stage_stream));
        BM_HIP(hipStreamSynchronize(h->stage_stream));
        BM_CHECK(*(const int *)h->stage_host.h == 0, "a chained propagation launch failed (status %d) before this snapshot: "
                 "it is invalid (bm_rbm_sync reports and recovers)", *(const int *)h->stage_host.h);
    }
    if (nm == "W" || nm == "dW") {
        BM_CHECK(n == (size_t)h->V * h->H, "variable '%s' has %zu elements, got %zu", name, (size_t)h->V * h->H, n);
        const Mat &m = nm == "W" ? sg.W : sg.dW;
        BM_HIP(hipMemcpy2DAsync(h->stage_host, (size_t)m.cols * sizeof(float), m.p, (size_t)m.ld * sizeof(float),
                                (size_t)m.cols * sizeof(float), m.rows, hipMemcpyDeviceToHost, h->stage_stream));
    } else {
        const char *names[] = {"vb", "hb", "dvb", "dhb", "q_means", "sigma"};
        DevBuf *bufs[] = {&sg.vb, &sg.hb, &sg.dvb, &sg.dhb, &sg.q, &sg.sigma};
        DevBuf *b = nullptr;
        for (int i = 0; i < 6; ++i) if (nm == names[i]) b = bufs[i];
        BM_CHECK(b, "unknown RBM variable '%s'", name ? name : "(null)");
        BM_CHECK(n == b->n, "variable '%s' has %zu elements, got %zu", name, b->n, n);
        BM_CHECK(n * sizeof(float) <= need, "variable '%s' larger than the bounce buffer", name);
        BM_HIP(hipMemcpyAsync(h->stage_host, b->p, n * sizeof(float), hipMemcpyDeviceToHost, h->stage_stream));
    }
    BM_HIP(hipStreamSynchronize(h->stage_stream));
    memcpy(host, h->stage_host, n * sizeof(float));
    return 0;
}

int bm_rbm_dev_ptr(bm_rbm *h, const char *name, void **out_dev, size_t *out_n) {
    const std::string nm(name ? name : "");
    DevBuf *b = (nm == "grad") ? &h->grad : find_vec(h, nm);
    BM_CHECK(b, "no device view for '%s' (matrices are pitched; use get/set_param)", name ? name : "(null)");
    *out_dev = b->p;
    if (out_n) *out_n = b->n;
    return 0;
}

int bm_rbm_seed(bm_rbm *h, uint64_t seed) { h->seed = seed; h->call = 0; return 0; }
int bm_rbm_set_row_offset(bm_rbm *h, int64_t row0) { h->row0 = row0; return 0; }

int bm_rbm_train_step(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k) {
    BM_TRY(check_dw(h, "bm_rbm_train_step"));
    ChainOpts o;
    o.need_vm = false;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    launch_update_fused(h, B, lr, mom);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_rbm_train_step_metrics(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k,
                              float *out4) {
    BM_TRY(check_dw(h, "bm_rbm_train_step_metrics"));
    ChainOpts o;
    o.fetch = true;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    BM_TRY(metrics_from_chain(h, B, out4));
    launch_update_fused(h, B, lr, mom);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// The same fetch WITHOUT the host wait: the reference reads the train metrics every `train_metrics_every_iter`-th
// iteration but only uses their mean at the end of the epoch (base_rbm.py:549-571), so the six device sums of a metrics
// iteration are copied into a pinned ring in stream order and converted when bm_rbm_collect_metrics is called (one
// synchronisation per epoch instead of one per fetch: fit() with the reference's default cadence ran 81 - 98 us per
// update against 68 without metrics, almost all of it the GPU idling behind the host round trips).
int bm_rbm_train_step_metrics_async(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k) {
    if (!h->mring) {                  // (the ring is set last: it marks the setup as complete)
        Pinned<double> ring;
        BM_TRY(create(ring, (size_t)bm_rbm::MRING * 6));
        BM_TRY(create(h->ev_mlast, hipEventDisableTiming));
        BM_HIP(hipHostGetDevicePointer((void **)&h->mring_dev, ring, 0));
        h->mring_B.resize(bm_rbm::MRING);
        h->mring = std::move(ring);
    }
    BM_CHECK(h->mring_n < bm_rbm::MRING, "%d metric fetches are pending: call bm_rbm_collect_metrics", h->mring_n);
    BM_TRY(check_dw(h, "bm_rbm_train_step_metrics_async"));
    ChainOpts o;
    o.fetch = true;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    BM_TRY(metrics_from_chain(h, B, nullptr));
    hipLaunchKernelGGL(scal_to_host_kernel, dim3(1), dim3(64), 0, h->stream, (const double *)h->scal.p,
                       h->mring_dev + (size_t)h->mring_n * 6);
    BM_HIP(hipEventRecord(h->ev_mlast, h->stream));
    h->mring_B[h->mring_n++] = B;
    launch_update_fused(h, B, lr, mom);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}
// out4n [max_n][4] <- the pending fetches in order (msre, pll, l2_loss, free energy each); *out_n their number
int bm_rbm_collect_metrics(bm_rbm *h, float *out4n, int32_t max_n, int32_t *out_n) {
    BM_CHECK(h && out_n && (out4n || max_n == 0), "null argument");
    BM_CHECK(h->mring_n <= max_n, "%d fetches pending, room for %d", h->mring_n, (int)max_n);
    // wait for the last FETCH, not for the stream: what was queued behind it keeps running while the host reads the ring
    if (h->mring_n > 0 && h->ev_mlast) BM_HIP(hipEventSynchronize(h->ev_mlast));
    if (h->chain.status || h->xchg_used) {
        // (status words are read with a blocking copy: that waits for the whole stream - only handles that use chained
        //  launches or a direct exchange pay it)
        BM_HIP(hipStreamSynchronize(h->stream));
        // the pending fetches are dropped either way: an error must not leave them for the next epoch's mean
        const int rc = check_device_status(h);
        if (rc) { h->mring_n = 0; *out_n = 0; return rc; }
    }
    for (int i = 0; i < h->mring_n; ++i) metrics_to_out4(h, h->mring + (size_t)i * 6, h->mring_B[i], out4n + 4 * (size_t)i);
    *out_n = h->mring_n;
    h->mring_n = 0;
    return 0;
}

// N rows of X_dev as consecutive minibatches of `batch` rows, driven from C: the same launches and RNG call counters
// as the caller's own loop over bm_rbm_train_step, without a host round trip per batch.  (Round 3 could replay recurring
// runs of updates from a HIP graph, bit-exactly, and measured it SLOWER on MI355X / ROCm 7.2 - 66.3 against 65.4 us per
// update over 2000 updates, 75 - 77 against 69 us for a single 20-update replay; removed in round 4, profiles/NOTES.md 3.10.)
int bm_rbm_train_epoch(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t k) {
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    for (int64_t s = 0; s < N; s += batch) {
        const int B = (int)((N - s < batch) ? (N - s) : batch);
        BM_TRY(bm_rbm_train_step(h, X_dev + (size_t)s * h->V, B, lr, mom, k));
    }
    return 0;
}

int bm_rbm_grad_step(bm_rbm *h, const float *X_dev, int32_t B, int32_t k) {
    BM_TRY(refuse_nrelu(h, "bm_rbm_grad_step"));
    BM_CHECK(!h->cen_on, "bm_rbm_grad_step: the split step has no centred form; switch centering off (bm_rbm_set_centering)");
    ChainOpts o;
    o.need_vm = false; o.split_step = true;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    rbm_grad(h, B, 0, (float)B, 0.f, 0.f, true);     // raw outer products + raw column sums, one launch
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// ---- delayed-gradient data parallelism (a documented NON-parity mode, SURVEY 8e / DESIGN 6): two gradient slots.
// Step t: grad_step into slot t % 2, its all-reduce goes out on the communication stream and runs under step t+1's
// Gibbs chain; the update applied at the end of step t is the (already reduced) one of step t-1.
static int ensure_delayed(bm_rbm *h) {
    if (h->comm_stream) return 0;
    BM_TRY(h->grad_alt.alloc(h->grad.n));
    for (int i = 0; i < 2; ++i) {
        BM_TRY(create(h->ev_ready[i], hipEventDisableTiming));
        BM_TRY(create(h->ev_reduced[i], hipEventDisableTiming));
    }
    return create(h->comm_stream);    // last: the setup is complete once it exists
}
int bm_rbm_set_grad_slot(bm_rbm *h, int32_t slot) {
    BM_CHECK(h && (slot == 0 || slot == 1), "slot must be 0 or 1");
    BM_TRY(refuse_nrelu(h, "bm_rbm_set_grad_slot"));
    if (slot == h->grad_slot) return 0;
    BM_TRY(ensure_delayed(h));
    std::swap(h->grad, h->grad_alt);
    h->grad_slot = slot;
    return 0;
}
int bm_rbm_allreduce_grads_async(bm_rbm *h, bm_comm *c) {
    BM_CHECK(h && c, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_allreduce_grads_async"));
    BM_TRY(ensure_delayed(h));
    const int s = h->grad_slot;
    BM_HIP(hipEventRecord(h->ev_ready[s], h->stream));
    BM_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_ready[s], 0));
    BM_TRY(bm_comm_allreduce_sum(c, h->grad.p, h->grad.n, (void *)h->comm_stream));
    BM_HIP(hipEventRecord(h->ev_reduced[s], h->comm_stream));
    return 0;
}
int bm_rbm_wait_grads(bm_rbm *h, int32_t slot) {
    BM_CHECK(h && (slot == 0 || slot == 1) && h->comm_stream, "no reduction was started on slot %d", slot);
    BM_HIP(hipStreamWaitEvent(h->stream, h->ev_reduced[slot], 0));
    return 0;
}

int bm_rbm_apply_step(bm_rbm *h, int32_t B_global, float lr, float mom) {
    BM_TRY(refuse_nrelu(h, "bm_rbm_apply_step"));
    BM_CHECK(!h->cen_on, "bm_rbm_apply_step: the split step has no centred form; switch centering off (bm_rbm_set_centering)");
    BM_TRY(check_dw(h, "bm_rbm_apply_step"));
    ProfScope _ps(h, KC_BIAS);
    RbmBiasArgs b;
    fill_bias(h, (float)B_global, lr, mom, b);
    ApplyWArgs a;
    memset(&a, 0, sizeof(a));
    a.raw = h->grad.p; a.raw2 = nullptr;
    a.W = h->W.p; a.dW = h->dW.p; a.Wt = nullptr;
    h->wt_valid = false;
    h->eff_valid = false;
    a.I = h->H; a.J = h->V; a.ldw = h->W.ld; a.ldwt = 0; a.form = 0;
    a.N = (float)B_global; a.M = a.N; a.l2 = h->cfg.l2; a.lr = lr; a.mom = mom;
    if (h->cfg.sparsity_cost != 0.f) {      // the W update needs the penalty: bias update first
        hipLaunchKernelGGL(rbm_bias_kernel, dim3((h->V + h->H + 255) / 256), dim3(256), 0, h->stream, b);
        a.pen = h->pen.p;
        launch_apply_w(a, nullptr, h->stream);
    } else {                                // penalty == 0 (pen stays 0): one launch for both
        a.pen = nullptr;
        launch_apply_w(a, &b, h->stream);
    }
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_rbm_transform(bm_rbm *h, const float *X_dev, int32_t B, int32_t k, float *H_dev) {
    BM_CHECK(H_dev, "null output");
    ChainOpts o;
    o.hm_out = H_dev;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// One prop-up of the handle's own hidden conditional from X_dev [B][V] (dense), the input taken as given - no division by sigma,
// no dropout: means and / or states to dense [B][H] outputs, drawn at SITE_H0, step 0, the handle's seed, call counter and row
// offset (bm355.h).  Every hidden unit type.  The counter advances by one
int bm_rbm_sample_h(bm_rbm *h, const float *X_dev, int32_t B, float *Hmean_dev, float *Hstate_dev) {
    BM_CHECK(h && X_dev, "null argument");
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    ensure_wt(h);
    // (Multinomial units without a means output: the softmax pair stages its logits in hm and shares one pitch between means
    //  and states - through the pitched workspaces, then one copy)
    const bool staged = h->multinomial() && Hstate_dev && !Hmean_dev;
    if (h->rsm_len) rsm_lengths_of(h, X_dev, h->V, B, h->rsm_D.p);      // replicated softmax: the lengths of the input rows
    issue(h, rbm_pass(h, true, B, LayerIn{X_dev, h->V}, staged ? rbm_out(h, 1, h->hm.p, h->hs.p, h->hm.ld, SITE_H0, 0)
                                                              : rbm_out(h, 1, Hmean_dev, Hstate_dev, h->H, SITE_H0, 0)));
    if (staged) hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)h->hs.p, h->hs.ld, Hstate_dev, h->H, B, h->H);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// replicated softmax: the entries that start from hidden states take the rows' lengths from the caller
// (bm_rbm_set_row_lengths), exactly B of them; a handle without the unit: nothing to do
static int rsm_use_row_lengths(bm_rbm *h, const char *what, int B) {
    if (!h->rsm_len) return 0;
    BM_CHECK(h->rsm_user_n == B, "%s on a handle with replicated softmax visible units needs the lengths of its %d rows: call "
             "bm_rbm_set_row_lengths(h, D_dev, %d) first (%d lengths are set)", what, B, B, h->rsm_user_n);
    h->rsm_cur = h->rsm_user.p;
    return 0;
}

// The visible counterpart: one prop-down of the handle's own visible conditional from H_dev [B][H] (dense), taken as given:
// means and / or states to dense [B][V] outputs, drawn at SITE_V, step 0, the handle's seed, call counter and row offset (bm355.h).
// Every visible unit type.  The counter advances by one
int bm_rbm_sample_v_from_h(bm_rbm *h, const float *H_dev, int32_t B, float *Vmean_dev, float *Vstate_dev) {
    BM_CHECK(h && H_dev, "null argument");
    BM_CHECK(Vmean_dev || Vstate_dev, "bm_rbm_sample_v_from_h: no output (means and states are both null)");
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_TRY(rsm_use_row_lengths(h, "bm_rbm_sample_v_from_h", B));
    issue(h, rbm_pass(h, false, B, LayerIn{H_dev, h->H}, rbm_out(h, 1, Vmean_dev, Vstate_dev, h->V, SITE_V, 0)));
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// Softmax visible units (bm355.h).  A property of the handle that issue() reads at every prop-down
int bm_rbm_set_visible_groups(bm_rbm *h, int32_t K) {
    BM_CHECK(h, "null argument");
    if (K == 0) {
        // (an ensemble of one-hot rows goes with the groups, DESIGN.md 3.29: a Bernoulli sweep never runs over it)
        if (h->pt_unit == PT_GROUPS) pt_drop(h);
        h->v_groups = 0; h->groups_missing = false;
        return 0;
    }
    BM_CHECK(K >= 2, "softmax visible units: the group width must be 0 (off) or >= 2 (got %d)", (int)K);
    BM_CHECK(h->V % K == 0, "softmax visible units: n_visible = %d is no multiple of the group width %d", h->V, (int)K);
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "softmax visible units replace Bernoulli visible units (this handle's are Gaussian)");
    BM_CHECK(h->cfg.h_unit == BM_UNIT_BERNOULLI, "softmax visible units need Bernoulli hidden units (this handle's are %s)",
             h->multinomial() ? "Multinomial" : "NReLU");
    BM_CHECK(!h->cfg.dbm_first && !h->cfg.dbm_last, "softmax visible units: no dbm_first / dbm_last handle (the DBM has no such layer)");
    BM_CHECK(h->cfg.dropout < 0.f, "softmax visible units do not combine with dropout (this handle's is %g)", (double)h->cfg.dropout);
    BM_CHECK(!h->cen_on, "softmax visible units do not combine with centering (bm_rbm_set_centering(off) first)");
    BM_CHECK(!h->n_classes, "softmax visible units do not combine with a class head (bm_rbm_set_classes(0) first)");
    BM_CHECK(!h->fw_on, "softmax visible units do not combine with fast weights (bm_rbm_set_fast_weights(off) first)");
    // (the ensemble of a handle that has this width already is bm_rbm_groups_pt_init's, DESIGN.md 3.29: nothing changes)
    BM_CHECK(h->pt_unit == PT_NONE || (h->pt_unit == PT_GROUPS && h->v_groups == K), "softmax visible units do not combine with a tempered ensemble (this handle holds one: bm_rbm_pt_init)");
    BM_CHECK(!h->rsm_len, "softmax visible units do not combine with replicated softmax visible units (bm_rbm_set_replicated_softmax(0) first)");
    h->v_groups = K;
    return 0;
}

// Replicated softmax visible units (bm355.h).  A property of the handle that issue() reads at every pass
int bm_rbm_set_replicated_softmax(bm_rbm *h, int32_t max_length) {
    BM_CHECK(h, "null argument");
    if (max_length == 0) {
        // (an ensemble of count rows goes with the unit, DESIGN.md 3.31: a Bernoulli sweep never runs over it)
        if (h->pt_unit == PT_COUNTS) pt_drop(h);
        h->rsm_len = 0; h->rsm_user_n = 0; h->rsm_cur = nullptr;
        return 0;
    }
    BM_CHECK(max_length >= 1 && max_length < (1 << 24), "replicated softmax visible units: max_length must be 0 (off) or in [1, 2^24) "
             "(got %d): the lengths are exact in float32", (int)max_length);
    BM_CHECK(h->V >= 2 && h->V <= RSM_MAX_V, "replicated softmax visible units: n_visible = %d is outside [2, %d] (a row's prefix sums and "
             "counts live in LDS)", h->V, RSM_MAX_V);
    BM_CHECK(h->cfg.v_unit == BM_UNIT_BERNOULLI, "replicated softmax visible units replace Bernoulli visible units (this handle's are Gaussian)");
    BM_CHECK(h->cfg.h_unit == BM_UNIT_BERNOULLI, "replicated softmax visible units need Bernoulli hidden units (this handle's are %s)",
             h->multinomial() ? "Multinomial" : "NReLU");
    BM_CHECK(!h->cfg.dbm_first && !h->cfg.dbm_last, "replicated softmax visible units: no dbm_first / dbm_last handle (the DBM has no such layer)");
    BM_CHECK(h->cfg.dropout < 0.f, "replicated softmax visible units do not combine with dropout (this handle's is %g)", (double)h->cfg.dropout);
    BM_CHECK(h->cfg.sparsity_cost == 0.f, "replicated softmax visible units do not combine with a sparsity penalty (this handle's "
             "sparsity_cost is %g)", (double)h->cfg.sparsity_cost);
    BM_CHECK(!h->cen_on, "replicated softmax visible units do not combine with centering (bm_rbm_set_centering(off) first)");
    BM_CHECK(!h->n_classes, "replicated softmax visible units do not combine with a class head (bm_rbm_set_classes(0) first)");
    BM_CHECK(!h->fw_on, "replicated softmax visible units do not combine with fast weights (bm_rbm_set_fast_weights(off) first)");
    // (the count ensemble of a handle that has the unit already is bm_rbm_rsm_pt_init's; a new max_length discards it)
    BM_CHECK(h->pt_unit == PT_NONE || h->pt_unit == PT_COUNTS, "replicated softmax visible units do not combine with a tempered ensemble (this handle holds one: bm_rbm_pt_init)");
    BM_CHECK(!h->v_groups, "replicated softmax visible units do not combine with visible groups (bm_rbm_set_visible_groups(0) first)");
    if (!h->rsm_bad.p) {          // (allocated last: the workspaces are complete once the flag exists)
        BM_TRY(h->rsm_D.alloc(h->maxB)); BM_TRY(h->rsm_user.alloc(h->maxB));
        DevArray<int> flag;
        BM_TRY(flag.alloc(1));
        BM_HIP(hipMemset(flag.p, 0, sizeof(int)));
        h->rsm_bad = std::move(flag);
    }
    if (h->pt_unit == PT_COUNTS && h->rsm_len != max_length) pt_drop(h);
    h->rsm_len = max_length;
    h->rsm_user_n = 0;
    h->rsm_cur = nullptr;
    return 0;
}

// ... and the lengths of the rows that bm_rbm_sample_v_from_h and bm_rbm_gibbs run on next: D_dev [B] float32 on the device,
// integers in [1, max_length], copied into the handle in stream order
int bm_rbm_set_row_lengths(bm_rbm *h, const float *D_dev, int32_t B) {
    BM_CHECK(h && D_dev, "null argument");
    BM_CHECK(h->rsm_len, "bm_rbm_set_row_lengths needs a handle with replicated softmax visible units (bm_rbm_set_replicated_softmax); "
             "this handle has none");
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_HIP(hipMemcpyAsync(h->rsm_user.p, D_dev, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    h->rsm_user_n = B;
    return 0;
}

// row_lengths_kernel's flag: reported ONCE, then cleared.  The stream is idle when this is called
static int check_row_lengths(bm_rbm *h) {
    if (!h->rsm_bad.p) return 0;
    int bad = 0;
    BM_HIP(hipMemcpy(&bad, h->rsm_bad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) {
        BM_HIP(hipMemset(h->rsm_bad.p, 0, sizeof(int)));
        BM_CHECK(false, "replicated softmax visible units: a row that is no count vector of 1 to max_length = %d tokens reached the "
                 "engine:%s%s%s%s%s", h->rsm_len, (bad & RSM_BAD_MISMATCH) ? " [a start row of bm_rbm_rsm_pt_init whose sum is not its chain's length]" : "",
                 (bad & RSM_BAD_NEGATIVE) ? " [a negative entry]" : "",
                 (bad & RSM_BAD_FRACTION) ? " [a non-integer entry]" : "", (bad & RSM_BAD_EMPTY) ? " [an empty row, length 0]" : "",
                 (bad & RSM_BAD_LONG) ? " [a row longer than max_length]" : "");
    }
    return 0;
}

int bm_rbm_metrics(bm_rbm *h, const float *X_dev, int32_t B, int32_t k, float *out4) {
    ChainOpts o;
    o.fetch = true;
    BM_TRY(run_chain(h, X_dev, B, k, o));
    BM_TRY(metrics_from_chain(h, B, out4));
    h->call++;
    return 0;
}

int bm_rbm_free_energy(bm_rbm *h, const float *X_dev, int32_t B, float *out1) {
    BM_TRY(refuse_nrelu(h, "bm_rbm_free_energy", true));
    BM_CHECK(!h->rsm_len, "bm_rbm_free_energy (the feg metric) is not available for replicated softmax visible units: its hidden kernel "
             "has no length-scaled bias; bm_rbm_free_energy_rows gives the rows' free energies (DESIGN.md 3.27)");
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    // free_energy_op is built from self._X_batch AFTER tf.nn.dropout replaced it (base_rbm.py:417-418,
    // :516): the `feg` metric sees the dropped input like msre / pll do
    const float *Xin;
    int ldx;
    bool dropped;
    prep_input(h, X_dev, B, &Xin, &ldx, &dropped);
    BM_HIP(hipMemsetAsync(h->scal.p, 0, 6 * sizeof(double), h->stream));
    BM_HIP(hipMemsetAsync(h->rowacc.p, 0, 3 * (size_t)h->maxB * sizeof(float), h->stream));
    launch_fe(h, Xin, ldx, B, false);
    double host[6];
    BM_HIP(hipMemcpyAsync(host, h->scal.p, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    *out1 = (float)(host[2] / B + mn_fe_const(h));
    if (h->multinomial() || dropped) h->call++;   // the random h_hat / the dropout mask consumed one call of the stream
    return 0;
}

// Per-row free energies F(x) = -x.vb - sum_j softplus(x W + hb)_j of the RBM's own parameters (no dropout, no multiplier, no
// change of the RNG call counter): one prop-up that only leaves its softplus slot partials, one row kernel
int bm_rbm_free_energy_rows(bm_rbm *h, const float *X_dev, int32_t B, float *out_host) {
    BM_CHECK(h && X_dev && out_host, "null argument");
    // (replicated softmax is served: F(v) = -v.vb - sum_j softplus(D hb_j + (vW)_j), the DB pass's own slot partials)
    BM_TRY(check_single_joint(h, "bm_rbm_free_energy_rows", true));
    BM_CHECK(B >= 1, "bad row count %d", (int)B);
    if (B > h->fer_rows || (h->rsm_len && !h->fer_len.p)) {
        const int rows = std::max((int)B, h->fer_rows);
        h->fer_rows = 0;
        BM_TRY(h->fer_part.alloc((size_t)nslots(h->H) * rows)); BM_TRY(h->fer_out.alloc(rows));
        if (h->rsm_len) BM_TRY(h->fer_len.alloc(rows));
        h->fer_rows = rows;
    }
    ensure_wt(h);
    if (h->rsm_len) rsm_lengths_of(h, X_dev, h->V, B, h->fer_len.p);     // the lengths of the input rows
    issue(h, rbm_pass(h, true, B, LayerIn{X_dev, h->V}, LayerOut{0, nullptr, nullptr, pad_ld(h->H), PhiloxKey{0, 0, 0, 0}, 0})
                 .softplus_rows(h->fer_part.p, h->fer_rows, 0.f, 1.0f, 1));
    hipLaunchKernelGGL(rbm_fe_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, h->stream, X_dev, h->V, (int)B, h->V, (const float *)h->vb.p,
                       (const float *)h->fer_part.p, h->fer_rows, nslots(h->H), h->fer_out.p);
    BM_HIP(hipGetLastError());
    BM_HIP(hipMemcpyAsync(out_host, h->fer_out.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_row_lengths(h));
    return 0;
}

// ---- class head (bm355.h; bm_class.h lists the launches)
static int ensure_class_rows(bm_rbm *h, int rows) {
    if (rows <= h->cls_rows) return 0;
    const size_t C = (size_t)h->n_classes;
    h->cls_rows = 0;                               // (set again once every buffer exists: a failure leaves none counted)
    BM_TRY(h->cls_part.alloc(C * nslots(h->H) * rows));
    BM_TRY(h->cls_logp.alloc(C * rows)); BM_TRY(h->cls_prob.alloc(C * rows)); BM_TRY(h->cls_coef.alloc(C * rows));
    BM_TRY(h->cls_rowlp.alloc(rows)); BM_TRY(h->cls_rowhit.alloc(rows)); BM_TRY(h->cls_tl.alloc(rows));
    h->cls_rows = rows;
    return 0;
}

int bm_rbm_set_classes(bm_rbm *h, int32_t n_classes) {
    BM_CHECK(h, "null argument");
    BM_CHECK(n_classes == 0 || n_classes >= 2, "bm_rbm_set_classes: n_classes must be 0 (detach) or >= 2 (got %d)", (int)n_classes);
    BM_HIP(hipStreamSynchronize(h->stream));
    if (n_classes == 0) {
        h->n_classes = 0; h->cls_rows = 0;
        for (DevBuf *b : {&h->U, &h->dU, &h->yb, &h->dyb, &h->cls_part, &h->cls_logp, &h->cls_prob, &h->cls_coef, &h->cls_rowlp, &h->cls_rowhit})
            *b = DevBuf();
        h->cls_tl = DevArray<int>();
        return 0;
    }
    BM_TRY(check_single_joint(h, "bm_rbm_set_classes"));
    const size_t C = (size_t)n_classes;
    h->n_classes = 0; h->cls_rows = 0;
    BM_TRY(h->U.alloc(C * h->H)); BM_TRY(h->dU.alloc(C * h->H)); BM_TRY(h->yb.alloc(C)); BM_TRY(h->dyb.alloc(C));
    if (!h->cls_bad.p) BM_TRY(h->cls_bad.alloc(1));
    if (!h->cls_acc.p) BM_TRY(h->cls_acc.alloc(2));
    h->n_classes = n_classes;
    if (ensure_class_rows(h, h->maxB)) { h->n_classes = 0; return 1; }
    return 0;
}

// the forward pass of B rows (B <= cls_rows): the CR prop-up (t into `T` when it is wanted) and the row kernel
static void class_forward(bm_rbm *h, const float *X_dev, int B, float *T, int ldt, const int *y_dev, int ldx = 0) {
    ensure_wt(h);
    LayerPass p = rbm_pass(h, true, B, LayerIn{X_dev, ldx ? ldx : h->V}, LayerOut{0, T, nullptr, ldt, PhiloxKey{0, 0, 0, 0}, 0}, 1.0f);
    p.a.kind = 3;                                  // stores t = z + hb
    issue(h, p.class_rows(h->cls_part.p, h->cls_rows, h->U.p, h->H, h->n_classes));
    ProfScope _ps(h, KC_OTHER);
    ClassRowArgs r;
    memset(&r, 0, sizeof(r));
    r.part = h->cls_part.p; r.ldp = h->cls_rows; r.nslots = nslots(h->H); r.C = h->n_classes; r.B = B;
    r.yb = h->yb.p; r.y = y_dev;
    r.logp = h->cls_logp.p; r.prob = h->cls_prob.p; r.coef = h->cls_coef.p; r.tl = h->cls_tl.p;
    r.rowlp = h->cls_rowlp.p; r.rowhit = h->cls_rowhit.p; r.bad = h->cls_bad.p;
    launch_class_row(r, h->stream);
}

int bm_rbm_class_log_proba(bm_rbm *h, const float *X_dev, int32_t B, float *logp_host) {
    BM_CHECK(h && X_dev && logp_host, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_class_log_proba"));
    BM_CHECK(h->n_classes, "bm_rbm_class_log_proba: no class head is attached (bm_rbm_set_classes)");
    BM_TRY(check_single_joint(h, "bm_rbm_class_log_proba"));
    BM_CHECK(B >= 1, "bad row count %d", (int)B);
    BM_TRY(ensure_class_rows(h, B));
    class_forward(h, X_dev, B, nullptr, pad_ld(h->H), nullptr);
    BM_HIP(hipGetLastError());
    BM_HIP(hipMemcpyAsync(logp_host, h->cls_logp.p, (size_t)B * h->n_classes * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int check_class_train(const bm_rbm *h, const char *what, int B) {
    BM_TRY(refuse_nrelu(h, what));
    BM_CHECK(h->n_classes, "%s: no class head is attached (bm_rbm_set_classes)", what);
    BM_TRY(check_single_joint(h, what));
    BM_CHECK(h->cfg.dropout < 0.f, "%s does not combine with dropout (this handle's is %g)", what, (double)h->cfg.dropout);
    BM_CHECK(h->cfg.sparsity_cost == 0.f, "%s does not combine with the sparsity penalty (this handle's sparsity_cost is %g)", what,
             (double)h->cfg.sparsity_cost);
    BM_CHECK(!h->cen_on, "%s has no centred form; switch centering off (bm_rbm_set_centering)", what);
    BM_CHECK(!h->xchg_used && !h->comm_stream && !h->dw_sharded && h->grad_slot == 0,
             "%s: this handle takes part in a data-parallel run; the discriminative update has no split form", what);
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    return 0;
}
// one discriminative update; `sum`: the batch's sums of log p(t|x) and of the hits are added to cls_acc (taken from the forward
// pass, before the update).  Queues only
struct StackBelow;
static void stack_backward(bm_rbm *top, const StackBelow &below, int B);
// `ldx`: the pitch of the input (0: dense); `below`: the layers under the head - their backward passes are queued
// behind class_hidden_kernel, ahead of every update
static int class_update(bm_rbm *h, const float *X_dev, const int *y_dev, int B, float lr, float mom, bool sum, int ldx = 0,
                        const StackBelow *below = nullptr) {
    if (!ldx) ldx = h->V;
    class_forward(h, X_dev, B, h->hm.p, h->hm.ld, y_dev, ldx);
    {   // (event timing, bm_rbm_profile: the classes this update leaves unused tell its kernels apart - the CR pass counts as
        //  KC_UP, class_row_kernel as KC_OTHER, class_hidden_kernel as KC_COLSUM, class_head_update_kernel as KC_BIAS)
        ProfScope _ps(h, KC_COLSUM);
        ClassHiddenArgs c;
        memset(&c, 0, sizeof(c));
        c.T = h->hm.p; c.ldt = h->hm.ld; c.U = h->U.p; c.ldu = h->H; c.prob = h->cls_prob.p; c.tl = h->cls_tl.p;
        c.pos = h->h0m.p; c.negm = h->hneg.p; c.ld = h->h0m.ld; c.B = B; c.H = h->H; c.C = h->n_classes;
        launch_class_hidden(c, h->stream);
        if (sum) launch_class_sum(h->cls_rowlp.p, h->cls_rowhit.p, B, h->cls_acc.p, h->stream);
    }
    if (below) stack_backward(h, *below, B);
    {
        ProfScope _ps(h, KC_BIAS);
        ClassHeadArgs u;
        memset(&u, 0, sizeof(u));
        u.T = h->hm.p; u.ldt = h->hm.ld; u.coef = h->cls_coef.p; u.U = h->U.p; u.dU = h->dU.p; u.yb = h->yb.p; u.dyb = h->dyb.p;
        u.ldu = h->H; u.B = B; u.H = h->H; u.C = h->n_classes;
        u.N = (float)B; u.l2 = h->cfg.l2; u.lr = lr; u.mom = mom;
        launch_class_head_update(u, h->stream);
    }
    // W, W^T, hb, vb: the fused update as it is, on pos (h0m), negm (hneg, "already negated") and the input on both sides -
    // dvb = colsum(X - X) / B = 0 by construction
    h->Xin = X_dev; h->Xin_ld = ldx;
    h->hm_is_neg = true;
    h->neg_v = X_dev; h->neg_v_ld = ldx;
    launch_update_fused(h, B, lr, mom);
    h->neg_v = nullptr; h->neg_v_ld = 0;
    BM_HIP(hipGetLastError());
    return 0;
}
static int class_fetch(bm_rbm *h, double rows, float *out2) {
    double host[2];
    BM_HIP(hipMemcpyAsync(host, h->cls_acc.p, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));
    BM_TRY(check_class_labels(h));
    out2[0] = (float)(host[0] / rows); out2[1] = (float)(host[1] / rows);
    return 0;
}

int bm_rbm_class_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int32_t B, float lr, float mom, float *out2) {
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_TRY(check_class_train(h, "bm_rbm_class_train_step", B));
    BM_TRY(check_dw(h, "bm_rbm_class_train_step"));
    if (out2) BM_HIP(hipMemsetAsync(h->cls_acc.p, 0, 2 * sizeof(double), h->stream));
    BM_TRY(class_update(h, X_dev, y_dev, B, lr, mom, out2 != nullptr));
    return out2 ? class_fetch(h, (double)B, out2) : 0;
}

// N rows as consecutive minibatches of `batch` rows, driven from C: the launches of the caller's own loop over
// bm_rbm_class_train_step, no host wait between the batches
int bm_rbm_class_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int64_t N, int32_t batch, float lr, float mom,
                             float *out2) {
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    BM_TRY(check_class_train(h, "bm_rbm_class_train_epoch", (int)((N < batch) ? N : batch)));
    BM_TRY(check_dw(h, "bm_rbm_class_train_epoch"));
    if (out2) BM_HIP(hipMemsetAsync(h->cls_acc.p, 0, 2 * sizeof(double), h->stream));
    for (int64_t s = 0; s < N; s += batch) {
        const int B = (int)((N - s < batch) ? (N - s) : batch);
        BM_TRY(class_update(h, X_dev + (size_t)s * h->V, y_dev + s, B, lr, mom, out2 != nullptr));
    }
    return out2 ? class_fetch(h, (double)N, out2) : 0;
}

// ---- fine-tuning a stack of sigmoid layers below the head by back-propagation (bm355.h; bm_stack.h)
// Every layer is a handle of its own with a stream of its own.  The launches of a stack are ordered with EVENTS: whenever the
// work moves from one handle to another, hand_over() records the giver's ev_stack on its stream and makes the taker's stream
// wait for it.  One update, in issue order (L_1 .. L_D the layers below, T the top):
//   L_1 .. L_D   the deterministic prop-up a_l = sigmoid(a_{l-1} W_l + hb_l) into the handle's hm         -> next handle
//   T            act_kernel CR, class_row_kernel, class_hidden_kernel (class_update)
//   T            stack_g_kernel: g = pos + negm into hs;  act_kernel BP: delta_D into L_D's h0m            -> L_D
//   L_D .. L_2   act_kernel BP: delta_{l-1} into L_{l-1}'s h0m                                            -> L_{l-1}
//   T            class_head_update_kernel, the fused update (class_update)                                -> L_D
//   L_D .. L_1   the zero fill of hneg, the fused update on (a_{l-1}, delta_l) against (a_{l-1}, 0)       -> L_{l-1}
// A backward pass reads W of the handle whose stream it runs on, and that handle's update is queued behind it on the same
// stream: no backward pass sees a weight written in its own step.  The closing hand-overs, top down, end on L_1's stream, where
// the next step begins: whatever that step overwrites (a_l in hm, delta_l in h0m) has been read by then.
struct StackBelow { bm_rbm *const *l; int n; };

static void hand_over(bm_rbm *from, bm_rbm *to) {
    if (from == to) return;
    (void)hipEventRecord(from->ev_stack, from->stream);
    (void)hipStreamWaitEvent(to->stream, from->ev_stack, 0);
}
// what a layer of a stack must be (the top as well: `head`); creates the hand-over event
static int check_stack_layer(bm_rbm *h, const char *what, int B, bool head) {
    BM_TRY(refuse_nrelu(h, what));
    if (head) BM_CHECK(h->n_classes, "%s: no class head is attached to the top handle (bm_rbm_set_classes)", what);
    BM_TRY(check_single_joint(h, what));
    BM_CHECK(h->cfg.dropout < 0.f, "%s does not combine with dropout (this handle's is %g)", what, (double)h->cfg.dropout);
    BM_CHECK(h->cfg.sparsity_cost == 0.f, "%s does not combine with the sparsity penalty (this handle's sparsity_cost is %g)", what,
             (double)h->cfg.sparsity_cost);
    BM_CHECK(!h->cen_on, "%s has no centred form; switch centering off (bm_rbm_set_centering)", what);
    BM_CHECK(!h->xchg_used && !h->comm_stream && !h->dw_sharded && h->grad_slot == 0,
             "%s: this handle takes part in a data-parallel run; back-propagation has no split form", what);
    BM_CHECK(B >= 1 && B <= h->maxB, "%s: batch %d outside [1, max_batch=%d]", what, B, h->maxB);
    BM_TRY(check_dw(h, what));
    if (!h->ev_stack) BM_TRY(create(h->ev_stack, hipEventDisableTiming));
    return 0;
}
static int check_stack(bm_rbm *top, bm_rbm *const *below, int n_below, const char *what, int B) {
    BM_CHECK(top && n_below >= 0 && (n_below == 0 || below), "null argument");
    for (int l = 0; l < n_below; ++l) {
        BM_CHECK(below[l], "null argument");
        BM_CHECK(below[l] != top, "%s: the same handle twice (layer %d is the top)", what, l);
        for (int m = 0; m < l; ++m) BM_CHECK(below[l] != below[m], "%s: the same handle twice (layers %d and %d)", what, m, l);
        bm_rbm *above = (l + 1 < n_below) ? below[l + 1] : top;
        BM_CHECK(below[l]->H == above->V, "%s: the widths do not chain (layer %d has %d hidden units, the layer above it %d visible)",
                 what, l, below[l]->H, above->V);
        BM_TRY(check_stack_layer(below[l], what, B, false));
    }
    return check_stack_layer(top, what, B, true);
}
// the deterministic prop-up of a layer below the head: means only, into hm
static void stack_up(bm_rbm *h, const float *in, int ldin, int B) {
    ensure_wt(h);
    issue(h, rbm_pass(h, true, B, LayerIn{in, ldin}, LayerOut{0, h->hm.p, nullptr, h->hm.ld, PhiloxKey{0, 0, 0, 0}, 0}, 1.0f));
}
// the BP pass of handle h: out = (delta W^T) .* A .* (1 - A), or delta W^T itself without A.  (vb stands in for the bias the raw
// pass loads and does not use)
static void stack_down(bm_rbm *h, const float *delta, int ldd, int B, const float *A, int lda, float *out, int ldo) {
    LayerPass p = rbm_pass(h, false, B, LayerIn{delta, ldd}, LayerOut{0, out, nullptr, ldo, PhiloxKey{0, 0, 0, 0}, 0}, 1.0f);
    p.raw();
    p.a.bp = 1; p.a.bp_act = A; p.a.bp_ld = lda;
    issue(h, p);
}
// the backward passes of one update, top down, queued behind the top's class_hidden_kernel: every delta_l lands in L_l's h0m
static void stack_backward(bm_rbm *top, const StackBelow &s, int B) {
    if (s.n == 0) return;
    {
        ProfScope _ps(top, KC_OTHER);
        launch_stack_g(top->h0m.p, top->hneg.p, top->hs.p, top->h0m.ld, B, top->H, top->stream);
    }
    bm_rbm *src = top;
    const float *delta = top->hs.p;
    int ldd = top->hs.ld;
    for (int l = s.n - 1; l >= 0; --l) {
        bm_rbm *lay = s.l[l];
        stack_down(src, delta, ldd, B, lay->hm.p, lay->hm.ld, lay->h0m.p, lay->h0m.ld);
        hand_over(src, lay);
        src = lay; delta = lay->h0m.p; ldd = lay->h0m.ld;
    }
}
// W, W^T, hb of a layer from its input and its delta: the fused update as it is, with the delta as the positive hidden operand,
// zeros as the negative one and the input on both visible sides - dvb = colsum(X - X) / B = 0 by construction.  Queues only
static int delta_update(bm_rbm *h, const float *X_dev, int ldx, const float *delta, int ldd, int B, float lr, float mom) {
    BM_HIP(hipMemsetAsync(h->hneg.p, 0, (size_t)B * h->hneg.ld * sizeof(float), h->stream));
    h->Xin = X_dev; h->Xin_ld = ldx;
    h->hm_is_neg = true;
    h->neg_v = X_dev; h->neg_v_ld = ldx;
    h->pos_h = delta; h->pos_h_ld = ldd;
    launch_update_fused(h, B, lr, mom);
    h->neg_v = nullptr; h->neg_v_ld = 0;
    h->pos_h = nullptr; h->pos_h_ld = 0;
    BM_HIP(hipGetLastError());
    return 0;
}
// one update of the whole stack (the table above).  Queues only
static int stack_update(bm_rbm *top, const StackBelow &s, const float *X_dev, const int *y_dev, int B, const float *lr, float mom, bool sum) {
    const float *in = X_dev;
    int ldin = s.n ? s.l[0]->V : top->V;
    for (int l = 0; l < s.n; ++l) {
        stack_up(s.l[l], in, ldin, B);
        hand_over(s.l[l], (l + 1 < s.n) ? s.l[l + 1] : top);
        in = s.l[l]->hm.p; ldin = s.l[l]->hm.ld;
    }
    BM_TRY(class_update(top, in, y_dev, B, lr[s.n], mom, sum, ldin, &s));
    bm_rbm *src = top;
    for (int l = s.n - 1; l >= 0; --l) {
        bm_rbm *lay = s.l[l];
        hand_over(src, lay);
        const float *x = l ? s.l[l - 1]->hm.p : X_dev;
        BM_TRY(delta_update(lay, x, l ? s.l[l - 1]->hm.ld : lay->V, lay->h0m.p, lay->h0m.ld, B, lr[l], mom));
        src = lay;
    }
    return 0;
}
// the fetch of a stack's train entries: the top's, after every layer's stream has drained
static int stack_fetch(bm_rbm *top, const StackBelow &s, double rows, float *out2) {
    for (int l = 0; l < s.n; ++l) {
        BM_HIP(hipStreamSynchronize(s.l[l]->stream));
        BM_TRY(check_device_status(s.l[l]));
    }
    return class_fetch(top, rows, out2);
}

int bm_rbm_backprop_down(bm_rbm *h, const float *Delta_dev, int32_t B, const float *A_dev, int32_t lda, float *Out_dev, int32_t ldo) {
    BM_CHECK(h && Delta_dev && Out_dev, "null argument");
    BM_TRY(check_stack_layer(h, "bm_rbm_backprop_down", B, false));
    BM_CHECK(ldo >= h->V && (!A_dev || lda >= h->V), "bm_rbm_backprop_down: a pitch below the row length %d (lda=%d, ldo=%d)", h->V,
             (int)lda, (int)ldo);
    stack_down(h, Delta_dev, h->H, B, A_dev, lda, Out_dev, ldo);
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_rbm_delta_update(bm_rbm *h, const float *X_dev, const float *Delta_dev, int32_t B, float lr, float mom) {
    BM_CHECK(h && X_dev && Delta_dev, "null argument");
    BM_TRY(check_stack_layer(h, "bm_rbm_delta_update", B, false));
    return delta_update(h, X_dev, h->V, Delta_dev, h->H, B, lr, mom);
}

int bm_rbm_class_stack_train_step(bm_rbm *top, bm_rbm *const *below, int32_t n_below, const float *X_dev, const int32_t *y_dev, int32_t B,
                                  const float *lr, float mom, float *out2) {
    BM_CHECK(top && X_dev && y_dev && lr, "null argument");
    BM_TRY(check_stack(top, below, n_below, "bm_rbm_class_stack_train_step", B));
    const StackBelow s{below, n_below};
    if (out2) BM_HIP(hipMemsetAsync(top->cls_acc.p, 0, 2 * sizeof(double), top->stream));
    BM_TRY(stack_update(top, s, X_dev, y_dev, B, lr, mom, out2 != nullptr));
    return out2 ? stack_fetch(top, s, (double)B, out2) : 0;
}

// N rows as consecutive minibatches of `batch` rows, driven from C: the launches of the caller's own loop over
// bm_rbm_class_stack_train_step, no host wait between the batches
int bm_rbm_class_stack_train_epoch(bm_rbm *top, bm_rbm *const *below, int32_t n_below, const float *X_dev, const int32_t *y_dev, int64_t N,
                                   int32_t batch, const float *lr, float mom, float *out2) {
    BM_CHECK(top && X_dev && y_dev && lr, "null argument");
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    BM_TRY(check_stack(top, below, n_below, "bm_rbm_class_stack_train_epoch", (int)((N < batch) ? N : batch)));
    const StackBelow s{below, n_below};
    const int V0 = n_below ? below[0]->V : top->V;
    if (out2) BM_HIP(hipMemsetAsync(top->cls_acc.p, 0, 2 * sizeof(double), top->stream));
    for (int64_t r = 0; r < N; r += batch) {
        const int B = (int)((N - r < batch) ? (N - r) : batch);
        BM_TRY(stack_update(top, s, X_dev + (size_t)r * V0, y_dev + r, B, lr, mom, out2 != nullptr));
    }
    return out2 ? stack_fetch(top, s, (double)N, out2) : 0;
}

// log p(c|x) of B rows through the stack (any B): slices of at most the smallest max_batch among the layers below go up the
// stack one after the other - the hm workspaces of the layers are never outgrown, the top's grow to the slice
int bm_rbm_class_stack_log_proba(bm_rbm *top, bm_rbm *const *below, int32_t n_below, const float *X_dev, int32_t B, float *logp_host) {
    BM_CHECK(top && X_dev && logp_host, "null argument");
    BM_CHECK(B >= 1, "bad row count %d", (int)B);
    BM_TRY(check_stack(top, below, n_below, "bm_rbm_class_stack_log_proba", 1));
    if (n_below == 0) return bm_rbm_class_log_proba(top, X_dev, B, logp_host);
    int slice = B;
    for (int l = 0; l < n_below; ++l) slice = std::min(slice, below[l]->maxB);
    BM_TRY(ensure_class_rows(top, slice));
    const size_t C = (size_t)top->n_classes;
    for (int r = 0; r < B; r += slice) {
        const int n = std::min(slice, B - r);
        const float *in = X_dev + (size_t)r * below[0]->V;
        int ldin = below[0]->V;
        for (int l = 0; l < n_below; ++l) {
            stack_up(below[l], in, ldin, n);
            hand_over(below[l], (l + 1 < n_below) ? below[l + 1] : top);
            in = below[l]->hm.p; ldin = below[l]->hm.ld;
        }
        class_forward(top, in, n, nullptr, pad_ld(top->H), nullptr, ldin);
        BM_HIP(hipGetLastError());
        BM_HIP(hipMemcpyAsync(logp_host + (size_t)r * C, top->cls_logp.p, (size_t)n * C * sizeof(float), hipMemcpyDeviceToHost, top->stream));
        hand_over(top, below[0]);          // the next slice overwrites hm of every layer: behind this slice's readers
    }
    BM_HIP(hipStreamSynchronize(top->stream));
    return 0;
}

// a_D of B rows (any B) to the device matrix A_dev [B][H_D] (dense): the prop-ups of bm_rbm_class_stack_log_proba, in its slices
int bm_rbm_stack_transform(bm_rbm *const *below, int32_t n_below, const float *X_dev, int32_t B, float *A_dev) {
    BM_CHECK(below && n_below >= 1 && X_dev && A_dev, "null argument");
    BM_CHECK(B >= 1, "bad row count %d", (int)B);
    int slice = B;
    for (int l = 0; l < n_below; ++l) {
        BM_CHECK(below[l], "null argument");
        for (int m = 0; m < l; ++m) BM_CHECK(below[l] != below[m], "bm_rbm_stack_transform: the same handle twice (layers %d and %d)", m, l);
        if (l) BM_CHECK(below[l - 1]->H == below[l]->V, "bm_rbm_stack_transform: the widths do not chain (layer %d has %d hidden units, "
                        "the layer above it %d visible)", l - 1, below[l - 1]->H, below[l]->V);
        BM_TRY(check_stack_layer(below[l], "bm_rbm_stack_transform", 1, false));
        slice = std::min(slice, below[l]->maxB);
    }
    bm_rbm *last = below[n_below - 1];
    for (int r = 0; r < B; r += slice) {
        const int n = std::min(slice, B - r);
        const float *in = X_dev + (size_t)r * below[0]->V;
        int ldin = below[0]->V;
        for (int l = 0; l < n_below; ++l) {
            stack_up(below[l], in, ldin, n);
            if (l + 1 < n_below) hand_over(below[l], below[l + 1]);
            in = below[l]->hm.p; ldin = below[l]->hm.ld;
        }
        BM_HIP(hipGetLastError());
        BM_HIP(hipMemcpy2DAsync(A_dev + (size_t)r * last->H, (size_t)last->H * sizeof(float), last->hm.p, (size_t)last->hm.ld * sizeof(float),
                                (size_t)last->H * sizeof(float), n, hipMemcpyDeviceToDevice, last->stream));
        hand_over(last, below[0]);
    }
    BM_HIP(hipStreamSynchronize(last->stream));
    return 0;
}

// ---- joint training of p(x, y) and sampling by class (bm355.h; bm_class.h)
static int ensure_class_joint(bm_rbm *h, bool disc) {
    if (!h->cj_yk.p) BM_TRY(h->cj_yk.alloc(h->maxB));
    if (disc && !h->cj_negm.p) {
        if (!h->cj_T.p) BM_TRY(h->cj_T.alloc(h->maxB, h->H));       // (the unlabelled update may have allocated it)
        BM_TRY(h->cj_pos.alloc(h->maxB, h->H)); BM_TRY(h->cj_negm.alloc(h->maxB, h->H));
    }
    return 0;
}
static int check_class_joint(const bm_rbm *h, const char *what, int B, int k, float gamma) {
    BM_TRY(check_class_train(h, what, B));
    BM_CHECK(k >= 1, "%s: n_gibbs_steps must be >= 1 (got %d)", what, k);
    BM_CHECK(gamma >= 0.f, "%s: disc_weight must be >= 0 (got %g)", what, (double)gamma);
    return 0;
}
// the prop-up given (x, y): the hidden pass with the class bias of row j's label
static LayerPass class_up(bm_rbm *h, int B, LayerIn vin, const int *y_dev, const LayerOut &out) {
    return rbm_pass(h, true, B, vin, out, 1.0f).class_bias(y_dev, h->U.p, h->H, h->n_classes, h->cls_bad.p);
}
// y ~ p(y | h) of B rows at Gibbs step t
static void class_draw(bm_rbm *h, LayerIn hin, int B, int t, int *y_out) {
    ProfScope _ps(h, KC_OTHER);
    ClassDrawArgs d;
    memset(&d, 0, sizeof(d));
    d.h = hin.p; d.ldh = hin.ld; d.U = h->U.p; d.ldu = h->H; d.yb = h->yb.p; d.y = y_out;
    d.B = B; d.H = h->H; d.C = h->n_classes;
    d.key = make_key(h, SITE_CLASS_Y, t); d.row0 = h->row0;
    launch_class_draw(d, h->stream);
}
// The CD-k chain on (x, y), run_chain as per-pass launches: h0 from (X, y); per step the plain visible pass and the class draw
// from the same hidden input, then the prop-up given (v_k, y_k).  Leaves h0m / h0s, vs, cj_yk and - last step - hneg = -h_k
// (keep_hm: hm = h_k instead), and Xin, as run_chain does
static int class_joint_chain(bm_rbm *h, const float *X_dev, const int *y_dev, int B, int k, bool keep_hm) {
    ensure_wt(h);
    h->Xin = X_dev; h->Xin_ld = h->V;
    h->fe_in_chain = false;
    issue(h, class_up(h, B, LayerIn{X_dev, h->V}, y_dev, rbm_out(h, 1, h->h0m.p, h->h0s.p, h->h0m.ld, SITE_H0, 0)));
    LayerIn hstate = in_of(h->cfg.sample_h_states ? h->h0s : h->h0m);
    for (int t = 0; t < k; ++t) {
        const bool last = t == k - 1, neg_only = last && !keep_hm;
        issue(h, rbm_pass(h, false, B, hstate, rbm_out(h, h->cfg.sample_v_states, nullptr, h->vs.p, h->vs.ld, SITE_V, t)));
        class_draw(h, hstate, B, t, h->cj_yk.p);
        LayerPass up = class_up(h, B, in_of(h->vs), h->cj_yk.p,
                                rbm_out(h, h->cfg.sample_h_states, neg_only ? nullptr : h->hm.p, last ? nullptr : h->hs.p, h->hm.ld, SITE_H, t));
        if (neg_only) up.negmeans_out(h->hneg.p);         // the last step as the plain update has it: only -h_k is consumed
        h->hm_is_neg = neg_only;
        issue(h, up);
        hstate = in_of(h->hs);
    }
    return 0;
}
// one update of L_gen + gamma L_disc; `sum`: the batch's sums of log p(t|x) and of the hits, taken before the update, are added
// to cls_acc.  Queues only
static int class_joint_update(bm_rbm *h, const float *X_dev, const int *y_dev, int B, int k, float lr, float mom, float gamma, bool sum) {
    const bool disc = gamma > 0.f;
    BM_TRY(ensure_class_joint(h, disc));
    if (disc || sum) {      // launches 1 - 3 of the discriminative update (3.18) into workspaces of their own; gamma == 0: 1 - 2, metric only
        class_forward(h, X_dev, B, disc ? h->cj_T.p : nullptr, disc ? h->cj_T.ld : pad_ld(h->H), y_dev);
        ProfScope _ps(h, KC_COLSUM);
        if (disc) {
            ClassHiddenArgs c;
            memset(&c, 0, sizeof(c));
            c.T = h->cj_T.p; c.ldt = h->cj_T.ld; c.U = h->U.p; c.ldu = h->H; c.prob = h->cls_prob.p; c.tl = h->cls_tl.p;
            c.pos = h->cj_pos.p; c.negm = h->cj_negm.p; c.ld = h->cj_pos.ld; c.B = B; c.H = h->H; c.C = h->n_classes;
            launch_class_hidden(c, h->stream);
        }
        if (sum) launch_class_sum(h->cls_rowlp.p, h->cls_rowhit.p, B, h->cls_acc.p, h->stream);
    }
    BM_TRY(class_joint_chain(h, X_dev, y_dev, B, k, false));
    {   // U, yb: from the chain's own h0m (before the hybrid objective rewrites it) and -h_k, the OLD U throughout
        ProfScope _ps(h, KC_BIAS);
        ClassJointArgs u;
        memset(&u, 0, sizeof(u));
        u.y = y_dev; u.yk = h->cj_yk.p; u.h0m = h->h0m.p; u.ldh0 = h->h0m.ld; u.hk = h->hneg.p; u.ldhk = h->hneg.ld; u.hk_neg = 1;
        u.gamma = gamma;
        if (disc) { u.coef = h->cls_coef.p; u.T = h->cj_T.p; u.ldt = h->cj_T.ld; }
        u.U = h->U.p; u.dU = h->dU.p; u.yb = h->yb.p; u.dyb = h->dyb.p; u.ldu = h->H; u.B = B; u.H = h->H; u.C = h->n_classes;
        u.N = (float)B; u.l2 = h->cfg.l2; u.lr = lr; u.mom = mom;
        launch_class_joint_update(u, h->stream);
        // dW = X^T (h0m + gamma g) - v_k^T h_k: the positive-phase operand takes the discriminative part, the fused update stays as it is
        if (disc) launch_class_mix(h->h0m.p, h->cj_pos.p, h->cj_negm.p, h->h0m.ld, B, h->H, gamma, h->stream);
    }
    launch_update_fused(h, B, lr, mom);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

int bm_rbm_class_joint_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int32_t B, int32_t k, float lr, float mom,
                                  float disc_weight, float *out2) {
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_TRY(check_class_joint(h, "bm_rbm_class_joint_train_step", B, k, disc_weight));
    BM_TRY(check_dw(h, "bm_rbm_class_joint_train_step"));
    if (out2) BM_HIP(hipMemsetAsync(h->cls_acc.p, 0, 2 * sizeof(double), h->stream));
    BM_TRY(class_joint_update(h, X_dev, y_dev, B, k, lr, mom, disc_weight, out2 != nullptr));
    return out2 ? class_fetch(h, (double)B, out2) : 0;
}

// N rows as consecutive minibatches of `batch` rows, driven from C: the launches of the caller's own loop over
// bm_rbm_class_joint_train_step, no host wait between the batches
int bm_rbm_class_joint_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int64_t N, int32_t batch, int32_t k, float lr,
                                   float mom, float disc_weight, float *out2) {
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    BM_TRY(check_class_joint(h, "bm_rbm_class_joint_train_epoch", (int)((N < batch) ? N : batch), k, disc_weight));
    BM_TRY(check_dw(h, "bm_rbm_class_joint_train_epoch"));
    if (out2) BM_HIP(hipMemsetAsync(h->cls_acc.p, 0, 2 * sizeof(double), h->stream));
    for (int64_t s = 0; s < N; s += batch) {
        const int B = (int)((N - s < batch) ? (N - s) : batch);
        BM_TRY(class_joint_update(h, X_dev + (size_t)s * h->V, y_dev + s, B, k, lr, mom, disc_weight, out2 != nullptr));
    }
    return out2 ? class_fetch(h, (double)N, out2) : 0;
}

// the chain of one joint update without the update, its states to the host (any pointer may be null); synchronises
int bm_rbm_class_joint_chain(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int32_t B, int32_t k, float *h0m_host, float *h0s_host,
                             float *vk_host, int32_t *yk_host, float *hk_host) {
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_TRY(check_class_joint(h, "bm_rbm_class_joint_chain", B, k, 0.f));
    BM_TRY(ensure_class_joint(h, false));
    BM_TRY(class_joint_chain(h, X_dev, y_dev, B, k, true));
    h->call++;
    BM_HIP(hipGetLastError());
    const struct { float *dst; const Mat *src; int cols; } out[4] = {{h0m_host, &h->h0m, h->H}, {h0s_host, &h->h0s, h->H}, {vk_host, &h->vs, h->V},
                                                                    {hk_host, &h->hm, h->H}};
    for (const auto &o : out)
        if (o.dst)
            BM_HIP(hipMemcpy2DAsync(o.dst, (size_t)o.cols * sizeof(float), o.src->p, (size_t)o.src->ld * sizeof(float), (size_t)o.cols * sizeof(float),
                                    (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (yk_host) BM_HIP(hipMemcpyAsync(yk_host, h->cj_yk.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));
    return check_class_labels(h);
}

// ---- semi-supervised training: the update on unlabelled rows and the interleaved epoch (bm355.h; bm_class.h)
static int ensure_class_semi(bm_rbm *h) {
    BM_TRY(ensure_class_joint(h, false));
    if (!h->cj_T.p) BM_TRY(h->cj_T.alloc(h->maxB, h->H));
    if (!h->cs_acc.p) {
        BM_TRY(h->cs_y0.alloc(h->maxB)); BM_TRY(h->cs_ent.alloc(h->maxB)); BM_TRY(h->cs_conf.alloc(h->maxB));
        BM_TRY(h->cs_acc.alloc(2));
    }
    return 0;
}
// launches 1 - 4 of the unlabelled update: the forward pass, the posterior draw, the chain on (X, y0), then h0m := em (AFTER the
// chain, whose h0 pass writes h0m).  `sum`: the batch's sums of the posterior entropy and of max_c p(c|x) are added to cs_acc
static int class_unsup_chain(bm_rbm *h, const float *X_dev, int B, int k, bool keep_hm, bool sum) {
    class_forward(h, X_dev, B, h->cj_T.p, h->cj_T.ld, nullptr);
    {
        ProfScope _ps(h, KC_OTHER);
        ClassPosteriorArgs q;
        memset(&q, 0, sizeof(q));
        q.prob = h->cls_prob.p; q.y0 = h->cs_y0.p; q.ent = h->cs_ent.p; q.conf = h->cs_conf.p; q.B = B; q.C = h->n_classes;
        q.key = make_key(h, SITE_CLASS_Y0, 0); q.row0 = h->row0;
        launch_class_posterior(q, h->stream);
        if (sum) launch_class_sum(h->cs_ent.p, h->cs_conf.p, B, h->cs_acc.p, h->stream);
    }
    BM_TRY(class_joint_chain(h, X_dev, h->cs_y0.p, B, k, keep_hm));
    ProfScope _ps(h, KC_COLSUM);
    ClassMarginalArgs m;
    memset(&m, 0, sizeof(m));
    m.T = h->cj_T.p; m.ldt = h->cj_T.ld; m.U = h->U.p; m.ldu = h->H; m.prob = h->cls_prob.p;
    m.em = h->h0m.p; m.ld = h->h0m.ld; m.B = B; m.H = h->H; m.C = h->n_classes;
    launch_class_marginal(m, h->stream);
    return 0;
}
// one update on B unlabelled rows.  Queues only
static int class_unsup_update(bm_rbm *h, const float *X_dev, int B, int k, float lr, float mom, bool sum) {
    BM_TRY(class_unsup_chain(h, X_dev, B, k, false, sum));
    {   // U, yb: from prob, t and -h_k, the OLD U throughout
        ProfScope _ps(h, KC_BIAS);
        ClassUnsupArgs u;
        memset(&u, 0, sizeof(u));
        u.yk = h->cj_yk.p; u.prob = h->cls_prob.p; u.T = h->cj_T.p; u.ldt = h->cj_T.ld; u.hkneg = h->hneg.p; u.ldhk = h->hneg.ld;
        u.U = h->U.p; u.dU = h->dU.p; u.yb = h->yb.p; u.dyb = h->dyb.p; u.ldu = h->H; u.B = B; u.H = h->H; u.C = h->n_classes;
        u.N = (float)B; u.l2 = h->cfg.l2; u.lr = lr; u.mom = mom;
        launch_class_unsup_update(u, h->stream);
    }
    launch_update_fused(h, B, lr, mom);                   // dW = (X^T em - v_k^T h_k) / B, dhb, dvb: the fused update as it is
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}
// the sums of cls_acc / cs_acc to the host as means over their own rows (a null target or no rows: skipped); synchronises
static int class_semi_fetch(bm_rbm *h, double rows, float *out_l, double rows_u, float *out_u) {
    double hl[2] = {0.0, 0.0}, hu[2] = {0.0, 0.0};
    if (out_l) BM_HIP(hipMemcpyAsync(hl, h->cls_acc.p, sizeof(hl), hipMemcpyDeviceToHost, h->stream));
    if (out_u && rows_u > 0) BM_HIP(hipMemcpyAsync(hu, h->cs_acc.p, sizeof(hu), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));
    BM_TRY(check_class_labels(h));
    if (out_l) { out_l[0] = (float)(hl[0] / rows); out_l[1] = (float)(hl[1] / rows); }
    if (out_u) { out_u[0] = rows_u > 0 ? (float)(hu[0] / rows_u) : 0.f; out_u[1] = rows_u > 0 ? (float)(hu[1] / rows_u) : 0.f; }
    return 0;
}

int bm_rbm_class_unsup_train_step(bm_rbm *h, const float *X_dev, int32_t B, int32_t k, float lr, float mom, float *out2) {
    BM_CHECK(h && X_dev, "null argument");
    BM_TRY(check_class_joint(h, "bm_rbm_class_unsup_train_step", B, k, 0.f));
    BM_TRY(check_dw(h, "bm_rbm_class_unsup_train_step"));
    BM_TRY(ensure_class_semi(h));
    if (out2) BM_HIP(hipMemsetAsync(h->cs_acc.p, 0, 2 * sizeof(double), h->stream));
    BM_TRY(class_unsup_update(h, X_dev, B, k, lr, mom, out2 != nullptr));
    return out2 ? class_semi_fetch(h, 0.0, nullptr, (double)B, out2) : 0;
}

// the chain and the positive operand of one unlabelled update without the update, to the host (any pointer may be null);
// synchronises
int bm_rbm_class_unsup_chain(bm_rbm *h, const float *X_dev, int32_t B, int32_t k, int32_t *y0_host, float *em_host, float *h0s_host,
                             float *vk_host, int32_t *yk_host, float *hk_host) {
    BM_CHECK(h && X_dev, "null argument");
    BM_TRY(check_class_joint(h, "bm_rbm_class_unsup_chain", B, k, 0.f));
    BM_TRY(ensure_class_semi(h));
    BM_TRY(class_unsup_chain(h, X_dev, B, k, true, false));
    h->call++;
    BM_HIP(hipGetLastError());
    const struct { float *dst; const Mat *src; int cols; } out[4] = {{em_host, &h->h0m, h->H}, {h0s_host, &h->h0s, h->H}, {vk_host, &h->vs, h->V},
                                                                    {hk_host, &h->hm, h->H}};
    for (const auto &o : out)
        if (o.dst)
            BM_HIP(hipMemcpy2DAsync(o.dst, (size_t)o.cols * sizeof(float), o.src->p, (size_t)o.src->ld * sizeof(float), (size_t)o.cols * sizeof(float),
                                    (size_t)B, hipMemcpyDeviceToHost, h->stream));
    if (y0_host) BM_HIP(hipMemcpyAsync(y0_host, h->cs_y0.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (yk_host) BM_HIP(hipMemcpyAsync(yk_host, h->cj_yk.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_TRY(check_device_status(h));
    return check_class_labels(h);
}

// One semi-supervised epoch, driven from C with no host wait between the batches: per labelled batch the joint update with lr,
// then one unlabelled update with lr * unl_weight on the next slice of `batch` rows of Xu (a short last slice; cyclic, from slice
// u_slice).  unl_weight == 0: bm_rbm_class_joint_train_epoch's launches and nothing else
int bm_rbm_class_semi_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int64_t N, const float *Xu_dev, int64_t Nu,
                                  int64_t u_slice, int32_t batch, int32_t k, float lr, float mom, float disc_weight, float unl_weight,
                                  float *out4) {
    const char *what = "bm_rbm_class_semi_train_epoch";
    BM_CHECK(h && X_dev && y_dev, "null argument");
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    BM_TRY(check_class_joint(h, what, (int)((N < batch) ? N : batch), k, disc_weight));
    BM_CHECK(unl_weight >= 0.f, "%s: unl_weight must be >= 0 (got %g)", what, (double)unl_weight);
    const bool unl = unl_weight > 0.f;
    if (unl) {
        BM_CHECK(Xu_dev && Nu >= 1, "%s: unl_weight > 0 needs unlabelled rows (Xu %s, Nu = %lld)", what, Xu_dev ? "given" : "null", (long long)Nu);
        BM_CHECK(((Nu < batch) ? Nu : batch) <= h->maxB, "batch %d outside [1, max_batch=%d]", batch, h->maxB);
    }
    const int64_t n_slices = Nu >= 1 ? (Nu + batch - 1) / batch : 0;
    BM_CHECK(u_slice >= 0 && u_slice < (n_slices > 1 ? n_slices : 1), "%s: u_slice %lld outside [0, %lld slices of Xu)", what, (long long)u_slice,
             (long long)(n_slices > 1 ? n_slices : 1));
    BM_TRY(check_dw(h, what));
    if (unl) BM_TRY(ensure_class_semi(h));
    const float lr_u = lr * unl_weight;
    if (out4) {
        BM_HIP(hipMemsetAsync(h->cls_acc.p, 0, 2 * sizeof(double), h->stream));
        if (unl) BM_HIP(hipMemsetAsync(h->cs_acc.p, 0, 2 * sizeof(double), h->stream));
    }
    int64_t u = u_slice, rows_u = 0;
    for (int64_t s = 0; s < N; s += batch) {
        const int B = (int)((N - s < batch) ? (N - s) : batch);
        BM_TRY(class_joint_update(h, X_dev + (size_t)s * h->V, y_dev + s, B, k, lr, mom, disc_weight, out4 != nullptr));
        if (!unl) continue;
        const int64_t r = u * batch;
        const int Bu = (int)((Nu - r < batch) ? (Nu - r) : batch);
        BM_TRY(class_unsup_update(h, Xu_dev + (size_t)r * h->V, Bu, k, lr_u, mom, out4 != nullptr));
        rows_u += Bu;
        u = (u + 1) % n_slices;
    }
    return out4 ? class_semi_fetch(h, (double)N, out4, (double)rows_u, out4 + 2) : 0;
}

// Class-conditional sampling: n_steps of h ~ p(h | v, y), v ~ p(v | h) with y clamped, from V_dev (dense [B][V]) or - null - from
// v_0 ~ Ber(1/2).  Per-pass fp32 launches, both layers sampled, rows drawn by global position (bm_rbm_set_row_offset)
int bm_rbm_class_gibbs(bm_rbm *h, const float *V_dev, const int32_t *y_dev, int32_t B, int32_t n_steps, float *out_v, float *out_vmeans) {
    BM_CHECK(h && y_dev && out_v, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_class_gibbs"));
    BM_CHECK(h->n_classes, "bm_rbm_class_gibbs: no class head is attached (bm_rbm_set_classes)");
    BM_TRY(check_single_joint(h, "bm_rbm_class_gibbs"));
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_CHECK(n_steps >= 1, "n_steps must be >= 1 (got %d)", (int)n_steps);
    ensure_wt(h);
    LayerIn vin{V_dev, h->V};
    if (!V_dev) {
        launch_class_v0(h->vs.p, h->vs.ld, B, h->V, make_key(h, SITE_CLASS_V0, 0), h->row0, h->stream);
        vin = in_of(h->vs);
    }
    for (int t = 0; t < n_steps; ++t) {
        const bool last = t == n_steps - 1;
        issue(h, class_up(h, B, vin, y_dev, rbm_out(h, 1, nullptr, h->hs.p, h->hs.ld, SITE_H, t)));
        issue(h, rbm_pass(h, false, B, in_of(h->hs), rbm_out(h, 1, last ? out_vmeans : nullptr, last ? out_v : h->vs.p, last ? h->V : h->vs.ld, SITE_V, t),
                          1.0f));
        vin = in_of(h->vs);
    }
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// AIS from the base-rate model p_0(v) ~ exp(a.v) to the RBM, the hidden layer summed out (Salakhutdinov & Murray 2008):
//   log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta z_j),   z = v W + hb,   beta_k = linspace(0, 1, n_betas)[k]
// Per beta step k: ONE prop-up scores v_{k-1} (softplus differences of (beta_{k-1}, beta_k) as slot partials) and samples h at
// beta_k from the same pre-activation; the score kernel adds them and (beta_k - beta_{k-1}) v_{k-1}.(vb - a) - the slot partials
// the prop-down that made v_{k-1} left - to the double log-weights; then the prop-down, and n_gibbs_steps - 1 more up / down
// pairs.  Between the uploads in front of the loop and the download behind it the host only enqueues.  fp32 path always.
//
// What the AIS entries of the handle share (bm_rbm_ais, bm_rbm_groups_ais, bm_rbm_rsm_ais): the beta ladder, the upload of the base
// logits, the table of mixed biases, the host loop with its seeds, the prop-up with its softplus partials, the score and the double
// log-weights.  An entry brings log Z_0 of its base model (one number, or logZ0_rows [R] where it differs by chain), start() - v_0
// into av and the partials of v_0.(vb - a) - and down(beta, kbeta, key, dot) - its visible transition from ah into av, which with
// `dot` leaves the partials of v.(vb - a); vdot [vdot_slots][ais_rows] is where those partials are; lengths: ais_up's.  The AIS
// workspaces for R rows exist (ensure_ais_rows)
static int ais_run(bm_rbm *h, int n_betas, int R, int k, const float *base_bias_host, uint64_t seed, int64_t chain0, const float *lengths,
                   const float *vdot, int vdot_slots, double logZ0, const double *logZ0_rows, float *values_host,
                   const std::function<void()> &start, const std::function<void(float, int, const PhiloxKey &, bool)> &down,
                   const float *vb_dev = nullptr) {
    // vb_dev: the device vector that stands where vb stands in dvec and in the table (bm_rbm_gauss_ais: the centre c); null: vb itself
    const int V = h->V, H = h->H;
    if (!h->abase.p) { BM_TRY(h->adot.alloc(V)); BM_TRY(h->abase.alloc(V)); }
    if (h->atable.n < (size_t)n_betas * V) { BM_TRY(h->abeta.alloc(n_betas)); BM_TRY(h->atable.alloc((size_t)n_betas * V)); }
    // beta_k as float(np.linspace(0, 1, n_betas)[k])
    std::vector<float> beta(n_betas);
    const double step = 1.0 / (double)(n_betas - 1);
    for (int b = 0; b < n_betas; ++b) beta[b] = (float)((double)b * step);
    beta[n_betas - 1] = 1.0f;
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipMemcpy(h->abeta.p, beta.data(), (size_t)n_betas * sizeof(float), hipMemcpyHostToDevice));
    if (base_bias_host) BM_HIP(hipMemcpy(h->abase.p, base_bias_host, (size_t)V * sizeof(float), hipMemcpyHostToDevice));
    else BM_HIP(hipMemset(h->abase.p, 0, (size_t)V * sizeof(float)));
    ensure_wt(h);
    hipLaunchKernelGGL(rbm_ais_prep_kernel, dim3(512), dim3(256), 0, h->stream, vb_dev ? vb_dev : (const float *)h->vb.p, (const float *)h->abase.p,
                       (const float *)h->abeta.p, (int)n_betas, V, h->adot.p, h->atable.p);
    BM_HIP(hipMemsetAsync(h->alogw.p, 0, (size_t)R * sizeof(double), h->stream));
    const int ldp = h->ais_rows;
    start();
    AisScoreArgs sc;
    memset(&sc, 0, sizeof(sc));
    sc.ne = 1; sc.pe[0] = h->apart_h.p; sc.ne_slots[0] = nslots(H);
    sc.no = 1; sc.po[0] = vdot; sc.no_slots[0] = vdot_slots;
    for (int b = 1; b < n_betas; ++b) {
        const bool last = b == n_betas - 1;            // no transition behind the last score
        const float ba = beta[b - 1], bb = beta[b];
        ais_up(h, R, bb, last ? 0 : 1, ais_key(seed, SITE_AIS_H, 0, (uint32_t)b), chain0, true, ba, lengths);
        hipLaunchKernelGGL(ais_score_kernel, dim3((R + 31) / 32), dim3(256), 0, h->stream, h->alogw.p, R, ldp, sc, bb - ba);
        if (last) break;
        for (int t = 0; t < k; ++t) {
            if (t > 0) ais_up(h, R, bb, 1, ais_key(seed, SITE_AIS_H, t, (uint32_t)b), chain0, false, 0.f, lengths);
            down(bb, b, ais_key(seed, SITE_AIS_V, t, (uint32_t)b), t == k - 1);
        }
    }
    BM_HIP(hipGetLastError());
    std::vector<double> w(R);
    BM_HIP(hipMemcpyAsync(w.data(), h->alogw.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    for (int r = 0; r < R; ++r) values_host[r] = (float)(w[r] + (logZ0_rows ? logZ0_rows[r] : logZ0));
    return 0;
}

int bm_rbm_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t k, const float *base_bias_host, uint64_t seed, int64_t chain0,
               float *values_host) {
    BM_CHECK(h && values_host, "null argument");
    BM_CHECK(!h->rsm_len, "bm_rbm_ais is not available for replicated softmax visible units (bm_rbm_set_replicated_softmax: max_length %d): "
             "log Z depends on the document length there, bm_rbm_rsm_ais estimates it; see DESIGN.md 3.28", h->rsm_len);
    BM_TRY(check_single_joint(h, "bm_rbm_ais"));
    BM_CHECK(n_betas >= 2 && n_runs >= 1 && k >= 1, "bad AIS arguments (n_betas %d >= 2, n_runs %d >= 1, n_gibbs_steps %d >= 1)",
             (int)n_betas, (int)n_runs, (int)k);
    const int R = n_runs, V = h->V, H = h->H;
    BM_TRY(ensure_ais_rows(h, R));
    // log Z_0 = H log 2 + sum_i softplus(a_i) in double
    double logZ0 = (double)H * log(2.0);
    for (int i = 0; i < V; ++i) {
        const double ai = base_bias_host ? (double)base_bias_host[i] : 0.0;
        logZ0 += fmax(ai, 0.0) + log1p(exp(-fabs(ai)));
    }
    return ais_run(h, n_betas, R, k, base_bias_host, seed, chain0, nullptr, h->apart_v.p, nslots(V), logZ0, nullptr, values_host,
                   [&] {
                       hipLaunchKernelGGL(rbm_ais_init_kernel, dim3((R + 3) / 4), dim3(256), 0, h->stream, h->av.p, h->av.ld, R, V,
                                          (const float *)h->abase.p, (const float *)h->adot.p, ais_key(seed, SITE_AIS_V0, 0, 0),
                                          (unsigned long long)chain0, h->apart_v.p, h->ais_rows, nslots(V));
                   },
                   [&](float bb, int b, const PhiloxKey &key, bool dot) { ais_down(h, R, bb, b, key, chain0, dot); });
}

int bm_rbm_gibbs(bm_rbm *h, float *H_dev, float *V_dev, int32_t B, int32_t n_steps) {
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_CHECK(H_dev && V_dev, "null state pointer");
    BM_CHECK(n_steps >= 1, "n_steps must be >= 1");
    struct FastScope { bm_rbm *h; ~FastScope() { h->fast_now = false; } } fast_scope{h};
    const bool fast = h->fast && h->cfg.v_unit == BM_UNIT_BERNOULLI && !h->multinomial() && !h->nrelu() && !h->v_groups && !h->rsm_len &&
                      h->cfg.sample_v_states && h->cfg.sample_h_states && h->cfg.dropout < 0.f;
    BM_TRY(rsm_use_row_lengths(h, "bm_rbm_gibbs", B));
    if (!fast && !h->multinomial()) {
        // The sweeps read and write the caller's dense buffers IN PLACE: the first prop-down takes H_dev (pitch H) as its
        // operand, the last sweep's launches store straight into V_dev / H_dev - no copy kernels (round 3 moved the
        // states through the pitched workspaces with three copy2d launches per call: 5 % of the sweep benchmark).
        ensure_wt(h);
        chain_begin(h);
        for (int t = 0; t < n_steps; ++t) {
            const bool first = t == 0, last = t == n_steps - 1;
            const LayerIn hin = first ? LayerIn{H_dev, h->H} : in_of(h->hs);
            float *vnew = last ? V_dev : h->vs.p, *hnew = last ? H_dev : h->hs.p;
            const int ldv = last ? h->V : h->vs.ld, ldh = last ? h->H : h->hs.ld;
            issue(h, rbm_pass(h, false, B, hin, rbm_out(h, h->cfg.sample_v_states, nullptr, vnew, ldv, SITE_V, t)));
            issue(h, rbm_pass(h, true, B, LayerIn{vnew, ldv}, rbm_out(h, h->cfg.sample_h_states, nullptr, hnew, ldh, SITE_H, t)));
        }
        BM_TRY(chain_end(h));
        h->call++;
        BM_HIP(hipGetLastError());
        return 0;
    }
    // fast-binary / Multinomial sweeps: dense user buffers <-> pitched workspaces (hs / vs, which carry the bf16 shadows)
    hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)H_dev, h->H, h->hs.p, h->hs.ld, B, h->H);
    if (fast) {
        // fast-binary sweep: both layers are sampled, so every contraction has a {0,1} operand (the caller's hidden
        // states must be a bitmap as well: checked on the device, reported by bm_rbm_sync)
        if (!h->nonbinary.p) {        // (allocated last: the planes and shadows are complete once it exists)
            BM_TRY(h->W3.alloc(3, h->V, h->H)); BM_TRY(h->W3t.alloc(3, h->H, h->V));
            BM_TRY(h->hs16.alloc(1, h->maxB, h->H)); BM_TRY(h->vs16.alloc(1, h->maxB, h->V));
            BM_TRY(h->nonbinary.alloc(1));
            BM_HIP(hipMemsetAsync(h->nonbinary.p, 0, sizeof(int), h->stream));
        }
        hipLaunchKernelGGL(split3_kernel, dim3(512), dim3(256), 0, h->stream, (const float *)h->W.p, h->W.ld, h->V, h->H,
                           h->W3.p, h->W3.plane_stride(), h->W3.ld, 0);
        hipLaunchKernelGGL(split3_kernel, dim3(512), dim3(256), 0, h->stream, (const float *)h->W.p, h->W.ld, h->V, h->H,
                           h->W3t.p, h->W3t.plane_stride(), h->W3t.ld, 1);
        hipLaunchKernelGGL(shadow16_check_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)h->hs.p, h->hs.ld, B, h->H,
                           h->hs16.p, h->hs16.ld, h->nonbinary.p);
        h->fast_now = true;
    }
    for (int t = 0; t < n_steps; ++t) {
        issue(h, rbm_pass(h, false, B, in_of(h->hs), rbm_out(h, h->cfg.sample_v_states, nullptr, h->vs.p, h->vs.ld, SITE_V, t)));
        issue(h, rbm_pass(h, true, B, in_of(h->vs), rbm_out(h, h->cfg.sample_h_states, nullptr, h->hs.p, h->hs.ld, SITE_H, t)));
    }
    hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)h->hs.p, h->hs.ld, H_dev, h->H, B, h->H);
    hipLaunchKernelGGL(copy2d_kernel, dim3(256), dim3(256), 0, h->stream, (const float *)h->vs.p, h->vs.ld, V_dev, h->V, B, h->V);
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// Block-Gibbs with clamped visible units: n_steps of v -> h -> v from the visible states in V_dev, the entries
// with a non-zero mask held at clamp_val - overwritten in V_dev first (clamp_apply_kernel), then in the epilogue of every
// prop-down (the CL flavour of act_kernel).  Always per-pass fp32 launches - no chained launch, no fast-binary sweep (clamp
// values may be grey levels) - so the call returns the same bits in every mode; both layers are sampled (as in bm_rbm_ais).
// The sweeps run in place on the caller's dense buffers like bm_rbm_gibbs; hs / vs are the only workspaces touched.
int bm_rbm_gibbs_clamped(bm_rbm *h, float *V_dev, float *H_dev, float *Vmean_dev, int32_t B, int32_t n_steps,
                         const float *clamp_val_dev, const float *clamp_mask_dev) {
    BM_CHECK(h, "null argument");
    BM_TRY(refuse_nrelu(h, "bm_rbm_gibbs_clamped"));
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_CHECK(V_dev && H_dev && clamp_val_dev && clamp_mask_dev, "null state or clamp pointer");
    BM_CHECK(n_steps >= 1, "n_steps must be >= 1 (got %d)", (int)n_steps);
    BM_CHECK(!h->multinomial(), "bm_rbm_gibbs_clamped: Multinomial hidden units are not supported (their sweep goes through the "
             "softmax pair and pitched copies, not the clamped epilogue)");
    ensure_wt(h);
    hipLaunchKernelGGL(clamp_apply_kernel, dim3(256), dim3(256), 0, h->stream, V_dev, h->V, clamp_val_dev, clamp_mask_dev, h->V, B, h->V);
    for (int t = 0; t < n_steps; ++t) {
        const bool first = t == 0, last = t == n_steps - 1;
        const LayerIn vin = first ? LayerIn{V_dev, h->V} : in_of(h->vs);
        float *hnew = last ? H_dev : h->hs.p, *vnew = last ? V_dev : h->vs.p;
        const int ldh = last ? h->H : h->hs.ld, ldv = last ? h->V : h->vs.ld;
        issue(h, rbm_pass(h, true, B, vin, rbm_out(h, 1, nullptr, hnew, ldh, SITE_H, t)));
        issue(h, rbm_pass(h, false, B, LayerIn{hnew, ldh}, rbm_out(h, 1, last ? Vmean_dev : nullptr, vnew, ldv, SITE_V, t))
                     .clamp(clamp_val_dev, clamp_mask_dev, h->V));
    }
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// ---- softmax visible units: incomplete rows, clamped groups, exact group conditionals (bm355.h)
static int need_groups(const bm_rbm *h, const char *what) {
    BM_CHECK(h, "null argument");
    BM_CHECK(h->v_groups, "%s needs a handle with visible groups (softmax visible units: bm_rbm_set_visible_groups); this handle has none", what);
    return 0;
}

int bm_rbm_groups_set_missing(bm_rbm *h, int32_t on) {
    BM_TRY(need_groups(h, "bm_rbm_groups_set_missing"));
    h->groups_missing = on != 0;
    return 0;
}

// bm_rbm_gibbs_clamped for a handle with visible groups: the mask is constant within every group (the caller's guarantee).  The
// same launches, sites, call counter and row offset; the prop-down is the clamped softmax pass (SM + CL, or the generic pair)
int bm_rbm_groups_gibbs_clamped(bm_rbm *h, float *V_dev, float *H_dev, float *Vmean_dev, int32_t B, int32_t n_steps,
                                const float *clamp_val_dev, const float *clamp_mask_dev) {
    BM_TRY(need_groups(h, "bm_rbm_groups_gibbs_clamped"));
    BM_CHECK(B >= 1 && B <= h->maxB, "batch %d outside [1, max_batch=%d]", B, h->maxB);
    BM_CHECK(V_dev && H_dev && clamp_val_dev && clamp_mask_dev, "null state or clamp pointer");
    BM_CHECK(n_steps >= 1, "n_steps must be >= 1 (got %d)", (int)n_steps);
    ensure_wt(h);
    hipLaunchKernelGGL(clamp_apply_kernel, dim3(256), dim3(256), 0, h->stream, V_dev, h->V, clamp_val_dev, clamp_mask_dev, h->V, B, h->V);
    for (int t = 0; t < n_steps; ++t) {
        const bool first = t == 0, last = t == n_steps - 1;
        const LayerIn vin = first ? LayerIn{V_dev, h->V} : in_of(h->vs);
        float *hnew = last ? H_dev : h->hs.p, *vnew = last ? V_dev : h->vs.p;
        const int ldh = last ? h->H : h->hs.ld, ldv = last ? h->V : h->vs.ld;
        issue(h, rbm_pass(h, true, B, vin, rbm_out(h, 1, nullptr, hnew, ldh, SITE_H, t)));
        issue(h, rbm_pass(h, false, B, LayerIn{hnew, ldh}, rbm_out(h, 1, last ? Vmean_dev : nullptr, vnew, ldv, SITE_V, t))
                     .clamp(clamp_val_dev, clamp_mask_dev, h->V));
    }
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// S [B][V] (host, double) of GsArgs: per slice of at most max_batch rows one kind-3 prop-up into a workspace of its own (z = x W +
// hb in float32) and one group_scores_kernel launch.  No RNG call, no parameter and no shared workspace is touched
int bm_rbm_groups_scores(bm_rbm *h, const float *X_dev, int32_t B, double *scores_host) {
    BM_TRY(need_groups(h, "bm_rbm_groups_scores"));
    BM_CHECK(X_dev && scores_host, "null argument");
    BM_CHECK(B >= 1, "bad row count %d", (int)B);
    if (!h->gs_out.p) {
        BM_TRY(h->gs_z.alloc(h->maxB, h->H));
        BM_TRY(h->gs_out.alloc((size_t)h->maxB * h->V));
    }
    ensure_wt(h);
    for (int s = 0; s < B; s += h->maxB) {
        const int n = (B - s < h->maxB) ? B - s : h->maxB;
        const float *Xs = X_dev + (size_t)s * h->V;
        LayerPass p = rbm_pass(h, true, n, LayerIn{Xs, h->V}, LayerOut{0, h->gs_z.p, nullptr, h->gs_z.ld, PhiloxKey{0, 0, 0, 0}, 0}, 1.0f);
        p.a.kind = 3;                                  // stores z + hb
        issue(h, p);
        GsArgs g;
        memset(&g, 0, sizeof(g));
        g.X = Xs; g.ldx = h->V; g.Z = h->gs_z.p; g.ldz = h->gs_z.ld; g.W = h->W.p; g.ldw = h->W.ld; g.vb = h->vb.p;
        g.S = h->gs_out.p; g.B = n; g.V = h->V; g.H = h->H; g.K = h->v_groups;
        {
            ProfScope _ps(h, KC_OTHER);
            launch_group_scores(g, h->stream);
        }
        BM_HIP(hipGetLastError());
        BM_HIP(hipMemcpyAsync(scores_host + (size_t)s * h->V, h->gs_out.p, (size_t)n * h->V * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        BM_HIP(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// ---- AIS over softmax visible units (bm355.h: bm_rbm_groups_ais)

// the two routes of issue()'s softmax prop-down; BM355_DEBUG=sm_fused=0 forces the generic one
static bool groups_fused(const bm_rbm *h) {
    static const bool fused_off = bm::dbg("sm_fused") && atoi(bm::dbg("sm_fused")) == 0;
    const int K = h->v_groups;
    return !fused_off && (K == 2 || K == 4 || K == 8 || K == 16) && (h->V & 3) == 0;
}
// the workspaces of bm_rbm_ais for `rows` chains and, on the generic route, the logits of the prop-down; a failed allocation leaves
// nothing counted (ensure_ais_rows)
static int ensure_groups_ais_rows(bm_rbm *h, int rows) {
    BM_TRY(ensure_ais_rows(h, rows));
    if (!h->ga_zero.p) {
        BM_TRY(h->ga_absent.alloc(h->V)); BM_TRY(h->ga_zero.alloc(h->V));
        BM_HIP(hipMemset(h->ga_zero.p, 0, (size_t)h->V * sizeof(float)));
    }
    if (groups_fused(h) || rows <= h->ga_rows) return 0;
    h->ga_rows = 0;
    BM_TRY(h->ga_l.alloc(rows, h->V));
    h->ga_rows = rows;
    return 0;
}
// v_g ~ softmax_k(beta (h W^T)_{gK+k} + a + beta (vb - a)) for the groups that are there, zeros elsewhere, from ah into av, the mixed
// bias from row `kbeta` of the table; dot: the slot partials of v.(vb - a) in apart_v for the next score.  Fused route: ONE launch,
// the SM + SA flavour (which leaves the partials whether they are read or not); generic route: the logits pass, softmax_groups_kernel
// with the pattern as its clamp mask (pitch 0: every row reads the same [V] vectors) and - dot - the row-dot kernel
static void groups_ais_down(bm_rbm *h, int R, float beta, int kbeta, const PhiloxKey &key, int64_t chain0, bool dot, const float *absent) {
    LayerPass p = rbm_pass(h, false, R, in_of(h->ah), LayerOut{1, nullptr, h->av.p, h->av.ld, key, chain0}, beta)
                      .bias(h->atable.p + (size_t)kbeta * h->V, 1.0f);
    ActArgs &a = p.a;
    if (groups_fused(h)) {
        ProfScope _ps(h, KC_DOWN);
        p.statedot_rows(h->apart_v.p, h->ais_rows, h->adot.p);
        a.kind = 3; a.sm_k = h->v_groups; a.sm_ais = 1; a.sm_absent = absent;
        launch_act_sm_ais(a, h->stream);
        return;
    }
    SgArgs g;
    memset(&g, 0, sizeof(g));
    g.L = h->ga_l.p; g.ld = h->ga_l.ld; g.states = h->av.p; g.ld_states = h->av.ld;
    g.V = h->V; g.K = h->v_groups; g.J = R; g.sample = 1; g.key = key; g.row0 = chain0;
    if (absent) { g.clamp_val = h->ga_zero.p; g.clamp_mask = absent; g.ld_clamp = 0; }
    a.kind = 3; a.sample = 0; a.states = nullptr; a.means = h->ga_l.p; a.ldo = h->ga_l.ld;
    {
        ProfScope _ps(h, KC_DOWN);
        launch_act(a, h->stream);
    }
    ProfScope _ps(h, KC_OTHER);                        // (per-class event timing: the route's extra launches are the class `other`)
    launch_softmax_groups(g, h->stream);
    if (dot) launch_softmax_ais_dot(h->av.p, h->av.ld, R, h->V, h->adot.p, h->apart_v.p, h->ais_rows, h->stream);
}

// bm_rbm_ais with a categorical base model and softmax transitions over the observed groups; the host loop, the prop-up with its
// softplus partials, the score kernel and the double accumulation are bm_rbm_ais's own
int bm_rbm_groups_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t k, const float *base_bias_host, const uint8_t *observed_host,
                      uint64_t seed, int64_t chain0, float *values_host) {
    BM_TRY(need_groups(h, "bm_rbm_groups_ais"));
    BM_CHECK(values_host, "null argument");
    BM_CHECK(n_betas >= 2 && n_runs >= 1 && k >= 1, "bad AIS arguments (n_betas %d >= 2, n_runs %d >= 1, n_gibbs_steps %d >= 1)",
             (int)n_betas, (int)n_runs, (int)k);
    const int R = n_runs, V = h->V, H = h->H, K = h->v_groups, G = V / K;
    int n_obs = G;
    if (observed_host) { n_obs = 0; for (int g = 0; g < G; ++g) n_obs += observed_host[g] != 0; }
    BM_CHECK(n_obs >= 1, "bm_rbm_groups_ais: the pattern observes none of the %d groups (a model without visible units has no chain)", G);
    BM_TRY(ensure_groups_ais_rows(h, R));
    // log Z_0 = H log 2 + sum over the observed groups of logsumexp_k a, in double
    double logZ0 = (double)H * log(2.0);
    std::vector<float> absent_host(observed_host ? V : 0);
    for (int g = 0; g < G; ++g) {
        const bool there = !observed_host || observed_host[g] != 0;
        if (observed_host) for (int q = 0; q < K; ++q) absent_host[(size_t)g * K + q] = there ? 0.f : 1.f;
        if (!there) continue;
        double mx = -INFINITY, se = 0.0;
        for (int q = 0; q < K; ++q) mx = fmax(mx, base_bias_host ? (double)base_bias_host[(size_t)g * K + q] : 0.0);
        for (int q = 0; q < K; ++q) se += exp((base_bias_host ? (double)base_bias_host[(size_t)g * K + q] : 0.0) - mx);
        logZ0 += mx + log(se);
    }
    if (observed_host) {
        BM_HIP(hipStreamSynchronize(h->stream));
        BM_HIP(hipMemcpy(h->ga_absent.p, absent_host.data(), (size_t)V * sizeof(float), hipMemcpyHostToDevice));
    }
    const float *absent = observed_host ? h->ga_absent.p : nullptr;
    return ais_run(h, n_betas, R, k, base_bias_host, seed, chain0, nullptr, h->apart_v.p, nslots(V), logZ0, nullptr, values_host,
                   [&] {
                       SaStartArgs s0;
                       memset(&s0, 0, sizeof(s0));
                       s0.v = h->av.p; s0.ld = h->av.ld; s0.rows = R; s0.V = V; s0.K = K;
                       s0.abase = h->abase.p; s0.dvec = h->adot.p; s0.absent = absent;
                       s0.key = ais_key(seed, SITE_AIS_V0, 0, 0); s0.row0 = (unsigned long long)chain0;
                       s0.part = h->apart_v.p; s0.ld_part = h->ais_rows; s0.nslot = nslots(V);
                       launch_softmax_ais_start(s0, h->stream);
                   },
                   [&](float bb, int b, const PhiloxKey &key, bool dot) { groups_ais_down(h, R, bb, b, key, chain0, dot, absent); });
}

// ---- AIS per document length over replicated softmax visible units (bm355.h: bm_rbm_rsm_ais)

// the workspaces of bm_rbm_ais for `rows` chains and the run's own logits, lengths and v.dvec pair at the same pitch; a failed
// allocation leaves nothing counted (ensure_ais_rows)
static int ensure_rsm_ais_rows(bm_rbm *h, int rows) {
    BM_TRY(ensure_ais_rows(h, rows));
    if (h->ra_rows == h->ais_rows) return 0;
    h->ra_rows = 0;
    BM_TRY(h->ra_l.alloc(h->ais_rows, h->V)); BM_TRY(h->ra_len.alloc(h->ais_rows)); BM_TRY(h->ra_dot.alloc(2 * (size_t)h->ais_rows));
    h->ra_rows = h->ais_rows;
    return 0;
}
// the rows of ra_l, logits, become the chains' counts in av - D_r draws each at (chain0 + r) max_length + d of `key` - and leave
// the pair of v.(vb - a) in ra_dot: the AIS flavour of multinomial_counts_kernel (bm_rsm.h)
static void rsm_ais_counts(bm_rbm *h, int R, const PhiloxKey &key, int64_t chain0) {
    McAisArgs m;
    memset(&m, 0, sizeof(m));
    m.L = h->ra_l.p; m.ld = h->ra_l.ld; m.states = h->av.p; m.ld_states = h->av.ld; m.lengths = h->ra_len.p;
    m.V = h->V; m.J = R; m.sample = 1; m.max_length = h->rsm_len; m.key = key; m.row0 = chain0;
    m.dvec = h->adot.p; m.part = h->ra_dot.p; m.ld_part = h->ais_rows;
    if (launch_multinomial_counts_ais(m, h->stream)) abort();      // (bm_rbm_set_replicated_softmax checked the width)
}
// v ~ Multinomial(D, softmax(beta h W^T + a + beta (vb - a))) from ah into av: the kind-3 logits pass with the mixed bias from row
// `kbeta` of the table into ra_l, then the count kernel on it in place
static void rsm_ais_down(bm_rbm *h, int R, float beta, int kbeta, const PhiloxKey &key, int64_t chain0) {
    LayerPass p = rbm_pass(h, false, R, in_of(h->ah), LayerOut{0, h->ra_l.p, nullptr, h->ra_l.ld, key, chain0}, beta)
                      .bias(h->atable.p + (size_t)kbeta * h->V, 1.0f);
    p.a.kind = 3;
    {
        ProfScope _ps(h, KC_DOWN);
        launch_act(p.a, h->stream);
    }
    ProfScope _ps(h, KC_OTHER);
    rsm_ais_counts(h, R, key, chain0);
}

// bm_rbm_ais with a multinomial base model, count transitions and a length per chain; the host loop, the score kernel and the double
// accumulation are bm_rbm_ais's own (ais_run), the prop-up is the DB pass at mult == bmult == beta
int bm_rbm_rsm_ais(bm_rbm *h, int32_t n_betas, int32_t n_rows, int32_t k, const float *base_logits_host, const float *lengths_host,
                   uint64_t seed, int64_t chain0, float *values_host) {
    BM_CHECK(h && lengths_host && values_host, "bm_rbm_rsm_ais: null argument");
    BM_CHECK(h->rsm_len, "bm_rbm_rsm_ais needs a handle with replicated softmax visible units (bm_rbm_set_replicated_softmax): log Z per "
             "document length is defined for word-count rows only; bm_rbm_ais / bm_rbm_groups_ais serve the other units");
    BM_CHECK(n_betas >= 2 && n_rows >= 1 && k >= 1 && chain0 >= 0, "bm_rbm_rsm_ais: bad AIS arguments (n_betas %d >= 2, n_rows %d >= 1, "
             "n_gibbs_steps %d >= 1, chain0 %lld >= 0)", (int)n_betas, (int)n_rows, (int)k, (long long)chain0);
    const int R = n_rows, V = h->V, H = h->H;
    for (int r = 0; r < R; ++r) {
        const float D = lengths_host[r];
        BM_CHECK(D >= 1.0f && D <= (float)h->rsm_len && D == truncf(D), "bm_rbm_rsm_ais: lengths_host[%d] = %g is no integer in "
                 "[1, max_length = %d]", r, (double)D, h->rsm_len);
    }
    BM_TRY(ensure_rsm_ais_rows(h, R));
    // log Z_0(D) = H log 2 + D logsumexp(a) in double
    double mx = -INFINITY, se = 0.0;
    for (int i = 0; i < V; ++i) mx = fmax(mx, base_logits_host ? (double)base_logits_host[i] : 0.0);
    for (int i = 0; i < V; ++i) se += exp((base_logits_host ? (double)base_logits_host[i] : 0.0) - mx);
    const double lse = mx + log(se);
    std::vector<double> logZ0(R);
    for (int r = 0; r < R; ++r) logZ0[r] = (double)H * log(2.0) + (double)lengths_host[r] * lse;
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipMemcpy(h->ra_len.p, lengths_host, (size_t)R * sizeof(float), hipMemcpyHostToDevice));
    return ais_run(h, n_betas, R, k, base_logits_host, seed, chain0, h->ra_len.p, h->ra_dot.p, 2, 0.0, logZ0.data(), values_host,
                   [&] {
                       ProfScope _ps(h, KC_OTHER);
                       launch_rsm_fill_rows(h->ra_l.p, h->ra_l.ld, R, V, h->abase.p, h->stream);
                       rsm_ais_counts(h, R, ais_key(seed, SITE_AIS_V0, 0, 0), chain0);
                   },
                   [&](float bb, int b, const PhiloxKey &key, bool) { rsm_ais_down(h, R, bb, b, key, chain0); });
}

// ---- Gaussian visible units as one joint model (bm355.h: bm_rbm_gauss_ais, bm_rbm_gauss_free_energy_rows; bm_rbm_gauss_pt_* are in
// bm_rbm_pt.hip; bm_gauss.h).  Everything runs on u = x / sigma with unit variance and the centre c = vb / sigma; the entries of the
// Bernoulli model (bm_rbm_ais, bm_rbm_free_energy_rows, bm_rbm_pt_*) keep refusing a Gaussian handle.
static int check_gauss_joint(const bm_rbm *h, const char *what) {
    BM_CHECK(h, "%s: null argument", what);
    BM_CHECK(h->cfg.v_unit == BM_UNIT_GAUSSIAN, "%s needs Gaussian visible units (this handle's are Bernoulli: bm_rbm_ais, "
             "bm_rbm_free_energy_rows and bm_rbm_pt_* serve those)", what);
    BM_CHECK(!h->nrelu(), "%s is not available for NReLU hidden units (noisy rectified-linear, BM_UNIT_NRELU): the unit has no "
             "closed-form free energy and real-valued hidden states; see DESIGN.md 3.23", what);
    BM_CHECK(!h->multinomial(), "%s needs Bernoulli hidden units (this handle's are Multinomial)", what);
    BM_CHECK(!h->cfg.dbm_first && !h->cfg.dbm_last, "%s: the conditionals of a dbm_first / dbm_last handle (one of them doubled) "
             "belong to no single joint distribution", what);
    return 0;
}
// c = vb / sigma and the ones vector under the parameters of NOW, in stream order
static int gauss_prep(bm_rbm *h) {
    if (!h->gc.p) { BM_TRY(h->gc.alloc(h->V)); BM_TRY(h->gones.alloc(h->V)); }
    launch_gauss_prep(h->vb.p, h->sigma.p, h->V, h->gc.p, h->gones.p, h->stream);
    return 0;
}

// u ~ N(table_k + beta W h, I) from ah into av: the Gaussian epilogue (kind 1) with mult = beta, the mixed centre of row `kbeta` of
// the table taken once (bmult = 1) and a UNIT sigma - the ones vector, not null: draw4's ragged path reads ActArgs::sigma itself;
// dot: the pass leaves the slot partials of u.(c - a) in apart_v for the next score
static void gauss_ais_down(bm_rbm *h, int R, float beta, int kbeta, const PhiloxKey &key, int64_t chain0, bool dot) {
    LayerPass p = rbm_pass(h, false, R, in_of(h->ah), LayerOut{1, nullptr, h->av.p, h->av.ld, key, chain0}, beta)
                      .bias(h->atable.p + (size_t)kbeta * h->V, 1.0f);
    p.a.kind = BM_UNIT_GAUSSIAN; p.a.sigma = h->gones.p;
    if (dot) p.statedot_rows(h->apart_v.p, h->ais_rows, h->adot.p);
    issue(h, p);
}

// bm_rbm_ais with the base model N(a, I) over u and Gaussian transitions; the host loop, the table kernel (with c in place of vb),
// the prop-up with its softplus partials, the score kernel and the double accumulation are bm_rbm_ais's own (ais_run).  The score's
// visible term is linear in u, (beta_k - beta_{k-1}) u.(c - a); its constant, 1/2 (|a|^2 - |c|^2) over the whole path, is part of log Z_0
int bm_rbm_gauss_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t k, const float *base_mean_host, uint64_t seed, int64_t chain0,
                     float *values_host) {
    BM_TRY(check_gauss_joint(h, "bm_rbm_gauss_ais"));
    BM_CHECK(values_host, "bm_rbm_gauss_ais: null argument");
    BM_CHECK(n_betas >= 2 && n_runs >= 1 && k >= 1 && chain0 >= 0, "bm_rbm_gauss_ais: bad AIS arguments (n_betas %d >= 2, n_runs %d >= 1, "
             "n_gibbs_steps %d >= 1, chain0 %lld >= 0)", (int)n_betas, (int)n_runs, (int)k, (long long)chain0);
    const int R = n_runs, V = h->V, H = h->H;
    BM_TRY(ensure_ais_rows(h, R));
    BM_TRY(gauss_prep(h));
    // log Z_0 = (V/2) log 2 pi + H log 2 + sum_i log sigma_i + 1/2 (|a|^2 - |c|^2) in double, c as the device formed it
    std::vector<float> c(V), sg(V);
    BM_HIP(hipMemcpyAsync(c.data(), h->gc.p, (size_t)V * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipMemcpyAsync(sg.data(), h->sigma.p, (size_t)V * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    double logZ0 = 0.5 * (double)V * log(2.0 * M_PI) + (double)H * log(2.0), half = 0.0;
    for (int i = 0; i < V; ++i) {
        BM_CHECK(sg[i] > 0.f, "bm_rbm_gauss_ais: sigma[%d] = %g is not positive", i, (double)sg[i]);
        const double ai = base_mean_host ? (double)base_mean_host[i] : 0.0;
        logZ0 += log((double)sg[i]);
        half += ai * ai - (double)c[i] * (double)c[i];
    }
    logZ0 += 0.5 * half;
    return ais_run(h, n_betas, R, k, base_mean_host, seed, chain0, nullptr, h->apart_v.p, nslots(V), logZ0, nullptr, values_host,
                   [&] {
                       GaStartArgs s0;
                       memset(&s0, 0, sizeof(s0));
                       s0.v = h->av.p; s0.ld = h->av.ld; s0.rows = R; s0.V = V; s0.abase = h->abase.p; s0.dvec = h->adot.p;
                       s0.key = ais_key(seed, SITE_AIS_V0, 0, 0); s0.row0 = (unsigned long long)chain0;
                       s0.part = h->apart_v.p; s0.ld_part = h->ais_rows; s0.nslot = nslots(V);
                       launch_gauss_ais_start(s0, h->stream);
                   },
                   [&](float bb, int b, const PhiloxKey &key, bool dot) { gauss_ais_down(h, R, bb, b, key, chain0, dot); }, h->gc.p);
}

// Per-row free energies F(u) = 1/2 |u - c|^2 - sum_j softplus((u W + hb)_j), u = x / sigma: the division of the training chain
// (div_cols_kernel), one prop-up that only leaves its softplus slot partials, one row kernel.  No dropout, no RNG call consumed
int bm_rbm_gauss_free_energy_rows(bm_rbm *h, const float *X_dev, int32_t B, double *out_host) {
    BM_TRY(check_gauss_joint(h, "bm_rbm_gauss_free_energy_rows"));
    BM_CHECK(X_dev && out_host, "bm_rbm_gauss_free_energy_rows: null argument");
    BM_CHECK(B >= 1, "bm_rbm_gauss_free_energy_rows: bad row count %d", (int)B);
    if (B > h->gfe_rows) {
        h->gfe_rows = 0;
        BM_TRY(h->gfe_u.alloc(B, h->V)); BM_TRY(h->gfe_part.alloc((size_t)nslots(h->H) * B)); BM_TRY(h->gfe_out.alloc(B));
        h->gfe_rows = B;
    }
    BM_TRY(gauss_prep(h));
    ensure_wt(h);
    hipLaunchKernelGGL(div_cols_kernel, dim3(256), dim3(256), 0, h->stream, X_dev, h->V, (const float *)h->sigma.p, h->gfe_u.p, h->gfe_u.ld,
                       (int)B, h->V);
    issue(h, rbm_pass(h, true, B, in_of(h->gfe_u), LayerOut{0, nullptr, nullptr, pad_ld(h->H), PhiloxKey{0, 0, 0, 0}, 0})
                 .softplus_rows(h->gfe_part.p, h->gfe_rows, 0.f, 1.0f, 1));
    launch_gauss_fe_rows(h->gfe_u.p, h->gfe_u.ld, B, h->V, h->gc.p, h->gfe_part.p, h->gfe_rows, nslots(h->H), h->gfe_out.p, h->stream);
    BM_HIP(hipGetLastError());
    BM_HIP(hipMemcpyAsync(out_host, h->gfe_out.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// the block -> tile map of a launch with tiles_i x tiles_j tiles (host evaluation of the device function, for tests and
// tools): out_ti / out_tj [tiles_i * tiles_j] receive the tile of every block, out_map5 = {xi, xj, gj, tiles_i, tiles_j}
int bm_debug_tile_map(int32_t tiles_i, int32_t tiles_j, double bytes_i, double bytes_j, int32_t *out_ti, int32_t *out_tj,
                      int32_t *out_map5) {
    BM_CHECK(tiles_i >= 1 && tiles_j >= 1 && out_ti && out_tj, "bad arguments");
    const TileMap m = make_tile_map(tiles_i, tiles_j, bytes_i, bytes_j);
    const int nb = tiles_i * tiles_j;
    for (int b = 0; b < nb; ++b) { int ti = -1, tj = -1; tile_of_block(m, b, nb, ti, tj); out_ti[b] = ti; out_tj[b] = tj; }
    if (out_map5) { out_map5[0] = m.xi; out_map5[1] = m.xj; out_map5[2] = m.gj; out_map5[3] = m.tiles_i; out_map5[4] = m.tiles_j; }
    return 0;
}

int bm_rbm_stream(bm_rbm *h, void **out_stream) { *out_stream = (void *)h->stream; return 0; }

int bm_rbm_profile(bm_rbm *h, int32_t enable) {
    BM_HIP(hipStreamSynchronize(h->stream));
    h->recs.clear();
    h->prof = enable != 0;
    return 0;
}

int bm_rbm_kernel_times(bm_rbm *h, float *ms6, int32_t *n6) {
    BM_HIP(hipStreamSynchronize(h->stream));
    for (int c = 0; c < BM_NUM_KERNEL_CLASSES; ++c) { ms6[c] = 0.f; n6[c] = 0; }
    for (auto &r : h->recs) {
        float ms = 0.f;
        BM_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        ms6[r.cls] += ms;
        n6[r.cls] += 1;
    }
    return 0;
}

int bm_rbm_chain_stats(bm_rbm *h, int64_t *out3) {
    BM_CHECK(h && out3, "null argument");
    out3[0] = (int64_t)h->chain.launches; out3[1] = (int64_t)h->chain.tiles_expected; out3[2] = (int64_t)chain_mode(h->chain);
    return 0;
}

int bm_rbm_timer_start(bm_rbm *h) { BM_HIP(hipEventRecord(h->ev0, h->stream)); return 0; }
// the two halves of timer_stop: the mark is enqueued inside a timed region, the read (a host wait) after it
int bm_rbm_timer_mark(bm_rbm *h) { BM_HIP(hipEventRecord(h->ev1, h->stream)); return 0; }
int bm_rbm_timer_elapsed(bm_rbm *h, float *out_ms) {
    BM_HIP(hipEventSynchronize(h->ev1));
    BM_HIP(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return 0;
}
int bm_rbm_timer_stop(bm_rbm *h, float *out_ms) {
    BM_HIP(hipEventRecord(h->ev1, h->stream));
    BM_HIP(hipEventSynchronize(h->ev1));
    BM_HIP(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return 0;
}

}  // extern "C"
