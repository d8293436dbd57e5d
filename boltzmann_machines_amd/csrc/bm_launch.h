// bm_launch.h — the host side of bm_kernels.h (included at its end): which instantiation of act_kernel, act_bf3_kernel
// and grad_kernel a call becomes, and the launch tuner that measures that choice once per shape.  No device code here.
//
// The rest of the library calls launch_act, launch_grad, launch_fe_hidden and launch_apply_w only.
//
// Flavours.  act_kernel has compile-time flavours that are NOT tuner cases, so that the kernels of the plain update carry
// none of their code (same-box A/B: a runtime branch in the shared epilogue cost the headline 0.5 us per update):
//   FE   the h0 pass of a fused metric fetch (ActArgs::fe_flip): the 8-wave 32 x 64 tile; the 32 x 32 tiles measured within 1 us
//   LIT  "reference arithmetic" (ActArgs::lit, bm_dbm_set_sigmoid_literal): the literal float32 tf.sigmoid in the epilogue, a
//        parity mode on the 32 x 32 tile.  Same canonical accumulation order as every other geometry (bm_gemm.h), hence the
//        same pre-activations bit for bit
//   MF   mean-field passes (ActArgs::prev / maxdiff / skip / chk_ctl / acc_init; ActSide<.., MF>).  Two tiles, by rule: 32 x 64
//        (8 waves, one workgroup per CU) where that gives every CU a tile, else 32 x 32 (4 waves) - what the tuner picked for
//        these passes at 784-512-1024 x 512 (profiles/r5_dbm_kernel_stats.csv); BM355_DEBUG=mf_geo=8|1 forces one
//   CL, RT, CR, CB, BP, NR, SM, DB   the flavours of the table below (ActFlavour): each is selected by one field of ActArgs, admits a
//        narrow kind of pass and is combined with NO other selector of a pass - another flavour's, the bf16 range, FE, the
//        mean-field plumbing, `lit`, a second K segment - except those its entry tolerates (act_route; anything else: "no such
//        kernel", abort).  None is a tile of its own: a pass runs on the geometry and the block -> tile map that the tuner chose
//        (or now chooses, with the plain kernels) for the same shape in the plain flavour - one memo, keyed on the pass stripped
//        of the flavour's fields, no tuning run with the flavour's loads; act_geo forces it like any pass
//        (launch_act_flavoured).  Always per-pass fp32 launches: never the chained launch or the bf16 x 3 strip kernel.  What differs:
//          CL   clamped outputs (conditional sampling): any single-segment pass; with `lit`, the 32 x 32 parity tile
//               of LIT; a bf16 range on the pass is ignored, not refused
//          RT   a temperature per row (parallel tempering): Bernoulli passes of one or two K segments (the
//               interior layer of a DBM: below first, above chained onto the same accumulator; k-major P)
//          CR   the class rows of a classification RBM's prop-up: logits passes (kind 3) without draw or row sums
//          CB   the class bias of a classification RBM's prop-up given (x, y): Bernoulli passes whose row j adds
//               U[y_j] to the bias
//          BP   the prop-down of a delta through a sigmoid layer: raw passes (kind 2) from W itself, means only,
//               whose epilogue multiplies by a (1 - a) of an activation matrix
//          NR   noisy rectified-linear hidden units: logits prop-ups in either operand layout whose epilogue
//               rectifies t = z + b and draws one normal per output
//          SM   softmax visible units: logits prop-downs from W itself whose epilogue turns every group of sm_k in
//               {2, 4, 8, 16} logits into its means and its one-hot state
//          DB   replicated softmax: Bernoulli prop-ups whose row j multiplies the bias ALONE by row_bmult[j], the
//               document length; the softplus slot partials of `rowacc` ride on it; mult == bmult is 1 or the beta of a tempered
//               pass, which multiplies the whole pre-activation; bm_rsm.hip
//        SM + CL is the one combination of two of them, and no entry of the table: act_route refuses a softmax-group pass with a clamp
//        mask as it always did; the caller that means clamped groups (a mask constant within every group) says so by
//        calling launch_act_sm_clamped, which runs the kernels of bm_softmax_cl.hip - the CL block behind the SM block
//        SM + SA is the other flavour asked for by name (launch_act_sm_ais; bm_softmax_ais.hip): the softmax-group pass of the AIS over
//        softmax visible units - free mult / bmult, absent groups held at zero, state . dot_vec from registers
//        RT + GT is asked for by name as well (launch_act_gauss_pt; bm_gauss.hip): the prop-down of parallel tempering over Gaussian
//        visible units - the row's temperature scales the variance of the draw, not the mean, and the slot partials
//        of -1/2 (s - bias)^2 come from registers
//        CR to SM take mult == bmult == 1 (BP: mult) and one K segment.  The instantiations of CL and RT live in bm355.hip, those of
//        the other five in translation units of their own (ActFlavour::as) so that the kernels of every other unit are compiled
//        exactly as before; BP and SM have the x-major kernels only (launch_act_xm_as)
// FE, LIT and MF stage through LDS-DMA in the slab order.  dispatch_act walks the one ladder they share with the plain flavour:
// x-major P / two K segments / one, each as the `fast` kernel (16-byte loads) or the one that passes every chunk through
// registers (STG_DMA whatever the geometry's staging: shapes without 16-byte loads have ONE flavour).
//
// The tuner.  The geometries of a kernel compute bit-identical results (tests run all of them); which one is fastest depends
// on how the output tiles fill the 256 CUs and on the K length, and did not follow a simple rule in measurements (784x1024x512:
// 8-wave; AIS 20000 chains and 3072x5000: 32x32 tiles with BK = 32, four workgroups per CU; DBM 784-512-1024 mean-field: 64x32;
// bf16 x 3: 20000 AIS chains take 2, the 3072 x 256 x 5000 top-down pass of BASELINE configs[2] takes 8 or 2 (68 / 71 us) where 4
// needs 117 us).  So the launchers measure, ONCE per distinct shape, process and device (TuneMemo), SYNCHRONOUSLY at the first
// launch of that shape: every candidate runs the caller's contraction on the caller's (read-only) operands with all OUTPUTS
// redirected to a scratch pool (tune_redirect; grad_kernel: scratch W / dW / raw, zeroed - the update is not idempotent), so the
// tuning launches have no side effects: no double-counted row accumulators, no early write of a mean-field result.  A sample
// is one HIP event pair around TUNE_REP back-to-back launches behind a warm one (time_us); a candidate's time is its best of
// TUNE_ROUNDS samples, taken in rotation (best_of).  The fp32 act tuner adds a run-off: candidates within 3 % of the winner meet
// it again, alternating, over runs of 16 (a pick that is wrong by noise costs a whole run 2 - 4 %).  The second dimension is the
// block -> tile map (TileMap), measured with the chosen geometry: the slab order unless an XCD grid is >= 2 % faster (which grid
// wins also depends on how the panels fall onto the memory channels).  After that the launch path is one table lookup: no
// event, no allocation, no synchronisation (round 1 rotated the candidates through the first 12 real launches, which put
// slower geometries and event markers into short timed runs).  Without memory or events for the measurement the default
// geometry is kept (and remembered), HIP's last error is cleared.
// BM355_DEBUG: act_geo / grad_geo / bf3_geo / mf_geo=<code> force a geometry (experiments, tests); xcd_map forces a tile map,
// tune_xcd=0 keeps the tuner from measuring the maps; tune_log=1 prints the decisions.
#pragma once
#include <array>
#include <map>
#include <mutex>
#include <utility>
#include "bm_common.h"

namespace bm {

template <class G> static inline int tile_grid(int I, int J) { return ((I + G::TI - 1) / G::TI) * ((J + G::TJ - 1) / G::TJ); }

static inline int device_cu_count() {
    static const int n = [] {
        hipDeviceProp_t pr;
        int d = 0;
        (void)hipGetDevice(&d);
        return (hipGetDeviceProperties(&pr, d) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    }();
    return n;
}
static inline int dbg_int(const char *name) { const char *e = dbg(name); return e ? atoi(e) : 0; }

// ---- tuner plumbing
constexpr int XI_MODEL = 0, XI_SLAB = -1;      // values of map_xi besides the XCD grids 8 | 4 | 2 | 1: the traffic model's choice, the slab order
struct Tuned { int geo = 0; int xi = XI_MODEL; };      // geo: the launch_*_as code; 0 = not measured yet
constexpr int TUNE_REP = 4, TUNE_ROUNDS = 3;
constexpr float NOT_TIMED = 1e30f;
static inline bool timed(float us) { return us < 1e29f; }

static inline std::mutex &tune_mutex() { static std::mutex mu; return mu; }
// one decision per key (shape and flags, N numbers) and device; tune() runs under the lock, at the first launch of a key
template <size_t N> struct TuneMemo {
    std::map<std::pair<std::array<long long, N>, int>, Tuned> table;
    template <class F> Tuned get(const std::array<long long, N> &key, F &&tune) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(tune_mutex());
        Tuned &T = table[{key, dev}];
        if (!T.geo) T = tune();
        return T;
    }
};

// scratch of the tuning launches (per process, used under tune_mutex; grown on demand, never on the hot path; it lives as
// long as the process: nothing is freed during static destruction).  Null: no memory, the caller keeps its default choice
static inline float *tune_scratch(size_t nfloats) {
    struct Pool { DevArray<float> buf; int dev = -1; };
    static Pool &pool = *new Pool;
    int d = 0;
    (void)hipGetDevice(&d);
    if (!pool.buf.p || d != pool.dev || nfloats > pool.buf.n) {
        if (pool.buf.alloc(nfloats)) return nullptr;
        pool.dev = d;
    }
    return pool.buf.p;
}

struct TuneTimer {
    hipStream_t st = nullptr;
    Event e0, e1;
    bool init(hipStream_t s) { st = s; return create(e0) == 0 && create(e1) == 0; }
};
// microseconds per launch of `reps` back-to-back launches behind a warm one (instruction cache, clocks); NOT_TIMED: lost
template <class F> static inline float time_us(hipStream_t st, hipEvent_t e0, hipEvent_t e1, int reps, F &&launch) {
    launch();
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < reps; ++r) launch();
    (void)hipEventRecord(e1, st);
    if (hipEventSynchronize(e1) != hipSuccess) { (void)hipGetLastError(); return NOT_TIMED; }
    float ms = 0.f;
    return hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? 1e3f * ms / reps : NOT_TIMED;
}
// us[c] = the best of `rounds` samples of launch(c), c < n, the candidates taken in rotation
template <class F> static inline void best_of(TuneTimer &tm, int rounds, int reps, int n, float *us, F &&launch, const bool *skip = nullptr) {
    std::fill(us, us + n, NOT_TIMED);
    for (int round = 0; round < rounds; ++round)
        for (int c = 0; c < n; ++c)
            if (!skip || !skip[c]) us[c] = std::min(us[c], time_us(tm.st, tm.e0, tm.e1, reps, [&] { launch(c); }));
}
static inline int fastest(const float *us, int n) {       // -1: nothing was timed
    int b = -1;
    for (int c = 0; c < n; ++c) if (timed(us[c]) && (b < 0 || us[c] < us[b])) b = c;
    return b;
}
// the tile map of args `t` (ActArgs / GradArgs: map_xi) for launch(); us: slab last, as the log lines print them
template <class Args, class F> static inline int tune_tile_map(TuneTimer &tm, Args &t, float (&us)[5], F &&launch) {
    static const int cand_xi[5] = {8, 4, 2, 1, XI_SLAB};
    static const bool on = !(dbg("xcd_map") || (dbg("tune_xcd") && dbg_int("tune_xcd") == 0));
    std::fill(us, us + 5, NOT_TIMED);
    if (!on) return XI_MODEL;
    best_of(tm, TUNE_ROUNDS, TUNE_REP, 5, us, [&](int c) { t.map_xi = cand_xi[c]; launch(); });
    int bx = 0;
    for (int c = 1; c < 4; ++c) if (us[c] < us[bx]) bx = c;
    return us[bx] < 0.98f * us[4] ? cand_xi[bx] : XI_SLAB;
}
static inline bool tune_log() { static const bool on = dbg("tune_log") != nullptr; return on; }

// ---- act_kernel: one dispatcher for every flavour
enum : unsigned { FL_FE = 1, FL_LIT = 2, FL_MF = 4, FL_XM = 8, FL_SEG2 = 16, FL_CL = 32, FL_RT = 64, FL_CR = 128, FL_CB = 256, FL_BP = 512, FL_NR = 1024, FL_SM = 2048, FL_SA = 4096, FL_DB = 8192, FL_GT = 16384 };      // FL_XM / FL_SEG2: the flavour HAS x-major P / two-segment kernels
template <class G, int MINB, int STG, unsigned FL, bool SEG2, int PL>
static inline void launch_act_kernel(bool fast, unsigned dyn_lds, hipStream_t st, const ActArgs &a, const TileMap &tmap) {
    const dim3 grid(tile_grid<G>(a.I, a.J)), blk(G::NT);
    constexpr bool FE = (FL & FL_FE) != 0, LIT = (FL & FL_LIT) != 0, MF = (FL & FL_MF) != 0, CL = (FL & FL_CL) != 0,
                   RT = (FL & FL_RT) != 0, CR = (FL & FL_CR) != 0, CB = (FL & FL_CB) != 0, BP = (FL & FL_BP) != 0, NR = (FL & FL_NR) != 0,
                   SM = (FL & FL_SM) != 0, SA = (FL & FL_SA) != 0, DB = (FL & FL_DB) != 0, GT = (FL & FL_GT) != 0;
    if (fast) hipLaunchKernelGGL((act_kernel<G, MINB, SEG2, true, 0, PL, STG, FE, LIT, MF, CL, RT, CR, CB, BP, NR, SM, SA, DB, GT>), grid, blk, dyn_lds, st, a, tmap);
    else      hipLaunchKernelGGL((act_kernel<G, MINB, SEG2, false, 0, PL, STG_DMA, FE, LIT, MF, CL, RT, CR, CB, BP, NR, SM, SA, DB, GT>), grid, blk, dyn_lds, st, a, tmap);
}
template <class G, int MINB, int STG, unsigned FL>
static inline void dispatch_act(const ActArgs &a, hipStream_t st, int map_xi, unsigned dyn_lds = 0) {
    constexpr bool HAS_XM = (FL & FL_XM) != 0, HAS_SEG2 = (FL & FL_SEG2) != 0;
    // operand bytes one tile row (TI outputs along i) / one tile column (TJ rows) pulls through the L2
    const double kt = HAS_SEG2 ? (double)a.K1 + (double)a.K2 : (double)a.K1;
    const TileMap tmap = make_tile_map((a.I + G::TI - 1) / G::TI, (a.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, map_xi);
    const bool seg2 = HAS_SEG2 && a.K2 > 0;
    const bool fast = operand_fast(a.P1, a.p_xm ? XM : KM, a.K1) && operand_fast(a.Q1, XM, a.K1) &&
                      (!seg2 || (operand_fast(a.P2, KM, a.K2) && operand_fast(a.Q2, XM, a.K2)));
    if constexpr (HAS_XM)                   // x-major P: single segment only (RBM prop-down from W)
        if (a.p_xm) { launch_act_kernel<G, MINB, STG, FL, false, XM>(fast, dyn_lds, st, a, tmap); return; }
    if constexpr (HAS_SEG2)
        if (seg2) { launch_act_kernel<G, MINB, STG, FL, true, KM>(fast, dyn_lds, st, a, tmap); return; }
    launch_act_kernel<G, MINB, STG, FL, false, KM>(fast, dyn_lds, st, a, tmap);
}
// ---- the flavours that run on the plain flavour's tuner entry: one table entry each, most specific first (act_route takes the
// first entry whose selector the pass carries)
constexpr unsigned FT_BF16 = 1u << 16;      // act_features: the pass carries a bf16 range (the strip kernel: no act_kernel flavour)
using ActAsFn = void (*)(int geo, const ActArgs &a, hipStream_t st);
// The geometry `geo` (launch_act_as codes) of the five flavours whose instantiations live in translation units of their own, as
// those of bm_grad_cen.hip do: bm_class.hip (CR; the plain kernels are to stay exactly what they were), bm_class_joint.hip (CB;
// beside the CB instantiations the compiler allocates the registers of a dozen CR instantiations differently, 1 - 4 VGPRs, and
// those are to stay exactly what they were as well), bm_stack.hip (BP), bm_nrelu.hip (NR), bm_softmax_v.hip (SM), bm_rsm.hip (DB).  Each is
// launch_act_as<FL> and nothing else
void launch_act_cr_as(int, const ActArgs &, hipStream_t), launch_act_cb_as(int, const ActArgs &, hipStream_t),
     launch_act_bp_as(int, const ActArgs &, hipStream_t), launch_act_nr_as(int, const ActArgs &, hipStream_t),
     launch_act_sm_as(int, const ActArgs &, hipStream_t), launch_act_db_as(int, const ActArgs &, hipStream_t);
// An entry states
//   seg2, xm_only, geo5   its kernel set: two-segment kernels exist / only the x-major-P kernels exist (a prop-down from W itself) /
//                         geometry 5 exists (else the pass takes 7, the same tile at two workgroups per CU: the epilogues of CR and
//                         CB do not fit the 168 registers of three workgroups per CU without scratch; NR takes that tile as well)
// and, where it differs from ActFlavourDefaults,
//   lit_tile              a Bernoulli pass with `lit` takes the 32 x 32 parity tile of LIT in this flavour (tolerates FL_LIT then)
//   tolerates             the foreign selectors (act_features) a pass may carry; every other one refuses it
//   as                    the geometry entry point in the flavour's own unit; null: launch_act_as<FL>, instantiated by the caller
//   no_kernel             what a refused pass prints before it aborts
//   selects / admits      the field that selects the flavour / what else the pass must look like
//   strip                 the flavour's fields taken out: the plain pass of the same shape, which the tuner memo is keyed on
struct ActFlavourDefaults {
    static constexpr bool lit_tile = false;
    static constexpr unsigned tolerates = 0;
    static constexpr ActAsFn as = nullptr;
};
template <unsigned FL> struct ActFlavour;
template <> struct ActFlavour<0> : ActFlavourDefaults { static constexpr bool seg2 = true, xm_only = false, geo5 = true; };      // plain: its kernel set only
template <> struct ActFlavour<FL_CL> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = true, lit_tile = true;
    static constexpr unsigned tolerates = FL_LIT | FT_BF16;      // (clamp values may be grey levels: no bf16 shadow is written either)
    static constexpr const char *no_kernel = "bm355: a clamped pass has one K segment and no metric-fetch or mean-field plumbing (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.clamp_mask != nullptr; }
    static bool admits(const ActArgs &) { return true; }
    static void strip(ActArgs &p) { p.clamp_mask = p.clamp_val = nullptr; p.ld_clamp = 0; }
};
template <> struct ActFlavour<FL_RT> : ActFlavourDefaults {
    static constexpr bool seg2 = true, xm_only = false, geo5 = true;
    static constexpr unsigned tolerates = FL_SEG2;
    static constexpr const char *no_kernel = "bm355: a row-tempered pass is a Bernoulli pass of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.row_mult != nullptr; }
    static bool admits(const ActArgs &a) { return a.kind == 0 && !(a.K2 > 0 && a.p_xm); }
    static void strip(ActArgs &p) {      // (the clamp fields as well: no flavour reads them without a mask, the memo's tuning run sees none)
        p.clamp_mask = p.clamp_val = nullptr; p.ld_clamp = 0;
        p.row_mult = nullptr; p.rowen_out = nullptr; p.sel_out = nullptr; p.mult = p.bmult = 1.0f;
    }
};
template <> struct ActFlavour<FL_CR> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = false;
    static constexpr ActAsFn as = launch_act_cr_as;
    static constexpr const char *no_kernel = "bm355: a class-rows pass is a single-segment logits pass of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.cr_part != nullptr; }
    static bool admits(const ActArgs &a) { return a.kind == 3 && a.mult == 1.0f && a.bmult == 1.0f && !a.sample && !a.rowacc && !a.rowdot_out; }
    static void strip(ActArgs &p) { p.cr_part = nullptr; p.cr_U = nullptr; p.cr_ldu = p.cr_C = p.cr_nslots = 0; p.ld_part = 0; }
};
template <> struct ActFlavour<FL_CB> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = false;
    static constexpr ActAsFn as = launch_act_cb_as;
    static constexpr const char *no_kernel = "bm355: a class-bias pass is a single-segment Bernoulli prop-up of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.cb_y != nullptr; }
    static bool admits(const ActArgs &a) { return a.kind == 0 && a.mult == 1.0f && a.bmult == 1.0f && !a.rowacc && !a.rowdot_out && a.cb_U && a.cb_bad; }
    static void strip(ActArgs &p) { p.cb_y = nullptr; p.cb_U = nullptr; p.cb_ldu = p.cb_C = 0; p.cb_bad = nullptr; }
};
template <> struct ActFlavour<FL_BP> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_bp_as;
    static constexpr const char *no_kernel = "bm355: a back-propagation pass is a single-segment raw prop-down of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.bp != 0; }
    static bool admits(const ActArgs &a) {
        return a.kind == 2 && a.mult == 1.0f && !a.sample && !a.rowacc && !a.rowdot_out && !a.negmeans && !a.states && a.means && a.p_xm && a.bias;
    }
    static void strip(ActArgs &p) { p.bp = 0; p.bp_act = nullptr; p.bp_ld = 0; }
};
template <> struct ActFlavour<FL_NR> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = false;
    static constexpr ActAsFn as = launch_act_nr_as;
    static constexpr const char *no_kernel = "bm355: a noisy rectified-linear pass is a single-segment prop-up of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.nrelu != 0; }
    static bool admits(const ActArgs &a) { return a.kind == 3 && a.mult == 1.0f && a.bmult == 1.0f && !a.rowacc && !a.rowdot_out; }
    static void strip(ActArgs &p) { p.nrelu = 0; p.kind = 0; }      // (the Bernoulli prop-up of the shape: the same contraction, a draw per output)
};
template <> struct ActFlavour<FL_SM> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_sm_as;
    static constexpr const char *no_kernel = "bm355: a softmax-group pass is a single-segment prop-down of its own flavour, groups of 2, 4, 8 or 16 (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.sm_k != 0; }
    static bool admits(const ActArgs &a) {
        const bool width_ok = a.sm_k == 2 || a.sm_k == 4 || a.sm_k == 8 || a.sm_k == 16;
        return a.kind == 3 && a.mult == 1.0f && a.bmult == 1.0f && !a.rowacc && !a.rowdot_out && !a.negmeans && a.p_xm && width_ok && (a.I & 3) == 0 &&
               a.I % a.sm_k == 0;
    }
    static void strip(ActArgs &p) { p.sm_k = 0; p.kind = 0; }       // (the Bernoulli prop-down of the shape: the same contraction, a draw per output)
};
template <> struct ActFlavour<FL_DB> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = false;
    static constexpr ActAsFn as = launch_act_db_as;
    static constexpr const char *no_kernel = "bm355: a length-scaled-bias pass is a single-segment Bernoulli prop-up of its own flavour (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.row_bmult != nullptr; }
    // (mult == bmult: 1, or the launch-uniform beta of a tempered pass; the slot partials are softplus terms, single or two-beta)
    static bool admits(const ActArgs &a) { return a.kind == 0 && a.mult == a.bmult && !a.rowdot_out && (!a.rowacc || !a.dot_mat); }
    static void strip(ActArgs &p) { p.row_bmult = nullptr; p.mult = p.bmult = 1.0f; }
};
// SM + CL, clamped groups of softmax visible units: not an entry of the table - act_route never yields it - but
// described like one, so that launch_act_sm_clamped runs it through launch_act_flavoured.  The kernel set is SM's, in a unit of its
// own (bm_softmax_cl.hip); the pass is an SM pass that carries clamp values and a mask and no other selector; the strip is SM's and CL's
void launch_act_smcl_as(int, const ActArgs &, hipStream_t);
template <> struct ActFlavour<FL_SM | FL_CL> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_smcl_as;
    static constexpr const char *no_kernel = "bm355: a clamped softmax-group pass is a softmax-group pass with clamp values and a mask and nothing else (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.sm_k != 0 && a.clamp_mask != nullptr; }
    static bool admits(const ActArgs &a) { return ActFlavour<FL_SM>::admits(a) && a.clamp_val != nullptr; }
    static void strip(ActArgs &p) { ActFlavour<FL_SM>::strip(p); ActFlavour<FL_CL>::strip(p); }
};
// SM + SA, the tempered softmax-group pass of the AIS over softmax visible units: like SM + CL no entry of the table -
// act_route sends a softmax-group pass with a temperature or row dots to SM, which refuses it, as it always did - but described like
// one, so that launch_act_sm_ais runs it through launch_act_flavoured.  The kernel set is SM's, in a unit of its own
// (bm_softmax_ais.hip); the pass is an SM pass with free mult / bmult that samples, stores its states and leaves state . dot_vec; ONE
// flavour serves runs with and without a pattern of absent groups (a null sm_absent is a wave-uniform branch around one 16-byte load)
void launch_act_smais_as(int, const ActArgs &, hipStream_t);
template <> struct ActFlavour<FL_SM | FL_SA> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_smais_as;
    static constexpr const char *no_kernel = "bm355: a tempered softmax-group pass (AIS) is a sampled softmax-group pass that leaves state . dot_vec and nothing else (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.sm_k != 0 && a.sm_ais != 0; }
    static bool admits(const ActArgs &a) {
        const bool width_ok = a.sm_k == 2 || a.sm_k == 4 || a.sm_k == 8 || a.sm_k == 16;
        return a.kind == 3 && !a.rowacc && !a.negmeans && a.p_xm && width_ok && (a.I & 3) == 0 && a.I % a.sm_k == 0 && a.sample && a.states &&
               a.rowdot_out && a.dot_vec && a.ld_part >= a.J;
    }
    static void strip(ActArgs &p) { ActFlavour<FL_SM>::strip(p); p.sm_ais = 0; p.sm_absent = nullptr; p.mult = p.bmult = 1.0f; }
};
// SM + SA + RT, the softmax-group prop-down of parallel tempering over softmax visible units: the SM + SA pass with a
// temperature PER ROW - row_mult[j] takes the place of mult and bmult in the logits, l = fl(fl(beta_j z) + fl(beta_j b)), the two
// multiplies and one add of RT - and RT's hand-over of the beta = 1 rows (sel_out).  Like SM + SA no entry of the table and asked for
// by name (launch_act_sm_pt; bm_softmax_pt.hip); the kernel set is SM's.  The pass carries no pattern of absent groups (an ensemble
// row has none) and no rowen_out (the hidden half of the swap energy is the prop-up's); row_mult == 1 gives the plain SM pass bit for bit
void launch_act_smpt_as(int, const ActArgs &, hipStream_t);
template <> struct ActFlavour<FL_SM | FL_SA | FL_RT> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_smpt_as;
    static constexpr const char *no_kernel = "bm355: a row-tempered softmax-group pass is a sampled softmax-group pass with a temperature per row that leaves state . dot_vec and nothing else (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.sm_k != 0 && a.sm_ais != 0 && a.row_mult != nullptr; }
    static bool admits(const ActArgs &a) {
        return ActFlavour<FL_SM | FL_SA>::admits(a) && !a.sm_absent && !a.rowen_out && (!a.sel_out || (a.sel_R >= 1 && a.sel_rows >= 0));
    }
    static void strip(ActArgs &p) { ActFlavour<FL_SM | FL_SA>::strip(p); ActFlavour<FL_RT>::strip(p); }
};
// RT + GT, the prop-down of parallel tempering over Gaussian visible units: a tempered Gaussian conditional keeps its
// mean and changes its variance, which RT - a multiplier of z and of the bias - cannot express.  No entry of the table and asked for by
// name (launch_act_gauss_pt; bm_gauss.hip), like SM + SA: a pass that carries gt_sd through launch_act is refused there.  The kernel
// set is the x-major one (a prop-down from W itself); the pass samples, stores its states and leaves the slot partials of
// -1/2 (s - bias)^2 where rowdot_out goes; no means, no hand-over of the beta = 1 rows (there is no tempered training of this model)
void launch_act_gtpt_as(int, const ActArgs &, hipStream_t);
template <> struct ActFlavour<FL_RT | FL_GT> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = true, geo5 = false;
    static constexpr ActAsFn as = launch_act_gtpt_as;
    static constexpr const char *no_kernel = "bm355: a variance-tempered Gaussian pass is a sampled single-segment prop-down from W itself that leaves -1/2 (s - bias)^2 and nothing else (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.gt_sd != nullptr; }
    static bool admits(const ActArgs &a) {
        return a.kind == 3 && a.p_xm && a.K2 == 0 && a.sample && a.states && !a.means && !a.negmeans && !a.rowacc && !a.rowen_out && !a.sel_out &&
               a.rowdot_out && a.ld_part >= a.J && a.row_mult && a.gt_idx && a.bias;
    }
    // (the Bernoulli prop-down of the shape: the same contraction, a draw per output; the plain row dots would read dot_vec)
    static void strip(ActArgs &p) { ActFlavour<FL_RT>::strip(p); p.gt_sd = nullptr; p.gt_idx = nullptr; p.kind = 0; p.rowdot_out = nullptr; p.ld_part = 0; }
};
// DB + RT, the prop-up of parallel tempering over replicated softmax visible units: the DB pass with a temperature
// PER ROW - x = __fmul_rn(row_mult[j], __fadd_rn(z, __fmul_rn(row_bmult[j], bias))), the tempered DB pass of 3.28 with the row's beta
// in place of the launch-uniform one - that leaves RT's rowen_out, the slot partials of sum_i s_i t_i with the UNTEMPERED t.  No entry
// of the table - act_route sends a pass with both selectors to DB, which refuses it - and asked for by name (launch_act_db_pt;
// bm_rsm_pt.hip); the kernel set is DB's.  No rowdot_out, no softplus partials, no hand-over (sel_out); row_mult == 1 gives the plain
// DB pass bit for bit
void launch_act_dbpt_as(int, const ActArgs &, hipStream_t);
template <> struct ActFlavour<FL_DB | FL_RT> : ActFlavourDefaults {
    static constexpr bool seg2 = false, xm_only = false, geo5 = false;
    static constexpr ActAsFn as = launch_act_dbpt_as;
    static constexpr const char *no_kernel = "bm355: a row-tempered length-scaled-bias pass is a single-segment Bernoulli prop-up with a temperature and a length per row that leaves its energy partials and nothing else (no such kernel)\n";
    static bool selects(const ActArgs &a) { return a.row_bmult != nullptr && a.row_mult != nullptr; }
    static bool admits(const ActArgs &a) { return a.kind == 0 && a.K2 == 0 && !a.rowdot_out && !a.rowacc && !a.sel_out && (!a.rowen_out || a.ld_part >= a.J); }
    static void strip(ActArgs &p) { ActFlavour<FL_DB>::strip(p); ActFlavour<FL_RT>::strip(p); }
};

// the table's order: most specific first.  first(f): f(std::integral_constant<unsigned, FL>) for each flavour until one returns true
template <unsigned... FL> struct ActFlavoursOf {
    static unsigned selected(const ActArgs &a) { return ((ActFlavour<FL>::selects(a) ? FL : 0u) | ...); }
    template <class F> static bool first(F &&f) { return (f(std::integral_constant<unsigned, FL>{}) || ...); }
};
using ActFlavours = ActFlavoursOf<FL_DB, FL_SM, FL_NR, FL_BP, FL_CB, FL_CR, FL_RT, FL_CL>;
// every selector the pass carries: the FL_ bits of the table's flavours, FL_FE, FL_MF, FL_LIT, FL_SEG2 (K2 > 0) and FT_BF16
static inline unsigned act_features(const ActArgs &a) {
    return ActFlavours::selected(a) | (a.b3.K1 > 0 ? FT_BF16 : 0u) | (a.fe_flip ? FL_FE : 0u) |
           ((a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init) ? FL_MF : 0u) | (a.lit ? FL_LIT : 0u) | (a.K2 > 0 ? FL_SEG2 : 0u);
}
// Where a pass goes: fl = the first flavour of the table that the pass selects (0: none - FE, MF, LIT, bf16 or plain), refusal =
// null if that flavour has a kernel for the pass, else its message.  The rule of exclusivity: a flavour's pass carries no selector
// but its own and those its entry tolerates.  No launch, no abort
struct ActRoute { unsigned fl; const char *refusal; };
static inline ActRoute act_route(const ActArgs &a) {
    const unsigned f = act_features(a);
    ActRoute r{0, nullptr};
    ActFlavours::first([&](auto fl) {
        using F = ActFlavour<decltype(fl)::value>;
        if (!(f & fl.value)) return false;
        r = {fl.value, (f & ~(fl.value | F::tolerates)) == 0 && F::admits(a) ? nullptr : F::no_kernel};
        return true;
    });
    return r;
}
// what the tuner memo of the fp32 passes keys on besides I, J, K1 and K2 (tuned_act), of a plain pass
static inline long long act_memo_flags(const ActArgs &a) {
    return (long long)((a.sample ? 1 : 0) | (a.kind << 1) | (a.prev ? 16 : 0) | (a.rowacc ? 32 : 0) | (a.acc_init ? 64 : 0) | (a.p_xm ? 128 : 0) |
                       (a.rowdot_out ? 256 : 0) | (a.dot_mat ? 512 : 0) | (a.negmeans ? 1024 : 0));
}

// (x-major P exists for the geometries with MI == 1)
template <class G, int MINB, int STG, unsigned FLX = 0>
static inline void launch_act_geo(const ActArgs &a, hipStream_t st) {
    dispatch_act<G, MINB, STG, FLX | (ActFlavour<FLX>::seg2 ? FL_SEG2 : 0) | (G::MI == 1 ? FL_XM : 0)>(a, st, a.map_xi);
}
#ifndef BM_KERNELS_ONLY
static inline void launch_act_fe(const ActArgs &a, hipStream_t st) { dispatch_act<GeoAct8, 1, STG_DMA, FL_FE | FL_XM>(a, st, XI_SLAB); }
static inline void launch_act_lit(const ActArgs &a, hipStream_t st) { dispatch_act<GeoActS, 2, STG_DMA, FL_LIT | FL_XM | FL_SEG2>(a, st, XI_SLAB); }
template <class G, int MINB, bool LIT>
static inline void launch_act_mf_geo(const ActArgs &a, hipStream_t st, unsigned dyn_lds = 0) {
    dispatch_act<G, MINB, STG_DMA, FL_MF | (LIT ? FL_LIT : 0) | FL_XM | FL_SEG2>(a, st, XI_SLAB, dyn_lds);
}
static inline void launch_act_mf(const ActArgs &a, hipStream_t st) {
    if (a.lit && a.kind == 0) { launch_act_mf_geo<GeoActS, 1, true>(a, st); return; }
    static const int force = dbg_int("mf_geo");
    const bool wide = force ? force == 8 : tile_grid<GeoAct8>(a.I, a.J) >= device_cu_count();
    // (the 32 x 32 tile of this flavour takes 64 KiB for its ring + 16 KiB for the control words: one workgroup per CU)
    if (wide) launch_act_mf_geo<GeoAct8, 1, false>(a, st);
    else      launch_act_mf_geo<GeoActS, 1, false>(a, st);
}

// fast-binary launch (a.b3 filled).  Three tiles: 64 x 64 / 8 waves and 64 x 32 / 4 waves (one workgroup per CU: the
// ring takes most of the LDS), 32 x 64 / 4 waves with TWO workgroups per CU (80 KiB each: one workgroup's epilogue -
// sigmoid, draw, the AIS softplus terms - runs under the other's matrix work).  Every workgroup owns a strip of
// tile columns.
template <class G, int WGS_PER_CU>
static inline void launch_act_bf3_geo(const ActArgs &a, hipStream_t st) {
    Bf3Strip sp;
    sp.tiles_i = (a.I + G::TI - 1) / G::TI; sp.tiles_j = (a.J + G::TJ - 1) / G::TJ;
    static const int abl_env = dbg_int("bf3_abl");
    sp.abl = abl_env;
    sp.strips = (device_cu_count() * WGS_PER_CU) / sp.tiles_i;
    if (sp.strips < 1) sp.strips = 1;
    if (sp.strips > sp.tiles_j) sp.strips = sp.tiles_j;
    const dim3 grid(sp.tiles_i * sp.strips), blk(G::NT);
    constexpr int MINW = WGS_PER_CU * G::NW / 4 > 0 ? WGS_PER_CU * G::NW / 4 : 1;          // waves per SIMD the grid needs
    if (a.b3.K2 > 0) hipLaunchKernelGGL((act_bf3_kernel<G, true, MINW>), grid, blk, 0, st, a, sp);
    else             hipLaunchKernelGGL((act_bf3_kernel<G, false, MINW>), grid, blk, 0, st, a, sp);
}
// geo: 2: 64 x 32 tiles, two workgroups per CU; 4: 64 x 64, one; 8: 128 x 32 with 8 waves
static inline void launch_act_bf3_as(int geo, const ActArgs &a, hipStream_t st) {
    if (geo == 8)      launch_act_bf3_geo<GeoGrad8, 1>(a, st);
    else if (geo == 2) launch_act_bf3_geo<GeoBf3S, 2>(a, st);
    else               launch_act_bf3_geo<GeoAct, 1>(a, st);
}
#endif  // BM_KERNELS_ONLY

// The ladder of a flavour with the x-major kernels only (ActFlavour::xm_only: its passes are prop-downs from W itself).  geo: the
// codes of launch_act_as, resolved as that ladder resolves them for an x-major P (6, 9, 4 -> 8; 5, 7 -> 3): every code lands on a
// geometry with MI == 1 - one quad per lane, no scratch (profiles/stack_resources.md, softmax_v_resources.md).  The tile map and
// the 16-byte / generic choice are dispatch_act's
template <class G, int MINB, int STG, unsigned FLX>
static inline void launch_act_xm_geo(const ActArgs &a, hipStream_t st) {
    const double kt = (double)a.K1;
    const TileMap tmap = make_tile_map((a.I + G::TI - 1) / G::TI, (a.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, a.map_xi);
    const bool fast = operand_fast(a.P1, XM, a.K1) && operand_fast(a.Q1, XM, a.K1);
    launch_act_kernel<G, MINB, STG, FLX, false, XM>(fast, 0, st, a, tmap);
}
template <unsigned FLX>
static inline void launch_act_xm_as(int geo, const ActArgs &a, hipStream_t st) {
    static_assert(ActFlavour<FLX>::xm_only, "this flavour's ladder is launch_act_as");
    if (geo == 208) { launch_act_xm_geo<GeoAct8, 1, STG_DMAH, FLX>(a, st); return; }
    if (geo == 6 || geo == 9) geo = 8;
    if (geo == 5 || geo == 7) geo = 3;
    const bool reg = geo >= 100;
    geo %= 100;
    if (reg) {
        if (geo == 1)      launch_act_xm_geo<GeoActS, 2, STG_REG, FLX>(a, st);
        else if (geo == 3) launch_act_xm_geo<GeoActS32, 4, STG_REG, FLX>(a, st);
        else               launch_act_xm_geo<GeoAct8, 1, STG_REG, FLX>(a, st);
    } else {
        if (geo == 1)      launch_act_xm_geo<GeoActS, 2, STG_DMA, FLX>(a, st);
        else if (geo == 3) launch_act_xm_geo<GeoActS32, 4, STG_DMA, FLX>(a, st);
        else               launch_act_xm_geo<GeoAct8, 1, STG_DMA, FLX>(a, st);
    }
}
// geo: tile geometry 8 | 4 | 1 | 3, + 100 for register staging of the full chunks (default: LDS-DMA), or one of the specials
// FLX: the flavour of the ladder's kernels (0 plain, or an entry of the table: what this instantiates follows its kernel-set facts)
template <unsigned FLX = 0>
static inline void launch_act_as(int geo, const ActArgs &a, hipStream_t st) {
    static_assert(!ActFlavour<FLX>::xm_only, "this flavour's ladder is launch_act_xm_as");
    // 208: 8 waves, DMA issued by waves 0-3 only (not a tuner candidate: within noise of 8 on every shape measured)
    if (geo == 208) { launch_act_geo<GeoAct8, 1, STG_DMAH, FLX>(a, st); return; }
    // 6: 64 x 64 tile, 8 waves of 32 x 16 (the outer-product geometry): half the operand traffic per flop of the
    // 32 x 64 tile, for outputs large enough to fill the chip with tiles of that size
    if (geo == 6 && !a.p_xm) { launch_act_geo<GeoGrad8, 1, STG_DMA, FLX>(a, st); return; }
    if (geo == 6) geo = 8;
    // 9: the 64 x 64 tile with BK = 32: 64 KiB LDS, two workgroups per CU (k-major P only)
    // (the second template argument is the kernel's waves per SIMD: 2 workgroups x 8 waves / 4 SIMDs)
    if (geo == 9 && !a.p_xm) { launch_act_geo<GeoGrad8h, 4, STG_DMA, FLX>(a, st); return; }
    if (geo == 9) geo = 8;
    // 5: 64 x 32 tile with BK = 32, three workgroups per CU (k-major P only)
    // (a flavour without it, ActFlavour::geo5, takes the same tile as 7)
    if constexpr (ActFlavour<FLX>::geo5) { if (geo == 5 && !a.p_xm) { launch_act_geo<GeoAct32, 3, STG_DMA, FLX>(a, st); return; } }
    else if (geo == 5 && !a.p_xm) geo = 7;
    // 7: the same with two workgroups per CU (256 registers per wave: the two-segment variant spills 140 bytes at 168)
    if (geo == 7 && !a.p_xm) { launch_act_geo<GeoAct32, 2, STG_DMA, FLX>(a, st); return; }
    if (geo == 5 || geo == 7) geo = 3;
    const bool reg = geo >= 100;
    geo %= 100;
    if (a.p_xm && geo == 4) geo = 8;        // x-major P exists for the MI == 1 geometries only
    if (reg) {
        if (geo == 8)      launch_act_geo<GeoAct8, 1, STG_REG, FLX>(a, st);
        else if (geo == 1) launch_act_geo<GeoActS, 2, STG_REG, FLX>(a, st);
        else if (geo == 3) launch_act_geo<GeoActS32, 4, STG_REG, FLX>(a, st);
        else               launch_act_geo<GeoAct, 1, STG_REG, FLX>(a, st);
    } else {
        if (geo == 8)      launch_act_geo<GeoAct8, 1, STG_DMA, FLX>(a, st);
        else if (geo == 1) launch_act_geo<GeoActS, 2, STG_DMA, FLX>(a, st);
        else if (geo == 3) launch_act_geo<GeoActS32, 4, STG_DMA, FLX>(a, st);
        else               launch_act_geo<GeoAct, 1, STG_DMA, FLX>(a, st);
    }
}
#ifndef BM_KERNELS_ONLY
// the caller's launch with every OUTPUT redirected into the scratch pool (false: no memory, keep the default choice)
static inline bool tune_redirect(const ActArgs &a, ActArgs &t) {
    const size_t mat = ((size_t)a.J * (size_t)a.ldo + 3) & ~(size_t)3;
    const size_t rowv = (((size_t)((a.I + 15) / 16) * (size_t)(a.ld_part > a.J ? a.ld_part : a.J)) + 3) & ~(size_t)3;   // slot partials
    const size_t sh16 = a.states16 ? ((size_t)a.J * (size_t)a.ld16 / 2 + 4) & ~(size_t)3 : 0;                           // bf16 shadow, in floats
    const size_t fe = a.fe_flip ? ((size_t)a.J * (size_t)a.fe_rm + 3) & ~(size_t)3 : 0;
    float *s = tune_scratch(3 * mat + 2 * rowv + BM_MF_SLOTS + 4 + sh16 + fe);
    if (!s) return false;
    t = a;
    if (a.fe_flip) t.fe_rowacc2 = s + 3 * mat + 2 * rowv + BM_MF_SLOTS + 4 + sh16;
    t.skip = nullptr;
    t.chk_ctl = nullptr;
    if (a.means) t.means = s;
    if (a.states) t.states = s + mat;
    if (a.negmeans) t.negmeans = s + 2 * mat;
    if (a.rowacc) t.rowacc = s + 3 * mat;        // (fe_flip: [J][fe_rm] <= rowv floats: fe_rm >= ceil(I/16), ld_part >= J)
    if (a.rowdot_out) t.rowdot_out = s + 3 * mat + rowv;
    if (a.maxdiff_blk) t.maxdiff_blk = s + 3 * mat + 2 * rowv;
    if (a.maxdiff) t.maxdiff = reinterpret_cast<unsigned *>(s + 3 * mat + 2 * rowv + BM_MF_SLOTS);
    if (a.states16) t.states16 = reinterpret_cast<uint16_t *>(s + 3 * mat + 2 * rowv + BM_MF_SLOTS + 4);
#ifdef BM_PROBE
    t.dbg = nullptr;
#endif
    return true;
}
static inline Tuned tune_act_shape(const ActArgs &a, hipStream_t st, long long flags) {
    constexpr int NC = 12;
    static const struct { int geo; bool xm; } cand[NC] = {{8, true}, {4, false}, {1, true}, {3, true}, {108, true}, {104, false}, {101, true}, {103, true},
                                                          {6, false}, {5, false}, {7, false}, {9, false}};      // xm: instantiated for an x-major P
    Tuned T;
    T.geo = a.p_xm ? 8 : 4;
    ActArgs t;
    TuneTimer tm;
    if (!tune_redirect(a, t) || !tm.init(st)) return T;
    float us[NC], xi_us[5];
    bool skip[NC];
    for (int c = 0; c < NC; ++c) skip[c] = a.p_xm && !cand[c].xm;
    best_of(tm, TUNE_ROUNDS, TUNE_REP, NC, us, [&](int c) { launch_act_as(cand[c].geo, t, st); }, skip);
    int b = fastest(us, NC);
    if (b >= 0) {
        int second = -1;                        // the run-off
        for (int c = 0; c < NC; ++c)
            if (c != b && us[c] < 1.03f * us[b] && (second < 0 || us[c] < us[second])) second = c;
        if (second >= 0) {
            float ro[2];
            const int pair[2] = {b, second};
            best_of(tm, 3, 16, 2, ro, [&](int q) { launch_act_as(cand[pair[q]].geo, t, st); });
            if (ro[1] < ro[0]) b = second;
        }
        T.geo = cand[b].geo;
    }
    T.xi = tune_tile_map(tm, t, xi_us, [&] { launch_act_as(T.geo, t, st); });
    if (tune_log()) {
        float s[NC];
        for (int c = 0; c < NC; ++c) s[c] = timed(us[c]) ? us[c] : -1.f;
        fprintf(stderr, "bm355 tune: act I=%d J=%d K=%d+%d flags=%lld -> geometry %d (us, dma: 8w %.1f, 64x32 %.1f, 32x32 %.1f, 32x32/bk32 %.1f; "
                        "reg: 8w %.1f, 64x32 %.1f, 32x32 %.1f, 32x32/bk32 %.1f; 64x64 8w: %.1f; 64x32/bk32 x3: %.1f, x2: %.1f; 64x64/bk32 x2: %.1f)\n",
                a.I, a.J, a.K1, a.K2, flags, T.geo, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11]);
        if (T.xi != XI_MODEL)
            fprintf(stderr, "bm355 tune: act I=%d J=%d K=%d+%d flags=%lld -> tile map %d (-1 slab, else XCD grid xi; us: slab %.1f, 8x1 %.1f, 4x2 %.1f, 2x4 %.1f, 1x8 %.1f)\n",
                    a.I, a.J, a.K1, a.K2, flags, T.xi, xi_us[4], xi_us[0], xi_us[1], xi_us[2], xi_us[3]);
    }
    return T;
}
static inline Tuned tune_bf3_shape(const ActArgs &a, hipStream_t st, long long flags) {
    static const int cand[3] = {2, 8, 4};
    Tuned T;
    T.geo = tile_grid<GeoBf3S>(a.I, a.J) >= 1024 ? 2 : 8;
    ActArgs t;
    TuneTimer tm;
    if (!tune_redirect(a, t) || !tm.init(st)) return T;
    float us[3];
    best_of(tm, TUNE_ROUNDS, TUNE_REP, 3, us, [&](int c) { launch_act_bf3_as(cand[c], t, st); });
    const int b = fastest(us, 3);
    if (b >= 0) T.geo = cand[b];
    if (tune_log()) fprintf(stderr, "bm355 tune: bf16x3 act I=%d J=%d K=%d+%d flags=%lld -> geometry %d (us: 64x32 %.1f, 128x32 8w %.1f, 64x64 %.1f)\n",
                            a.I, a.J, a.b3.K1, a.b3.K2, flags, T.geo, us[0], us[1], us[2]);
    return T;
}
static inline void launch_act_bf3(const ActArgs &a, hipStream_t st) {
    static const int geo_env = dbg_int("bf3_geo");
    if (geo_env) { launch_act_bf3_as(geo_env, a, st); return; }
    static TuneMemo<5> memo;
    const long long flags = (long long)((a.sample ? 1 : 0) | (a.kind << 1) | (a.rowacc ? 32 : 0) | (a.rowdot_out ? 256 : 0) |
                                        (a.dot_mat ? 512 : 0) | (a.states ? 1024 : 0) | (a.means ? 2048 : 0));
    const Tuned T = memo.get({a.I, a.J, a.b3.K1, a.b3.K2, flags}, [&] { return tune_bf3_shape(a, st, flags); });
    launch_act_bf3_as(T.geo, a, st);
}
// the tuner's decision for the shape of the PLAIN pass `a` (ONE memo for the plain flavour and every flavour of the table, which
// hands in its pass stripped; measured with the plain kernels)
static inline Tuned tuned_act(const ActArgs &a, hipStream_t st) {
    static TuneMemo<5> memo;
    const long long flags = act_memo_flags(a);
    return memo.get({a.I, a.J, a.K1, a.K2, flags}, [&] { return tune_act_shape(a, st, flags); });
}
// a per-pass fp32 launch of flavour FL (0: plain) on the geometry that is forced (act_geo, geo_hint) or tuned for the plain pass of
// the shape, with the tuned tile map unless the caller chose one
template <unsigned FL>
static inline void launch_act_flavoured(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL>;
    const auto as = [&](int geo, const ActArgs &x) { if constexpr (F::as != nullptr) F::as(geo, x, st); else launch_act_as<FL>(geo, x, st); };
    if constexpr (F::lit_tile)
        if (a.lit && a.kind == 0) { dispatch_act<GeoActS, 2, STG_DMA, FL | FL_LIT | FL_XM>(a, st, XI_SLAB); return; }
    static const int geo_env = dbg_int("act_geo");
    const int ov = geo_env ? geo_env : a.geo_hint;
    if (ov) { as(ov, a); return; }
    Tuned T;
    if constexpr (FL == 0) T = tuned_act(a, st);        // (nothing to strip, no copy)
    else { ActArgs plain = a; F::strip(plain); T = tuned_act(plain, st); }
    if (T.xi != XI_MODEL && !a.map_xi) {
        ActArgs a2 = a;
        a2.map_xi = T.xi;
        as(T.geo, a2);
        return;
    }
    as(T.geo, a);
}
// a clamped softmax-group pass (ActFlavour<FL_SM | FL_CL>): the caller's explicit choice, not a route of launch_act
static inline void launch_act_sm_clamped(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL_SM | FL_CL>;
    if (!F::selects(a) || (act_features(a) & ~(FL_SM | FL_CL)) != 0 || !F::admits(a)) { fputs(F::no_kernel, stderr); abort(); }
    launch_act_flavoured<FL_SM | FL_CL>(a, st);
}
// a tempered softmax-group pass (ActFlavour<FL_SM | FL_SA>): the caller's explicit choice, not a route of launch_act
static inline void launch_act_sm_ais(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL_SM | FL_SA>;
    if (!F::selects(a) || (act_features(a) & ~FL_SM) != 0 || !F::admits(a)) { fputs(F::no_kernel, stderr); abort(); }
    launch_act_flavoured<FL_SM | FL_SA>(a, st);
}
// a row-tempered softmax-group pass (ActFlavour<FL_SM | FL_SA | FL_RT>): the caller's explicit choice, not a route of launch_act
static inline void launch_act_sm_pt(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL_SM | FL_SA | FL_RT>;
    if (!F::selects(a) || (act_features(a) & ~(FL_SM | FL_RT)) != 0 || !F::admits(a)) { fputs(F::no_kernel, stderr); abort(); }
    launch_act_flavoured<FL_SM | FL_SA | FL_RT>(a, st);
}
// a variance-tempered Gaussian pass (ActFlavour<FL_RT | FL_GT>): the caller's explicit choice, not a route of launch_act
static inline void launch_act_gauss_pt(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL_RT | FL_GT>;
    if (!F::selects(a) || (act_features(a) & ~FL_RT) != 0 || !F::admits(a)) { fputs(F::no_kernel, stderr); abort(); }
    launch_act_flavoured<FL_RT | FL_GT>(a, st);
}
// a row-tempered length-scaled-bias pass (ActFlavour<FL_DB | FL_RT>): the caller's explicit choice, not a route of launch_act
static inline void launch_act_db_pt(const ActArgs &a, hipStream_t st) {
    using F = ActFlavour<FL_DB | FL_RT>;
    if (!F::selects(a) || (act_features(a) & ~(FL_DB | FL_RT)) != 0 || !F::admits(a)) { fputs(F::no_kernel, stderr); abort(); }
    launch_act_flavoured<FL_DB | FL_RT>(a, st);
}
static inline void launch_act(const ActArgs &a, hipStream_t st) {
    if (a.gt_sd) { fputs("bm355: a variance-tempered Gaussian pass is asked for by name, launch_act_gauss_pt (no such route)\n", stderr); abort(); }
    if (a.sm_ais) { fputs("bm355: a tempered softmax-group pass (AIS) is asked for by name, launch_act_sm_ais (no such route)\n", stderr); abort(); }
    const ActRoute r = act_route(a);
    if (r.refusal) { fputs(r.refusal, stderr); abort(); }
    if (ActFlavours::first([&](auto fl) { return r.fl == fl.value && (launch_act_flavoured<decltype(fl)::value>(a, st), true); })) return;
    if (a.b3.K1 > 0) { launch_act_bf3(a, st); return; }
    if (a.fe_flip) { launch_act_fe(a, st); return; }
    if (a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init) { launch_act_mf(a, st); return; }
    if (a.lit && a.kind == 0) { launch_act_lit(a, st); return; }
    launch_act_flavoured<0>(a, st);
    // fast-binary mode, an fp32 launch whose sampled states the NEXT launches read as a bf16 shadow: converted here (the
    // strip kernel writes its shadow itself; keeping the branch out of the fp32 epilogue is worth ~0.2 us per launch)
    if (a.states16 && a.states)
        hipLaunchKernelGGL(shadow16_kernel, dim3(256), dim3(256), 0, st, (const float *)a.states, a.ldo, a.J, a.I, a.states16, a.ld16);
}

// ---- grad_kernel: 4 waves of 32 x 32 or 8 waves of 32 x 16 (bit-identical results)
template <class G, int STG, int MINB = 1>
static inline void launch_grad_geo(const GradArgs &g, hipStream_t st) {
    const double kt = (double)g.Kpos + (double)g.Kneg;
    const TileMap tmap = make_tile_map((g.I + G::TI - 1) / G::TI, (g.J + G::TJ - 1) / G::TJ, kt * G::TI * 4.0, kt * G::TJ * 4.0, g.map_xi);
    const bool fast = operand_fast(g.Ppos, KM, g.Kpos) && operand_fast(g.Qpos, KM, g.Kpos) &&
                      operand_fast(g.Pneg, KM, g.Kneg) && operand_fast(g.Qneg, KM, g.Kneg);
    const dim3 grid(tile_grid<G>(g.I, g.J) + g.nbias), blk(G::NT);
    if (fast) hipLaunchKernelGGL((grad_kernel<G, true, 0, STG, MINB>), grid, blk, 0, st, g, tmap);
    else      hipLaunchKernelGGL((grad_kernel<G, false, 0, STG_DMA, MINB>), grid, blk, 0, st, g, tmap);
}
// centred flavour (grad_kernel<..., GradCen>): instantiated for the geometries 4 and 8 with DMA staging.  A forced
// geometry (BM355_DEBUG=grad_geo) runs as asked when it is 8 and FALLS BACK TO 4 otherwise; a tuned one takes the centred
// kernel of its wave count (8, 9, 108, 208 -> 8; 4, 104 -> 4).  Bit-identical results either way.
// Defined in bm_grad_cen.hip, a translation unit of its own: with the centred instantiations in the same module the compiler
// allocates the plain 8-wave instantiations' registers differently (170 / 188 instead of 173 / 190 VGPRs), and the plain
// kernels are to stay exactly what they were.
void launch_grad_cen(int geo, const GradArgs &g, const GradCen &cen, hipStream_t st);
// geo: 4 | 8 waves, + 100 for register staging of the full chunks, or one of the specials
static inline void launch_grad_as(int geo, const GradArgs &g, hipStream_t st) {
    // 9: 8 waves, BK = 32, two workgroups per CU - for outputs of many tiles per CU and a short K (3072 x 5000 x 512:
    // a tile's fill and read-modify-write epilogue take as long as its K loop)
    if (geo == 9 && g.nbias == 0) launch_grad_geo<GeoGrad8h, STG_DMA, 4>(g, st);       // 4 waves per SIMD = 2 workgroups per CU
    else if (geo == 9)   launch_grad_geo<GeoGrad8, STG_DMA>(g, st);
    else if (geo == 208) launch_grad_geo<GeoGrad8, STG_DMAH>(g, st);
    else if (geo == 108) launch_grad_geo<GeoGrad8, STG_REG>(g, st);
    else if (geo == 104) launch_grad_geo<GeoGrad, STG_REG>(g, st);
    else if (geo == 8)   launch_grad_geo<GeoGrad8, STG_DMA>(g, st);
    else                 launch_grad_geo<GeoGrad, STG_DMA>(g, st);
}
static inline Tuned tune_grad_shape(const GradArgs &g, hipStream_t st) {
    constexpr int NC = 5;
    static const int cand[NC] = {4, 8, 104, 108, 9};          // 208 (half-wave DMA) is forceable, never the fastest
    Tuned T;
    T.geo = 4;
    // the tile workgroups only: scratch W / dW / raw, no bias groups
    const size_t mat = (((size_t)g.J * (size_t)g.ldw) + 3) & ~(size_t)3;
    float *s = tune_scratch(4 * mat);
    if (!s) return T;
    GradArgs t = g;
    t.nbias = 0; t.pen = nullptr; t.Wt = nullptr;
    t.W = s; t.dW = s + mat; t.raw = s + 2 * mat; t.raw2 = s + 3 * mat;
    (void)hipMemsetAsync(s, 0, 4 * mat * sizeof(float), st);
#ifdef BM_PROBE
    t.dbg = nullptr;
#endif
    TuneTimer tm;
    if (!tm.init(st)) return T;
    float us[NC], xi_us[5];
    best_of(tm, TUNE_ROUNDS, TUNE_REP, NC, us, [&](int c) { launch_grad_as(cand[c], t, st); });
    const int b = fastest(us, NC);
    if (b >= 0) T.geo = cand[b];
    T.xi = tune_tile_map(tm, t, xi_us, [&] { launch_grad_as(T.geo, t, st); });
    if (tune_log())      // (the slab order prints as 9 in this line)
        fprintf(stderr, "bm355 tune: grad I=%d J=%d K=%d+%d form=%d fused=%d -> geometry %d (us, dma: 4w %.1f, 8w %.1f; reg: 4w %.1f, 8w %.1f; 8w bk32 x2: %.1f), "
                        "tile map %d (9 slab, else XCD grid xi; us: slab %.1f, 8x1 %.1f, 4x2 %.1f, 2x4 %.1f, 1x8 %.1f)\n",
                g.I, g.J, g.Kpos, g.Kneg, g.form, g.fused, T.geo, us[0], us[1], us[2], us[3], us[4], T.xi == XI_SLAB ? 9 : T.xi, xi_us[4], xi_us[0], xi_us[1], xi_us[2], xi_us[3]);
    return T;
}
// fast-weights flavour (grad_kernel<..., GradFast>): as the centred one, the geometries 4 and 8 with DMA staging in
// a translation unit of its own (bm_grad_fast.hip); the bias tail and the penalty are both legal in it
void launch_grad_fast(int geo, const GradArgs &g, const GradFast &f, hipStream_t st);
// cen: the centred flavour (fused, no bias tail - its callers see to both); fw: the fast-weights flavour (fused); never both
static inline void launch_grad(const GradArgs &g_in, hipStream_t st, const GradCen *cen = nullptr, const GradFast *fw = nullptr) {
    static const int fetch_env = std::max(0, dbg_int("grad_fetch")), geo_env = dbg_int("grad_geo");   // overrides (experiments)
    GradArgs g = g_in;
    g.fetch_at_fill = fetch_env;      // measured (same box, 784x1024x512): epilogue 66.6 us/update, fill 67.5
    if (geo_env) {
        if (fw) launch_grad_fast(geo_env, g, *fw, st);
        else if (cen) launch_grad_cen(geo_env, g, *cen, st);
        else launch_grad_as(geo_env, g, st);
        return;
    }
    static TuneMemo<6> memo;
    // (the centred flavour shares the plain flavour's entry for the shape, as CL and RT do for act_kernel)
    const Tuned T = memo.get({g.I, g.J, g.Kpos, g.Kneg, g.form | (g.fused << 1), g.ldw}, [&] { return tune_grad_shape(g, st); });
    if (T.xi != XI_MODEL && !g.map_xi) g.map_xi = T.xi;
    // (a tuned 8-wave geometry - 8, 9, 108, 208 - takes the centred 8-wave kernel, the others the 4-wave one)
    const int geo48 = (T.geo == 8 || T.geo == 9 || T.geo == 108 || T.geo == 208) ? 8 : 4;
    if (fw) launch_grad_fast(geo48, g, *fw, st);
    else if (cen) launch_grad_cen(geo48, g, *cen, st);
    else launch_grad_as(T.geo, g, st);
}

static inline void launch_fe_hidden(const FeArgs &f, hipStream_t st) {
    const bool fast = operand_fast(f.P, KM, f.K) && operand_fast(f.Q, XM, f.K);
    const dim3 grid(tile_grid<GeoAct>(f.I, f.J)), blk(NT);
    if (fast) hipLaunchKernelGGL((fe_hidden_kernel<true>), grid, blk, 0, st, f);
    else      hipLaunchKernelGGL((fe_hidden_kernel<false>), grid, blk, 0, st, f);
}

// split apply (data-parallel step): the tiled kernel needs whole 16-byte groups (I % 4 == 0, pitches % 4 == 0); else the
// elementwise kernels
static inline void launch_apply_w(const ApplyWArgs &a, const RbmBiasArgs *bias, hipStream_t st) {
    const bool tiled = (a.I % 4 == 0) && (a.ldw % 4 == 0) && (!a.Wt || a.ldwt % 4 == 0);
    if (tiled) {
        RbmBiasArgs b;
        memset(&b, 0, sizeof(b));
        int nb = 0;
        if (bias) { b = *bias; nb = (b.V + b.H + 255) / 256; }
        const int ntile = ((a.I + 63) / 64) * ((a.J + 63) / 64);
        hipLaunchKernelGGL(apply_w_tiled_kernel, dim3(ntile + nb), dim3(256), 0, st, a, b, nb);
    } else {
        if (bias) hipLaunchKernelGGL(rbm_bias_kernel, dim3((bias->V + bias->H + 255) / 256), dim3(256), 0, st, *bias);
        hipLaunchKernelGGL(apply_w_kernel, dim3(1024), dim3(256), 0, st, a);
    }
}
#endif  // BM_KERNELS_ONLY

}  // namespace bm
