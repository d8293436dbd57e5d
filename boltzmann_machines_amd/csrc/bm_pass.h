// bm_pass.h — a propagation pass as a value, the vocabulary both engines describe their passes in (DESIGN.md 3.2, 3.5 "Host
// side"):  out = act(mult * (below.W_lo [+ above.W_hi^T]) + bmult * bias).  An engine's describer (bm_rbm.hip rbm_pass,
// bm_dbm.hip layer_pass) fills a LayerPass and queues nothing; named options say what else the pass leaves behind; the
// engine's issue() is the one place that launches.  The RBM is the one-layer stack: layer -1 is the visible pass, layer 0 the
// hidden pass.  Host code only.
#pragma once
#include "bm_common.h"
#include "bm_kernels.h"

namespace bm {

// a state matrix a pass reads: [J][n] with pitch ld
struct LayerIn { const float *p; int ld; };
static constexpr LayerIn NO_IN{nullptr, 0};
static inline LayerIn in_of(const Mat &m) { return LayerIn{m.p, m.ld}; }
// what a pass writes (either pointer may be null) and draws with
struct LayerOut { int sample; float *means, *states; int ld; PhiloxKey key; int64_t row0; };
// the layer's value: its sample, or - without sampling - its mean, written as `means` only
static inline LayerOut value_out(int sample, float *p, int ld, const PhiloxKey &key, int64_t row0) {
    return LayerOut{sample, sample ? nullptr : p, sample ? p : nullptr, ld, key, row0};
}

struct LayerPass {
    ActArgs a;
    int layer;                        // hidden layer index, -1 = visible
    const float *below, *above;       // the state matrices the segments read (fast-binary: their shadows)
    // ---- optional parts of the request
    LayerPass &raw() { a.kind = 2; return *this; }                       // the raw pre-activation mult * z (mean-field hoist)
    // another bias vector and its multiplier (AIS: the mixed visible bias of a temperature, taken once)
    LayerPass &bias(const float *b, float bmult) { a.bias = b; a.bmult = bmult; return *this; }
    LayerPass &negmeans_out(float *p) { a.negmeans = p; return *this; }              // -means as well (pitch of the outputs)
    // mean-field residual max |out - prev| into the atomic cell and / or the workgroups' slots
    LayerPass &residual(const float *prev, unsigned *cell, float *slots) { a.prev = prev; a.maxdiff = cell; a.maxdiff_blk = slots; return *this; }
    LayerPass &skip_if(const int *skip) { a.skip = skip; return *this; }             // device int != 0: the launch returns at once
    // the first kernel of a sweep evaluates the loop control of the previous sweep from the slots it left
    LayerPass &check(MfCtl *ctl, const float *slots, int n, float tol) { a.chk_ctl = ctl; a.chk_slots = slots; a.chk_n = n; a.chk_tol = tol; return *this; }
    // row-reduction epilogues into slot partials of pitch ldp: softplus(beta_b .) - softplus(beta_a .), or softplus(beta_b .)
    // alone (single); states . vec; z . mat; states . (z + bias) untempered (row_tempered passes)
    LayerPass &softplus_rows(float *out, int ldp, float beta_a, float beta_b, int single) {
        a.rowacc = out; a.ld_part = ldp; a.beta_a = beta_a; a.beta_b = beta_b; a.rowacc_single = single;
        return *this;
    }
    LayerPass &statedot_rows(float *out, int ldp, const float *vec) { a.rowdot_out = out; a.ld_part = ldp; a.dot_vec = vec; return *this; }
    LayerPass &zdot_rows(float *out, int ldp, const Mat &mat) { a.rowacc = out; a.ld_part = ldp; a.dot_mat = mat.p; a.ld_dot = mat.ld; return *this; }
    LayerPass &energy_rows(float *out, int ldp) { a.rowen_out = out; a.ld_part = ldp; return *this; }
    // conditional sampling: outputs with a non-zero mask entry hold `val` (both [J][I], pitch ld; ActArgs::clamp_mask)
    LayerPass &clamp(const float *val, const float *mask, int ld) { a.clamp_val = val; a.clamp_mask = mask; a.ld_clamp = ld; return *this; }
    // parallel tempering: row j's multiplier of z and of the bias is row_mult[j] instead of mult / bmult (the RT flavour)
    LayerPass &row_tempered(const float *row_mult) { a.row_mult = row_mult; return *this; }
    // ... and, rows grouped in runs of R, the row_mult == 1 row of every group c < rows also stores its states at out + c * ld
    LayerPass &select_rows(float *out, int ld, int R, int rows) { a.sel_out = out; a.sel_ld = ld; a.sel_R = R; a.sel_rows = rows; return *this; }
    // class head: the slot partials, per class c < C, of sum_i softplus(t_i + U[c][i]) at part[(c * nslots(I) + slot) * ldp + j], of a
    // logits pass (kind 3, mult 1: t = z + bias is what it stores); the CR flavour (ActArgs::cr_part)
    LayerPass &class_rows(float *part, int ldp, const float *U, int ldu, int C) {
        a.cr_part = part; a.ld_part = ldp; a.cr_U = U; a.cr_ldu = ldu; a.cr_C = C; a.cr_nslots = nslots(a.I);
        return *this;
    }
    // joint chain of the classification RBM: row j's bias is bias[i] + U[y[j]][i] (one rounded add; mult == bmult == 1); a label
    // outside [0, C) keeps the plain bias and raises *bad; the CB flavour (ActArgs::cb_y)
    LayerPass &class_bias(const int *y, const float *U, int ldu, int C, int *bad) {
        a.cb_y = y; a.cb_U = U; a.cb_ldu = ldu; a.cb_C = C; a.cb_bad = bad;
        return *this;
    }
    // metric fetch riding on a prop-up of x [J][K] (pitch ldx) through w [K][I] (pitch ldw): the row-major slot partials
    // ([ldp][rm] each) of sum softplus(z + b) for x and, behind them, for its PLL partner - the flip column drawn from
    // `flip_key`; the pass also zeroes the fetch's accumulators `zero` (ActArgs::fe_flip)
    LayerPass &free_energy_fetch(float *part, int rm, int ldp, const PhiloxKey &flip_key, double *zero, const float *x, int ldx,
                                 const float *w, int ldw) {
        a.rowacc = part; a.rowacc_single = 1; a.beta_b = 1.f; a.ld_part = ldp; a.fe_rm = rm;
        a.fe_rowacc2 = part + (size_t)rm * ldp;
        a.fe_flip = FE_FLIP_FROM_KEY; a.fe_key = flip_key; a.fe_zero = zero;
        a.fe_x = x; a.fe_ldx = ldx; a.fe_w = w; a.fe_ldw = ldw;
        return *this;
    }
};

}  // namespace bm
