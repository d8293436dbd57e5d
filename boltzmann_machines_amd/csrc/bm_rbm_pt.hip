// bm_rbm_pt.hip - parallel tempering on an RBM handle, for every visible unit that has it (bm355.h; DESIGN.md 3.13 "Structure"):
// Bernoulli (bm_rbm_pt_*, 3.13 / 3.14), softmax groups (bm_rbm_groups_pt_*, 3.29), replicated softmax (bm_rbm_rsm_pt_*, 3.31) and
// Gaussian (bm_rbm_gauss_pt_*, 3.30).  Part of the main translation unit: bm355.hip includes it right after bm_rbm.hip, whose
// handle, passes and checks it uses.  What does not depend on the model - the ensemble, its start, the replica exchange, the
// rescore, the gather, the sweep loop and the read tail - is bm_pt.h, shared with bm_dbm_pt_*.
//
// A family is its *_pt_init, its step function and one PtFamily that names what the shared bodies below ask of it: pt_sweep,
// pt_read, pt_train_step and pt_train_epoch are written once, and every exported entry but the inits is a wrapper that names its
// family.  The handle holds ONE ensemble (bm_rbm::pt) and the tag of the family that built it (bm_rbm::pt_unit): a *_pt_init
// drops what is there (pt_drop) and sets its tag once the start went through; every other entry asks for an ensemble of its own
// family.

struct PtFamily {
    PtUnit unit;
    const char *prefix;                                        // the entries are <prefix>_pt_sweep, <prefix>_train_step_pt, ...
    int (*check)(const bm_rbm *h, const char *what);           // the model check (a null handle included)
    void (*step)(bm_rbm *h, int t, int sel_rows);              // step t of a tempered call
    // the rest is the tempered update's (null where the family has none: Gaussian) ...
    bool (*can_select)(const bm_rbm *h);                       // the last prop-down can select the beta = 1 rows; null: always
    void (*rescore)(bm_rbm *h);                                // the v.vb partials of the swap energy under the vb of now
    void (*before_positive)(bm_rbm *h, const float *X_dev, int B);      // launches in front of the positive pass; null: none
    void (*negmeans)(bm_rbm *h, LayerPass &neg);               // what the negative-means pass reads besides; null: nothing
    void (*update)(bm_rbm *h, int B, float lr, float mom);
    // ... and the read's: what happens to the gathered rows V_dev [M][V] in stream order; null: nothing
    void (*after_gather)(bm_rbm *h, float *V_dev);
};

// "<prefix><suffix>", the name of an entry in its messages
struct PtEntry {
    char s[48];
    PtEntry(const PtFamily &f, const char *suffix) { snprintf(s, sizeof(s), "%s%s", f.prefix, suffix); }
};

// the raw z of the ensemble's prop-down for `rows` rows; a failed allocation leaves nothing counted
static int ensure_pt_z(bm_rbm *h, int rows) {
    if (rows <= h->ptz_rows) return 0;
    h->ptz_rows = 0;
    BM_TRY(h->pt_z.alloc(rows, h->V));
    h->ptz_rows = rows;
    return 0;
}

// the model check of the entry `what`, then an ensemble of the family's own
static int pt_need(const bm_rbm *h, const PtFamily &f, const char *what) {
    BM_TRY(f.check(h, what));
    BM_CHECK(h->pt_unit == f.unit, "%s: no ensemble (call %s_pt_init first)", what, f.prefix);
    return 0;
}

// ---- the shared bodies

static int pt_sweep(bm_rbm *h, const PtFamily &f, int n_steps) {
    const PtEntry what(f, "_pt_sweep");
    BM_TRY(pt_need(h, f, what.s));
    BM_CHECK(n_steps >= 1, "%s: n_steps must be >= 1 (got %d)", what.s, n_steps);
    ensure_wt(h);
    pt_sweep_with(h->pt, n_steps, [&](int t) { f.step(h, t, 0); });
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

static int pt_read(bm_rbm *h, const PtFamily &f, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    const PtEntry what(f, "_pt_read");
    BM_TRY(pt_need(h, f, what.s));
    BM_CHECK(V_dev || !H_dev, "%s: H_dev without V_dev", what.s);
    float *const dst[3] = {V_dev, H_dev, nullptr};
    const int ldd[3] = {h->V, h->H, 0};
    return pt_read_with(h->pt, h->stream, dst, ldd, swaps_host, ladder_idx_host,
                        [&] { if (f.after_gather && V_dev) f.after_gather(h, V_dev); });
}

// One update whose negative phase is the tempered ensemble (bm355.h).  No host synchronisation.  The seven steps
// are one family's as another's; ensure_eff and EffScope do nothing on a handle without fast weights, and only a Bernoulli handle
// has them (or dropout)
static int pt_train_step(bm_rbm *h, const PtFamily &f, const float *X_dev, int B, float lr, float mom, int k) {
    const PtEntry what(f, "_train_step_pt");
    BM_TRY(f.check(h, what.s));
    BM_CHECK(X_dev, "null argument");
    BM_TRY(check_dw(h, what.s));
    BM_CHECK(h->pt_unit == f.unit, "%s: no ensemble (call %s_pt_init first)", what.s, f.prefix);
    BM_CHECK(h->cfg.dropout < 0.f, "%s: the tempered family has no dropout (this handle's is %g)", what.s, (double)h->cfg.dropout);
    PtEnsemble &e = h->pt;
    BM_CHECK(B >= 1 && B <= std::min(h->maxB, e.M), "%s: batch %d outside [1, min(max_batch=%d, n_chains=%d)]", what.s, B, h->maxB, e.M);
    BM_CHECK(k >= 1, "n_gibbs_steps must be >= 1 (got %d)", k);
    static const bool sel_env = !dbg("pt_sel") || atoi(dbg("pt_sel")) != 0;         // BM355_DEBUG=pt_sel=0: a gather launch instead
    const bool sel_in_pass = sel_env && (!f.can_select || f.can_select(h));
    ensure_wt(h);
    ensure_eff(h);
    // 1. the v.vb partials of the swap energy under the vb of NOW (the previous update changed it; fast weights: the effective vb)
    f.rescore(h);
    // 2. positive phase: the h0 means alone
    h->Xin = X_dev; h->Xin_ld = h->V;
    h->fe_in_chain = false;
    if (f.before_positive) f.before_positive(h, X_dev, B);
    issue(h, rbm_pass(h, true, B, LayerIn{X_dev, h->V}, rbm_out(h, 0, h->h0m.p, nullptr, h->h0m.ld, SITE_H0, 0)));
    {
        EffScope eff(h);      // fast weights: the whole negative phase lives under the effective set
        // 3. + 4. the tempered steps; the last prop-down leaves the beta = 1 rows of the chains [0, B) in vs
        for (int t = 0; t < k; ++t) f.step(h, t, (sel_in_pass && t == k - 1) ? B : 0);
        if (!sel_in_pass) {
            float *const dst[3] = {h->vs.p, nullptr, nullptr};
            const int ldd[3] = {h->vs.ld, 0, 0};
            pt_launch_gather(e, h->stream, B, dst, ldd);
        }
        // 5. negative means: only -h is consumed (run_chain's neg_only form)
        LayerPass neg = rbm_pass(h, true, B, in_of(h->vs), rbm_out(h, 0, nullptr, nullptr, h->hm.ld, SITE_H, 0)).negmeans_out(h->hneg.p);
        if (f.negmeans) f.negmeans(h, neg);
        issue(h, neg);
        h->hm_is_neg = true;
    }
    // 6. + 7.
    f.update(h, B, lr, mom);
    e.step += k;
    h->call++;
    BM_HIP(hipGetLastError());
    return 0;
}

// the native batch loop of pt_train_step (as bm_rbm_train_epoch is to bm_rbm_train_step)
static int pt_train_epoch(bm_rbm *h, const PtFamily &f, const float *X_dev, int64_t N, int batch, float lr, float mom, int k) {
    const PtEntry what(f, "_train_epoch_pt");
    BM_TRY(f.check(h, what.s));
    BM_CHECK(X_dev, "null argument");
    BM_CHECK(batch >= 1 && N >= 1, "bad N=%lld batch=%d", (long long)N, batch);
    for (int64_t s = 0; s < N; s += batch) {
        const int B = (int)((N - s < batch) ? (N - s) : batch);
        BM_TRY(pt_train_step(h, f, X_dev + (size_t)s * h->V, B, lr, mom, k));
    }
    return 0;
}

// ---- Bernoulli visible units

// step t of a tempered call: the RT prop-up, the swap of the parity of the global step number, the RT prop-down.  The passes are
// row-tempered (the RT flavour of act_kernel): up = h ~ Ber(sigmoid(beta_row (vW + hb))) from pt.v into pt.h1, leaving the slot
// partials of h.(vW + hb); down = v ~ Ber(sigmoid(beta_row (hW^T + vb))) from pt.h1 into pt.v, leaving those of v.vb
// sel_rows > 0: the prop-down also leaves the beta = 1 row of every chain c < sel_rows in vs[c] (ActArgs::sel_out)
static void pt_step(bm_rbm *h, int t, int sel_rows = 0) {
    PtEnsemble &e = h->pt;
    const int rows = e.nrows();
    issue(h, rbm_pass(h, true, rows, in_of(e.v.x), value_out(1, e.h1.x.p, e.h1.x.ld, make_key(h, SITE_H, t), e.row0()))   // (mult: not read)
                 .energy_rows(e.h1.part.p, e.rows).row_tempered(e.mult.p));
    pt_launch_swap(h->pt, h->stream, t, make_key(h, SITE_PT_SWAP, t));
    LayerPass down = rbm_pass(h, false, rows, in_of(e.h1.x), value_out(1, e.v.x.p, e.v.x.ld, make_key(h, SITE_V, t), e.row0()))
                         .statedot_rows(e.v.part.p, e.rows, pass_vb(h)).row_tempered(e.mult.p);
    if (sel_rows > 0) down.select_rows(h->vs.p, h->vs.ld, e.R, sel_rows);
    issue(h, down);
}
static int check_bernoulli_pt(const bm_rbm *h, const char *what) {
    BM_CHECK(h, "null argument");
    return refuse_nrelu(h, what);
}
// (fast weights: the effective vb; the groups' rescore too - a handle with groups has no fast weights)
static void pt_rescore_vb(bm_rbm *h) { pt_launch_rescore(h->pt, h->stream, h->fw_on ? h->vbe.p : h->vb.p, nullptr); }
// (fast weights: the fast and effective sets move in the same launches)
static void pt_update(bm_rbm *h, int B, float lr, float mom) {
    if (h->fw_on) launch_update_fast(h, B, lr, mom);
    else launch_update_fused(h, B, lr, mom);
}
static const PtFamily PT_FAMILY_BERNOULLI = {PT_BERNOULLI, "bm_rbm", check_bernoulli_pt, pt_step,
                                             nullptr, pt_rescore_vb, nullptr, nullptr, pt_update, nullptr};

// ---- softmax visible units.  A handle with visible groups holds no other ensemble (bm_rbm_pt_init refuses it,
// bm_rbm_set_visible_groups refuses a handle that holds another), and turning the groups off discards it.
static int check_groups_pt(const bm_rbm *h, const char *what) {
    BM_TRY(need_groups(h, what));
    BM_CHECK(!h->groups_missing, "%s: not built for incomplete rows (bm_rbm_groups_set_missing is on): a row of the tempered ensemble "
             "has no pattern of observed groups; see DESIGN.md 3.29", what);
    return 0;
}
// The prop-down of step t: v_g ~ softmax_k(beta_row (h W^T + vb)_{gK+k}) from pt.h1 into pt.v, leaving the slot partials of v.vb.
// Fused route: ONE launch, the SM + SA + RT flavour; sel_rows > 0: it also leaves the beta = 1 row of every chain c < sel_rows in
// vs[c].  Generic route: a raw pass (z = h W^T, the plain kernels), the tempered groups kernel, the row-dot kernel - the same bits;
// its hand-over is the caller's gather launch
static void groups_pt_down(bm_rbm *h, int t, int sel_rows) {
    PtEnsemble &e = h->pt;
    const int rows = e.nrows();
    const PhiloxKey key = make_key(h, SITE_V, t);
    LayerPass p = rbm_pass(h, false, rows, in_of(e.h1.x), value_out(1, e.v.x.p, e.v.x.ld, key, e.row0()));
    ActArgs &a = p.a;
    if (groups_fused(h)) {
        ProfScope _ps(h, KC_DOWN);
        p.statedot_rows(e.v.part.p, e.rows, h->vb.p).row_tempered(e.mult.p);
        if (sel_rows > 0) p.select_rows(h->vs.p, h->vs.ld, e.R, sel_rows);
        a.kind = 3; a.sm_k = h->v_groups; a.sm_ais = 1; a.sm_absent = nullptr;
        launch_act_sm_pt(a, h->stream);
        return;
    }
    a.kind = 2; a.sample = 0; a.states = nullptr; a.means = h->pt_z.p; a.ldo = h->pt_z.ld;
    {
        ProfScope _ps(h, KC_DOWN);
        launch_act(a, h->stream);
    }
    ProfScope _ps(h, KC_OTHER);                        // (per-class event timing: the route's extra launches are the class `other`)
    SpGroupsArgs g;
    memset(&g, 0, sizeof(g));
    g.Z = h->pt_z.p; g.ldz = h->pt_z.ld; g.states = e.v.x.p; g.ld_states = e.v.x.ld;
    g.V = h->V; g.K = h->v_groups; g.J = rows; g.bias = h->vb.p; g.row_mult = e.mult.p; g.key = key; g.row0 = e.row0();
    launch_softmax_pt_groups(g, h->stream);
    launch_softmax_ais_dot(e.v.x.p, e.v.x.ld, rows, h->V, h->vb.p, e.v.part.p, e.rows, h->stream);
}
// step t of a tempered call: the RT prop-up and the swap of pt_step, unchanged - for one-hot v they are this model's - then the
// tempered softmax prop-down
static void groups_pt_step(bm_rbm *h, int t, int sel_rows = 0) {
    PtEnsemble &e = h->pt;
    issue(h, rbm_pass(h, true, e.nrows(), in_of(e.v.x), value_out(1, e.h1.x.p, e.h1.x.ld, make_key(h, SITE_H, t), e.row0()))   // (mult: not read)
                 .energy_rows(e.h1.part.p, e.rows).row_tempered(e.mult.p));
    pt_launch_swap(e, h->stream, t, make_key(h, SITE_PT_SWAP, t));
    groups_pt_down(h, t, sel_rows);
}
// (the generic route always gathers)
static const PtFamily PT_FAMILY_GROUPS = {PT_GROUPS, "bm_rbm_groups", check_groups_pt, groups_pt_step,
                                          groups_fused, pt_rescore_vb, nullptr, nullptr, launch_update_fused, nullptr};

// ---- replicated softmax visible units.  The ensemble has a two-slot visible partial array (the float32 pair of the
// double v.vb).  A handle with the unit holds no other ensemble (bm_rbm_pt_init refuses it, bm_rbm_set_replicated_softmax refuses a
// handle that holds another), and turning the unit off or changing max_length discards it.
static int check_rsm_pt(const bm_rbm *h, const char *what) {
    BM_CHECK(h, "%s: null argument", what);
    BM_CHECK(h->rsm_len, "%s needs a handle with replicated softmax visible units (bm_rbm_set_replicated_softmax): bm_rbm_pt_* / "
             "bm_rbm_groups_pt_* serve the other units", what);
    return 0;
}
// the prop-up of step t: h ~ Ber(sigmoid(beta_row (v W + D_row hb))) from pt.v into pt.h1, leaving the slot partials of h.(vW + D hb):
// the DB + RT flavour, asked for by name (issue() goes through launch_act, which has no such route); W^T x-major where the handle
// keeps a valid one, as issue() reads it
static void rsm_pt_up(bm_rbm *h, int t) {
    PtEnsemble &e = h->pt;
    LayerPass p = rbm_pass(h, true, e.nrows(), in_of(e.v.x), value_out(1, e.h1.x.p, e.h1.x.ld, make_key(h, SITE_H, t), e.row0()));   // (mult: not read)
    p.energy_rows(e.h1.part.p, e.rows).row_tempered(e.mult.p);
    ActArgs &a = p.a;
    a.row_bmult = h->rp_len.p;
    if (h->use_wt && h->wt_valid) { a.P1 = make_operand(h->Wt.p, h->Wt.ld, h->H); a.p_xm = 1; }
    ProfScope _ps(h, KC_UP);
    launch_act_db_pt(a, h->stream);
}
// the prop-down of step t: a raw pass z = h W^T (kind 2, mult 1: the plain kernels) into pt_z, then the PT flavour of the count kernel:
// v ~ Multinomial(D_row, softmax(beta_row (z + vb))) into pt.v, the pair of v.vb into pt.v.part; sel_rows > 0: the beta = 1 row of
// every chain c < sel_rows also goes to vs[c]
static void rsm_pt_down(bm_rbm *h, int t, int sel_rows) {
    PtEnsemble &e = h->pt;
    const int rows = e.nrows();
    const PhiloxKey key = make_key(h, SITE_V, t);
    LayerPass p = rbm_pass(h, false, rows, in_of(e.h1.x), LayerOut{0, h->pt_z.p, nullptr, h->pt_z.ld, key, e.row0()}, 1.0f);
    p.a.kind = 2; p.a.sample = 0; p.a.states = nullptr;
    {
        ProfScope _ps(h, KC_DOWN);
        launch_act(p.a, h->stream);
    }
    ProfScope _ps(h, KC_OTHER);                        // (per-class event timing: the count kernel is the class `other`, as in 3.27)
    McPtArgs m;
    memset(&m, 0, sizeof(m));
    m.L = h->pt_z.p; m.ld = h->pt_z.ld; m.states = e.v.x.p; m.ld_states = e.v.x.ld; m.lengths = h->rp_len.p;
    m.V = h->V; m.J = rows; m.sample = 1; m.max_length = h->rsm_len; m.key = key; m.row0 = e.row0();
    m.dvec = h->vb.p; m.part = e.v.part.p; m.ld_part = e.rows;
    m.bias = h->vb.p; m.row_mult = e.mult.p;
    if (sel_rows > 0) { m.sel_out = h->vs.p; m.sel_ld = h->vs.ld; m.sel_R = e.R; m.sel_rows = sel_rows; }
    if (launch_multinomial_counts_pt(m, h->stream)) abort();       // (bm_rbm_set_replicated_softmax checked the width)
}
static void rsm_pt_step(bm_rbm *h, int t, int sel_rows = 0) {
    rsm_pt_up(h, t);
    pt_launch_swap(h->pt, h->stream, t, make_key(h, SITE_PT_SWAP, t));
    rsm_pt_down(h, t, sel_rows);
}
// the tempered update's own: the v.vb pair under the vb of now; the batch's lengths for the positive pass (plain DB); the CHAINS'
// lengths Dn_c, c < B, for the negative means; the bias block with the two length vectors in front, then the unchanged grad_kernel
// without its bias tail
static void rsm_pt_rescore(bm_rbm *h) {
    PtEnsemble &e = h->pt;
    launch_rsm_pt_rescore(e.v.x.p, e.v.x.ld, e.nrows(), h->V, h->vb.p, e.v.part.p, e.rows, h->stream);
}
static void rsm_pt_batch_lengths(bm_rbm *h, const float *X_dev, int B) { rsm_lengths_of(h, X_dev, h->V, B, h->rsm_D.p); }
static void rsm_pt_negmeans(bm_rbm *h, LayerPass &neg) { neg.a.row_bmult = h->rp_clen.p; }
static void rsm_pt_update(bm_rbm *h, int B, float lr, float mom) {
    {
        ProfScope _ps(h, KC_COLSUM);
        RbmBiasFusedArgs a;
        fill_bias_fused(h, B, lr, mom, a);
        launch_rsm_bias2(a, h->rsm_D.p, h->rp_clen.p, h->stream);
    }
    rbm_grad(h, B, 1, (float)B, lr, mom, false);
}
static const PtFamily PT_FAMILY_COUNTS = {PT_COUNTS, "bm_rbm_rsm", check_rsm_pt, rsm_pt_step,
                                          nullptr, rsm_pt_rescore, rsm_pt_batch_lengths, rsm_pt_negmeans, rsm_pt_update, nullptr};

// ---- Gaussian visible units (check_gauss_joint, gauss_prep and the unit's other entries: bm_rbm.hip)

// The one-launch route of the tempered prop-down (the RT + GT flavour) unless BM355_DEBUG=gt_fused=0 asks for the generic one
static bool gauss_pt_fused() {
    static const bool off = bm::dbg("gt_fused") && atoi(bm::dbg("gt_fused")) == 0;
    return !off;
}
// Step t of a tempered call: the RT prop-up and the swap of pt_step, unchanged - h | u at beta is Ber(sigmoid(beta (u W + hb))), and
// with part_v = the slots of -1/2 |u - c|^2 the swap's E = -(sum part_v + sum part_h1) is 1/2 |u - c|^2 - h.(u W + hb) - then the
// prop-down u ~ N(c + W h, I / beta_row).  Fused route: ONE launch.  Generic route: a raw pass (z = h W^T, the plain kernels) and the
// row kernel - the same bits.  (No tempered update: nothing selects rows)
static void gauss_pt_step(bm_rbm *h, int t, int /*sel_rows*/ = 0) {
    PtEnsemble &e = h->pt;
    const int rows = e.nrows();
    issue(h, rbm_pass(h, true, rows, in_of(e.v.x), value_out(1, e.h1.x.p, e.h1.x.ld, make_key(h, SITE_H, t), e.row0()))   // (mult: not read)
                 .energy_rows(e.h1.part.p, e.rows).row_tempered(e.mult.p));
    pt_launch_swap(e, h->stream, t, make_key(h, SITE_PT_SWAP, t));
    const PhiloxKey key = make_key(h, SITE_V, t);
    LayerPass p = rbm_pass(h, false, rows, in_of(e.h1.x), value_out(1, e.v.x.p, e.v.x.ld, key, e.row0()), 1.0f);
    ActArgs &a = p.a;
    a.bias = h->gc.p; a.sigma = nullptr;
    if (gauss_pt_fused()) {
        ProfScope _ps(h, KC_DOWN);
        a.kind = 3;
        a.rowdot_out = e.v.part.p; a.ld_part = e.rows; a.row_mult = e.mult.p; a.gt_sd = h->gpt_sd.p; a.gt_idx = e.idx.p;
        launch_act_gauss_pt(a, h->stream);
        return;
    }
    a.kind = 2; a.sample = 0; a.states = nullptr; a.means = h->pt_z.p; a.ldo = h->pt_z.ld;
    {
        ProfScope _ps(h, KC_DOWN);
        launch_act(a, h->stream);
    }
    ProfScope _ps(h, KC_OTHER);
    GpRowsArgs g;
    memset(&g, 0, sizeof(g));
    g.Z = h->pt_z.p; g.ldz = h->pt_z.ld; g.states = e.v.x.p; g.ld_states = e.v.x.ld; g.V = h->V; g.J = rows;
    g.c = h->gc.p; g.sd = h->gpt_sd.p; g.idx = e.idx.p; g.key = key; g.row0 = e.row0(); g.part = e.v.part.p; g.ld_part = e.rows;
    launch_gauss_pt_rows(g, h->stream);
}
// the read: x = u sigma on the dense result of the gather
static void gauss_pt_scale(bm_rbm *h, float *V_dev) { launch_gauss_scale_rows(V_dev, h->pt.M, h->V, h->sigma.p, h->stream); }
static const PtFamily PT_FAMILY_GAUSS = {PT_GAUSS, "bm_rbm_gauss", check_gauss_joint, gauss_pt_step,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, gauss_pt_scale};

extern "C" {

// ---- the starts: each drops the ensemble that is there once its own arguments are checked, and tags the new one as its last act

// Parallel tempering (replica exchange).  The ensemble lives in the handle; see bm355.h for the contract.
int bm_rbm_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0) {
    BM_CHECK(h, "null argument");
    BM_TRY(check_single_joint(h, "bm_rbm_pt_init"));
    BM_TRY(pt_check_ladder(n_chains, n_temps, betas_host, chain0));
    pt_drop(h);
    const int widths[3] = {h->V, h->H, 0};
    const PhiloxKey key = make_key(h, SITE_PT_V0, 0);
    BM_TRY(pt_begin(h->pt, h->stream, widths, n_chains, n_temps, chain0, betas_host, V0_dev, h->vb.p, nullptr, key, key));
    h->pt_unit = PT_BERNOULLI;
    return 0;
}

int bm_rbm_groups_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0) {
    BM_TRY(check_groups_pt(h, "bm_rbm_groups_pt_init"));
    BM_TRY(pt_check_ladder(n_chains, n_temps, betas_host, chain0));
    pt_drop(h);
    if (!groups_fused(h)) BM_TRY(ensure_pt_z(h, n_chains * n_temps));
    const int widths[3] = {h->V, h->H, 0};
    const PhiloxKey key = make_key(h, SITE_PT_V0, 0);
    BM_TRY(pt_begin_with(h->pt, h->stream, widths, n_chains, n_temps, chain0, betas_host, [&](PtEnsemble &e, int rows) {
        SpStartArgs s0;
        memset(&s0, 0, sizeof(s0));
        s0.v = e.v.x.p; s0.ld = e.v.x.ld; s0.rows = rows; s0.R = n_temps; s0.V = h->V; s0.K = h->v_groups;
        s0.V0 = V0_dev; s0.vb = h->vb.p; s0.beta = e.beta.p;
        s0.key = key; s0.row0 = (unsigned long long)chain0 * (unsigned long long)n_temps;
        s0.part = e.v.part.p; s0.ld_part = e.rows; s0.row_mult = e.mult.p; s0.idx = e.idx.p;
        launch_softmax_pt_init(s0, h->stream);
    }));
    h->pt_unit = PT_GROUPS;
    return 0;
}

int bm_rbm_rsm_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *lengths_host, const float *V0_dev,
                       int64_t chain0) {
    BM_TRY(check_rsm_pt(h, "bm_rbm_rsm_pt_init"));
    BM_TRY(pt_check_ladder(n_chains, n_temps, betas_host, chain0));
    BM_CHECK(lengths_host, "bm_rbm_rsm_pt_init: null argument");
    for (int c = 0; c < n_chains; ++c) {
        const float D = lengths_host[c];
        BM_CHECK(D >= 1.0f && D <= (float)h->rsm_len && D == truncf(D), "bm_rbm_rsm_pt_init: lengths_host[%d] = %g is no integer in "
                 "[1, max_length = %d]", c, (double)D, h->rsm_len);
    }
    pt_drop(h);
    const int M = n_chains, R = n_temps, rows = M * R;
    BM_TRY(ensure_pt_z(h, rows));
    if (rows > h->rp_rows) {                           // (a failed allocation leaves nothing counted)
        h->rp_rows = 0;
        BM_TRY(h->rp_len.alloc(rows)); BM_TRY(h->rp_clen.alloc(rows)); BM_TRY(h->rp_v0len.alloc(rows));
        h->rp_rows = rows;
    }
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipMemcpy(h->rp_clen.p, lengths_host, (size_t)M * sizeof(float), hipMemcpyHostToDevice));
    // row_lengths_kernel's flag is the handle's: what an earlier batch left there and bm_rbm_sync has not reported yet is set aside
    // for the start (the stream is idle) and put back behind it, so that the start answers for its own rows alone
    int pending = 0;
    if (V0_dev) {
        BM_HIP(hipMemcpy(&pending, h->rsm_bad.p, sizeof(int), hipMemcpyDeviceToHost));
        if (pending) BM_HIP(hipMemset(h->rsm_bad.p, 0, sizeof(int)));
    }
    const int widths[3] = {h->V, h->H, 0};
    const PhiloxKey key = make_key(h, SITE_PT_V0, 0);
    BM_TRY(pt_begin_with(h->pt, h->stream, widths, M, R, chain0, betas_host, [&](PtEnsemble &e, int nrows) {
        // the sums of the start rows, with row_lengths_kernel's own flags; the start kernel compares them with the chains' lengths
        if (V0_dev) launch_row_lengths(RowLenArgs{V0_dev, h->V, h->V, M, h->rp_v0len.p, h->rsm_len, h->rsm_bad.p}, h->stream);
        RsmPtStartArgs s0;
        memset(&s0, 0, sizeof(s0));
        s0.v = e.v.x.p; s0.ld = e.v.x.ld; s0.rows = nrows; s0.R = R; s0.V = h->V;
        s0.V0 = V0_dev; s0.V0_len = V0_dev ? h->rp_v0len.p : nullptr; s0.chain_len = h->rp_clen.p; s0.beta = e.beta.p;
        s0.row_mult = e.mult.p; s0.len = h->rp_len.p; s0.idx = e.idx.p; s0.bad = h->rsm_bad.p;
        launch_rsm_pt_start(s0, h->stream);
        if (!V0_dev) {                                 // v_0 ~ Multinomial(D_c, uniform): the count flavour on zero z and zero bias
            McPtArgs m;
            memset(&m, 0, sizeof(m));
            m.states = e.v.x.p; m.ld_states = e.v.x.ld; m.lengths = h->rp_len.p;
            m.V = h->V; m.J = nrows; m.sample = 1; m.max_length = h->rsm_len; m.key = key;
            m.row0 = (long long)chain0 * (long long)R;
            m.dvec = h->vb.p; m.part = e.v.part.p; m.ld_part = e.rows; m.row_mult = e.mult.p;
            if (launch_multinomial_counts_pt(m, h->stream)) abort();
        }
        launch_rsm_pt_rescore(e.v.x.p, e.v.x.ld, nrows, h->V, h->vb.p, e.v.part.p, e.rows, h->stream);
    }, 2));
    if (V0_dev) {                                      // a start row that is no count row of its chain's length: no ensemble
        BM_HIP(hipStreamSynchronize(h->stream));
        const int rc = check_row_lengths(h);
        if (pending) BM_HIP(hipMemcpy(h->rsm_bad.p, &pending, sizeof(int), hipMemcpyHostToDevice));
        if (rc) { pt_drop(h); return rc; }
    }
    h->pt_unit = PT_COUNTS;
    return 0;
}

int bm_rbm_gauss_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0) {
    BM_TRY(check_gauss_joint(h, "bm_rbm_gauss_pt_init"));
    BM_TRY(pt_check_ladder(n_chains, n_temps, betas_host, chain0));
    pt_drop(h);
    if (!gauss_pt_fused()) BM_TRY(ensure_pt_z(h, n_chains * n_temps));
    // sd[r] = float32(1 / sqrt(double(beta_r))): exactly 1 at beta = 1
    std::vector<float> sd(n_temps);
    for (int r = 0; r < n_temps; ++r) sd[r] = (float)(1.0 / sqrt((double)betas_host[r]));
    if (h->gpt_sd.n < (size_t)n_temps) BM_TRY(h->gpt_sd.alloc(n_temps));
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipMemcpy(h->gpt_sd.p, sd.data(), (size_t)n_temps * sizeof(float), hipMemcpyHostToDevice));
    BM_TRY(gauss_prep(h));
    const int widths[3] = {h->V, h->H, 0};
    const PhiloxKey key = make_key(h, SITE_PT_V0, 0);
    BM_TRY(pt_begin_with(h->pt, h->stream, widths, n_chains, n_temps, chain0, betas_host, [&](PtEnsemble &e, int nrows) {
        GpStartArgs s0;
        memset(&s0, 0, sizeof(s0));
        s0.v = e.v.x.p; s0.ld = e.v.x.ld; s0.rows = nrows; s0.R = n_temps; s0.V = h->V;
        s0.V0 = V0_dev; s0.c = h->gc.p; s0.sigma = h->sigma.p; s0.beta = e.beta.p; s0.sd = h->gpt_sd.p;
        s0.key = key; s0.row0 = (unsigned long long)chain0 * (unsigned long long)n_temps;
        s0.part = e.v.part.p; s0.ld_part = e.rows; s0.row_mult = e.mult.p; s0.idx = e.idx.p;
        launch_gauss_pt_init(s0, h->stream);
    }));
    h->pt_unit = PT_GAUSS;
    return 0;
}

// ---- every other entry names its family (the Bernoulli ones keep their null-argument check in front of the model's)

int bm_rbm_pt_sweep(bm_rbm *h, int32_t n_steps) { return pt_sweep(h, PT_FAMILY_BERNOULLI, n_steps); }
int bm_rbm_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    return pt_read(h, PT_FAMILY_BERNOULLI, V_dev, H_dev, swaps_host, ladder_idx_host);
}
int bm_rbm_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k) {
    BM_CHECK(h && X_dev, "null argument");
    return pt_train_step(h, PT_FAMILY_BERNOULLI, X_dev, B, lr, mom, k);
}
int bm_rbm_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t k) {
    BM_CHECK(h && X_dev, "null argument");
    return pt_train_epoch(h, PT_FAMILY_BERNOULLI, X_dev, N, batch, lr, mom, k);
}

int bm_rbm_groups_pt_sweep(bm_rbm *h, int32_t n_steps) { return pt_sweep(h, PT_FAMILY_GROUPS, n_steps); }
int bm_rbm_groups_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    return pt_read(h, PT_FAMILY_GROUPS, V_dev, H_dev, swaps_host, ladder_idx_host);
}
int bm_rbm_groups_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k) {
    return pt_train_step(h, PT_FAMILY_GROUPS, X_dev, B, lr, mom, k);
}
int bm_rbm_groups_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t k) {
    return pt_train_epoch(h, PT_FAMILY_GROUPS, X_dev, N, batch, lr, mom, k);
}

int bm_rbm_rsm_pt_sweep(bm_rbm *h, int32_t n_steps) { return pt_sweep(h, PT_FAMILY_COUNTS, n_steps); }
int bm_rbm_rsm_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    return pt_read(h, PT_FAMILY_COUNTS, V_dev, H_dev, swaps_host, ladder_idx_host);
}
int bm_rbm_rsm_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t k) {
    return pt_train_step(h, PT_FAMILY_COUNTS, X_dev, B, lr, mom, k);
}
int bm_rbm_rsm_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t k) {
    return pt_train_epoch(h, PT_FAMILY_COUNTS, X_dev, N, batch, lr, mom, k);
}

int bm_rbm_gauss_pt_sweep(bm_rbm *h, int32_t n_steps) { return pt_sweep(h, PT_FAMILY_GAUSS, n_steps); }
// the beta = 1 rows: the gather of bm_rbm_pt_read, then x = u sigma on the dense result
int bm_rbm_gauss_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host) {
    return pt_read(h, PT_FAMILY_GAUSS, V_dev, H_dev, swaps_host, ladder_idx_host);
}

// A launch-level probe of the two tempered prop-ups (tests): h ~ Ber(sigmoid(beta (v W + D_j hb))) of the J rows of V_dev [J][V]
// with the lengths lengths_dev [J] into H_dev [J][H] (dense), drawn at SITE_H, step 0, the handle's seed, call counter and row
// offset.  per_row != 0: the DB + RT flavour with row_mult[j] == beta for every row (launch_act_db_pt), which also leaves its
// energy partials in part_dev [ceil(H/16)][J] where that is not null; per_row == 0: the existing DB pass at mult == bmult == beta,
// the pass of bm_rbm_rsm_ais.  The call counter does not advance: the two forms read the same stream
int bm_debug_rsm_up(bm_rbm *h, const float *V_dev, int32_t J, const float *lengths_dev, float beta, int32_t per_row, float *H_dev,
                    float *part_dev) {
    BM_TRY(check_rsm_pt(h, "bm_debug_rsm_up"));
    BM_CHECK(V_dev && lengths_dev && H_dev && J >= 1 && beta > 0.f, "bm_debug_rsm_up: bad arguments");
    BM_CHECK(per_row || !part_dev, "bm_debug_rsm_up: the energy partials are the per-row form's");
    ensure_wt(h);
    LayerPass p = rbm_pass(h, true, J, LayerIn{V_dev, h->V}, LayerOut{1, nullptr, H_dev, h->H, make_key(h, SITE_H, 0), h->row0}, beta);
    p.a.row_bmult = lengths_dev;
    if (!per_row) {
        issue(h, p);
        BM_HIP(hipGetLastError());
        return 0;
    }
    if (h->rp_probe.n < (size_t)J) BM_TRY(h->rp_probe.alloc(J));
    const std::vector<float> mult((size_t)J, beta);
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipMemcpy(h->rp_probe.p, mult.data(), (size_t)J * sizeof(float), hipMemcpyHostToDevice));
    ActArgs &a = p.a;
    a.mult = a.bmult = 1.0f;                           // (not read: the row's beta takes their place)
    p.row_tempered(h->rp_probe.p);
    if (part_dev) p.energy_rows(part_dev, J);
    if (h->use_wt && h->wt_valid) { a.P1 = make_operand(h->Wt.p, h->Wt.ld, h->H); a.p_xm = 1; }
    launch_act_db_pt(a, h->stream);
    BM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
