// launch_route_check.hip - is act_route (csrc/bm_launch.h: the flavour table, the feature mask, the rule of exclusivity) the
// routing that launch_act had when every flavour carried a hand-written precondition?  A stand-alone host program: no HIP
// runtime call, no launch, no abort.  Built and run by tests/test_launch_route.py.
//
// The oracle below is FROZEN: the ladder of launch_act, the seven preconditions, the seven strips to the plain pass and the memo's
// flags word as they stood before the table existed, copied verbatim.  It is not to follow later changes of bm_launch.h - a new
// flavour adds a start point and, if older flavours are to refuse its selector, an oracle line that says so.
//
// From each of eight start points (a canonical admitted pass of every flavour, and a plain pass) every single field and every
// pair of fields of FIELDS takes each of its values; each time the flavour, the verdict and - for an admitted pass - the stripped
// ActArgs (bytewise) and the flags word must be the oracle's.
#define BM_KERNELS_ONLY
#include <cstdio>
#include <cstring>
#include <vector>
#include "bm_common.h"
#include "bm_kernels.h"

using namespace bm;

// ---------------------------------------------------------------- the frozen oracle
struct Legacy { unsigned fl; bool refused; ActArgs plain; long long flags; };

static long long legacy_flags(const ActArgs &a) {
    const long long flags = (long long)((a.sample ? 1 : 0) | (a.kind << 1) | (a.prev ? 16 : 0) | (a.rowacc ? 32 : 0) |
                                        (a.acc_init ? 64 : 0) | (a.p_xm ? 128 : 0) | (a.rowdot_out ? 256 : 0) |
                                        (a.dot_mat ? 512 : 0) | (a.negmeans ? 1024 : 0));
    return flags;
}
// CL and RT: the flags of the pass itself, the strip of tuned_act's tuning run
static void legacy_tuned_act(const ActArgs &a, Legacy &r) {
    r.flags = legacy_flags(a);
    ActArgs plain = a;
    if (!a.clamp_mask && !a.row_mult) { r.plain = plain; return; }
    plain.clamp_mask = plain.clamp_val = nullptr; plain.ld_clamp = 0;
    if (a.row_mult) { plain.row_mult = nullptr; plain.rowen_out = nullptr; plain.sel_out = nullptr; plain.mult = plain.bmult = 1.0f; }
    r.plain = plain;
}
static void legacy_cl(const ActArgs &a, Legacy &r) {
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init) {
        r.refused = true;
        return;
    }
    legacy_tuned_act(a, r);
}
static void legacy_rt(const ActArgs &a, Legacy &r) {
    if ((a.K2 > 0 && a.p_xm) || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.b3.K1 > 0 || a.lit ||
        a.kind != 0) {
        r.refused = true;
        return;
    }
    legacy_tuned_act(a, r);
}
static void legacy_cr(const ActArgs &a, Legacy &r) {
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.row_mult || a.b3.K1 > 0 ||
        a.lit || a.kind != 3 || a.mult != 1.0f || a.bmult != 1.0f || a.sample || a.rowacc || a.rowdot_out) {
        r.refused = true;
        return;
    }
    ActArgs plain = a;
    plain.cr_part = nullptr; plain.cr_U = nullptr; plain.cr_ldu = plain.cr_C = plain.cr_nslots = 0; plain.ld_part = 0;
    legacy_tuned_act(plain, r);
}
static void legacy_cb(const ActArgs &a, Legacy &r) {
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.row_mult || a.cr_part ||
        a.b3.K1 > 0 || a.lit || a.kind != 0 || a.mult != 1.0f || a.bmult != 1.0f || a.rowacc || a.rowdot_out || !a.cb_U || !a.cb_bad) {
        r.refused = true;
        return;
    }
    ActArgs plain = a;
    plain.cb_y = nullptr; plain.cb_U = nullptr; plain.cb_ldu = plain.cb_C = 0; plain.cb_bad = nullptr;
    legacy_tuned_act(plain, r);
}
static void legacy_bp(const ActArgs &a, Legacy &r) {
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.row_mult || a.cr_part ||
        a.cb_y || a.b3.K1 > 0 || a.lit || a.kind != 2 || a.mult != 1.0f || a.sample || a.rowacc || a.rowdot_out || a.negmeans ||
        a.states || !a.means || !a.p_xm || !a.bias) {
        r.refused = true;
        return;
    }
    ActArgs plain = a;
    plain.bp = 0; plain.bp_act = nullptr; plain.bp_ld = 0;
    legacy_tuned_act(plain, r);
}
static void legacy_nr(const ActArgs &a, Legacy &r) {
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.row_mult || a.cr_part ||
        a.cb_y || a.bp || a.b3.K1 > 0 || a.lit || a.kind != 3 || a.mult != 1.0f || a.bmult != 1.0f || a.rowacc || a.rowdot_out) {
        r.refused = true;
        return;
    }
    ActArgs plain = a;
    plain.nrelu = 0; plain.kind = 0;        // (the Bernoulli prop-up of the shape: the same contraction, a draw per output)
    legacy_tuned_act(plain, r);
}
static void legacy_sm(const ActArgs &a, Legacy &r) {
    const bool width_ok = a.sm_k == 2 || a.sm_k == 4 || a.sm_k == 8 || a.sm_k == 16;
    if (a.K2 > 0 || a.fe_flip || a.prev || a.maxdiff || a.skip || a.chk_ctl || a.acc_init || a.clamp_mask || a.row_mult || a.cr_part ||
        a.cb_y || a.bp || a.nrelu || a.b3.K1 > 0 || a.lit || a.kind != 3 || a.mult != 1.0f || a.bmult != 1.0f || a.rowacc || a.rowdot_out ||
        a.negmeans || !a.p_xm || !width_ok || (a.I & 3) != 0 || a.I % a.sm_k != 0) {
        r.refused = true;
        return;
    }
    ActArgs plain = a;
    plain.sm_k = 0; plain.kind = 0;         // (the Bernoulli prop-down of the shape: the same contraction, a draw per output)
    legacy_tuned_act(plain, r);
}
static Legacy legacy_route(const ActArgs &a) {
    Legacy r;
    memset(&r, 0, sizeof(r));
    if (a.sm_k) { r.fl = FL_SM; legacy_sm(a, r); return r; }
    if (a.nrelu) { r.fl = FL_NR; legacy_nr(a, r); return r; }
    if (a.bp) { r.fl = FL_BP; legacy_bp(a, r); return r; }
    if (a.cb_y) { r.fl = FL_CB; legacy_cb(a, r); return r; }
    if (a.cr_part) { r.fl = FL_CR; legacy_cr(a, r); return r; }
    if (a.row_mult) { r.fl = FL_RT; legacy_rt(a, r); return r; }
    if (a.clamp_mask) { r.fl = FL_CL; legacy_cl(a, r); return r; }
    legacy_tuned_act(a, r);     // (what launch_act_f32 hands to the memo: the pass itself)
    return r;
}

// ---------------------------------------------------------------- the cases
static float dummy[64];
struct Field { const char *name; int nvals; void (*set)(ActArgs &, int); };
#define PTR(f) {#f, 2, [](ActArgs &a, int v) { a.f = v ? reinterpret_cast<decltype(a.f)>(dummy) : nullptr; }}
static const Field FIELDS[] = {
    {"K2", 2, [](ActArgs &a, int v) { a.K2 = v ? 16 : 0; }},
    {"p_xm", 2, [](ActArgs &a, int v) { a.p_xm = v; }},
    {"kind", 4, [](ActArgs &a, int v) { a.kind = v; }},
    {"mult", 2, [](ActArgs &a, int v) { a.mult = v ? 0.5f : 1.0f; }},
    {"bmult", 2, [](ActArgs &a, int v) { a.bmult = v ? 0.5f : 1.0f; }},
    {"sample", 2, [](ActArgs &a, int v) { a.sample = v; }},
    {"lit", 2, [](ActArgs &a, int v) { a.lit = v; }},
    {"bp", 2, [](ActArgs &a, int v) { a.bp = v; }},
    {"nrelu", 2, [](ActArgs &a, int v) { a.nrelu = v; }},
    {"sm_k", 6, [](ActArgs &a, int v) { static const int k[6] = {0, 2, 3, 4, 8, 16}; a.sm_k = k[v]; }},
    {"I", 3, [](ActArgs &a, int v) { static const int n[3] = {16, 18, 24}; a.I = n[v]; }},
    {"b3.K1", 2, [](ActArgs &a, int v) { a.b3.K1 = v ? 64 : 0; }},
    PTR(fe_flip), PTR(prev), PTR(maxdiff), PTR(skip), PTR(chk_ctl), PTR(acc_init), PTR(clamp_mask), PTR(row_mult), PTR(cr_part),
    PTR(cb_y), PTR(cb_U), PTR(cb_bad), PTR(rowacc), PTR(rowdot_out), PTR(negmeans), PTR(means), PTR(states), PTR(bias),
};
constexpr int NF = sizeof(FIELDS) / sizeof(FIELDS[0]);

static long cases = 0, admitted = 0, bad = 0;
static void check(const char *start, const ActArgs &a, const char *f1, int v1, const char *f2, int v2) {
    const Legacy want = legacy_route(a);
    const ActRoute got = act_route(a);
    ++cases;
    const char *why = nullptr;
    if (got.fl != want.fl) why = "flavour";
    else if ((got.refusal != nullptr) != want.refused) why = "verdict";
    else if (!want.refused) {
        ++admitted;
        ActArgs plain = a;
        ActFlavours::first([&](auto fl) { return got.fl == fl.value && (ActFlavour<decltype(fl)::value>::strip(plain), true); });
        if (memcmp(&plain, &want.plain, sizeof(ActArgs)) != 0) why = "stripped args";
        else if (act_memo_flags(plain) != want.flags) why = "flags word";
    }
    if (why && ++bad <= 20)
        printf("MISMATCH (%s) from %s with %s=#%d %s=#%d: oracle flavour %u %s, table flavour %u %s\n", why, start, f1, v1, f2 ? f2 : "-", v2,
               want.fl, want.refused ? "refused" : "admitted", got.fl, got.refusal ? "refused" : "admitted");
}

int main() {
    ActArgs base;
    memset(&base, 0, sizeof(base));
    base.I = 16; base.J = 8; base.K1 = 32; base.ldo = 16;
    base.mult = base.bmult = 1.0f;
    base.bias = dummy; base.means = dummy;
    struct Start { const char *name; unsigned fl; ActArgs a; };
    std::vector<Start> starts;
    const auto add = [&](const char *name, unsigned fl, auto &&fill) { ActArgs a = base; fill(a); starts.push_back({name, fl, a}); };
    int *const idummy = reinterpret_cast<int *>(dummy);
    add("plain", 0, [&](ActArgs &a) { a.states = dummy; a.sample = 1; });
    add("CL", FL_CL, [&](ActArgs &a) { a.states = dummy; a.sample = 1; a.clamp_mask = a.clamp_val = dummy; a.ld_clamp = 16; });
    add("RT", FL_RT, [&](ActArgs &a) { a.states = dummy; a.sample = 1; a.row_mult = dummy; a.rowen_out = dummy; a.ld_part = 8; });
    add("CR", FL_CR, [&](ActArgs &a) { a.kind = 3; a.cr_part = dummy; a.cr_U = dummy; a.cr_ldu = 16; a.cr_C = 3; a.cr_nslots = 1; a.ld_part = 8; });
    add("CB", FL_CB, [&](ActArgs &a) { a.states = dummy; a.sample = 1; a.cb_y = idummy; a.cb_U = dummy; a.cb_ldu = 16; a.cb_C = 3; a.cb_bad = idummy; });
    add("BP", FL_BP, [&](ActArgs &a) { a.kind = 2; a.p_xm = 1; a.bp = 1; a.bp_act = dummy; a.bp_ld = 16; });
    add("NR", FL_NR, [&](ActArgs &a) { a.kind = 3; a.states = dummy; a.sample = 1; a.nrelu = 1; });
    add("SM", FL_SM, [&](ActArgs &a) { a.kind = 3; a.p_xm = 1; a.states = dummy; a.sample = 1; a.sm_k = 4; });
    for (const Start &s : starts) {
        const ActRoute r = act_route(s.a);
        if (r.fl != s.fl || r.refusal) { printf("start point %s is not an admitted pass of its flavour\n", s.name); ++bad; }
        check(s.name, s.a, "-", 0, nullptr, 0);
        for (int f = 0; f < NF; ++f)
            for (int v = 0; v < FIELDS[f].nvals; ++v) {
                ActArgs a1 = s.a;
                FIELDS[f].set(a1, v);
                check(s.name, a1, FIELDS[f].name, v, nullptr, 0);
                for (int g = f + 1; g < NF; ++g)
                    for (int w = 0; w < FIELDS[g].nvals; ++w) {
                        ActArgs a2 = a1;
                        FIELDS[g].set(a2, w);
                        check(s.name, a2, FIELDS[f].name, v, FIELDS[g].name, w);
                    }
            }
    }
    printf("launch_route_check: %ld cases from %zu start points, %ld admitted, %ld mismatches\n", cases, starts.size(), admitted, bad);
    return bad ? 1 : 0;
}
