"""The cases shared by tests/test_mf_control.py (CPU) and tests/test_mf_control_gpu.py: DBMs whose mean-field trip count
(dbm.py:429-478) is decided by ONE (layer, row, unit), the planted element, and a float64 restatement of the loop that keeps every
sweep's residual matrix, so that the trip count can be recomputed with one tile's residuals ignored.  Nothing here touches the
engine.

The construction:
  * every weight is N(0, S^2), S small: the unplanted model ends by the tolerance in 2-3 sweeps;
  * the planted unit u of layer p is tied to M partner units of a neighbouring layer q (p + 1, for the top layer p - 1) by weights
    wi = 4 sqrt(RHO / M), with biases that centre all of them at 0.5: the sweep-to-sweep contraction of that star is RHO, the
    partners' residual is sqrt(RHO / M) of the planted unit's, so without the planted tile the loop would end several sweeps early;
  * u carries an extra bias -GATE that row r alone cancels through the layer below: for p = 0 one visible j* with W[j*, u] = GATE and
    X[r, j*] = x (zero in every other row), for p > 0 a chain of saturated indicator units, one per layer below p, switched on by
    X[r, j*] = 1; the chain's weights fall by 16 per layer so that no indicator can be held up from above.  Every other row has u
    saturated near 0 and converges at once;
  * x, a grey level (p = 0), or an offset on u's bias (p > 0) moves the fixed point away from the start of the iteration and thereby
    sets the trip count; the persistent mu starts at 0.5."""
import functools

import numpy as np

from oracle import oracle as orc

SEED = 535353
S = 0.004              # scale of the background weights
GATE = 8.0             # the extra bias of the planted unit (and the weight that cancels it)
RHO = 0.78             # contraction of the planted star per sweep
M_MAX = 24             # partners of the planted unit
IND = 3                # the indicator unit of every layer below p; the partners are units 4 .. 4 + M - 1
MF_TOL = 1e-4
MAX_MF = 40
MARGIN = 0.02          # no sweep's residual within this, relative, of MF_TOL (float32 round-off moves a residual by ~1e-7,
                       # 1e-3 of the tolerance: the cases keep twenty times that, so that the float32 oracle cannot disagree)
GAP = 3                # ignoring the planted tile ends the loop at least this many sweeps early
NARROW, WIDE = (32, 32), (32, 64)      # (units, rows) per workgroup of the two mean-field kernels

TWO = dict(V=45, n=(75, 41), N=70)
FOUR = dict(V=45, n=(40, 70, 36, 33), N=70)
OVER = dict(V=24, n=(1000, 24), N=1056)       # 32 x 33 = 1056 > 1024 narrow workgroups in the h1 pass: not self-controlled


def sfx(i):
    return '' if i == 0 else '_%d' % i


def names(L, bases=('mu',)):
    return [b + sfx(i) for b in bases for i in range(L)]


def placements(n_units, N):
    """(unit, row) in the first tile | the last, ragged unit tile | the last, ragged row tile (of both kernels) | both"""
    ul, rl = 32 * ((n_units - 1) // 32), 64 * ((N - 1) // 64)
    assert n_units % 32 and N % 64 and N % 32 and rl == 32 * ((N - 1) // 32)
    return [(7, 5), (n_units - 1, 31), (31, rl + 1), (min(ul + 2, n_units - 1), N - 1)]


def tile_of(unit, row, tile):
    return unit // tile[0], row // tile[1]


# (shape, planted layer, unit, row): every layer of both shapes at the four placements, + a row in the second half of a wide tile
def _list():
    out = []
    for shape in (TWO, FOUR):
        for p, n_units in enumerate(shape['n']):
            for u, r in placements(n_units, shape['N']):
                out.append((shape, p, u, r))
    out.append((TWO, 0, 40, 45))
    return out


def case_id(key):
    shape, p, u, r = key
    return '%dx%s-N%d-layer%d-unit%d-row%d' % (shape['V'], 'x'.join(map(str, shape['n'])), shape['N'], p, u, r)


CASES = _list()
OVER_CASES = [(OVER, 0, 999, 1055), (OVER, 0, 2, 3)]
# the tuning knob, tried in this order until the float64 run meets the conditions: 1 - x for p = 0, the bias offset for p > 0
KNOBS = (0.06, 0.05, 0.07, 0.04, 0.08, 0.03, 0.1, 0.02)


def _normal(site, shape):
    return (orc.normal(SEED, site, 0, int(np.prod(shape))) * np.float32(S)).reshape(shape).astype(np.float32)


def model(shape, p, u, r, knob, site=0):
    """(params, X): float32 W*, hb* of the planted model and the [N, V] input whose row r opens the gate"""
    V, n, N = shape['V'], shape['n'], shape['N']
    L = len(n)
    dims = (V,) + tuple(n)
    P = {}
    for i in range(L):
        P['W' + sfx(i)] = _normal(10 + i, (dims[i], dims[i + 1]))
        P['hb' + sfx(i)] = _normal(20 + i, (dims[i + 1],))
    X = (orc.uniform(SEED, 30 + site, 0, N * V) < 0.3).astype(np.float32).reshape(N, V)
    q = p + 1 if p + 1 < L else p - 1
    m = min(M_MAX, n[q] - 4)
    wi = np.float32(4.0 * np.sqrt(RHO / m))
    partners = np.arange(4, 4 + m)
    if q > p:
        P['W' + sfx(q)][u, partners] = wi
    else:
        P['W' + sfx(p)][partners, u] = wi
    P['hb' + sfx(q)][partners] = -wi / 2
    jstar = V - 2
    X[:, jstar] = 0
    if p == 0:
        P['W'][jstar, u] = GATE
        P['hb'][u] = -m * wi / 2 - GATE
        X[r, jstar] = 1 - knob
    else:
        # links X -> g_0 -> ... -> g_(p-1) -> u of weights s_0 > s_1 > ... > s_p = GATE, 16 apart; g_k's bias -(s_k + s_(k+1)) / 2
        s = [GATE + 16.0 * (p - k) for k in range(p + 1)]
        P['W'][jstar, IND] = s[0]
        for k in range(1, p):
            P['W' + sfx(k)][IND, IND] = s[k]
        P['W' + sfx(p)][IND, u] = s[p]
        for k in range(p):
            P['hb' + sfx(k)][IND] = -(s[k] + s[k + 1]) / 2
        P['hb' + sfx(p)][u] = -m * wi / 2 - GATE - knob
        X[r, jstar] = 1
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}, X


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def mf_trace(P, L, X, mu, sweeps):
    """dbm.py:429-478 in float64, every sweep run: res[t][i] = |mu - mu_new| of layer i as the loop condition sees it in front
    of sweep t (t = 0: the persistent mu against the approximate-inference init), states[t] = the mu after t sweeps, init"""
    X = np.asarray(X, np.float64)
    W = [np.asarray(P['W' + sfx(i)], np.float64) for i in range(L)]
    hb = [np.asarray(P['hb' + sfx(i)], np.float64) for i in range(L)]
    init, T = [], None
    for i in range(L):                                                          # :434-446
        T = 2. * X.dot(W[0]) if i == 0 else T.dot(W[i]) * (2. if i < L - 1 else 1.)
        T = sigmoid(T + hb[i])
        init.append(T)
    cur = [np.asarray(m, np.float64) for m in mu]
    res, states = [[np.abs(cur[i] - init[i]) for i in range(L)]], [cur]
    for _ in range(sweeps):                                                     # :385-416 with sample = False, update_v = False
        new = []
        for i in range(L):
            z = (X if i == 0 else new[i - 1]).dot(W[i]) + hb[i]
            if i + 1 < L:
                z = z + cur[i + 1].dot(W[i + 1].T)
            new.append(sigmoid(z))
        res.append([np.abs(new[i] - cur[i]) for i in range(L)])
        cur = new
        states.append(cur)
    return res, states, init


def resid_max(res_t, ignore=None):
    """max over layers, rows, units; ignore = (layer, unit tile, row tile, (units, rows) per tile) leaves that tile out"""
    m = 0.0
    for i, R in enumerate(res_t):
        if ignore is not None and ignore[0] == i:
            (tu, tr), (ti, tj) = ignore[1:3], ignore[3]
            R = R.copy()
            R[tr * tj:(tr + 1) * tj, tu * ti:(tu + 1) * ti] = 0
        m = max(m, float(R.max()))
    return m


def trip_count(res, tol, max_mf, ignore=None):
    """:449-452: the sweeps run while step < max_step and the residual > tol"""
    t = 0
    while t < max_mf and resid_max(res[t], ignore) > tol:
        t += 1
    return t


def margin(res, tol, T):
    """the least relative distance of an evaluated residual from tol"""
    return min(abs(resid_max(res[t]) - tol) / tol for t in range(T + 1))


def conditions(shape, p, u, r, knob, mu=None, site=0, max_mf=MAX_MF, P=None):
    """float64: dict(T, margin, T_narrow, T_wide, ...) of the planted model (P: these parameters, the input alone from the knob)"""
    P0, X = model(shape, p, u, r, knob, site)
    P = P if P is not None else P0
    L, N = len(shape['n']), shape['N']
    mu = mu if mu is not None else [np.full((N, k), 0.5) for k in shape['n']]
    res, states, _ = mf_trace(P, L, X, mu, max_mf)
    T = trip_count(res, MF_TOL, max_mf)
    out = dict(T=T, margin=margin(res, MF_TOL, T), P=P, X=X, mu=states[T], resid=[resid_max(x) for x in res[:T + 1]])
    for name, tile in (('T_narrow', NARROW), ('T_wide', WIDE)):
        out[name] = trip_count(res, MF_TOL, max_mf, (p,) + tile_of(u, r, tile) + (tile,))
    return out


def good(c, max_mf=MAX_MF):
    return c['T'] < max_mf and c['margin'] > MARGIN and max(c['T_narrow'], c['T_wide']) <= c['T'] - GAP


@functools.lru_cache(maxsize=None)
def _case(shape_key, p, u, r):
    shape = dict(V=shape_key[0], n=shape_key[1], N=shape_key[2])
    for knob in KNOBS:
        c = conditions(shape, p, u, r, knob)
        if good(c) and 5 <= c['T']:
            break
    else:
        raise AssertionError('no knob of %r gives a case at %r' % (KNOBS, (shape, p, u, r)))
    # the second call on the same handle: other data, the gate opened in another row, from the mu the first call leaves
    # (the same parameters: for p > 0 only the background input, `site`, can move a residual away from the tolerance)
    r2 = (r + 37) % shape['N']
    for site, knob2 in [(s, k) for s in (1, 2, 3, 4) for k in (KNOBS[::-1] if p == 0 else KNOBS[:1])]:
        c2 = conditions(shape, p, u, r2, knob2, mu=c['mu'], site=site, P=c['P'])
        if 5 <= c2['T'] < MAX_MF and c2['margin'] > MARGIN:
            break
    else:
        raise AssertionError('no input gives a second call at %r' % ((shape, p, u, r),))
    L = len(shape['n'])
    runs = {}
    for literal in (False, True):
        twin = oracle_twin(shape, c['P'], literal=literal)
        T1 = twin.mean_field(c['X'])
        mu1 = {k: twin.p[k].copy() for k in names(L)}
        T2 = twin.mean_field(c2['X'])
        mu2 = {k: twin.p[k].copy() for k in names(L)}
        runs[literal] = dict(T=(T1, T2), mu=(mu1, mu2))
    return dict(shape=shape, L=L, planted=(p, u, r), knob=knob, P=c['P'], X=(c['X'], c2['X']), ref=(c, c2), oracle=runs)


def case(key):
    """dict(shape, L, planted, P, X = (first call, second call), ref = the float64 conditions of both calls,
    oracle[literal] = dict(T = (T1, T2), mu = (after call 1, after call 2))).  Computed once, shared, never modified."""
    shape, p, u, r = key
    return _case((shape['V'], tuple(shape['n']), shape['N']), p, u, r)


def oracle_twin(shape, P, literal=False, max_mf=MAX_MF, **kw):
    """the float32 oracle of a handle with these parameters, its persistent mu at 0.5"""
    n = list(shape['n'])
    twin = orc.OracleDBM(shape['V'], n, n_particles=shape['N'], batch_size=shape['N'], max_mf_updates=max_mf, mf_tol=MF_TOL, **kw)
    for k, v in P.items():
        twin.p[k][...] = v
    for k in names(len(n)):
        twin.p[k][...] = 0.5
    twin.set_sigmoid_literal(literal)
    return twin


# ---- the driver's boundaries: one handle of the two-layer shape, planted at layer 0 in the last tile both ways, 30 sweeps at most.
# A call is (x, T): the grey level X[r, j*] and the trip count it is meant to give from the state the calls before it leave;
# x = None: mu is first preset to the approximate-inference init of the call's input (x of the call before), so that the step-0
# residual is 0, the loop makes no sweep and the handle's prediction falls back to "unprimed".
DRIVER = dict(shape=TWO, planted=(0, 66, 69), max_mf=30)
DRIVER_TRAIN_AFTER = 5         # one train_step and one metrics fetch in front of the call of this index
DRIVER_LR, DRIVER_MOM, DRIVER_K, DRIVER_SEED, DRIVER_TRAIN_X = 1e-3, 0.5, 1, 7, 0.9
DRIVER_CALLS = [(0.9, 9), (0.944, 10), (0.956, 10), (0.966, 12), (0.3, 3), (0.65, 4), (None, 0), (0.91, 8), (None, 0), (0.934, 9),
                (0.3, 3), (None, 0), (0.95, 12), (0.3, 3), (None, 0), (0.956, 13)]
# on handles of their own, the first case of the list (its trip count is 14): the cap reached above the tolerance, no sweep, one
CAPS = (6, 0, 1)


def driver_input(x):
    p, u, r = DRIVER['planted']
    return model(DRIVER['shape'], p, u, r, 1.0 - x)[1]


def driver_params():
    p, u, r = DRIVER['planted']
    return model(DRIVER['shape'], p, u, r, 0.0)[0]


def driver_twin(max_mf=None):
    twin = oracle_twin(DRIVER['shape'], driver_params(), max_mf=DRIVER['max_mf'] if max_mf is None else max_mf)
    N, V = DRIVER['shape']['N'], DRIVER['shape']['V']
    twin.p['v'][...] = (orc.uniform(SEED, 40, 0, N * V) < 0.3).astype(np.float32).reshape(N, V)
    twin.set_seed(DRIVER_SEED)
    return twin


def init_of(twin, X):
    """what the init passes (:434-446) give for X under twin's parameters: the mu_new of a handle that makes no sweep"""
    L = twin.L
    t0 = oracle_twin(DRIVER['shape'], {k: twin.p[k] for k in names(L, ('W', 'hb'))}, max_mf=0)
    assert t0.mean_field(X) == 0
    return {k: t0.p['mu_new' + k[2:]].copy() for k in names(L)}


@functools.lru_cache(maxsize=None)
def driver_oracle():
    """the call sequence on the oracle: a list of dict(x, X, preset = the mu set in front of the call or None, T, mu = after the call,
    start = the mu the call started from, P = the parameters it ran with, aside = (n_mf of the train_step, n_mf of the metrics
    fetch) made in front of it or None)"""
    twin = driver_twin()
    L = twin.L
    out, X = [], None
    for idx, (x, _) in enumerate(DRIVER_CALLS):
        aside = None
        if idx == DRIVER_TRAIN_AFTER:
            Xt = driver_input(DRIVER_TRAIN_X)
            aside = (twin.train_step(Xt, DRIVER_LR, DRIVER_MOM, DRIVER_K)[0], twin.metrics(Xt, DRIVER_K)[0])
        preset = None
        if x is None:
            preset = init_of(twin, X)
            for k, v in preset.items():
                twin.p[k][...] = v
        else:
            X = driver_input(x)
        start = {k: twin.p[k].copy() for k in names(L)}
        P = {k: twin.p[k].copy() for k in names(L, ('W', 'hb'))}
        T = twin.mean_field(X)
        out.append(dict(x=x, X=X, preset=preset, T=T, mu={k: twin.p[k].copy() for k in names(L)}, start=start, P=P, aside=aside))
    return out


@functools.lru_cache(maxsize=None)
def capped(cap):
    """the first case under max_mf_updates = cap: dict(T, mu of the oracle, resid = the float64 residual the loop stopped in front of)"""
    c = case(CASES[0])
    twin = oracle_twin(c['shape'], c['P'], max_mf=cap)
    T = twin.mean_field(c['X'][0])
    mu0 = [np.full((c['shape']['N'], k), 0.5) for k in c['shape']['n']]
    res, _, _ = mf_trace(c['P'], c['L'], c['X'][0], mu0, cap)
    return dict(T=T, mu={k: twin.p[k].copy() for k in names(c['L'])}, resid=resid_max(res[cap]))
