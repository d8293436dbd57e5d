"""Replicated softmax visible units without a GPU: the CPU twin (tests/rsm_twin.py) against a float64 softmax
and against the model's exact distribution over count vectors, its prefix order, its draws by position, learning on the twin, and
what the Python class refuses.  tests/test_rsm_gpu.py holds the engine to the same twin bit for bit."""
import numpy as np
import pytest

from tests import multinomial_probes as P
from tests import rsm_twin as T

f32 = np.float32
WIDTHS = (2, 5, 16, 17, 256, 257, 1000)
SEED = 20251


def undrawable(e):
    """the units no draw can land on under the twin's prefix order: c[i] == c[i-1]"""
    c = T.prefix_order(e)
    m = np.zeros(len(c), dtype=bool)
    m[1:] = c[1:] == c[:-1]
    return m


# ---- 1. the twin against a float64 softmax
@pytest.mark.parametrize('V', WIDTHS)
def test_twin_against_float64_softmax(V):
    """Every logit family of tests/multinomial_probes.logit_sets at width V, 8 rows of lengths 1, 2, 37 and 100: the means inside
    the module's derived bound ((V - 1) + d) 2^-24 + 1e-6 for d <= 80 and 1.81e-35 beyond the clamp (the hierarchy's sums carry at
    most 16 + 16 + V / 256 roundings, fewer than the V - 1 of the sequential sum the bound was derived for); every state row a
    non-negative integer vector that sums to exactly D; a unit with c[i] == c[i-1] never drawn; the hot unit of family d takes
    every draw."""
    D = np.array([1, 2, 37, 100, 100, 37, 2, 1], f32)
    for name, l in P.logit_sets(V):
        L = np.tile(l, (len(D), 1)).astype(f32)
        m, s = T.softmax_counts(L, D, 1, SEED, 3, 0, 0, 100)
        what = 'twin %s V=%d' % (name, V)
        for j in range(len(D)):
            P.check_means(l, m[j], int(D[j]), P.F32, what)
        assert np.all(s >= 0) and np.all(s == np.round(s)) and np.all(s.sum(axis=1) == D), what
        assert np.all(s[:, undrawable(T.softmax_e(l))] == 0), what + ': a unit with c[i] == c[i-1] was drawn'
        hot = P.hot_unit(name, V)
        if hot is not None:
            assert np.all(s[:, hot] == D), what + ': a draw left the hot unit'
        m0, s0 = T.softmax_counts(L, D, 0, SEED, 3, 0, 0, 100)
        P.assert_bits(m0, m, what)
        P.assert_bits(s0, m, what + ' (no draw: states = means)')


def test_prefix_order_is_monotone():
    """c is non-decreasing for every probe family at every level boundary of the prefix order, +- 1 (runs of 16, blocks of 256,
    the 4096-unit edge between the kernel's two instantiations, the last block and the limit), and over random positive rows"""
    widths = sorted(set(T.level_boundaries()) | set(WIDTHS))
    assert {15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 16383, 16384} <= set(widths)
    for V in widths:
        for name, l in P.logit_sets(V):
            e = T.softmax_e(l)
            c = T.prefix_order(e)
            assert c.dtype == f32 and len(c) == V
            assert np.all(np.diff(c) >= 0), (name, V)
            assert np.all(c[e > 0] > 0) and c[0] == e[0], (name, V)
    rng = np.random.RandomState(1)
    for V in (300, 4097, 16384):
        c = T.prefix_order(rng.uniform(0, 1, V).astype(f32) ** 8)
        assert np.all(np.diff(c) >= 0)


def test_prefix_order_is_a_function_of_the_width_alone():
    """the order regroups nothing when the row is cut differently: c of a row equals c of the same row inside a taller batch, and
    the hierarchy (not a sequential sum) is what is computed - at V = 1000 the two differ in some bits"""
    l = dict(P.logit_sets(1000))['a_normal']
    e = T.softmax_e(l)
    c = T.prefix_order(e)
    assert c[15] == np.cumsum(e[:16], dtype=f32)[-1]                       # level 0 is the sequential sum of the first run
    assert c[255] == T.prefix_order(e[:256])[-1]
    assert c[256] == f32(c[255] + e[256])                                   # the carry of a block is the last c before it
    assert np.any(c != np.cumsum(e, dtype=f32))


# ---- 2. the model's exact distribution
def test_log_z_two_ways():
    p = T.small_model()
    X, logc = T.count_vectors(4, 3)
    assert len(X) == 20 and np.all(X.sum(axis=1) == 3) and abs(np.exp(logc).sum() - 4 ** 3) < 1e-9
    a, b = T.log_z_visible(p, 3), T.log_z_hidden(p, 3)
    print('log Z_3 over the 20 count vectors %.12f, over the 4 hidden states %.12f' % (a, b))
    assert abs(a - b) <= 1e-9


CHAIN = dict(rows=256, steps=100, burn=20, every=5, seed=4242, h_seed=6)


def chain_cells(run):
    """the cell counts of a block-Gibbs run over the 20 count vectors of the small model: `run(H0, D, steps, keep)`"""
    c = CHAIN
    X, pv = T.exact_pv(T.small_model(), 3)
    counts = np.zeros(len(X))

    def keep(t, v):
        if t >= c['burn'] and t % c['every'] == 0:
            assert np.all(v.sum(axis=1) == 3)
            np.add.at(counts, T.cell_index(X, v), 1)
    H0 = (np.random.RandomState(c['h_seed']).uniform(size=(c['rows'], 2)) < 0.5).astype(f32)
    run(H0, np.full(c['rows'], 3, f32), c['steps'], keep)
    assert counts.sum() == c['rows'] * len(range(c['burn'], c['steps'], c['every']))
    return counts, pv


def test_gibbs_chain_samples_the_model():
    """V = 4, H = 2, D = 3: 256 twin chains, 100 block-Gibbs steps, every 5th state from step 20 on - 4096 states over the 20 count
    vectors - against the exact p(v) = (3! / prod v_i!) exp(-F(v)) / Z_3: z = (chi2 - 19) / sqrt(38), |z| <= 4 (the project's cap).
    Seeds fixed here before any GPU run."""
    twin = T.RsmRBM(T.small_model(), 3, seed=CHAIN['seed'], sample_v_states=True, sample_h_states=True)
    counts, pv = chain_cells(lambda H0, D, steps, keep: twin.gibbs(H0, D, steps, keep=keep))
    z, exmin = T.chi_square_z(counts, pv)
    print('chi-square of %d states over 20 cells: z = %+.2f, smallest expected cell %.1f' % (counts.sum(), z, exmin))
    assert exmin >= 5.0
    assert abs(z) <= P.Z_CAP


def test_counts_given_h():
    """the counts given one fixed h over 4096 rows: every unit's mean within 5 sqrt(D p (1 - p) / 4096) of D p"""
    rng = np.random.RandomState(3)
    V, H, D, R = 7, 3, 20, 4096
    W, vb = rng.randn(V, H).astype(f32), (0.5 * rng.randn(V)).astype(f32)
    h = np.tile(np.array([[1, 0, 1]], f32), (R, 1))
    _, s = T.visible_pass(h, W, vb, np.full(R, D, f32), 1, SEED, 3, 0, 0, 64)
    l = vb.astype(np.float64) + W.astype(np.float64).dot([1, 0, 1])
    pr = np.exp(l - l.max()); pr /= pr.sum()
    err = np.abs(s.mean(axis=0) - D * pr)
    tol = 5 * np.sqrt(D * pr * (1 - pr) / R)
    print('largest deviation / tolerance: %.3f' % float((err / tol).max()))
    assert np.all(s.sum(axis=1) == D) and np.all(err <= tol)


# ---- 3. draws by position
def test_draws_by_position():
    """a row's means and counts depend on its global row and its length alone: a slice at its row offset repeats the bits"""
    rng = np.random.RandomState(9)
    V, H, ML = 37, 6, 50
    W, vb = (0.5 * rng.randn(V, H)).astype(f32), (0.5 * rng.randn(V)).astype(f32)
    h = (rng.uniform(size=(12, H)) < 0.5).astype(f32)
    D = rng.randint(1, ML + 1, 12).astype(f32)
    m, s = T.visible_pass(h, W, vb, D, 1, SEED, 3, 3, 0, ML)
    m7, s7 = T.visible_pass(h[5:9], W, vb, D[5:9], 1, SEED, 3, 3, 5, ML)
    P.assert_bits(m7, m[5:9], 'means')
    P.assert_bits(s7, s[5:9], 'states')
    assert np.all(s.sum(axis=1) == D)


def test_db_pre_activation_and_weighted_sums():
    """the DB pre-activation is z + fl(D hb): at W = 0 the means are sigmoid(fl(D hb)) exactly, whatever the row; the weighted
    bias sums run over the rows in ascending order"""
    from oracle import oracle as orc
    hb = np.array([0.3, -0.2, 0.017], f32)
    X = np.array([[1, 0, 0, 0], [2, 3, 0, 1], [0, 0, 40, 0]], f32)
    m, _ = T.db_up(X, np.zeros((4, 3), f32), hb, T.lengths(X), 0, 1, 2, 0)
    for j, D in enumerate((1, 6, 40)):
        want = [orc.lib().orc_sigmoid(float(f32(D) * b)) for b in hb]
        assert np.array_equal(m[j], np.array(want, f32))
    h0, hk = np.array([[0.5, 0.25], [1, 0], [0.125, 1]], f32), np.array([[0.25, 0.5], [0, 1], [1, 0.5]], f32)
    s = T.weighted_bias_sums([1, 6, 40], h0, hk)
    assert np.array_equal(s, np.array([0.25 + 6 - 35, -0.25 - 6 + 20], f32))


# ---- 4. learning on the twin
PLANTED = dict(V=24, H=4, n_train=120, n_val=60, batch=20, lr=0.02, mom=0.5, epochs=12, seed=31, max_length=30)


def planted_twin():
    c = PLANTED
    X, _ = T.planted_corpus(c['n_train'], 1, c['V'])
    p0 = dict(W=np.zeros((c['V'], c['H']), f32), vb=np.zeros(c['V'], f32), hb=np.zeros(c['H'], f32))
    twin = T.RsmRBM(p0, c['max_length'], seed=c['seed'], l2=1e-4)
    for _ in range(c['epochs']):
        for s in range(0, len(X), c['batch']):
            twin.train_step(X[s:s + c['batch']], c['lr'], c['mom'], 1)
    return twin, p0


def test_twin_learns_planted_topics():
    """a planted two-topic corpus (24 words, 10 - 30 tokens per document, 90 % of a document's mass on its topic's half of the
    vocabulary): after CD-1 training the mean free energy of held-out documents of the planted kind lies below that of the same
    documents with their counts shuffled over the vocabulary; before training it does not (at W = 0, vb = 0, hb = 0 the free
    energy of every document is -H log 2)."""
    c = PLANTED
    twin, p0 = planted_twin()
    Xv, _ = T.planted_corpus(c['n_val'], 2, c['V'])
    Xs = T.shuffled_vocabulary(Xv, 9)
    assert np.array_equal(Xs.sum(axis=1), Xv.sum(axis=1))
    before = float(T.free_energy64(p0, Xv).mean()), float(T.free_energy64(p0, Xs).mean())
    after = float(T.free_energy64(twin.p, Xv).mean()), float(T.free_energy64(twin.p, Xs).mean())
    print('mean free energy before: held-out %.4f, shuffled %.4f; after: held-out %.3f, shuffled %.3f' % (before + after))
    assert not before[0] < before[1]
    assert after[0] < after[1]


# ---- 5. the Python class without an engine
def _no_engine(monkeypatch):
    """any attempt to build an engine fails the test"""
    from boltzmann_machines_amd import rbm as rbm_mod

    def boom(*a, **k):
        raise AssertionError('an engine call was made')
    monkeypatch.setattr(rbm_mod, 'RbmEngine', boom)
    monkeypatch.setattr(rbm_mod, 'RbmEngine64', boom)


def _refused(f, method):
    with pytest.raises(ValueError) as e:
        f()
    msg = str(e.value)
    assert 'replicated softmax visible units' in msg and method in msg, msg


def test_class_exists(tmp_path):
    import boltzmann_machines_amd as bm
    m = bm.ReplicatedSoftmaxRBM(30, 4, 50)
    assert m.n_visible == 30 and m.n_hidden == 4 and m.max_length == 50
    assert m._model_dirpath.endswith('rs_rbm_model/') and m._engine is None
    assert m.get_params()['max_length'] == 50
    for bad in (dict(max_length=0), dict(max_length=1 << 24), dict(n_visible=1), dict(n_visible=16385)):
        with pytest.raises(ValueError):
            bm.ReplicatedSoftmaxRBM(**dict(dict(n_visible=30, n_hidden=4, max_length=50), **bad))


def test_encode_and_lengths():
    import boltzmann_machines_amd as bm
    m = bm.ReplicatedSoftmaxRBM(6, 3, 10)
    docs = [[0, 0, 5], [3], [1, 2, 1, 2, 1, 4, 4, 4, 4, 0]]
    X = m.encode(docs)
    assert X.dtype == f32 and X.shape == (3, 6)
    assert np.array_equal(X, [[2, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0], [1, 3, 2, 0, 4, 0]])
    assert np.array_equal(m.lengths(X), [len(d) for d in docs])
    assert np.array_equal(T.lengths(X), [len(d) for d in docs])
    for bad in ([[6]], [[-1]]):
        with pytest.raises(ValueError):
            m.encode(bad)


def test_fit_validates_rows(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    m = bm.ReplicatedSoftmaxRBM(4, 3, 5, batch_size=2, model_path=str(tmp_path) + '/m/')
    good = np.array([[1, 0, 2, 0], [0, 5, 0, 0]], f32)
    for bad, word in ((np.array([[1, 0.5, 0, 0]]), 'integer'), (np.array([[2, -1, 0, 0]]), 'negative'),
                      (np.zeros((1, 4)), 'empty'), (np.array([[3, 3, 0, 0]]), 'max_length')):
        for args in ((np.vstack([good, bad]),), (good, np.vstack([good, bad]))):
            with pytest.raises(ValueError) as e:
                m.fit(*args)
            assert word in str(e.value) and 'row 2' in str(e.value) and 'replicated softmax' in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        m.lengths(np.zeros((2, 3)))
    assert m._engine is None


def test_python_refusals(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    mk = lambda **kw: bm.ReplicatedSoftmaxRBM(6, 4, 9, batch_size=4, model_path=str(tmp_path) + '/m/', **kw)
    _refused(lambda: mk(metrics_config=dict(pll=True)), '__init__')
    _refused(lambda: mk(metrics_config=dict(feg=True)), '__init__')
    _refused(lambda: mk(dropout=0.5), '__init__')
    _refused(lambda: mk(sparsity_cost=0.1), '__init__')
    _refused(lambda: mk(dbm_first=True), '__init__')
    _refused(lambda: mk(dbm_last=True), '__init__')
    _refused(lambda: mk(dtype='float64'), '__init__')
    m = mk()
    X = m.encode([[0, 1, 1], [5]])
    m.set_params(sparsity_cost=0.5)
    _refused(lambda: m.fit(X), 'fit')                      # (set_params may change a keyword: checked again before the engine is built)
    m.set_params(sparsity_cost=0.)
    _refused(lambda: m.set_negative_phase('tempered'), 'set_negative_phase')
    assert m.set_negative_phase('cd') is m
    _refused(lambda: m.set_centering(), 'set_centering')
    _refused(lambda: m.set_classes(3), 'set_classes')
    _refused(lambda: m.sample_v_given(X, np.ones(6)), 'sample_v_given')
    _refused(lambda: m.log_Z(), 'log_Z')
    _refused(lambda: m.log_proba(X, 0.0), 'log_proba')
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    _refused(lambda: m.fit(X), 'fit')
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    assert m._engine is None


def test_python_refusals_as_a_layer(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    rs = bm.ReplicatedSoftmaxRBM(6, 4, 9, batch_size=4, model_path=str(tmp_path) + '/m/')
    _refused(lambda: bm.DBM(rbms=[rs], model_path=str(tmp_path) + '/d/'), 'DBM')
    _refused(lambda: bm.StackClassifier.from_rbms([rs], n_classes=3, model_path=str(tmp_path) + '/s/'), 'from_rbms')
    assert rs._engine is None
