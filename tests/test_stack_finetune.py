"""CPU: fine-tuning a stack below a class head - the NumPy restatement against finite differences and autograd,
the twin's association of the sigmoid derivative, the stale-weight order, the C ABI's new entries and every Python refusal."""
import os
import re

import numpy as np
import pytest

from tests import np_reference_stack as S
from tests import stack_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('bm_rbm_backprop_down', 'bm_rbm_delta_update', 'bm_rbm_class_stack_train_step', 'bm_rbm_class_stack_train_epoch',
           'bm_rbm_class_stack_log_proba', 'bm_rbm_stack_transform')


def rel_err(a, b):
    """max |a - b| over the entries, relative to max |b|"""
    return S.max_dev(a, b) / float(np.max(np.abs(b)))


# ---- the float64 restatement: loss and every gradient
def test_gradients_agree_with_central_differences():
    """S1, every parameter tensor: relative error <= 1e-6 with step 1e-5, in float64"""
    c = K.case('S1')
    p = S.cast(c['p0'], np.float64)
    X, y = c['X'][:c['B']], c['y'][:c['B']]
    lg, tg, _ = S.gradients(p, X, y, np.float64)
    h = 1e-5
    tensors = [(p['layers'][i], n, lg[i][n], '%s%d' % (n, i + 1)) for i in range(c['D']) for n in ('W', 'hb')]
    tensors += [(p['top'], n, tg[n], n) for n in ('W', 'hb', 'U', 'yb')]
    for owner, n, g, label in tensors:
        fd = np.zeros_like(owner[n])
        flat, out = owner[n].reshape(-1), fd.reshape(-1)
        for e in range(flat.size):
            keep = flat[e]
            flat[e] = keep + h
            up = S.mean_log_proba(p, X, y)
            flat[e] = keep - h
            down = S.mean_log_proba(p, X, y)
            flat[e] = keep
            out[e] = (up - down) / (2 * h)
        err = rel_err(g, fd)
        print('finite differences, %-4s: relative error %.3g' % (label, err))
        assert err <= 1e-6, (label, err)
    # vb of no layer enters the loss
    assert all(not g['vb'].any() for g in lg) and not tg['vb'].any()


def test_gradients_agree_with_autograd():
    """the same gradients against CPU autograd at 1e-10 (this leg is left out where torch does not import)"""
    c = K.case('S1')
    p = S.cast(c['p0'], np.float64)
    X, y = c['X'][:c['B']], c['y'][:c['B']]
    lg, tg, out2 = S.gradients(p, X, y, np.float64)
    assert abs(out2[0] - S.mean_log_proba(p, X, y)) <= 1e-12
    try:
        import torch
    except ImportError:
        return
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tl = [dict(W=leaf(l['W']), hb=leaf(l['hb'])) for l in p['layers']]
    tt = {n: leaf(p['top'][n]) for n in ('W', 'hb', 'U', 'yb')}
    a = torch.tensor(np.asarray(X, np.float64))
    for l in tl:
        a = torch.sigmoid(a @ l['W'] + l['hb'])
    z = a @ tt['W'] + tt['hb']
    s = tt['yb'][None, :] + torch.nn.functional.softplus(z[:, None, :] + tt['U'][None, :, :]).sum(dim=2)
    loss = torch.log_softmax(s, dim=1)[torch.arange(len(y)), torch.tensor(y.astype(np.int64))].mean()
    loss.backward()
    for i, l in enumerate(tl):
        for n in ('W', 'hb'):
            assert rel_err(lg[i][n], l[n].grad.numpy()) <= 1e-10, (i, n)
    for n in ('W', 'hb', 'U', 'yb'):
        assert rel_err(tg[n], tt[n].grad.numpy()) <= 1e-10, n


def test_twin_restates_the_association():
    """(z * a) * (1 - a), every step rounded to float32 once - and not z * (a * (1 - a))"""
    from boltzmann_machines_amd.utils import philox
    z = (philox.normal(K.SEED, 98, 0, 4096) * np.float32(3)).astype(np.float32)
    a = philox.uniform(K.SEED, 99, 0, 4096).astype(np.float32)
    got = S.sigmoid_derivative(z, a, np.float32)
    r32 = lambda x: np.asarray(x, np.float64).astype(np.float32)          # (products of two float32 are exact in float64)
    z64, a64 = z.astype(np.float64), a.astype(np.float64)
    stated = r32(r32(z64 * a64).astype(np.float64) * r32(1.0 - a64).astype(np.float64))
    other = r32(z64 * r32(a64 * r32(1.0 - a64).astype(np.float64)).astype(np.float64))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), stated.view(np.uint32))
    assert not np.array_equal(stated.view(np.uint32), other.view(np.uint32))
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '__fmul_rn(__fmul_rn(z, a), __fsub_rn(1.0f, a))' in design


@pytest.mark.parametrize('name', sorted(K.STACKS))
def test_twin_bounds_are_usable(name):
    """every bound of test 1 is a positive number, and three steps move every trained tensor of the reference"""
    c = K.case(name)
    assert all(np.isfinite(v) and v > 0 for v in c['grad_tol'].values()), c['grad_tol']
    start, end = S.tensors(c['p0']), S.tensors(c['ref'][-1])
    assert all(S.max_dev(start[k], end[k]) > 0 for k in start)


def test_stale_weights_violate_the_bound():
    """the wrong order - a backward pass that reads weights its own step has updated - misses the bound of the stale-weight test
    on S1 by orders of magnitude in the layer below the top"""
    c = K.case('S1')
    worst = 0.0
    for u in range(K.UPDATES):
        ref, twin, stale = S.tensors(c['ref'][u]), S.tensors(c['twin'][u]), S.tensors(c['stale'][u])
        for k in ('W1', 'hb1'):
            tol = K.FACTOR * S.max_dev(twin[k], ref[k])
            err = S.max_dev(stale[k], ref[k])
            print('stale order, step %d, %-3s: twin deviation %.3g, stale deviation %.3g, bound %.3g' % (u, k, tol / K.FACTOR, err, tol))
            assert err > tol, (u, k, err, tol)
            worst = max(worst, err / tol)
    assert worst > 100.0, worst


def test_toy_problem_is_learned_by_the_twin():
    """the public-API test's condition, checked on the CPU first: five epochs lower the mean NLL and reach accuracy 1.0"""
    c = K.toy_case()
    for name in ('ref', 'twin'):
        start, end, acc = c[name]
        print('toy, %s: mean log p %.4f -> %.4f, accuracy %.3f' % (name, start, end, acc))
        assert end > start and acc == 1.0, (name, c[name])


# ---- the C ABI
def test_signatures_and_header_carry_the_entries():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd import build
    header = open(os.path.join(ROOT, 'include', 'bm355.h')).read()
    for e in ENTRIES:
        assert e in _ffi.SIGNATURES, e
        m = re.search(r'\bint %s\(([^;]*)\);' % e, header)
        assert m, e
        assert len(re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')) == len(_ffi.SIGNATURES[e]), e
    assert 'bm_stack.hip' in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'bm_stack.hip'))


# ---- Python: every refusal raises before a device is touched
@pytest.fixture
def no_device(monkeypatch):
    from boltzmann_machines_amd import _ffi

    def refuse(*a, **kw):
        raise AssertionError('the library was loaded: a refusal came too late')
    monkeypatch.setattr(_ffi, 'load', refuse)


def rbm(V, H, cls=None, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    kw.setdefault('batch_size', 8)
    return (cls or BernoulliRBM)(n_visible=V, n_hidden=H, verbose=False, random_seed=1, **kw)


def test_python_refusals(no_device, monkeypatch, tmp_path):
    from boltzmann_machines_amd import GaussianRBM, MultinomialRBM, StackClassifier
    mk = lambda layers, **kw: StackClassifier(layers, **dict(dict(n_classes=3, model_path=str(tmp_path) + '/'), **kw))
    ok = mk([rbm(12, 8), rbm(8, 6)])
    assert ok.n_classes == 3 and ok.batch_size == 8 and ok.layers[1].n_classes == 3
    for layers, match in (([rbm(12, 8, GaussianRBM), rbm(8, 6)], 'Gaussian'),
                          ([rbm(12, 8, MultinomialRBM), rbm(8, 6)], 'Multinomial'),
                          ([rbm(12, 8, dtype='float64'), rbm(8, 6)], 'float64'),
                          ([rbm(12, 8, dbm_first=True), rbm(8, 6)], 'dbm_first'),
                          ([rbm(12, 8), rbm(8, 6, dbm_last=True)], 'dbm_last'),
                          ([rbm(12, 8, dropout=0.5), rbm(8, 6)], 'dropout'),
                          ([rbm(12, 8, sparsity_cost=0.1), rbm(8, 6)], 'sparsity'),
                          ([rbm(12, 8), rbm(9, 6)], 'chain'),
                          ([], 'empty')):
        with pytest.raises(ValueError, match=match):
            mk(layers)
    same = rbm(8, 8)
    with pytest.raises(ValueError, match='twice'):
        mk([same, same])
    centred = rbm(12, 8)
    centred.set_centering(True)
    with pytest.raises(ValueError, match='centering'):
        mk([centred, rbm(8, 6)])
    with pytest.raises(ValueError, match='n_classes'):
        mk([rbm(12, 8), rbm(8, 6)], n_classes=None)
    with pytest.raises(ValueError, match='n_classes'):
        mk([rbm(12, 8), rbm(8, 6)], n_classes=1)
    with pytest.raises(ValueError, match='max_batch'):
        mk([rbm(12, 8), rbm(8, 6, batch_size=4)], batch_size=8)
    with pytest.raises(ValueError, match='learning_rate'):
        mk([rbm(12, 8), rbm(8, 6)], learning_rate=[0.1, 0.1, 0.1])
    X, y = np.zeros((10, 12), np.float32), np.zeros(10, np.int64)
    with pytest.raises(ValueError, match='labels for'):
        ok.fit(X, y[:9])
    with pytest.raises(ValueError, match='outside'):
        ok.fit(X, np.full(10, 3))
    with pytest.raises(ValueError, match='outside'):
        ok.fit(X, np.full(10, -1))
    with pytest.raises(ValueError, match='invalid shape'):
        ok.fit(X[:, :11], y)
    with pytest.raises(ValueError, match='invalid shape'):
        ok.predict(X[:, :11])
    with pytest.raises(ValueError, match='go together'):
        ok.fit(X, y, X_val=X)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(ValueError, match='BM355_DATA_PARALLEL'):
        ok.fit(X, y)
    with pytest.raises(ValueError, match='BM355_DATA_PARALLEL'):
        mk([rbm(12, 8), rbm(8, 6)])


def test_from_dbm_builds_the_documented_weights(no_device, tmp_path):
    from boltzmann_machines_amd import StackClassifier
    rng = np.random.RandomState(3)
    P = dict(W=rng.randn(9, 7).astype(np.float32), W_1=rng.randn(7, 5).astype(np.float32), W_2=rng.randn(5, 4).astype(np.float32),
             vb=rng.randn(9).astype(np.float32), hb=rng.randn(7).astype(np.float32), hb_1=rng.randn(5).astype(np.float32),
             hb_2=rng.randn(4).astype(np.float32))
    before = {k: v.copy() for k, v in P.items()}
    s = StackClassifier.from_dbm(P, 3, batch_size=6, model_path=str(tmp_path) + '/')
    assert [(m.n_visible, m.n_hidden) for m in s.layers] == [(9, 7), (7, 5), (5, 4)] and s.n_classes == 3 and s.batch_size == 6
    for i, (w, scale) in enumerate((('W', 2.0), ('W_1', 2.0), ('W_2', 1.0))):
        assert np.array_equal(s.layers[i].W_init, P[w] * np.float32(scale))
    for i, (hb, vb) in enumerate((('hb', 'vb'), ('hb_1', 'hb'), ('hb_2', 'hb_1'))):
        assert np.array_equal(s.layers[i].hb_init, P[hb]) and np.array_equal(s.layers[i].vb_init, P[vb])
    assert all(np.array_equal(P[k], before[k]) for k in P)
    half = StackClassifier.from_dbm(P, 3, bottom_up_scale=1.5, batch_size=6, model_path=str(tmp_path) + '/')
    assert np.array_equal(half.layers[0].W_init, P['W'] * np.float32(1.5)) and np.array_equal(half.layers[2].W_init, P['W_2'])
    with pytest.raises(ValueError, match='chain|W'):
        StackClassifier.from_dbm(dict(P, W_1=P['W_1'][:6]), 3, batch_size=6)
