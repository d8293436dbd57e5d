"""CPU half of the float64 lattice (tests/f64_lattice.py): the lattice reaches every branch class of the path model, the
data-dependent labels hold on the oracle, OracleRBM64.train_step agrees with the independent matrix-form restatement on
every lattice row, and the oracle's sigmoid holds 4 ulp against long double on the probe set the device test uses."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import f64_lattice as lat
from tests import np_reference as ref

# the rows the lattice was built from; a row may be added, none may leave
PINNED_RBM = ['64x64x32', '96x128x64', '160x66x33', '35x70x67-dropout-sparsity_cost', '70x35x100-dbm_first', '64x24x32',
              '1x1x1', '2x1x3', '1x2x2', '130x194x300-sample_h_states', '64x64x32-row5', '96x64x40-gauss',
              '96x128x64-k3-dbm_last', '120x192x48', '66x64x32-row3-dropout-sample_v_states']
PINNED_DBM = ['64-64_64-32-32', '96-66_35-33-65', '35-130_96_40-67-34', '166-128-64-96', '64-64_32-32-32-gauss',
              '20-12_16-10-10-row3-p7']


def test_lattice_reaches_every_required_label():
    got = lat.lattice_labels()
    assert not (lat.REQUIRED - got), 'no lattice row reaches %s' % sorted(lat.REQUIRED - got)


def test_no_lattice_row_has_left():
    assert [c['id'] for c in lat.RBM_LATTICE][:len(PINNED_RBM)] == PINNED_RBM
    assert [c['id'] for c in lat.DBM_LATTICE][:len(PINNED_DBM)] == PINNED_DBM


def test_model_on_shapes_read_off_the_kernels():
    """the model against values worked out by hand from t64_mainloop / launch_update"""
    up, down, up2, grad = lat.rbm_launches(160, 66, 33)
    assert up == up2 and (up['I'], up['J'], up['segs']) == (66, 33, [(160, 66, 160)])
    assert lat.tile_path(up, 0, 0) == ('fast',) and lat.tile_path(up, 64, 0) == ('generic',) and lat.tile_path(up, 0, 32) == ('generic',)
    assert lat.tile_path(grad, 0, 128) == ('fast', 'fast') and lat.tile_path(grad, 64, 0) == ('generic', 'generic')
    assert {'seg:nfull=odd>=5', 'seg:tail=0', 'launch:mixed', 'seg:generic-chunks=>=3'} <= lat.launch_labels(up)
    assert {'seg:nfull=2', 'seg:tail=1', 'seg:K%4=2'} <= lat.launch_labels(down)
    assert {'seg:nfull=1&tail=1', 'seg:K%4=1', 'order:(fast,fast)', 'order:seg1-tail&seg2-fast'} <= lat.launch_labels(grad)
    assert 'bias:extra>=2&nbias%4!=0' in lat.bias_labels(160, 66, 33, fused=True)          # 15 jobs, 2 x 8 wave slots
    assert 'bias:extra>=2' not in lat.bias_labels(160, 66, 33, fused=False)
    # odd leading dimension: never fast, scalar loads on that operand only
    up = lat.rbm_launches(35, 70, 67)[0]
    assert lat.tile_path(up, 0, 0) == ('generic',)
    assert {'fetch:P-vector&Q-scalar', 'seg:generic-chunks=2', 'seg:K%4=3'} <= lat.launch_labels(up)
    assert {'fetch:P-scalar&Q-vector', 'fetch:scalar&chunks>=3'} <= lat.launch_labels(lat.rbm_launches(35, 70, 67)[1])
    sweep0 = [l for l in lat.dbm_launches(96, [66, 35], 33, 65) if l['name'] == 'mf_sweep_0'][0]
    assert lat.tile_path(sweep0, 0, 0) == ('fast', 'generic')
    sweep0 = [l for l in lat.dbm_launches(35, [130, 96, 40], 67, 34) if l['name'] == 'mf_sweep_0'][0]
    assert lat.tile_path(sweep0, 64, 32) == ('generic', 'fast') and lat.tile_path(sweep0, 128, 0) == ('generic', 'generic')
    assert sorted(lat.UNREACHABLE) == ['even-ld-odd-ncols', 'misaligned-pointer']


# ------------------------------------------------------------------------------------------- oracle against NumPy
def _twin(c):
    kw = dict(c['kw'])
    if c['gaussian']:
        kw['v_unit'] = 1
    twin = orc.OracleRBM64(c['V'], c['H'], **kw)
    for nm, val in lat.rbm_params(c['V'], c['H']).items():
        twin.p[nm][...] = val
    if c['gaussian']:
        twin.p['sigma'][...] = lat.rbm_sigma(c['V'])
    twin.set_seed(lat.RBM_SEED)
    twin.row0 = c['row']
    return twin


def _cd_step_gaussian(P, sigma, X, lr, momentum, k, seed, call, l2, bern):
    """np_reference.cd_step for Gaussian visible units without visible sampling (rbm.py:107, layers.py:84-89): the input is
    divided by sigma, the visible means are (h W^T) * sigma + vb"""
    W, vb, hb = P['W'], P['vb'], P['hb']
    X = X / sigma[None, :]
    h0_means = ref.sigmoid(X.dot(W) + hb)
    h_states, u_h0 = bern(h0_means, seed, 2, call)
    us = []
    for t in range(k):
        v_states = h_states.dot(W.T) * sigma[None, :] + vb
        h_means = ref.sigmoid(v_states.dot(W) + hb)
        h_states, u = bern(h_means, seed, 4 + 16 * t, call)
        us.append((u, h_means))
    N = float(len(X))
    dW = (X.T.dot(h0_means) - v_states.T.dot(h_means)) / N - l2 * W
    dvb = np.mean(X - v_states, axis=0)
    dhb = np.mean(h0_means - h_means, axis=0)
    P['q_means'][...] = 0.9 * P['q_means'] + (1 - 0.9) * np.sum(h_means, axis=0)
    P['dW'][...] = lr * (momentum * P['dW'] + dW); P['W'] += P['dW']
    P['dvb'][...] = lr * (momentum * P['dvb'] + dvb); P['vb'] += P['dvb']
    P['dhb'][...] = lr * (momentum * P['dhb'] + dhb); P['hb'] += P['dhb']
    return dict(h0_means=h0_means, u_h0=u_h0, us=us)


@pytest.mark.parametrize('c', lat.RBM_LATTICE, ids=[c['id'] for c in lat.RBM_LATTICE])
def test_oracle_rbm64_vs_numpy_restatement(c, monkeypatch):
    """two OracleRBM64.train_step calls against np_reference.cd_step drawing from the float64 Philox stream.  Bound:
    4 * max(V, H, B) * 2**-52 absolute - the reordering error of a sum of at most K terms of magnitude <= 1, times 4 for
    the three chained contractions and the update.  No draw may sit within 1e-9 of its probability (no tie to excuse)."""
    V, H, B, k, row = c['V'], c['H'], c['B'], c['k'], c['row']

    def bernoulli64(p, seed, site, call, row0=0):
        n = p.shape[1]
        u = orc.uniform_d(seed, site, call, p.size, idx0=row * n).reshape(p.shape)
        return (u < p).astype(np.float64), u

    def dropout64(X, keep, seed, call):
        u = orc.uniform_d(seed, 1, call, X.size, idx0=row * V).reshape(X.shape)
        return (X / keep) * np.floor(keep + u)
    monkeypatch.setattr(ref, 'bernoulli', bernoulli64)
    monkeypatch.setattr(ref, 'dropout_input', dropout64)
    twin = _twin(c)
    P = {n: twin.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
    kw = c['kw']
    lr = lat.RBM_LR_GAUSS if c['gaussian'] else lat.RBM_LR
    tol = 4 * max(V, H, B) * 2.0 ** -52
    worst, margin = 0.0, np.inf
    for s in range(2):
        X = lat.rbm_data(c['rows'], V, s, c['gaussian'])[row:row + B]
        call = twin.call
        twin.train_step(X, lr, lat.RBM_MOM, k)
        if c['gaussian']:
            r = _cd_step_gaussian(P, lat.rbm_sigma(V), X, lr, lat.RBM_MOM, k, lat.RBM_SEED, call, 1e-4, bernoulli64)
        else:
            r = ref.cd_step(P, X, lr, lat.RBM_MOM, k, lat.RBM_SEED, call, l2=kw.get('l2', 1e-4),
                            sample_v=kw.get('sample_v_states', False), sample_h=kw.get('sample_h_states', True),
                            dropout=kw.get('dropout'), sp_cost=kw.get('sparsity_cost', 0.),
                            dbm_first=kw.get('dbm_first', False), dbm_last=kw.get('dbm_last', False))
        draws = list(r['us'])
        if kw.get('sample_h_states', True):
            draws.append((r['u_h0'], r['h0_means']))
        for u, p in draws:
            margin = min(margin, float(np.min(np.abs(u - p))))
        for n in P:
            worst = max(worst, float(np.max(np.abs(twin.p[n] - P[n]))))
            np.testing.assert_allclose(twin.p[n], P[n], rtol=0, atol=tol, err_msg='%s after step %d' % (n, s))
    print('%s: max |oracle - numpy| = %.3e (bound %.3e), closest draw %.3e' % (c['id'], worst, tol, margin))
    assert margin > 1e-9


# ------------------------------------------------------------------------------------- data-dependent labels, DBM
def _dbm_twin(c):
    kw = dict(c['kw'])
    if c['gaussian']:
        kw['v_unit'] = 1
    twin = orc.OracleDBM64(c['V'], c['nh'], n_particles=c['M'], batch_size=c['N'], **kw)
    for nm, val in lat.dbm_params(c['V'], c['nh'], c['M']).items():
        twin.p[nm][...] = val
    if c['gaussian']:
        twin.p['sigma'][...] = np.linspace(0.6, 1.4, c['V'])
    twin.set_seed(42)
    twin.prow0 = c['particle0']
    return twin


@pytest.mark.parametrize('c', lat.DBM_LATTICE, ids=[c['id'] for c in lat.DBM_LATTICE])
def test_dbm_rows_reach_their_data_dependent_labels(c):
    """mean-field exit (tolerance / cap) and max-norm (clipped and unclipped columns in one matrix) as the row declares"""
    twin = _dbm_twin(c)
    lr = 1e-3 if c['gaussian'] else 0.05
    X = lat.dbm_data(c['rows'], c['V'], 0, c['gaussian'])[c['row']:c['row'] + c['N']]
    n_mf, _ = twin.train_step(X, lr, 0.5, 2)
    cap = c['kw'].get('max_mf_updates', 10)
    assert ('dbm:mf-exit-tol' in c['expect']) == (0 < n_mf < cap), n_mf
    assert ('dbm:mf-exit-cap' in c['expect']) == (n_mf == cap), n_mf
    mn = c['kw'].get('max_norm', np.inf)
    both = False
    for i in range(len(c['nh'])):
        nrm = twin.p['W_norm' + ('' if i == 0 else '_%d' % i)]
        both |= bool(np.any(nrm > mn) and np.any(nrm < mn))
    assert ('dbm:maxnorm-clipped&unclipped' in c['expect']) == both


# ---------------------------------------------------------------------------------------------- the oracle's sigmoid
def test_oracle_sigmoid_within_4ulp_of_long_double():
    L = orc.lib()
    orc.OracleRBM64(2, 2)                                   # registers the double signatures
    x = lat.sigmoid_probes()
    got = np.array([L.orc_sigmoid_d(float(v)) for v in x])
    err = lat.ulp_error(got, lat.sigmoid_exact(x))
    i = int(np.argmax(err))
    print('orc_sigmoid_d: max %.3f ulp at x = %r over %d points' % (float(err[i]), float(x[i]), x.size))
    assert float(err[i]) <= 4.0
    assert got[x == 0.0].tolist() == [0.5] * int(np.sum(x == 0.0))


def test_softplus_host_error_is_small():
    """E of the device softplus bound (tests/test_f64_numerics_gpu.py) is a property of the host libm, measured here"""
    E = lat.softplus_host_error()
    print('softplus under host libm: E = %.3f ulp' % E)
    assert E < 4.0


def test_oracle_max_norm_edges_within_2ulp_of_long_double():
    """lr = 0: the update is d = 0 and only the rescale acts.  Zero column, a column under the 1e-8 floor, a clipped one"""
    V, nh, N, M = lat.MAXNORM_SHAPE
    twin = orc.OracleDBM64(V, nh, n_particles=M, batch_size=N, max_norm=lat.MAXNORM_LIMIT)
    P = lat.maxnorm_edge_params()
    for nm, val in P.items():
        twin.p[nm][...] = val
    twin.set_seed(42)
    twin.train_step(lat.dbm_data(N, V, 0), 0.0, 0.5, 1)
    for nm, nn in (('W', 'W_norm'), ('W_1', 'W_norm_1')):
        n, Wx = lat.maxnorm_exact(P[nm])
        assert float(np.max(lat.ulp_error(twin.p[nn][1:], n[1:]))) <= 2.0 and twin.p[nn][0] == 0.0
        nz = Wx != 0
        err = lat.ulp_error(twin.p[nm][nz], Wx[nz])
        print('%s: max %.3f ulp' % (nm, float(np.max(err))))
        assert float(np.max(err)) <= 2.0
        assert np.all(twin.p[nm][:, 0] == 0.0)
        np.testing.assert_allclose(twin.p[nm][:, 1], 1e-10 * float(n[1]) / 1e-8, rtol=1e-15)
        np.testing.assert_allclose(np.sqrt(np.sum(twin.p[nm][:, 2].astype(np.longdouble) ** 2)), lat.MAXNORM_LIMIT, rtol=1e-15)
