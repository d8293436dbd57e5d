"""GaussianRBM as one joint model - AIS log Z, log-density, parallel tempering - the part that needs no GPU: the CPU
twin (tests/gauss_twin.py) against ground truth by enumeration of the hidden layer, and the host-side surface.

What the twin is held to here is what the GPU file then holds the engine to, bit for bit: if the twin's variance law, its swap energy
or its AIS path were wrong, these tests fail without a GPU."""
import os
import re

import numpy as np
import pytest

from tests import gauss_twin as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ---- 1. the enumeration itself
def test_enumeration_agrees_with_quadrature():
    """V = 1: log Z over x by enumeration of h equals the integral of exp(-F(x / sigma)) on a fine grid, and the tempered moments
    equal the grid's"""
    p = dict(W=np.array([[1.5, -0.75]], f32), vb=np.array([0.4], f32), hb=np.array([-0.3, 0.6], f32), sigma=np.array([0.7], f32))
    x = np.linspace(-14., 14., 400001)
    W, hb, c, sigma = (a.astype(f64) for a in G.params(p))
    u = x / sigma[0]

    def neg_f(beta):           # log sum_h exp(-beta E(u, h))
        return -beta * 0.5 * (u - c[0]) ** 2 + np.sum(np.logaddexp(0., beta * (u[:, None] * W[0][None, :] + hb[None, :])), axis=1)
    dx = x[1] - x[0]
    assert abs(np.log(np.sum(np.exp(neg_f(1.0))) * dx) - G.exact_log_Z(p)) < 1e-9
    for beta in (0.25, 1.0):
        w = np.exp(neg_f(beta))
        w /= w.sum()
        _, mean, cov, m4 = G.exact_tempered(p, beta)
        gm = np.sum(w * u)
        assert abs(gm - mean[0]) < 1e-9 and abs(np.sum(w * (u - gm) ** 2) - cov[0, 0]) < 1e-8
        assert abs(np.sum(w * (u - gm) ** 4) - m4[0]) < 1e-7


def test_log_density_integrates_to_one():
    """-F - log Z against a float64 statement: on a V = 2 grid in data units the density sums to one"""
    p = G.make_params(2, 3, std=0.8, seed=11)
    g = np.linspace(-12., 12., 1201)
    X = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)
    # (free_energy64 rounds x / sigma to float32 as the engine does: the grid's sum is held to 1e-5, not to quadrature accuracy)
    lp = -G.free_energy64(p, X) - G.exact_log_Z(p)
    assert abs(np.sum(np.exp(lp)) * (g[1] - g[0]) ** 2 - 1.0) < 1e-5


# ---- 2. the twin's AIS against enumeration
AIS_CASE = dict(V=6, H=4, std=0.5, pseed=21, n_betas=200, n_runs=200, k=1, seed=4242)


def test_twin_ais_against_enumeration():
    """V = 6, H = 4, sigma not all 1, a from data: |log_mean - exact| <= 3 s, s the delta-method standard error of the run's own values
    (the criterion of tests/test_rsm_ais_gpu.py); the case and the seed are fixed"""
    c = AIS_CASE
    p = G.make_params(c['V'], c['H'], std=c['std'], seed=c['pseed'])
    assert np.all(p['sigma'] != 1)
    a = G.base_mean(G.data(50, c['V'], 5, p['sigma']), p['sigma'])
    values, _, _ = G.ais(p, c['n_betas'], c['n_runs'], c['k'], c['seed'], a=a)
    est, s = G.log_mean_and_se(values)
    exact = G.exact_log_Z(p)
    print('log_mean %.6f exact %.6f s %.4g ratio %.2f' % (est, exact, s, abs(est - exact) / s))
    assert abs(est - exact) <= 3.0 * s
    # ... and under the zero base mean
    values0, _, _ = G.ais(p, c['n_betas'], c['n_runs'], c['k'], c['seed'] + 1)
    est0, s0 = G.log_mean_and_se(values0)
    print('a = 0: log_mean %.6f exact %.6f s %.4g ratio %.2f' % (est0, exact, s0, abs(est0 - exact) / s0))
    assert abs(est0 - exact) <= 3.0 * s0


def test_twin_ais_closed_forms():
    """W = 0: every score's softplus part is beta-linear in nothing but hb and the visible part is exact in expectation; with
    a = c as well every chain returns log Z exactly.  n_betas = 2 is one importance weight.  Slices by chain0"""
    p = G.make_params(5, 3, seed=4)
    flat = dict(p, W=np.zeros_like(p['W']))
    c = G.params(flat)[2]
    values, _, _ = G.ais(flat, 7, 5, 2, seed=3, a=c)
    np.testing.assert_allclose(values, G.exact_log_Z(flat), rtol=0, atol=1e-10)
    # n_betas = 2: value = log p*_1(u_0) - log p*_0(u_0) + log Z_0, u_0 = a + n
    a = G.base_mean(G.data(20, 5, 2, p['sigma']), p['sigma'])
    values, _, _ = G.ais(p, 2, 9, 3, seed=31, chain0=4, a=a)
    u0 = (a + G.normals(31, G.SITE_AIS_V0, 0, 4, 9, 5)).astype(f32).astype(f64)
    W, hb, cc, _ = (x.astype(f64) for x in G.params(p))
    lp1 = -0.5 * np.sum((u0 - cc) ** 2, axis=1) + np.sum(np.logaddexp(0., u0.dot(W) + hb), axis=1)
    lp0 = -0.5 * np.sum((u0 - a.astype(f64)) ** 2, axis=1) + 3 * np.log(2.)
    want = lp1 - lp0 + 0.5 * 5 * np.log(2 * np.pi) + 3 * np.log(2.) + np.sum(np.log(p['sigma'].astype(f64)))
    np.testing.assert_allclose(values, want, rtol=0, atol=1e-5)          # (dvec = fl32(c - a): the twin's linear term is the engine's)
    big, ub, hb_ = G.ais(p, 6, 30, 2, seed=11, a=a)
    part, up, hp = G.ais(p, 6, 10, 2, seed=11, chain0=15, a=a)
    assert np.array_equal(big[15:25], part) and np.array_equal(ub[15:25], up) and np.array_equal(hb_[15:25], hp)


# ---- 3. the twin's tempering against enumeration
PT_CASE = dict(V=6, H=4, std=0.6, pseed=22, betas=(0.25, 0.5, 1.0), M=3000, steps=25, seed=9001)
PT_SIGMAS = 4.5           # 36 comparisons: P(|z| > 4.5 anywhere) < 3e-4 for a correct sampler


def test_twin_tempering_moments_per_temperature():
    """For EACH temperature of the ladder the sample mean and the per-unit variance of u over the independent chains agree with
    E_beta[u] and diag Cov_beta[u] within PT_SIGMAS standard errors, computed from the exact covariance and the exact fourth
    moments.  A variance law sd = beta or sqrt(beta) instead of 1 / sqrt(beta) fails this at beta = 0.25 by tens of standard errors"""
    c = PT_CASE
    p = G.make_params(c['V'], c['H'], std=c['std'], seed=c['pseed'])
    e = G.Ensemble(p, c['M'], c['betas'], c['seed'])
    e.sweep(c['steps'])
    worst = 0.0
    for r, beta in enumerate(c['betas']):
        u = e.v[e.idx == r].astype(f64)
        assert len(u) == c['M']                                           # one replica of every chain at every temperature
        _, mean, cov, m4 = G.exact_tempered(p, float(f32(beta)))
        var = np.diag(cov)
        z_mean = (u.mean(axis=0) - mean) / np.sqrt(var / len(u))
        z_var = (u.var(axis=0) - var) / np.sqrt((m4 - var ** 2) / len(u))
        print('beta %.2f: max |z| mean %.2f variance %.2f (variance %.3f .. %.3f)' % (beta, np.abs(z_mean).max(), np.abs(z_var).max(), var.min(), var.max()))
        worst = max(worst, np.abs(z_mean).max(), np.abs(z_var).max())
        # (what a wrong law would show: noise of variance beta where 1 / beta belongs moves every unit's variance by 1 / beta - beta)
        assert beta == 1.0 or np.min((1.0 / beta - beta) / np.sqrt((m4 - var ** 2) / len(u))) > 3 * PT_SIGMAS
    assert worst <= PT_SIGMAS
    acc = e.cnt[1] / np.maximum(e.cnt[0], 1)
    print('acceptance', acc)
    assert np.all(acc > 0.2)


BIMODAL = dict(w=8.0, p1=0.3, betas=(0.05, 0.2, 0.6, 1.0), M=400, steps=150, seed=77)


def test_twin_bimodal_single_temperature_stays_ladder_mixes():
    """two modes 8 sqrt(2) standard deviations apart: with one temperature every chain started in one mode stays there; with the
    ladder the beta = 1 occupancy of the other mode is within 4 standard errors of the exact 0.3"""
    c = BIMODAL
    p = G.bimodal_params(c['w'], c['p1'])
    ph = G.exact_tempered(p, 1.0)[0]
    assert abs(ph[1] - c['p1']) < 1e-5                                    # (hb is float32)
    _, _, centre, sigma = G.params(p)
    V0 = np.tile(G.scale_out(centre, sigma), (c['M'], 1))                 # every chain starts at the centre of mode 0
    single = G.Ensemble(p, c['M'], [1.0], c['seed'], V0=V0)
    single.sweep(c['steps'])
    assert G.mode_of(p, single.read()[0]).sum() == 0
    e = G.Ensemble(p, c['M'], c['betas'], c['seed'], V0=V0)
    e.sweep(c['steps'])
    occ = G.mode_of(p, e.read()[0]).mean()
    se = np.sqrt(c['p1'] * (1 - c['p1']) / c['M'])
    print('occupancy of mode 1 at beta = 1: %.4f (exact %.4f, se %.4f), acceptance %s' % (occ, ph[1], se, e.cnt[1] / np.maximum(e.cnt[0], 1)))
    assert abs(occ - ph[1]) <= 4.0 * se


def test_twin_one_temperature_from_V_init_is_the_plain_chain():
    p = G.make_params(7, 5, seed=8)
    V0 = G.data(6, 7, 3, p['sigma'])
    e = G.Ensemble(p, 6, [1.0], 123, chain0=4, V0=V0)
    e.sweep(5)
    X, H = G.plain_chain(p, V0, 5, 123, row0=4)
    got_x, got_h = e.read()
    assert np.array_equal(got_x.view(np.uint32), X.view(np.uint32)) and np.array_equal(got_h, H)
    # slices by chain0: chains [2, 5) of a run are the run of 3 chains at chain0 + 2
    big = G.Ensemble(p, 6, [0.3, 0.6, 1.0], 5, chain0=10)
    big.sweep(4)
    part = G.Ensemble(p, 3, [0.3, 0.6, 1.0], 5, chain0=12)
    part.sweep(4)
    assert np.array_equal(big.v[6:15].view(np.uint32), part.v.view(np.uint32)) and np.array_equal(big.idx[6:15], part.idx)


# ---- 4. the surface
NEW_ENTRIES = {'bm_rbm_gauss_ais': 8, 'bm_rbm_gauss_free_energy_rows': 4, 'bm_rbm_gauss_pt_init': 6, 'bm_rbm_gauss_pt_sweep': 2,
               'bm_rbm_gauss_pt_read': 5}


def test_header_declares_and_ffi_binds():
    from boltzmann_machines_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'bm355.h')).read()
    for name, nargs in NEW_ENTRIES.items():
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name
        assert len(m.group(1).split(',')) == nargs, name
        assert len(_ffi.SIGNATURES[name]) == nargs, name
    from boltzmann_machines_amd import build
    assert 'bm_gauss.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'bm_gauss.hip'))


def test_model_surface_and_refusals_build_no_engine(tmp_path):
    from boltzmann_machines_amd import BernoulliRBM, GaussianReLURBM, GaussianRBM
    from boltzmann_machines_amd.engine import RbmEngine
    for name in ('ais_log_Z', 'free_energy', 'log_density', 'sample_v_tempered'):
        assert callable(getattr(GaussianRBM, name, None)), name
        assert not hasattr(BernoulliRBM, name), name                      # (new names on the Gaussian class alone)
    for name in ('gauss_ais', 'gauss_free_energy_rows', 'gauss_pt_init', 'gauss_pt_sweep', 'gauss_pt_read'):
        assert callable(getattr(RbmEngine, name, None)), name
    kw = dict(n_visible=6, n_hidden=4, verbose=False)
    X = np.zeros((2, 6), f32)
    calls = (('ais_log_Z', lambda m: m.ais_log_Z(n_betas=5, n_runs=4)), ('free_energy', lambda m: m.free_energy(X)),
             ('log_density', lambda m: m.log_density(X, 0.)), ('sample_v_tempered', lambda m: m.sample_v_tempered(3, n_gibbs_steps=2)))
    relu = GaussianReLURBM(model_path=str(tmp_path / 'r') + '/', **kw)
    for name, call in calls:
        with pytest.raises(ValueError, match=r'%s.*NReLU' % name):
            call(relu)
    assert relu._engine is None
    for tag, extra, word in (('d', dict(dtype='float64'), 'float64'), ('f', dict(dbm_first=True), 'dbm_first'),
                             ('l', dict(dbm_last=True), 'dbm_last')):
        m = GaussianRBM(model_path=str(tmp_path / tag) + '/', **dict(kw, **extra))
        state = m._rng.get_state()
        for name, call in calls:
            with pytest.raises(NotImplementedError, match=word):
                call(m)
        assert m._engine is None and m._rng.get_state() == state        # no engine built, no seed drawn
    # the old names keep refusing Gaussian visible units with the same words
    g = GaussianRBM(model_path=str(tmp_path / 'g') + '/', **kw)
    for call in (lambda: g.log_Z(n_betas=5, n_runs=4), lambda: g.log_proba(X, 0.), lambda: g.sample_v(3)):
        with pytest.raises(NotImplementedError, match='Gaussian visible units are not supported'):
            call()
    with pytest.raises(NotImplementedError, match='Gaussian visible units are not supported'):
        g.set_negative_phase('tempered')
    assert g._engine is None
    # the base mean: None, data -> mean(X / sigma), a vector in data units -> X / sigma
    gs = GaussianRBM(model_path=str(tmp_path / 's') + '/', sigma=[0.5, 1, 2, 4, 0.25, 3], **kw)
    sigma = np.array([0.5, 1, 2, 4, 0.25, 3], f32)
    Xb = G.data(9, 6, 1, sigma)
    assert gs._base_mean(None) is None
    np.testing.assert_array_equal(gs._base_mean(Xb), G.base_mean(Xb, sigma))
    np.testing.assert_array_equal(gs._base_mean(Xb[0]), G.scale_in(Xb[0], sigma))
    with pytest.raises(ValueError):
        gs._base_mean(np.zeros(5))
    with pytest.raises(ValueError, match='n_betas'):
        gs.ais_log_Z(n_betas=1)
    with pytest.raises(ValueError):
        gs.sample_v_tempered(0)
    with pytest.raises(ValueError):
        gs.sample_v_tempered(3, betas=[0.5, 0.9])
    assert gs._engine is None
