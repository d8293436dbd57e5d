"""The Multinomial layer of the ORACLE at the edges (no GPU): every assertion tests/test_multinomial_edges_gpu.py makes on the
device is one the reference passes here, with the same logit sets, seeds, bounds and caps (tests/multinomial_probes.py).
The printed error-to-bound ratios and |z| values are the record of that."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import multinomial_probes as mp

SEED = 7


def test_what_the_probes_return():
    """the W = 0 probe hands every row the logits hb whatever X is; the one-hot probe reaches the FIRST prop-up only (h0),
    and what transform returns is a different softmax"""
    I, M = 65, 100
    l = dict(mp.logit_sets(I))['c_uniform']
    t = mp.twin_rbm(I, M, l)
    a = mp.twin_means(t)
    assert np.all(mp.bits(a) == mp.bits(a[0])), 'rows of the W = 0 probe differ'
    t.set_seed(SEED)
    b = t.transform(1.0 - mp.probe_x(mp.ROWS), 1)
    mp.assert_bits(a, b, 'the W = 0 probe with another X')
    mp.check_means(l, a, M, what='W = 0 probe')
    # one-hot: h0 sees W[r, :]
    W = np.stack([dict(mp.logit_sets(I))[n] for n in ('a_normal', 'c_uniform', 'g_ramp_up', 'e_tied')])
    t = orc.OracleRBM(4, I, h_unit=2, n_samples=M)
    t.p['W'][...] = W
    t.set_seed(SEED)
    out = t.transform(np.eye(4, dtype=np.float32), 1)
    for r in range(4):
        mp.check_means(W[r], t.work['h0m'][r], M, what='one-hot probe, h0 of row %d' % r)
    assert not np.array_equal(out, t.work['h0m'])            # transform returns the means after the Gibbs step


@pytest.mark.parametrize('prec', [mp.F32, mp.F64], ids=['float32', 'float64'])
def test_means_within_the_derived_bound(prec):
    worst = 0.0
    for I in mp.WIDTHS:
        for name, l in mp.logit_sets(I, prec):
            for M in mp.N_SAMPLES:
                t = mp.twin_rbm(I, M, l, prec, SEED)
                worst = max(worst, mp.check_means(l, mp.twin_means(t), M, prec, 'oracle ' + name))
    print('oracle %s: largest error / bound %.3f' % (prec.name, worst))


@pytest.mark.parametrize('prec', [mp.F32, mp.F64], ids=['float32', 'float64'])
def test_counts_exact_and_chi_square(prec):
    tally = mp.Tally()
    for I in mp.WIDTHS:
        for name, l in mp.logit_sets(I, prec):
            for M in mp.N_SAMPLES:
                tally.add(l, mp.twin_counts(mp.twin_rbm(I, M, l, prec, SEED)), M, prec, name, 'oracle ' + name)
    assert len(tally.assert_statistical_leg()) >= 30


@pytest.mark.parametrize('prec', [mp.F32, mp.F64], ids=['float32', 'float64'])
def test_n_samples_far_above_the_width(prec):
    I, M = 64, 100000
    tally = mp.Tally()
    for name, l in mp.logit_sets(I, prec):
        t = mp.twin_rbm(I, M, l, prec, SEED)
        mp.check_means(l, mp.twin_means(t), M, prec, 'oracle ' + name)
        t.set_seed(SEED)
        tally.add(l, mp.twin_counts(t), M, prec, name, 'oracle ' + name)
    assert len([r for r in tally.rows if r[5] >= 10]) >= 4


def test_states_equal_means_without_sampling():
    for I in (1, 65, 8192):
        for name, l in mp.logit_sets(I):
            t = mp.twin_rbm(I, 100, l, sample_h_states=False)
            h = mp.twin_counts(t)
            t.set_seed(SEED)
            mp.assert_bits(h, mp.twin_means(t), 'states against means, ' + name)


def test_absorption_bound_and_the_two_masses():
    """the mass no draw can reach stays below (I - 1) eps for every set; family f at the widest row, both orders (the
    figures DESIGN.md 5 quotes)"""
    for prec in (mp.F32, mp.F64):
        worst = 0.0
        for I in mp.WIDTHS:
            for name, l in mp.logit_sets(I, prec):
                worst = max(worst, mp.absorbed_mass(l, prec) / max((I - 1) * prec.eps, 1e-300))
        f = dict(mp.logit_sets(8192, prec))
        fwd, rev = mp.absorbed_mass(f['f_absorbed'], prec), mp.absorbed_mass(f['f_absorbed_reversed'], prec)
        print('%s: absorbed mass at I = 8192 forward %.6e, reversed %.6e; largest mass / bound over all sets %.3f'
              % (prec.name, fwd, rev, worst))
        assert rev == 0.0 and fwd > 0.3 * 8191 * prec.eps
        assert int(mp.undrawable(f['f_absorbed'], prec).sum()) == 8191


def test_draw_index_beyond_2_pow_33():
    I, M = 65, 3
    l = dict(mp.logit_sets(I))['a_normal']
    base = mp.twin_counts(mp.twin_rbm(I, M, l, row0=0))
    far = mp.twin_counts(mp.twin_rbm(I, M, l, row0=2 ** 33))
    again = mp.twin_counts(mp.twin_rbm(I, M, l, row0=2 ** 33))
    mp.check_counts(l, far, M, what='row offset 2^33')
    mp.assert_bits(far, again, 'row offset 2^33, repeated')
    assert not np.array_equal(far, base)
    assert (2 ** 33 + mp.ROWS) * M > 2 ** 34                  # the high word of the Philox block counter is in use


def dbm_twin(widths, prec=mp.F32, **kw):
    hu, ns, P = mp.dbm_layers(widths, prec)
    t = orc.OracleDBM(mp.V_PROBE, list(widths), n_particles=mp.ROWS, batch_size=mp.ROWS, h_units=hu, n_samples=ns,
                      max_mf_updates=10, mf_tol=1e-7, **kw)
    for name, val in P.items():
        t.p[name][...] = val
    t.set_seed(SEED)
    return t, hu, ns, P


@pytest.mark.parametrize('widths', [(63, 64, 65), (65, 64, 63), (64, 65)], ids=str)
def test_dbm_layers_with_zero_weights(widths):
    """W = 0 inside the stack: the means are the same in every sweep (residual exactly 0), mu = M softmax(hb) within the
    bound, the h particles pass the count checks"""
    t, hu, ns, P = dbm_twin(widths)
    n = t.mean_field(mp.probe_x(mp.ROWS))
    print('mean-field trip count with zero weights: %d' % n)
    assert 1 <= n <= 2
    t.sample_v(1)
    tally = mp.Tally()
    for i, w in enumerate(widths):
        if hu[i]:
            sfx = '' if i == 0 else '_%d' % i
            mp.check_means(P['hb' + sfx], t.p['mu' + sfx], ns[i], what='oracle DBM mu' + sfx)
            tally.add(P['hb' + sfx], t.p['h' + sfx], ns[i], mp.F32, 'dbm', 'oracle DBM h' + sfx)
