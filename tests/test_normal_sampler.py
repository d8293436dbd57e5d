"""The Normal sampler (`box_muller` = `pin_log_unit` / `pin_sincos_2pi`, csrc/bm_rng.h) held to float64 without a GPU: the
oracle's restatement (oracle/bm_oracle.c, bit for bit what the device computes - tests/test_normal_sampler_gpu.py asserts
that at the same words) over ALL 2^23 words, at every edge word of tests/normal_probes.py and on a bulk of the stream, and
the constructions the GPU file relies on (the edge-word search, the twin at a row offset, the cases' own premises).

Out of scope: the float64 engines.  They draw with the device's log / sin / cos, compared at 1e-12
(csrc/bm_rbm64.hip), and RbmEngine64 has no `gibbs` that would return raw draws."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import normal_probes as nb

SEED, SITE = nb.SEED, nb.SITE_V


@pytest.fixture(scope='module')
def found():
    return nb.find_words(SEED, SITE, 0)


# ---- a. every word
def test_exhaustive_sweep_of_log_sincos_and_radius():
    """all 2^23 values of a uniform: caps over the exhaustive maximum of a pure function (no sampling error; the margin is
    the round-up to a power of two).  The maxima printed here are quoted in DESIGN.md 4 and csrc/bm_rng.h."""
    ld = np.longdouble
    two_pi = ld(8) * np.arctan(ld(1))
    worst = dict(log=(0.0, -1), sin=(0.0, -1), cos=(0.0, -1), r=(0.0, -1), unit=(0.0, -1))
    step = 2 ** 20
    for m0 in range(0, 2 ** 23, step):
        m = np.arange(m0, m0 + step, dtype=np.uint32)
        u = nb.unit(m)
        u1 = np.maximum(u, nb.EPS)
        lg32 = orc.pin_log_unit(u1)
        sn32, cs32 = orc.pin_sincos_2pi(u)
        r32 = np.sqrt(np.float32(-2.0) * lg32)                                  # sqrtf(-2.0f * log): float32 throughout
        assert r32.dtype == np.float32
        lg = np.log(u1.astype(ld))
        a = two_pi * u.astype(ld)
        s64 = sn32.astype(np.float64)
        c64 = cs32.astype(np.float64)
        errs = dict(log=np.abs(lg32.astype(ld) - lg) / np.abs(lg), sin=np.abs(sn32.astype(ld) - np.sin(a)),
                    cos=np.abs(cs32.astype(ld) - np.cos(a)), r=np.abs(r32.astype(ld) - np.sqrt(ld(-2) * lg)),
                    unit=np.abs(s64 * s64 + c64 * c64 - 1.0))
        for name, e in errs.items():
            k = int(np.argmax(e))
            if float(e[k]) > worst[name][0]:
                worst[name] = (float(e[k]), m0 + k)
    print('pin_log_unit: max relative error %.4g at word mantissa %d (u = %.6f)' % (worst['log'] + (worst['log'][1] / 2.0 ** 23,)))
    print('pin_sincos_2pi: max absolute error sin %.4g at %d, cos %.4g at %d' % (worst['sin'] + worst['cos']))
    print('sqrtf(-2 ln u1): max absolute error %.4g at %d' % worst['r'])
    print('|sin^2 + cos^2 - 1|: max %.4g at %d' % worst['unit'])
    assert worst['log'][0] < nb.LOG_RTOL, worst['log']
    assert worst['sin'][0] < nb.SINCOS_ATOL and worst['cos'][0] < nb.SINCOS_ATOL, (worst['sin'], worst['cos'])
    assert worst['r'][0] <= nb.R_ATOL, worst['r']
    assert worst['unit'][0] <= 4 * 2.0 ** -23, worst['unit']


# ---- b. a draw against the real-number Box-Muller of the same words
def test_draw_bound_is_the_derived_one():
    r_clamp = float(np.sqrt(-2.0 * np.log(np.float64(nb.EPS))))
    assert r_clamp < nb.R_MAX < r_clamp + 1e-3
    assert nb.DRAW_ATOL == nb.R_MAX * 2.0 ** -23 + 2.0 ** -21 + 2.0 ** -22 and 1.3e-6 < nb.DRAW_ATOL < 1.4e-6


def test_every_edge_word_is_in_the_stream(found):
    assert set(found) == set(nb.TARGETS) and len(nb.TARGETS) == 27
    print('edge pairs of seed %d, site %d: last at element %d' % (SEED, SITE, max(found.values())))
    assert max(found.values()) < 2 ** 26
    for (k, mant), idx in found.items():
        assert idx % 2 == 0
        assert nb.pair_words(SEED, SITE, 0, idx)[k] & nb.M23 == mant
    # the chained probe's two targets (site 3 + 16 * 2) and the DBM probe's clamp word (site 12)
    site = SITE + 16 * (nb.CHAIN_STEPS - 1)
    assert set(nb.find_words(SEED, site, 0, nb.CHAIN_TARGETS)) == set(nb.CHAIN_TARGETS)
    assert nb.find_words(SEED, nb.SITE_DBM_V, 0, (nb.CLAMP,))[nb.CLAMP] < 2 ** 26


def test_draws_at_the_edge_pairs(found):
    worst = 0.0
    for tgt, idx in sorted(found.items()):
        x0, x1 = nb.pair_words(SEED, SITE, 0, idx)
        n0, n1 = orc.box_muller_words([x0], [x1])
        ref = nb.box_muller64([x0], [x1])
        err = max(abs(float(n0[0]) - ref['n0'][0]), abs(float(n1[0]) - ref['n1'][0]))
        assert err < nb.DRAW_ATOL, (tgt, idx, err)
        worst = max(worst, err)
        nb.assert_bits(orc.normal(SEED, SITE, 0, 2, idx0=idx), np.float32([n0[0], n1[0]]), 'orc.normal at %r' % (tgt,))
    print('edge pairs: worst draw %.3e from float64 (bound %.3e)' % (worst, nb.DRAW_ATOL))


def test_draws_of_a_bulk_of_the_stream():
    n = 2 ** 22
    got = orc.normal(SEED, SITE, 0, n)
    worst = nb.assert_draws(got, SEED, SITE, n, 0, 'orc.normal, 2^22 consecutive draws')
    print('bulk: worst draw %.3e from float64 (bound %.3e)' % (worst, nb.DRAW_ATOL))


def test_draws_of_every_edge_radius_with_every_edge_angle():
    """the cross product of the first-word and second-word targets - with the nine high bits of the words set and clear:
    only the mantissa may count"""
    for high in (0, 0xff800000, 0xaa800000):
        x0, x1 = np.meshgrid(np.uint32(nb.FIRST) | np.uint32(high), np.uint32(nb.SECOND) | np.uint32(high), indexing='ij')
        n0, n1 = orc.box_muller_words(x0, x1)
        ref = nb.box_muller64(x0, x1)
        err = np.maximum(np.abs(n0 - ref['n0']), np.abs(n1 - ref['n1']))
        assert err.max() < nb.DRAW_ATOL, (high, float(err.max()), np.argwhere(err == err.max())[0])
        if high:
            nb.assert_bits(n0, base[0], 'high bits %#x' % high)
            nb.assert_bits(n1, base[1], 'high bits %#x' % high)
        else:
            base = (n0, n1)


# ---- c. exact identities at the edges
def test_exact_values_at_the_quadrant_boundaries_and_the_clamp():
    sn, cs = orc.pin_sincos_2pi(nb.unit([0, 0x200000, 0x400000, 0x600000]))
    assert np.array_equal(sn, np.float32([0, 1, 0, -1])) and np.array_equal(cs, np.float32([1, 0, -1, 0]))
    assert not np.signbit(sn[0]) and not np.signbit(cs[3])          # (+0, 1) and (-1, +0); the other two zeros are -0
    assert np.signbit(cs[1]) and np.signbit(sn[2])
    r_clamp = np.sqrt(np.float32(-2.0) * orc.pin_log_unit(np.float32([1e-7])))[0]
    assert abs(float(r_clamp) - 5.6777) < 1e-4
    n0, n1 = orc.box_muller_words([0, 0], [0x200000, 0])            # the clamp word with sin = 1, then with cos = 1
    assert n0[0] == r_clamp and n1[1] == r_clamp and n1[0] == 0 and n0[1] == 0
    assert nb.bits(n0)[0] == nb.bits(r_clamp)
    # the first unclamped value is larger than the clamp: a smaller radius
    assert nb.unit([1])[0] > nb.EPS and orc.box_muller_words([1], [0x200000])[0][0] < r_clamp
    # the smallest radius: u1 = 1 - 2^-23
    r_min = orc.box_muller_words([0x7fffff], [0x200000])[0][0]
    assert r_min == pytest.approx(np.sqrt(2.0 * 2.0 ** -23), rel=1e-6)


@pytest.mark.parametrize('idx0', [0, 1, 2, 3, 4093, 57981372, 57981373])
def test_pair_and_sin_cos_selection(idx0):
    """orc.normal picks word pair (idx & 3) >> 1 of block idx >> 2 and sin for an even, cos for an odd element"""
    n = 64
    got = orc.normal(SEED, SITE, 0, n, idx0=idx0)
    b0 = idx0 // 4
    w = orc.philox_words(SEED, SITE, 0, b0, (idx0 + n + 3) // 4 - b0).reshape(-1, 2)
    n0, n1 = orc.box_muller_words(w[:, 0], w[:, 1])
    want = np.stack([n0, n1], axis=1).reshape(-1)[idx0 - 4 * b0:][:n]
    nb.assert_bits(got, want, 'orc.normal from element %d' % idx0)


# ---- d. the bit comparison of the GPU file can fail
def test_a_libm_restatement_differs_bitwise():
    from boltzmann_machines_amd.utils import philox
    n = 2 ** 22
    libm = philox.normal(SEED, SITE, 0, n)
    pinned = orc.normal(SEED, SITE, 0, n)
    differ = nb.bits(libm) != nb.bits(pinned)
    print('numpy-libm Box-Muller against the pinned one: %.1f %% of 2^22 draws differ bitwise, max |diff| %.3e'
          % (100.0 * differ.mean(), np.abs(libm - pinned).max()))
    assert differ.any()
    assert np.abs(libm - pinned).max() < 2 * nb.DRAW_ATOL            # (both are within DRAW_ATOL-ish of the real value)


# ---- e. the twin at the offsets the GPU file uses
@pytest.mark.parametrize('V', [64, 37])
def test_twin_returns_the_raw_draws_at_every_edge_pair(found, V):
    for tgt, idx in sorted(found.items()):
        row0, B = nb.rows_for(idx, V)
        assert row0 * V <= idx and idx + 1 < (row0 + B) * V
        Vt = nb.twin_gibbs(V, B, row0)
        assert np.array_equal(Vt.reshape(-1), orc.normal(SEED, SITE, 0, B * V, idx0=row0 * V)), tgt      # == : -0 * 1 + 0 = +0
    idx = found[nb.CLAMP]
    row0, B = nb.rows_for(idx, V)
    nb.check_clamp_pair(nb.twin_gibbs(V, B, row0), SEED, SITE, idx, row0)


def test_twin_at_the_later_sites_of_a_chained_run():
    V, H, B = nb.CHAIN_SHAPE
    site = SITE + 16 * (nb.CHAIN_STEPS - 1)
    for tgt, idx in sorted(nb.find_words(SEED, site, 0, nb.CHAIN_TARGETS).items()):
        row0 = idx // V - 1
        Vt = nb.twin_gibbs(V, B, row0, n_steps=nb.CHAIN_STEPS, H=H)
        nb.assert_draws(Vt, SEED, site, B * V, row0 * V, 'twin, three steps, %r' % (tgt,))


@pytest.mark.parametrize('V,row0', nb.CARRY)
def test_twin_across_the_block_counter_carry(V, row0):
    assert (row0 + 1) * V in (2 ** 34 - 4, 2 ** 34)
    Vt = nb.twin_gibbs(V, 3, row0)
    nb.assert_draws(Vt, SEED, SITE, 3 * V, row0 * V, 'twin across block 2^32')
    # the words really come from a counter whose high word is 1, not from a wrapped one
    off = 2 ** 34 - row0 * V
    assert not np.array_equal(Vt.reshape(-1)[off:], orc.normal(SEED, SITE, 0, 3 * V - off, idx0=0))
    Bt = nb.twin_gibbs(V, 3, row0, v_unit=0)
    assert np.array_equal(Bt.reshape(-1), (orc.uniform(SEED, SITE, 0, 3 * V, idx0=row0 * V) < 0.5).astype(np.float32))


def test_two_roundings_case_can_tell_a_contracted_fma():
    sigma, vb, n, want, fused = nb.two_roundings_case()
    assert np.sum(nb.bits(want) != nb.bits(fused)) > 100
    B, V = n.shape
    nb.assert_bits(nb.twin_gibbs(V, B, 3, sigma=sigma, vb=vb), want, 'twin against float32(float32(n * sigma) + vb)')


@pytest.mark.parametrize('V', [64, 37])
@pytest.mark.parametrize('H', nb.DBM_HIDDEN)
def test_dbm_twin_keeps_the_sampled_visible_layer_in_v_new(V, H):
    idx = nb.find_words(SEED, nb.SITE_DBM_V, 0, (nb.CLAMP,))[nb.CLAMP]
    p0 = idx // V - 1
    twin, v = nb.dbm_twin(V, H, p0)
    sigma, vb = nb.dbm_case(V)
    nb.assert_bits(v, np.tile(vb, (3, 1)), 'sample_v: the means of the mean sweep')
    n = orc.normal(SEED, nb.SITE_DBM_V, 0, 3 * V, idx0=p0 * V).reshape(3, V)
    nb.assert_bits(twin.p['v_new'], ((n * sigma[None, :]).astype(np.float32) + vb[None, :]).astype(np.float32), 'v_new')
    nb.check_dbm_draws(twin.p['v_new'], V, p0, 'DBM twin')


def test_dbm_twin_across_the_block_counter_carry():
    V, p0 = nb.CARRY[0]
    for H in nb.DBM_HIDDEN:
        twin, _ = nb.dbm_twin(V, H, p0)
        nb.check_dbm_draws(twin.p['v_new'], V, p0, 'DBM twin across block 2^32')
