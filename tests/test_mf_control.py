"""The mean-field loop-control cases (tests/mf_control_cases.py), the part that needs no GPU: every case that
tests/test_mf_control_gpu.py runs is shown to have a trip count that the float32 oracle and a float64 restatement of
dbm.py:429-478 agree on, that no last bit can move, and that ONE tile of ONE layer decides - and the list is shown to put that
tile where the kernels' slot arithmetic can go wrong."""
import numpy as np
import pytest

from tests import mf_control_cases as K
from tests.np_reference import NumpyDBM

ALL = K.CASES + K.OVER_CASES
IDS = [K.case_id(k) for k in ALL]


def test_float64_restatement_is_the_numpy_reference():
    """mf_trace keeps the residuals; NumpyDBM.mean_field (the suite's float64 dbm.py:429-478) gives the same count and mu"""
    c = K.case(K.CASES[-1])
    L, N = c['L'], c['shape']['N']
    P = {k: np.asarray(v, np.float64) for k, v in c['P'].items()}
    for i, n in enumerate(c['shape']['n']):
        P['mu' + K.sfx(i)] = np.full((N, n), 0.5)
    ref = NumpyDBM(P, L, N, N, max_mf=K.MAX_MF, mf_tol=K.MF_TOL)
    T = ref.mean_field(np.asarray(c['X'][0], np.float64))
    assert T == c['ref'][0]['T']
    for i in range(L):
        assert np.abs(ref.P['mu' + K.sfx(i)] - c['ref'][0]['mu'][i]).max() < 1e-12      # (two spellings of the float64 sigmoid)


@pytest.mark.parametrize('key', ALL, ids=IDS)
def test_reference_agreement_and_robustness(key):
    c = K.case(key)
    for call in (0, 1):
        ref = c['ref'][call]
        print('%s call %d: T %d, residuals %s, margin %.3g' % (K.case_id(key), call, ref['T'], ' '.join('%.3g' % x for x in ref['resid']),
                                                              ref['margin']))
        for literal in (False, True):
            assert c['oracle'][literal]['T'][call] == ref['T'], (call, literal, c['oracle'][literal]['T'], ref['T'])
        assert ref['T'] < K.MAX_MF
        assert ref['margin'] > K.MARGIN >= 1e-3
        # float32 against float64: the oracle's mu is the reference's to round-off (the bit comparisons on the device are
        # against the oracle; this says the oracle computes the right thing)
        for i, k in enumerate(K.names(c['L'])):
            assert np.abs(c['oracle'][False]['mu'][call][k] - ref['mu'][i]).max() < 2e-5


@pytest.mark.parametrize('key', ALL, ids=IDS)
def test_one_tile_decides(key):
    """without the planted element's tile - 32 x 32 of the narrow kernel, 32 units x 64 rows of the wide one - the loop of the
    first call ends at least 3 sweeps early"""
    ref = K.case(key)['ref'][0]
    print('%s: T %d, without the narrow tile %d, without the wide tile %d' % (K.case_id(key), ref['T'], ref['T_narrow'], ref['T_wide']))
    assert 5 <= ref['T'] < K.MAX_MF
    assert ref['T_narrow'] <= ref['T'] - K.GAP and ref['T_wide'] <= ref['T'] - K.GAP


def test_placement_covers_the_tile_grid():
    layers = sorted({p for _, p, _, _ in K.CASES})
    assert layers == [0, 1, 2, 3]
    for p in layers:
        for tile in (K.NARROW, K.WIDE):
            seen = set()
            for shape, q, u, r in K.CASES:
                if q != p:
                    continue
                n, N = shape['n'][p], shape['N']
                assert n % tile[0] and N % tile[1]                   # both directions end in a ragged tile
                tu, tr = K.tile_of(u, r, tile)
                seen.add((tu == 0, tu == (n - 1) // tile[0], tr == 0, tr == (N - 1) // tile[1]))
            for want in ((True, False, True, False), (False, True, True, False), (True, False, False, True), (False, True, False, True)):
                assert want in seen, (p, tile, want)
    # a workgroup index >= 4 within a layer, whatever order the tile map takes: a layer with more than 4 tiles is planted
    # in its last tile both ways and in its first
    assert any(((s['n'][p] + 31) // 32) * ((s['N'] + 31) // 32) > 4 for s, p, _, _ in K.CASES)
    # K tails in both segments of the h1 pass, more than one workgroup per pass for both kernels
    for shape in (K.TWO, K.FOUR):
        assert shape['V'] % 16 and shape['n'][1] % 16 and shape['N'] > 64


def test_oversize_shape_is_past_the_self_control_rule():
    s = K.OVER
    assert ((s['n'][0] + 31) // 32) * ((s['N'] + 31) // 32) > 1024                   # mf_self_ctl() is false, the narrow h1 pass takes atomicMax
    assert ((s['n'][0] + 31) // 32) * ((s['N'] + 63) // 64) <= 1024                  # the wide h1 pass writes slots
    rows = sorted(K.tile_of(u, r, K.NARROW)[1] for _, _, u, r in K.OVER_CASES)
    assert rows[0] == 0 and rows[-1] == (s['N'] - 1) // 32


def test_driver_sequence_is_what_it_intends():
    """every call of the boundary sequence: the oracle's count is the intended one, the float64 run from the same start agrees
    and stays clear of the tolerance; the sequence holds every boundary of the group arithmetic (first group pred + 1 or 8,
    follow-up groups of 4, verdicts read one group late)"""
    runs = K.driver_oracle()
    L, cap = len(K.DRIVER['shape']['n']), K.DRIVER['max_mf']
    pred, unprimed, seen = None, True, set()
    for (x, want), run in zip(K.DRIVER_CALLS, runs):
        assert run['T'] == want < cap, (x, want, run['T'])
        res, states, init = K.mf_trace(run['P'], L, run['X'], [run['start'][k] for k in K.names(L)], cap)
        T64 = K.trip_count(res, K.MF_TOL, cap)
        assert T64 == want and K.margin(res, K.MF_TOL, T64) > K.MARGIN, (x, want, T64, K.margin(res, K.MF_TOL, T64))
        if run['aside']:
            pred, unprimed = run['aside'][1], run['aside'][1] == 0
        if x is None:
            assert want == 0 and K.resid_max(res[0]) < 1e-6 and all(np.array_equal(run['mu'][k], run['preset'][k]) for k in run['mu'])
            seen.add('zero')
        elif unprimed:
            seen.add('unprimed %d' % want)
        elif pred is not None:
            seen.add({0: 'pred', 1: 'pred + 1', 2: 'pred + 2'}.get(want - pred, 'far below' if want <= pred - 8 else 'other'))
        seen.add('odd' if want & 1 else 'even')
        pred, unprimed = want, want == 0
    assert runs[K.DRIVER_TRAIN_AFTER]['aside'] is not None
    assert seen >= {'pred + 1', 'pred', 'pred + 2', 'far below', 'unprimed 8', 'unprimed 9', 'unprimed 12', 'unprimed 13', 'odd', 'even', 'zero'}, seen


def test_capped_handles():
    T = K.case(K.CASES[0])['ref'][0]['T']
    for cap in K.CAPS:
        c = K.capped(cap)
        assert cap < T and c['T'] == cap
        assert c['resid'] > K.MF_TOL * (1 + K.MARGIN)             # the loop stops at the cap with the residual still above
    assert 0 in K.CAPS and 1 in K.CAPS
