"""The host side of parallel tempering that BernoulliRBM and DBM share (boltzmann_machines_amd/tempering.py): the ladder and
the acceptance rates.  No GPU."""
import warnings

import numpy as np
import pytest

from boltzmann_machines_amd.tempering import acceptance_rates, resolve_ladder


@pytest.mark.parametrize('n', [1, 2, 10])
def test_default_ladder_is_the_float32_linspace(n):
    betas = resolve_ladder(n, None)
    want = np.float32(np.linspace(0, 1, n + 1)[1:])
    assert betas.dtype == np.float32 and betas.shape == (n,)
    assert np.array_equal(betas.view(np.uint32), want.view(np.uint32))
    assert betas[-1].view(np.uint32) == np.float32(1.0).view(np.uint32)
    if n == 1:
        assert betas.tolist() == [1.]


def test_a_given_ladder_is_kept_as_float32():
    betas = resolve_ladder(10, [[0.25, 0.5], [0.75, 1.0]])     # (n_temperatures is not read; any shape is flattened)
    assert betas.dtype == np.float32 and betas.tolist() == [0.25, 0.5, 0.75, 1.0]


def test_no_temperatures_is_refused():
    with pytest.raises(ValueError, match='`n_temperatures` must be >= 1'):
        resolve_ladder(0, None)


@pytest.mark.parametrize('betas', [
    [],                       # empty
    [0.25, 0.5],              # does not end at 1
    [0.5, 0.5, 1.0],          # a repeated value
    [0.75, 0.5, 1.0],         # a decreasing value
    [0.0, 0.5, 1.0],          # a value <= 0
    [-0.5, 0.5, 1.0],
], ids=['empty', 'no_one', 'repeated', 'decreasing', 'zero', 'negative'])
def test_bad_ladders_are_refused(betas):
    with pytest.raises(ValueError, match=r'`betas` must increase strictly inside \(0, 1\] and end at 1'):
        resolve_ladder(3, betas)


def test_acceptance_of_a_pair_never_attempted_is_zero():
    swaps = np.array([[4, 0, 10], [1, 0, 10]], dtype=np.int64)   # [2, R - 1]: attempts, accepts
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        rates = acceptance_rates(swaps)
    assert rates.dtype == np.float64 and rates.tolist() == [0.25, 0.0, 1.0]
    assert not np.isnan(rates).any()
