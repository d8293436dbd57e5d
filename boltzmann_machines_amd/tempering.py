"""Parallel tempering, the host side that BernoulliRBM and DBM share: the ladder, the acceptance rates,
the tempered sampler over an engine's `pt_init / pt_sweep / pt_read` and the bookkeeping of a tempered negative phase.
Everything that touches the device goes through the engine (engine.py: _PtCalls)."""
import numpy as np

from . import _ffi


def resolve_ladder(n_temperatures, betas):
    """the ladder as float32 [R]: `betas`, or float32(linspace(0, 1, n_temperatures + 1)[1:]) where it is None"""
    if betas is None:
        if int(n_temperatures) < 1:
            raise ValueError('`n_temperatures` must be >= 1 (got {0})'.format(n_temperatures))
        betas = np.linspace(0., 1., int(n_temperatures) + 1)[1:]
    betas = np.asarray(betas, dtype=np.float32).ravel()
    if len(betas) < 1 or betas[-1] != 1. or betas[0] <= 0. or np.any(np.diff(betas) <= 0.):
        raise ValueError('`betas` must increase strictly inside (0, 1] and end at 1 (got {0})'.format(betas))
    return betas


def acceptance_rates(swaps):
    """accepts / attempts per ladder pair from pt_read's counters [2, R - 1]; 0 where a pair was never attempted"""
    return swaps[1] / np.maximum(swaps[0], 1).astype(np.float64)


def run_tempered_sampler(eng, n_samples, n_gibbs_steps, betas, V_init, n_visible, return_stats, **init_kwargs):
    """a fresh ensemble of n_samples chains on `eng` (it replaces the ensemble of a tempered negative phase: _pt_train_key),
    n_gibbs_steps tempered steps, the visible states of the beta = 1 replicas [n_samples, n_visible] (and the acceptance rates);
    init_kwargs: what the engine's pt_init takes besides (the chains' `lengths` of a count ensemble)"""
    V0d = None
    if V_init is not None:
        V_init = np.ascontiguousarray(V_init, dtype=np.float32)
        if V_init.shape != (n_samples, n_visible):
            raise ValueError('`V_init` has invalid shape {0}: expected [{1}, {2}]'.format(V_init.shape, n_samples, n_visible))
        V0d = _ffi.DeviceArray.from_numpy(V_init, np.float32)
    eng.pt_init(n_samples, betas, V0d, **init_kwargs)
    eng.pt_sweep(int(n_gibbs_steps))
    Vd = _ffi.DeviceArray((n_samples, n_visible), np.float32)
    swaps, _ = eng.pt_read(Vd)
    V = Vd.numpy()
    if return_stats:
        return V, acceptance_rates(swaps)
    return V


class TemperedNegativePhase(object):
    """The training side: `self._neg_phase` is None (the model's default negative phase) or (betas, n_chains) of the tempered
    ensemble.  A model class names the attribute that bounds n_chains from below and supplies `_check_tempered_setting`."""
    _PT_MIN_CHAINS = None                         # 'batch_size' / 'n_particles'
    _PT_VIEW = None                               # the engine attribute that holds the ensemble's calls; None: the engine itself
    _PT_SETTER = "set_negative_phase('tempered')"  # what switches the tempered negative phase on, for messages

    def _check_tempered_setting(self, what):
        """raise where the model as configured has no tempered negative phase (`what`: the calling method's name)"""
        raise NotImplementedError

    def _set_negative_phase(self, kind, n_temperatures, betas, n_chains):
        if kind == 'cd':
            self._neg_phase = None
            return self
        if kind != 'tempered':
            raise ValueError("`kind` must be 'cd' or 'tempered' (got {0!r})".format(kind))
        self._check_tempered_setting('set_negative_phase')
        betas = resolve_ladder(n_temperatures, betas)
        least = getattr(self, self._PT_MIN_CHAINS)
        n_chains = least if n_chains is None else int(n_chains)
        if n_chains < least:
            raise ValueError('`n_chains` must be >= {0} (got {1} < {2})'.format(self._PT_MIN_CHAINS, n_chains, least))
        self._neg_phase = (tuple(float(b) for b in betas), n_chains)
        return self

    def _ensure_train_ensemble(self, eng):
        """build the ensemble where this fit() call has none yet or the ladder / n_chains changed (random start under the call's
        seed: no host seed is drawn)"""
        betas, n_chains = self._neg_phase
        if getattr(self, '_pt_fresh', True) or getattr(eng, '_pt_train_key', None) != self._neg_phase:
            eng.pt_init(n_chains, betas)
            eng._pt_train_key = self._neg_phase
            self._pt_fresh = False

    def tempering_stats(self):
        """Acceptance rate (accepts / attempts) of every neighbouring pair of temperatures, [n_temperatures - 1], since the
        ensemble of the tempered negative phase was built.  Waits for the device; copies no states."""
        eng = self._engine
        if self._PT_VIEW is not None:
            eng = getattr(eng, self._PT_VIEW, None) if eng is not None else None
        if getattr(eng, '_pt_train_key', None) is None:   # (no engine, a float64 engine, or an ensemble that sampling built)
            raise RuntimeError('`tempering_stats`: no tempered ensemble (call %s and fit first)' % self._PT_SETTER)
        swaps, _ = eng.pt_read()
        return acceptance_rates(swaps)
