"""Centred training (the centering trick): the Python side shared by BernoulliRBM and DBM.

Montavon & Mueller 2012, "Deep Boltzmann Machines and the Centering Trick"; Melchior, Fischer & Wiskott 2016, "How to
Center Deep Boltzmann Machines".  The model stays in standard parameters (W, vb, hb); the engine's update takes the gradient
between units minus running offsets (bm_rbm_set_centering / bm_dbm_set_centering, include/bm355.h).  The offsets are
optimiser state, like the momentum buffers: they live on the engine as the variables 'ov', 'oh', 'oh_1', ... and go into
model.npz - `centering_ov`, `centering_oh[_i]`, `centering_nu` - only while the mode is on.  Neither the setting nor the
sliding factors are constructor keywords: params.json keeps the reference's schema.
"""
import os

import numpy as np


class CenteredTraining(object):
    """`self._centering` is None (plain updates) or dict(nu=[one sliding factor per layer, visible first],
    offsets=[per layer: None = the default at the next fit(), an array = waiting for the engine, True = on the engine])."""
    _centering = None

    # ---- supplied by the model class
    def _centering_sizes(self):
        """units per layer, visible first"""
        raise NotImplementedError

    def _check_centering(self, what):
        """raise NotImplementedError where the model as configured has no centred update"""
        raise NotImplementedError

    def _engine_set_centering(self, on, nus):
        raise NotImplementedError

    # ---- shared
    @staticmethod
    def _centering_engine_names(n_layers):
        return ['ov'] + ['oh' + ('' if i == 0 else '_%d' % i) for i in range(n_layers - 1)]

    def _check_centering_common(self, what):
        name = '%s.%s' % (self.__class__.__name__, what)
        if np.dtype(self.dtype) != np.float32:
            raise NotImplementedError("%s: centering runs in float32 only (the float64 engines have no centred update; dtype=%r)"
                                      % (name, self.dtype))
        if os.environ.get('BM355_DATA_PARALLEL', '0') == '1' or getattr(self, '_dp', None) is not None:
            raise NotImplementedError('%s: centering is not combined with data parallelism (BM355_DATA_PARALLEL): the split '
                                      'and exchange steps have no centred form' % name)
        return name

    def _set_centering(self, enabled, nus, offsets):
        if not enabled:             # (always possible: also on a model that could not be centred)
            was, self._centering = self._centering, None
            if was is not None and self._engine is not None:
                self._engine_set_centering(False, was['nu'])
            return self
        self._check_centering('set_centering')
        sizes = self._centering_sizes()
        nus = [float(x) for x in nus]
        if len(nus) != len(sizes) or not all(0. <= x <= 1. for x in nus):
            raise ValueError('centering: {0} sliding factors in [0, 1] are needed (got {1!r})'.format(len(sizes), nus))
        offsets = list(offsets) if offsets is not None else [None] * len(sizes)
        if len(offsets) != len(sizes):
            raise ValueError('centering: {0} offset vectors are needed (got {1})'.format(len(sizes), len(offsets)))
        for l, n in enumerate(sizes):
            if offsets[l] is not None:
                offsets[l] = np.ascontiguousarray(np.broadcast_to(np.asarray(offsets[l], dtype=np.float32), (n,)))
        self._centering = dict(nu=nus, offsets=offsets)
        if self._engine is not None:
            self._apply_centering()
        return self

    def _apply_centering(self):
        """the engine exists: switch its mode on and hand over the offsets that wait for it"""
        c = self._centering
        if c is None:
            return
        self._check_centering('fit')
        self._engine_set_centering(True, c['nu'])
        for l, name in enumerate(self._centering_engine_names(len(c['nu']))):
            if isinstance(c['offsets'][l], np.ndarray):
                self._engine.set(name, c['offsets'][l])
                c['offsets'][l] = True

    def _centering_begin_fit(self, X):
        """the defaults of offsets left at None: the data mean (in float64 over the X of this fit) for the visible layer, 0.5
        for every hidden one"""
        c = self._centering
        if c is None:
            return
        self._apply_centering()
        for l, name in enumerate(self._centering_engine_names(len(c['nu']))):
            if c['offsets'][l] is None:
                o = np.asarray(X, dtype=np.float64).mean(axis=0).astype(np.float32) if l == 0 else np.float32(0.5)
                self._engine.set(name, o)
                c['offsets'][l] = True

    def centering_offsets(self):
        """the offsets, visible layer first: a list of float32 vectors (None for a layer whose offset is still the default of
        the next fit()); None while centering is off"""
        c = self._centering
        if c is None:
            return None
        out = []
        for l, name in enumerate(self._centering_engine_names(len(c['nu']))):
            o = c['offsets'][l]
            if o is True:
                o = self._engine.get(name)
            out.append(None if o is None else np.array(o, dtype=np.float32))
        return out

    # ---- checkpoints
    def _centering_variables(self):
        """what model.npz additionally holds while centering is on"""
        c = self._centering
        if c is None:
            return {}
        out = dict(centering_nu=np.asarray(c['nu'], dtype=np.float32))
        for name, o in zip(self._centering_engine_names(len(c['nu'])), self.centering_offsets()):
            if o is not None:
                out['centering_' + name] = o
        return out

    def _centering_restore(self, d):
        """load_model only: `d` holds the arrays of a checkpoint.  Re-enables the mode where they hold it and TAKES the
        centering_* arrays out of `d`, so that the later upload of `d` to the engine cannot undo what the caller sets in
        between (set_centering(False), another nu, other offsets)"""
        keys = [k for k in d if k.startswith('centering_')]
        taken = {k: d.pop(k) for k in keys}
        if 'centering_nu' not in taken:
            return
        nus = [float(x) for x in np.asarray(taken['centering_nu']).ravel()]
        offsets = [taken.get('centering_' + name) for name in self._centering_engine_names(len(nus))]
        self._set_centering(True, nus, offsets)

    def _centering_detach(self):
        """the engine is about to be closed (a rebuild after set_params): take the offsets it holds back to the host; the
        next engine receives them from _apply_centering"""
        c = self._centering
        if c is None or self._engine is None:
            return
        for l, name in enumerate(self._centering_engine_names(len(c['nu']))):
            if c['offsets'][l] is True:
                c['offsets'][l] = np.array(self._engine.get(name), dtype=np.float32)
