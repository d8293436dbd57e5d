"""BernoulliRBM / GaussianRBM with the reference's sklearn-like API on the MI355X engine.

Drop-in for boltzmann_machines/rbm/{base_rbm,rbm}.py of the reference:
same constructor keywords (base_rbm.py:95-105, rbm.py:88-99), `fit`, `init`,
`transform`, `get_tf_params`, `init_from`, `load_model`, `get_params`/
`set_params`, attributes `epoch_`, `iter_`; same schedules (1-based epoch index,
base_rbm.py:535-541), metric cadence (:549-571), validation metrics (:573-590),
free-energy gap (:592-621) and per-epoch checkpoint (:665-666).  The TF graph
of `_make_train_op` (:415-525) is executed by libbm355 (csrc/bm_rbm.hip).

BernoulliRBM, MultinomialRBM (rbm.py:25-65) and GaussianRBM (rbm.py:68-116) in float32 and float64.
"""
import os
import sys
from functools import wraps

import numpy as np

from . import _ffi
from .base import EngineModel, is_attribute_name, run_on_engine
from .centering import CenteredTraining
from .classification import ClassHead
from .engine import RbmEngine, RbmEngine64
from .tempering import TemperedNegativePhase, resolve_ladder, run_tempered_sampler
from .utils import epoch_iter, make_list_from, write_during_training
from .utils import log_sum_exp, log_mean_exp, log_diff_exp, log_std_exp
from .utils import philox


def assert_shape(obj, name, desired_shape):
    actual_shape = getattr(obj, name).shape
    if actual_shape != desired_shape:
        raise ValueError('`{0}` has invalid shape {1} != {2}'.format(name, actual_shape, desired_shape))


def assert_len(obj, name, desired_len):
    actual_len = len(getattr(obj, name))
    if actual_len != desired_len:
        raise ValueError('`{0}` has invalid len {1} != {2}'.format(name, actual_len, desired_len))


def single_joint_only(f):
    """`log_Z` / `log_proba` are about the joint p(v, h) of ONE Bernoulli-Bernoulli RBM in float32: every other model is
    refused before anything is touched (no seed drawn, no engine built)."""
    @wraps(f)
    def checked(model, *args, **kwargs):
        model._check_single_joint(f.__name__)
        return f(model, *args, **kwargs)
    return checked


def clampable_only(f):
    """`sample_v_given` needs the clamped epilogue of the float32 engine: other models are refused before anything is touched"""
    @wraps(f)
    def checked(model, *args, **kwargs):
        model._check_clampable(f.__name__)
        return f(model, *args, **kwargs)
    return checked


class BaseRBM(CenteredTraining, ClassHead, TemperedNegativePhase, EngineModel):
    """Restricted Boltzmann machine trained with CD-k (reference base_rbm.py:14-94)."""

    _V_UNIT = _ffi.UNIT_BERNOULLI
    _H_UNIT = _ffi.UNIT_BERNOULLI
    _V_GROUP_WIDTH = 0           # softmax visible units (CategoricalRBM): the width of a one-hot group; 0: none
    _RSM_MAX_LENGTH = 0          # replicated softmax visible units (ReplicatedSoftmaxRBM): the longest document; 0: none

    def __init__(self,
                 n_visible=784, v_layer_cls=None, v_layer_params=None,
                 n_hidden=256, h_layer_cls=None, h_layer_params=None,
                 W_init=0.01, vb_init=0., hb_init=0., n_gibbs_steps=1,
                 learning_rate=0.01, momentum=0.9, max_epoch=10, batch_size=10, l2=1e-4,
                 sample_v_states=False, sample_h_states=True, dropout=None,
                 sparsity_target=0.1, sparsity_cost=0., sparsity_damping=0.9,
                 dbm_first=False, dbm_last=False,
                 metrics_config=None, verbose=True, save_after_each_epoch=True,
                 display_filters=0, display_hidden_activations=0, v_shape=(28, 28),
                 model_path='rbm_model/', *args, **kwargs):
        # (`n_classes` is no keyword of the reference: params.json carries it while a class head is attached, and load_model hands
        #  it back here; the head itself is re-attached from model.npz, ClassHead._class_restore)
        kwargs.pop('n_classes', None)
        super(BaseRBM, self).__init__(model_path=model_path, *args, **kwargs)
        self.n_visible = n_visible
        self.n_hidden = n_hidden

        self.W_init = W_init
        if hasattr(self.W_init, '__iter__'):
            self.W_init = np.asarray(self.W_init)
            assert_shape(self, 'W_init', (self.n_visible, self.n_hidden))
        self.vb_init = vb_init
        if hasattr(self.vb_init, '__iter__'):
            self.vb_init = np.asarray(self.vb_init)
            assert_len(self, 'vb_init', self.n_visible)
        self.hb_init = hb_init
        if hasattr(self.hb_init, '__iter__'):
            self.hb_init = np.asarray(self.hb_init)
            assert_len(self, 'hb_init', self.n_hidden)

        # these can be set by `init_from`
        self._dW_init = None
        self._dvb_init = None
        self._dhb_init = None

        self.n_gibbs_steps = make_list_from(n_gibbs_steps)
        self.learning_rate = make_list_from(learning_rate)
        self.momentum = make_list_from(momentum)
        self.max_epoch = max_epoch
        self.batch_size = batch_size
        self.l2 = l2

        self.sample_h_states = sample_h_states
        self.sample_v_states = sample_v_states
        self.dropout = dropout

        self.sparsity_target = sparsity_target
        self.sparsity_cost = sparsity_cost
        self.sparsity_damping = sparsity_damping

        self.dbm_first = dbm_first
        self.dbm_last = dbm_last

        self.metrics_config = metrics_config or {}
        self.metrics_config.setdefault('l2_loss', False)
        self.metrics_config.setdefault('msre', False)
        self.metrics_config.setdefault('pll', False)
        self.metrics_config.setdefault('feg', False)
        self.metrics_config.setdefault('l2_loss_fmt', '.2e')
        self.metrics_config.setdefault('msre_fmt', '.4f')
        self.metrics_config.setdefault('pll_fmt', '.3f')
        self.metrics_config.setdefault('feg_fmt', '.2f')
        self.metrics_config.setdefault('train_metrics_every_iter', 10)
        self.metrics_config.setdefault('val_metrics_every_epoch', 1)
        self.metrics_config.setdefault('feg_every_epoch', 2)
        self.metrics_config.setdefault('n_batches_for_feg', 10)
        self._train_metrics_names = ('l2_loss', 'msre', 'pll')
        self._val_metrics_names = ('msre', 'pll')

        self.verbose = verbose
        self.save_after_each_epoch = save_after_each_epoch

        assert self.n_hidden >= display_filters
        self.display_filters = display_filters
        assert self.n_hidden >= display_hidden_activations
        self.display_hidden_activations = display_hidden_activations
        self.v_shape = v_shape
        if len(self.v_shape) == 2:
            self.v_shape = (self.v_shape[0], self.v_shape[1], 1)

        # current epoch and iteration
        self.epoch_ = 0
        self.iter_ = 0

        # the negative phase of fit(): None = CD-k from the batch, else (betas, n_chains) of the tempered ensemble
        # (set_negative_phase; not a constructor keyword and not written to checkpoints)
        self._neg_phase = None
        # fast weights of the tempered negative phase: None or (fast_learning_rate, fast_decay) (set_negative_phase; as _neg_phase)
        self._fast_weights = None

    # ---- variables -----------------------------------------------------------------
    def _sigma_vector(self):
        return np.ones(self.n_visible, dtype=self._np_dtype)

    def _initial_variables(self):
        """The initialisers of `_make_vars` (reference base_rbm.py:271-327).

        W ~ tf.random_normal(stddev=W_init, seed=random_seed): with the graph seed of
        the enclosing public call when there is one (`fit`), else TF's
        DEFAULT_GRAPH_SEED (`init()`; pinned by rbm/tests/test_rbm.py:64-67)."""
        dt = self._np_dtype
        V, H = self.n_visible, self.n_hidden
        if hasattr(self.W_init, '__iter__'):
            W = np.asarray(self.W_init, dtype=dt)
        else:
            op_seed = self.random_seed
            if op_seed is None:      # TF: non-deterministic when no seed is given
                op_seed = int(np.random.randint(2 ** 31 - 1))
            graph_seed = self._graph_seed if self._graph_seed is not None else philox.DEFAULT_GRAPH_SEED
            W = (philox.normal(graph_seed, int(op_seed) & 0xFFFFFFFF, (int(op_seed) >> 32) & 0xFFFFFFFF, V * H, dt)
                 * dt(self.W_init)).reshape(V, H).astype(dt)
        vb = np.asarray(self.vb_init, dtype=dt) if hasattr(self.vb_init, '__iter__') \
            else np.repeat(dt(self.vb_init), V)
        hb = np.asarray(self.hb_init, dtype=dt) if hasattr(self.hb_init, '__iter__') \
            else np.repeat(dt(self.hb_init), H)
        z = lambda a, shape: np.zeros(shape, dtype=dt) if a is None else np.asarray(a, dtype=dt).reshape(shape)
        return dict(W=W, vb=vb, hb=hb, dW=z(self._dW_init, (V, H)), dvb=z(self._dvb_init, (V,)),
                    dhb=z(self._dhb_init, (H,)), q_means=np.zeros(H, dtype=dt), sigma=self._sigma_vector())

    _VAR_SCOPES = (('W', 'weights'), ('vb', 'weights'), ('hb', 'weights'),
                   ('dW', 'grads_accumulators'), ('dvb', 'grads_accumulators'), ('dhb', 'grads_accumulators'),
                   ('q_means', 'hidden_activations_means'), ('sigma', 'input_data'))

    def _make_engine(self):
        variables = self._initial_variables()
        f64 = np.dtype(self.dtype) == np.float64
        if np.dtype(self.dtype) == np.float32 or f64:
            # (softmax visible units, CategoricalRBM: a property of the float32 handle)
            groups = {} if f64 or not self._V_GROUP_WIDTH else dict(v_groups=int(self._V_GROUP_WIDTH))
            if not f64 and self._RSM_MAX_LENGTH:      # (replicated softmax visible units: likewise)
                groups['rsm_max_length'] = int(self._RSM_MAX_LENGTH)
            self._engine = (RbmEngine64 if f64 else RbmEngine)(
                                     self.n_visible, self.n_hidden, v_unit=self._V_UNIT, **groups,
                                     sample_v_states=self.sample_v_states, sample_h_states=self.sample_h_states,
                                     dbm_first=self.dbm_first, dbm_last=self.dbm_last, max_batch=self.batch_size,
                                     l2=self.l2, sparsity_target=self.sparsity_target,
                                     sparsity_cost=self.sparsity_cost, sparsity_damping=self.sparsity_damping,
                                     dropout=self.dropout, h_unit=self._H_UNIT,
                                     n_samples=getattr(self, 'n_samples', 0))
            self._upload_variables(variables)
            # multi-GPU job (one process per GPU): data-parallel CD-k, rank r takes rows [r*batch_size, ...) of every
            # global minibatch of world*batch_size rows; ONE all-reduce(sum) of the fused [dW|dvb|dhb|q] buffer per
            # update through the library's communicator (parallel.DataParallelRBM)
            self._dp = None
            if getattr(self, '_comm', None) is not None and not f64:
                from . import parallel
                self._dp = parallel.DataParallelRBM(self._engine, self._rank, self._world, self.batch_size,
                                                    parallel.native_allreduce_on_engine_stream(self._engine, self._comm))
            self._apply_centering()
            self._apply_class_head()
        else:
            raise NotImplementedError("%s: dtype must be 'float32' or 'float64' (got %r)" % (self.__class__.__name__, self.dtype))

    def _needs_device(self):
        return False

    def _on_device(self):
        if not isinstance(self._engine, (RbmEngine, RbmEngine64)):
            raise NotImplementedError("no device path for %s with dtype='%s'" % (self.__class__.__name__, self.dtype))
        return self._engine

    def _to_device(self, X, slot=None):
        """host array -> DeviceArray in the engine's dtype; `slot` names a buffer of this model that is reused
        across calls (the training / validation set of repeated fit() calls)"""
        dt = self._engine.dtype
        if slot is None:
            return _ffi.DeviceArray.from_numpy(np.ascontiguousarray(X, dtype=dt), dt)
        pool = self.__dict__.setdefault('_dev_pool', {})
        pool[slot] = _ffi.DeviceArray.from_numpy_reusing(pool.get(slot), X, dt)
        return pool[slot]

    def _upload_variables(self, d):
        for name, _ in self._VAR_SCOPES:
            if name in d:
                self._engine.set(name, d[name])

    def _seed_engine(self, seed):
        if isinstance(self._engine, (RbmEngine, RbmEngine64)):
            self._engine.seed(seed)

    def _variables(self):
        out = {name: self._engine.get(name) for name, _ in self._VAR_SCOPES}
        out.update(self._centering_variables())       # (nothing unless centering is on)
        out.update(self._class_variables())           # (nothing unless a class head is attached)
        return out

    def _scoped_variables(self):
        # the reference's variable names (base_rbm.py:271-327); `sigma` is a variable of the GaussianRBM only, created
        # under a second 'input_data' name scope (rbm.py:101-105 -> 'input_data_1/sigma')
        names = {name: '%s/%s' % (scope, name) for name, scope in self._VAR_SCOPES}
        names['sigma'] = 'input_data_1/sigma' if self._V_UNIT == _ffi.UNIT_GAUSSIAN else None
        return {name: (names[name], self._engine.get(name)) for name, _ in self._VAR_SCOPES}

    def _stage_variables(self, slot):
        """checkpoint snapshot without stopping the stream (bm_rbm_stage): float32 engine only; BM355_STAGED_SAVE=0
        restores the host-side snapshot"""
        eng = self._engine
        if (not isinstance(eng, RbmEngine) or os.environ.get('BM355_STAGED_SAVE', '1') == '0' or self._centering is not None
                or self._class_head is not None):
            return None          # (the staged slots hold the reference's variables only: a centred model, or one with a class
                                 #  head, snapshots on the host)
        eng.stage(slot)
        names = [name for name, _ in self._VAR_SCOPES]
        return lambda: {name: eng.get_staged(slot, name) for name in names}

    def set_params(self, **params):
        # the handle bakes in the graph constants: rebuild it if one of them changes
        rebuild = {'batch_size', 'l2', 'dropout', 'sample_v_states', 'sample_h_states', 'sparsity_target',
                   'sparsity_cost', 'sparsity_damping', 'dbm_first', 'dbm_last'}
        super(BaseRBM, self).set_params(**params)
        if self._engine is not None and isinstance(self._engine, (RbmEngine, RbmEngine64)) and rebuild & set(params):
            self._pending_vars = {name: self._engine.get(name) for name, _ in self._VAR_SCOPES}
            self._centering_detach()          # (the offsets wait on the host for the next engine: _apply_centering)
            self._class_detach()              # (so do the class head's variables: _apply_class_head)
            self._engine.close()
            self._engine = None
        return self

    # ---- schedules (reference base_rbm.py:533-547) -----------------------------------
    def _schedule(self, values):
        return values[min(self.epoch_, len(values) - 1)]

    def _feed(self):
        return (float(self._schedule(self.learning_rate)), float(self._schedule(self.momentum)),
                int(self._schedule(self.n_gibbs_steps)))

    # ---- training loop (reference base_rbm.py:549-666) -------------------------------
    def _train_epoch(self, Xd, N, after_first=None, defer=False):
        """one epoch of updates.  `after_first`: called once, right after the first engine call of the epoch (or at its start
        when the epoch opens with a metrics iteration) - `_fit` hands in the PREVIOUS epoch's report there, so that its one
        wait for the device and its host work run under this epoch's first run of updates instead of in front of it.
        `defer=True`: return a callable that collects the epoch's train metrics later instead of the metrics themselves."""
        eng = self._on_device()
        names = sorted(m for m in self._train_metrics_names if self.metrics_config[m])
        results = {m: [] for m in names}
        lr, mom, k = self._feed()
        every = self.metrics_config['train_metrics_every_iter']
        if self._neg_phase is not None:
            out = self._train_epoch_tempered(eng, Xd, N, names, results, lr, mom, k, every, after_first)
            return (lambda: out) if defer else out
        if getattr(self, '_dp', None) is not None:
            # data-parallel epoch: global minibatches of world * batch_size rows (train metrics are not fetched:
            # they would be rank-local numbers; validation metrics are evaluated on this rank's replica)
            step_rows = self.batch_size * self._world
            if N % step_rows:
                raise ValueError('data-parallel fit: {0} rows are not a multiple of batch_size x world_size = {1}'
                                 .format(N, step_rows))
            for start in range(0, N, step_rows):
                self.iter_ += 1
                self._dp.train_step(Xd, lr, mom, k, row=start + self._rank * self.batch_size)
            if after_first is not None:
                after_first()
            none = {m: None for m in names}
            return (lambda: none) if defer else none
        # runs of batches without a metrics fetch go to the engine as ONE call (bm_rbm_train_epoch loops in
        # C: same launches, same RNG call counters, no Python per batch)
        # ... and the metrics iterations leave their sums in a pinned ring (train_step_metrics_async): the reference
        # only uses the epoch mean (base_rbm.py:571), so the host waits for the stream once per epoch
        run_start, fused = None, hasattr(eng, 'train_epoch')
        deferred, pending = hasattr(eng, 'train_step_metrics_async'), 0

        def collect():
            for out in eng.collect_metrics():
                vals = dict(msre=out[0], pll=out[1], l2_loss=out[2])
                for m in names:
                    results[m].append(vals[m])
            return 0

        def first_done():
            nonlocal after_first
            if after_first is not None:
                f, after_first = after_first, None
                f()
        deferred_result = None
        try:
            for start in range(0, N, self.batch_size):
                B = min(self.batch_size, N - start)
                self.iter_ += 1
                if self.iter_ % every == 0:
                    if run_start is not None:
                        eng.train_epoch(Xd, start - run_start, self.batch_size, lr, mom, k, row=run_start)
                        run_start = None
                    first_done()          # (before this epoch's first fetch: the ring then holds the previous epoch's only)
                    if deferred:
                        if pending >= eng.MAX_PENDING_METRICS:
                            pending = collect()
                        eng.train_step_metrics_async(Xd, B, lr, mom, k, row=start)
                        pending += 1
                    else:
                        out = eng.train_step_metrics(Xd, B, lr, mom, k, row=start)
                        vals = dict(msre=out[0], pll=out[1], l2_loss=out[2])
                        for m in names:
                            results[m].append(vals[m])
                elif fused:
                    if run_start is None:
                        run_start = start
                else:
                    eng.train_step(Xd, B, lr, mom, k, row=start)
                    first_done()
            if run_start is not None:
                eng.train_epoch(Xd, N - run_start, self.batch_size, lr, mom, k, row=run_start)
            first_done()
            if defer and deferred:
                n_pending, pending = pending, 0            # (the `finally` below must not drain what the caller will collect)

                def deferred_result():
                    if n_pending:
                        collect()
                    return {m: (np.mean(r) if r else None) for m, r in results.items()}
            elif pending:
                pending = collect()
        finally:
            # An epoch that aborts BEFORE its first run of updates was queued still owes the previous epoch's report (its
            # fetches are the only ones in the ring then): make it now - progress line, scalar logs - instead of dropping
            # it with the drain below (round-5 advisor).  A report that cannot be made any more is announced, never silent.
            if after_first is not None and sys.exc_info()[0] is not None:
                try:
                    first_done()
                except Exception as e:       # noqa: BLE001
                    sys.stderr.write('fit: the report of the previous epoch was lost with the aborted one (%s)\n' % (str(e)[:200],))
            # an aborted epoch (KeyboardInterrupt, an engine error in a later batch) must not leave its deferred fetches
            # in the ring: the next epoch's collect() would average them into ITS metrics (round-4 advisor)
            if deferred and pending:
                try:
                    eng.collect_metrics()
                except Exception:
                    pass
        if deferred_result is not None:
            return deferred_result
        out = {m: (np.mean(r) if r else None) for m, r in results.items()}
        return (lambda: out) if defer else out

    # ---- centred training (no counterpart in the reference) ---------------------
    def _centering_sizes(self):
        return [self.n_visible, self.n_hidden]

    def _check_centering(self, what):
        name = self._check_centering_common(what)
        if self._V_UNIT != _ffi.UNIT_BERNOULLI:
            raise NotImplementedError('%s: centering needs Bernoulli visible units (Gaussian visible units are not centred)' % name)
        if self._H_UNIT != _ffi.UNIT_BERNOULLI:
            raise NotImplementedError('%s: centering needs Bernoulli hidden units (Multinomial hidden units are not centred)' % name)
        if self.dbm_first or self.dbm_last:
            raise NotImplementedError('%s: centering is not defined for `dbm_first` / `dbm_last` models (one conditional doubled)' % name)
        if self.dropout is not None:
            raise NotImplementedError('%s: centering is not combined with dropout' % name)

    def _engine_set_centering(self, on, nus):
        self._engine.set_centering(on, nus[0], nus[1])

    def set_centering(self, enabled=True, nu_v=0.01, nu_h=0.01, offset_v=None, offset_h=None):
        """Centred updates in `fit` (the centering trick: Montavon & Mueller 2012; Melchior, Fischer & Wiskott 2016).

        The weight gradient is taken between units minus running offsets, <(v - o_v)(h - o_h)^T>, and the bias gradients are
        corrected accordingly; the model itself stays in the standard parameters W, vb, hb, so everything but the update is
        unchanged.  Learning becomes invariant to flips of the data's coding.  Every update first moves the offsets,
        o <- (1 - nu) o + nu * mean of the positive phase, with the sliding factors `nu_v`, `nu_h` in [0, 1].

        offset_v, offset_h : the offsets to start from; None: at the first update of the next `fit(X)` the mean of X
        (float64 sum, rounded to float32) for the visible layer and 0.5 for the hidden layer.
        Works with both negative phases of `set_negative_phase`.  The offsets are optimiser state like the momentum buffers:
        while centering is on they are written to model.npz (`centering_ov`, `centering_oh`, `centering_nu`) and
        `load_model` re-enables the mode from them; params.json keeps the reference's schema.  BernoulliRBM in float32 only:
        GaussianRBM, MultinomialRBM, float64, `dbm_first` / `dbm_last`, dropout and BM355_DATA_PARALLEL jobs raise
        NotImplementedError, and so does switching it on while `set_negative_phase` has fast weights on.  Returns self."""
        if enabled and self._fast_weights is not None:
            raise NotImplementedError('%s.set_centering: centering is not combined with fast weights (set_negative_phase(..., '
                                      'fast_learning_rate=0) first)' % self.__class__.__name__)
        return self._set_centering(enabled, [nu_v, nu_h], [offset_v, offset_h])

    @classmethod
    def load_model(cls, model_path):
        model = super(BaseRBM, cls).load_model(model_path)
        model._centering_restore(model._pending_vars)
        model._class_restore(model._pending_vars)
        return model

    # ---- tempered negative phase (no counterpart in the reference) --------------
    _PT_MIN_CHAINS = 'batch_size'

    def _check_tempered_setting(self, what):
        self._check_single_joint(what)
        name = '%s.%s' % (self.__class__.__name__, what)
        if self.dropout is not None:
            raise NotImplementedError('%s: a tempered negative phase is not combined with dropout (the tempered family '
                                      'p_beta has none)' % name)
        if os.environ.get('BM355_DATA_PARALLEL', '0') == '1':
            raise NotImplementedError('%s: a tempered negative phase is not combined with BM355_DATA_PARALLEL (chains are '
                                      'not sharded over ranks)' % name)

    def set_negative_phase(self, kind='cd', n_temperatures=10, betas=None, n_chains=None, fast_learning_rate=0.0, fast_decay=0.95):
        """Where the negative particles of `fit` come from.

        kind='cd' (the default, the reference's training graph): a k-step Gibbs chain started at the minibatch.
        kind='tempered': parallel tempering (Desjardins et al. 2010, Cho et al. 2010).  A persistent ensemble of `n_chains`
        chains with one replica per temperature of the ladder 0 < betas[0] < ... < betas[-1] = 1 lives on the device; every
        update sweeps all of it for `n_gibbs_steps` tempered steps (h ~ p_beta(h|v), exchange of neighbouring temperatures,
        v ~ p_beta(v|h) - as `sample_v`) and takes the beta = 1 replicas of the first len(batch) chains as its negative
        particles; the positive phase, momentum, l2 and the sparsity terms are those of CD.  The hot replicas keep crossing
        between the modes a CD or single persistent chain stays in.

        betas : the ladder; None: float32(linspace(0, 1, n_temperatures + 1)[1:]), `sample_v`'s default.
        n_chains : None: `batch_size`; must be >= `batch_size`.
        The ensemble is built at the first update of every `fit()` call (v_0 ~ Ber(1/2) under that call's seed from the host
        stream: no further seed is drawn) and again whenever the ladder or `n_chains` changed; `sample_v` replaces it.
        Neither the ensemble nor this setting is written to checkpoints - params.json keeps the reference's schema - so a
        loaded model trains with CD until this method is called again, and a resumed fit starts a fresh ensemble.
        A train-metrics iteration reports the metrics of the CD reconstruction (as `kind='cd'` would) and then makes its
        tempered update.  BernoulliRBM in float32 only: GaussianRBM, MultinomialRBM, float64, `dbm_first` / `dbm_last`,
        dropout and BM355_DATA_PARALLEL jobs raise NotImplementedError.

        fast_learning_rate > 0 (kind='tempered' only): fast weights (FPCD, Tieleman & Hinton 2009).  A second parameter set
        W_fast, vb_fast, hb_fast learns from every update's gradient at this rate and decays by `fast_decay` in [0, 1) per
        update; the ensemble and the negative means run under model + fast set, which raises the energy wherever the chains sit
        and pushes them out of their modes at once, while the model itself is updated as before.  n_temperatures=1 is FPCD
        proper; more temperatures run the whole ladder under model + fast set.  The fast set starts at zero whenever the
        ensemble is built (so at the first update of every `fit()` call), is read by `fast_weights()` and is not written to
        checkpoints; calling this method again between `fit()` calls changes the rate.  Not combined with `set_centering`
        (NotImplementedError, whichever is set second).  Returns self."""
        rate, decay = float(fast_learning_rate), float(fast_decay)
        if not (np.isfinite(rate) and rate >= 0.):
            raise ValueError('`fast_learning_rate` must be a finite number >= 0 (got {0!r})'.format(fast_learning_rate))
        if not 0. <= decay < 1.:
            raise ValueError('`fast_decay` must lie in [0, 1) (got {0!r})'.format(fast_decay))
        if rate > 0.:
            if kind != 'tempered':
                raise ValueError("`fast_learning_rate` > 0 needs kind='tempered' (got kind={0!r})".format(kind))
            if self._centering is not None:
                raise NotImplementedError('%s.set_negative_phase: fast weights are not combined with centering '
                                          '(set_centering(False) first)' % self.__class__.__name__)
        self._set_negative_phase(kind, n_temperatures, betas, n_chains)
        self._fast_weights = (rate, decay) if rate > 0. else None
        if self._fast_weights is None:
            self._engine_fast_weights_off()
        return self

    def _engine_fast_weights_off(self):
        eng = self._engine
        if eng is not None and getattr(eng, '_fast_on', False):
            eng.set_fast_weights(False)
            eng._fast_on = False

    def _ensure_train_ensemble(self, eng):
        """... and the engine's fast-weights mode as set_negative_phase left it: a zero fast set wherever the ensemble is built"""
        built = getattr(self, '_pt_fresh', True) or getattr(eng, '_pt_train_key', None) != self._neg_phase
        super(BaseRBM, self)._ensure_train_ensemble(eng)
        if self._fast_weights is None:
            self._engine_fast_weights_off()
            return
        if built:
            self._engine_fast_weights_off()               # (off -> on starts from zero)
        eng.set_fast_weights(True, *self._fast_weights)
        eng._fast_on = True

    def fast_weights(self):
        """The fast parameter set of the tempered negative phase, dict(W=[n_visible, n_hidden], vb=, hb=) in float32.  Raises
        RuntimeError where there is none (fast weights off, or no update made yet)."""
        eng = self._engine
        if self._fast_weights is None or eng is None or not getattr(eng, '_fast_on', False):
            raise RuntimeError('`fast_weights`: no fast weights (call set_negative_phase(\'tempered\', fast_learning_rate=...) '
                               'and fit first)')
        return dict(W=eng.get('W_fast'), vb=eng.get('vb_fast'), hb=eng.get('hb_fast'))

    def _check_tempered_fit(self):
        """what may have changed since set_negative_phase (set_params): refused before an epoch starts"""
        self._check_tempered_setting('fit')
        if getattr(self, '_dp', None) is not None:
            raise NotImplementedError('%s.fit: a tempered negative phase is not combined with data parallelism' % self.__class__.__name__)
        if self._neg_phase[1] < self.batch_size:
            raise ValueError('`n_chains` must be >= batch_size (got {0} < {1})'.format(self._neg_phase[1], self.batch_size))

    def _train_epoch_tempered(self, eng, Xd, N, names, results, lr, mom, k, every, after_first):
        """one epoch with the tempered negative phase: runs of batches go to bm_rbm_train_epoch_pt; a metrics iteration
        fetches synchronously (bm_rbm_metrics, the CD reconstruction), then updates (not optimised)"""
        self._check_tempered_fit()
        self._ensure_train_ensemble(eng)
        run_start = None
        for start in range(0, N, self.batch_size):
            B = min(self.batch_size, N - start)
            self.iter_ += 1
            if self.iter_ % every == 0:
                if run_start is not None:
                    eng.train_epoch_pt(Xd, start - run_start, self.batch_size, lr, mom, k, row=run_start)
                    run_start = None
                out = eng.metrics(Xd, B, k, row=start)
                vals = dict(msre=out[0], pll=out[1], l2_loss=out[2])
                for m in names:
                    results[m].append(vals[m])
                eng.train_step_pt(Xd, B, lr, mom, k, row=start)
            elif run_start is None:
                run_start = start
        if run_start is not None:
            eng.train_epoch_pt(Xd, N - run_start, self.batch_size, lr, mom, k, row=run_start)
        if after_first is not None:
            after_first()
        return {m: (np.mean(r) if r else None) for m, r in results.items()}

    def _run_val_metrics(self, Xvd, N):
        eng = self._on_device()
        names = sorted(m for m in self._val_metrics_names if self.metrics_config[m])
        results = {m: [] for m in names}
        _, _, k = self._feed()
        for start in range(0, N, self.batch_size):
            B = min(self.batch_size, N - start)
            out = eng.metrics(Xvd, B, k, row=start)
            vals = dict(msre=out[0], pll=out[1])
            for m in names:
                results[m].append(vals[m])
        return {m: (np.mean(r) if r else None) for m, r in results.items()}

    def _run_feg(self, Xd, N, Xvd, Nv):
        """Free-energy gap between validation and training subsets (reference base_rbm.py:592-621)."""
        eng = self._on_device()
        nb = self.metrics_config['n_batches_for_feg']
        train_fes, val_fes = [], []
        for b, start in zip(range(nb), range(0, N, self.batch_size)):
            train_fes.append(eng.free_energy(Xd, min(self.batch_size, N - start), row=start))
        for b, start in zip(range(nb), range(0, Nv, self.batch_size)):
            val_fes.append(eng.free_energy(Xvd, min(self.batch_size, Nv - start), row=start))
        return np.mean(val_fes) - np.mean(train_fes)

    def _fit(self, X, X_val=None, *args, **kwargs):
        self._on_device()
        self._centering_begin_fit(X)
        self._pt_fresh = True          # a tempered negative phase builds its ensemble at this call's first update
        if self._neg_phase is not None:
            self._check_tempered_fit()
        Xd = self._to_device(X, 'fit_X')
        N = len(X)
        Xvd, Nv = None, 0
        if X_val is not None:
            Xvd, Nv = self._to_device(X_val, 'fit_X_val'), len(X_val)
        # The epoch's train metrics are device sums in a pinned ring (train_step_metrics_async); reading them is the ONE host wait
        # of an epoch.  Where nothing else needs the device idle at the epoch's end (no validation fetch, no display dump), the
        # checkpoint snapshot is staged in stream order at once and the REPORT of the epoch - wait, scalar logs, progress line -
        # is made after the next epoch's first run of updates has been queued (`after_first`): the device never waits for the
        # host's epoch-end work (75 -> 69 us per update with the reference's default cadence of one fetch per 10 updates).
        try:
            self._fit_epochs(X, X_val, Xd, N, Xvd, Nv)
        except BaseException:
            # fetches of an epoch whose report was still to come must not reach a later call's metrics (round-4 advisor)
            try:
                if hasattr(self._engine, 'collect_metrics'):
                    self._engine.collect_metrics()
            except Exception:
                pass
            raise
        self._engine.sync()

    def _fit_epochs(self, X, X_val, Xd, N, Xvd, Nv):
        report_later = None
        for self.epoch_ in epoch_iter(start_epoch=self.epoch_, max_epoch=self.max_epoch, verbose=self.verbose):
            val_now = X_val is not None and self.epoch_ % self.metrics_config['val_metrics_every_epoch'] == 0
            feg_now = X_val is not None and self.metrics_config['feg'] and self.epoch_ % self.metrics_config['feg_every_epoch'] == 0
            pipelined = (not val_now and not feg_now and not self.display_filters and not self.display_hidden_activations
                         and getattr(self, '_dp', None) is None)
            train_later = self._train_epoch(Xd, N, after_first=report_later, defer=True)
            report_later = None

            def report(train_later=train_later, epoch=self.epoch_, it=self.iter_, val_now=val_now, feg_now=feg_now):
                train_results = train_later()
                val_results = self._run_val_metrics(Xvd, Nv) if val_now else {}
                feg = self._run_feg(Xd, N, Xvd, Nv) if feg_now else None
                self._log_scalars('train', it, dict(train_results, epoch=epoch))
                self._log_scalars('val', it, dict(val_results, feg=feg))
                if self.verbose:
                    self._report_epoch(train_results, val_results, feg, epoch=epoch)
            if pipelined:
                if self.save_after_each_epoch:
                    self._save_model(global_step=self.epoch_)       # (the snapshot is taken in stream order, here)
                report_later = report
            else:
                report()
                self._display_dumps(X)
                if self.save_after_each_epoch:
                    self._save_model(global_step=self.epoch_)
        if report_later is not None:
            report_later()

    def _display_dumps(self, X):
        """`display_filters` / `display_hidden_activations` (base_rbm.py:300-306, :429-435): where the reference adds
        image summaries to the train summary, one .npy per epoch goes to logs/train: `W_filters` [n, h, w, c] (the
        first n columns of W as images, the reference's transposes) and `hidden_activation_means` [batch, n] (means
        of the first n hidden units for the first minibatch, computed on the host from the fetched parameters so that
        the device RNG stream of the run does not depend on the display options; the reference shows the last Gibbs
        step's means instead)."""
        if not (self.display_filters or self.display_hidden_activations):
            return
        W = np.asarray(self._engine.get('W'), dtype=np.float64)
        if self.display_filters and self.n_visible == int(np.prod(self.v_shape)):
            self._dump_array('W_filters', self._as_images(W.T[:self.display_filters]))
        if self.display_hidden_activations:
            n = self.display_hidden_activations
            Xb = np.asarray(X[:self.batch_size], dtype=np.float64)
            if self._V_UNIT == _ffi.UNIT_GAUSSIAN:
                Xb = Xb / np.asarray(self._sigma_vector(), dtype=np.float64)
            z = (1.0 + float(bool(self.dbm_first))) * (Xb.dot(W[:, :n]) + np.asarray(self._engine.get('hb'), dtype=np.float64)[:n])
            if self._H_UNIT == _ffi.UNIT_MULTINOMIAL:      # means of the whole layer are needed for the softmax
                zz = (1.0 + float(bool(self.dbm_first))) * (Xb.dot(W) + np.asarray(self._engine.get('hb'), dtype=np.float64))
                e = np.exp(zz - zz.max(axis=1, keepdims=True))
                hm = (self.n_samples if hasattr(self, 'n_samples') else 1) * (e / e.sum(axis=1, keepdims=True))[:, :n]
            else:
                hm = 1.0 / (1.0 + np.exp(-z))
            self._dump_array('hidden_activation_means', hm)

    def _report_epoch(self, train_results, val_results, feg, epoch=None):
        """one progress line per epoch in the reference's wording (`epoch: 3/10; msre: ...; val.pll: ...; feg: ...`,
        base_rbm.py:652-666), formats from metrics_config['<metric>_fmt']"""
        fmt = lambda name, value: format(value, self.metrics_config[name + '_fmt'])
        parts = ['epoch: %*d/%d' % (len(str(self.max_epoch)), self.epoch_ if epoch is None else epoch, self.max_epoch)]
        parts += ['%s: %s' % (m, fmt(m, v)) for m, v in sorted(train_results.items()) if v is not None]
        parts += ['val.%s: %s' % (m, fmt(m, v)) for m, v in sorted(val_results.items()) if v is not None]
        line = '; '.join(parts)
        if feg is not None:
            line += ' ; feg: ' + fmt('feg', feg)
        write_during_training(line)

    def init_from(self, rbm):
        """Warm start from another RBM of the same class: its weights become this model's initialisers, its
        momentum buffers the initial accumulators, and its run-time attributes (epoch_, iter_, ...) carry over
        (reference base_rbm.py:668-685)."""
        if type(self) != type(rbm):
            raise ValueError('an attempt to initialize `{0}` from `{1}`'
                             .format(type(self).__name__, type(rbm).__name__))
        w, acc = rbm.get_tf_params(scope='weights'), rbm.get_tf_params(scope='grads_accumulators')
        self.W_init, self.vb_init, self.hb_init = w['W'], w['vb'], w['hb']
        self._dW_init, self._dvb_init, self._dhb_init = acc['dW'], acc['dvb'], acc['dhb']
        for name, value in vars(rbm).items():
            if is_attribute_name(name):
                setattr(self, name, value)

    @run_on_engine(update_seed=True)
    def transform(self, X, np_dtype=None):
        """Hidden activation probabilities at the END of the k-step chain, stochastic
        (reference base_rbm.py:687-700 with the op of :438-440)."""
        np_dtype = np_dtype or self._np_dtype
        eng = self._on_device()
        N = len(X)
        Xd = self._to_device(X)
        Hd = _ffi.DeviceArray((N, self.n_hidden), eng.dtype)
        _, _, k = self._feed()
        for start in range(0, N, self.batch_size):
            eng.transform(Xd, min(self.batch_size, N - start), k, Hd, row=start, out_row=start)
        eng.sync()
        return Hd.numpy().astype(np_dtype)

    @run_on_engine(update_seed=True)
    def sample_h(self, X, return_means=False):
        """One draw of the hidden units given X, h ~ p(h | v = X), by a single prop-up of the model's own hidden conditional
        (no counterpart in the reference).

        X : [N, n_visible], taken as given: a GaussianRBM's input is NOT divided by `sigma` here, dropout is not applied.
        Returns the hidden states [N, n_hidden] (with `return_means`: a pair, states and means).  The layer is always sampled,
        whatever `sample_h_states` says.  The rows are processed in slices of at most `batch_size`, every row drawing from its
        own position of the call's random stream: the result does not depend on the slicing.  One seed is drawn from the
        model's host stream, as by every stochastic public call.  No parameter is changed.  float32 models only."""
        eng = self._on_device()
        if not isinstance(eng, RbmEngine):
            raise NotImplementedError("%s.sample_h: dtype='%s' models are not supported (float32 only)"
                                      % (self.__class__.__name__, np.dtype(self.dtype).name))
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        N = len(X)
        Xd = self._to_device(X)
        Sd = _ffi.DeviceArray((N, self.n_hidden), np.float32)
        Md = _ffi.DeviceArray((N, self.n_hidden), np.float32) if return_means else None
        home = self._rank * self.batch_size if getattr(self, '_dp', None) is not None else 0
        try:
            for start in range(0, N, self.batch_size):
                # every slice at call 0 of the call's seed and at its own rows of the stream, as sample_v_given
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.sample_h(Xd, min(self.batch_size, N - start), Md, Sd, row=start, out_row=start)
            eng.sync()
        finally:
            eng.set_row_offset(home)
        return (Sd.numpy(), Md.numpy()) if return_means else Sd.numpy()

    @run_on_engine(update_seed=True)
    def sample_v_from_h(self, H, return_means=False):
        """One draw of the visible units given H, v ~ p(v | h = H), by a single prop-down of the model's own visible conditional
        (no counterpart in the reference): the visible counterpart of `sample_h`.

        H : [N, n_hidden], taken as given.  Returns the visible states [N, n_visible] (with `return_means`: a pair, states and
        means) - for a GaussianRBM in the units of the chain (the input divided by `sigma`).  The layer is always sampled,
        whatever `sample_v_states` says.  The rows are processed in slices of at most `batch_size`, every row drawing from its
        own position of the call's random stream: the result does not depend on the slicing.  One seed is drawn from the
        model's host stream, as by every stochastic public call.  No parameter is changed.  float32 models only."""
        eng = self._on_device()
        if not isinstance(eng, RbmEngine):
            raise NotImplementedError("%s.sample_v_from_h: dtype='%s' models are not supported (float32 only)"
                                      % (self.__class__.__name__, np.dtype(self.dtype).name))
        H = np.ascontiguousarray(H, dtype=np.float32)
        if H.ndim != 2 or H.shape[1] != self.n_hidden:
            raise ValueError('`H` has invalid shape {0}: expected [N, {1}]'.format(H.shape, self.n_hidden))
        N = len(H)
        Hd = self._to_device(H)
        Sd = _ffi.DeviceArray((N, self.n_visible), np.float32)
        Md = _ffi.DeviceArray((N, self.n_visible), np.float32) if return_means else None
        home = self._rank * self.batch_size if getattr(self, '_dp', None) is not None else 0
        try:
            for start in range(0, N, self.batch_size):
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.sample_v_from_h(Hd, min(self.batch_size, N - start), Md, Sd, row=start, out_row=start)
            eng.sync()
        finally:
            eng.set_row_offset(home)
        return (Sd.numpy(), Md.numpy()) if return_means else Sd.numpy()

    # ---- conditional sampling (no counterpart in the reference) ------------------------------------
    def _check_clampable(self, what):
        name = '%s.%s' % (self.__class__.__name__, what)
        if self._H_UNIT != _ffi.UNIT_BERNOULLI:
            raise NotImplementedError('%s: Multinomial hidden units are not supported (their sweep goes through the softmax '
                                      'kernels, which have no clamped epilogue)' % name)
        if np.dtype(self.dtype) != np.float32:
            raise NotImplementedError("%s: dtype='%s' models are not supported (the float64 engine has no clamped sweep; "
                                      'float32 only)' % (name, np.dtype(self.dtype).name))

    @clampable_only
    @run_on_engine(update_seed=True)
    def sample_v_given(self, X, mask, n_gibbs_steps=None, return_means=False):
        """Conditional sampling: draw the unobserved visible units from p(v_free | v_observed) by block-Gibbs with the
        observed ones clamped (inpainting, imputation of missing values, completion of a partial pattern).

        X : [N, n_visible] - observed values where `mask` is non-zero; the other entries are the chain's starting values.
        mask : [N, n_visible], or [n_visible] for the same pattern in every row; non-zero = observed.
        n_gibbs_steps : sweeps h ~ p(h|v), v ~ p(v|h) with the observed entries re-imposed inside every visible pass;
            None: the model's `n_gibbs_steps` of the current epoch.
        Returns the visible states [N, n_visible] after the last sweep (with `return_means`: a pair, states and the
        means of the last visible pass); observed entries hold X in both.

        Both layers are always sampled (`sample_v_states` / `sample_h_states` and dropout do not apply).  The rows are
        processed in slices of at most `batch_size`, every row drawing from its own position of the call's random
        stream: the result does not depend on the slicing.  One seed is drawn from the model's host stream, as by
        every stochastic public call.  No parameter is changed.
        GaussianRBM: X is pre-processed like `fit`'s input (divided by `sigma`, reference rbm.py:107) - so are the
        observed values the chain holds - and the chain is the engine's own Gibbs chain of the training graph, whose
        visible pass yields sigma * (hW^T) + vb (+ sigma * noise).  The returned observed entries are X as given."""
        eng = self._on_device()
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        mask = np.asarray(mask)
        if mask.shape not in (X.shape, (self.n_visible,)):
            raise ValueError('`mask` has invalid shape {0}: expected {1} or ({2},)'.format(mask.shape, X.shape, self.n_visible))
        observed = np.broadcast_to(mask != 0, X.shape)
        k = int(n_gibbs_steps) if n_gibbs_steps is not None else self._feed()[2]
        if k < 1:
            raise ValueError('`n_gibbs_steps` must be >= 1 (got {0})'.format(k))
        N = len(X)
        Xin = X
        if self._V_UNIT == _ffi.UNIT_GAUSSIAN:
            Xin = np.ascontiguousarray(X / np.asarray(self._sigma_vector(), dtype=np.float32)[None, :], dtype=np.float32)
        Vd = self._to_device(Xin)                    # in/out: starting values -> last states
        Cd = self._to_device(Xin)                    # the clamp values (only the observed entries are read)
        Md = self._to_device(observed.astype(np.float32))
        Hd = _ffi.DeviceArray((N, self.n_hidden), np.float32)
        Pd = _ffi.DeviceArray((N, self.n_visible), np.float32) if return_means else None
        home = self._rank * self.batch_size if getattr(self, '_dp', None) is not None else 0
        try:
            for start in range(0, N, self.batch_size):
                # every slice at call 0 of the call's seed and at its own rows of the stream (`row0`): a row's
                # draws depend on its index alone
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.gibbs_clamped(Vd, Hd, min(self.batch_size, N - start), k, Cd, Md, Pd, row=start)
            eng.sync()
        finally:
            eng.set_row_offset(home)
        V = np.where(observed, X, Vd.numpy())
        if return_means:
            return V, np.where(observed, X, Pd.numpy())
        return V

    # ---- unconditional sampling by parallel tempering (no counterpart in the reference) -----------
    @single_joint_only
    @run_on_engine(update_seed=True)
    def sample_v(self, n_samples, n_gibbs_steps=1000, n_temperatures=10, betas=None, V_init=None, return_stats=False):
        """Unconditional samples of the visible units by parallel tempering (replica exchange; Desjardins et al. 2010,
        Cho et al. 2010): `n_samples` independent chains, each with one replica per temperature of the ladder
        0 < betas[0] < ... < betas[-1] = 1, run `n_gibbs_steps` steps of (h ~ p_beta(h|v), exchange of neighbouring
        temperatures, v ~ p_beta(v|h)); the replica at beta = 1 of every chain is returned.  The hot replicas cross between
        modes a single Gibbs chain stays in, and the exchanges carry those moves down to beta = 1.

        betas : the ladder; None: float32(linspace(0, 1, n_temperatures + 1)[1:]).  `n_temperatures=1` is plain Gibbs.
        V_init : [n_samples, n_visible] start of every chain (all its replicas); None: v_0 ~ Ber(1/2).
        Returns [n_samples, n_visible]; with `return_stats` also the acceptance rate of every neighbouring pair of
        temperatures, [n_temperatures - 1] (accepts / attempts).
        Both layers are always sampled, dropout is not applied.  One seed is drawn from the model's host stream; no
        parameter is changed.  In a multi-GPU job every rank runs all chains."""
        eng = self._on_device()
        n_samples = int(n_samples)
        if n_samples < 1 or int(n_gibbs_steps) < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        return run_tempered_sampler(eng, n_samples, int(n_gibbs_steps), resolve_ladder(n_temperatures, betas), V_init,
                                    self.n_visible, return_stats)

    # ---- likelihood (no counterpart in the reference: its only AIS is the DBM's) ----------------
    def _check_single_joint(self, what):
        name = '%s.%s' % (self.__class__.__name__, what)
        if self._V_UNIT != _ffi.UNIT_BERNOULLI:
            raise NotImplementedError('%s: Gaussian visible units are not supported (Bernoulli visible units only)' % name)
        if self._H_UNIT != _ffi.UNIT_BERNOULLI:
            raise NotImplementedError('%s: Multinomial hidden units are not supported (Bernoulli hidden units only)' % name)
        if np.dtype(self.dtype) != np.float32:
            raise NotImplementedError("%s: dtype='%s' models are not supported (float32 only)" % (name, np.dtype(self.dtype).name))
        if self.dbm_first or self.dbm_last:
            raise NotImplementedError('%s: a dbm_first / dbm_last model doubles one of its conditionals, which then belong to '
                                      'no single joint distribution' % name)

    def _base_rate_bias(self, X_base):
        """the bias `a` of the AIS base model p_0(v) ~ exp(a.v): None (uniform), `a` itself [V], or data [N][V] ->
        logit((sum_n X[n, i] + 1) / (N + 2)) (Laplace smoothing)"""
        if X_base is None:
            return None
        X = np.asarray(X_base, dtype=np.float64)
        if X.ndim == 2 and X.shape[1] == self.n_visible:
            p = (X.sum(axis=0) + 1.) / (len(X) + 2.)
            return (np.log(p) - np.log1p(-p)).astype(np.float32)
        if X.shape != (self.n_visible,):
            raise ValueError('`X_base` has invalid shape {0}: expected [N, {1}] or [{1}]'.format(X.shape, self.n_visible))
        return X.astype(np.float32)

    @single_joint_only
    @run_on_engine(update_seed=True)
    def log_Z(self, n_betas=100, n_runs=100, n_gibbs_steps=5, X_base=None):
        """AIS estimate of the log partition function of this RBM (Salakhutdinov & Murray 2008).
        Returns log_mean, (log_low, log_high), values - as `DBM.log_Z`.

        `n_runs` chains run from the base model p_0(v) ~ exp(a.v) through `n_betas` temperatures linspace(0, 1, n_betas)
        with `n_gibbs_steps` transitions each, the hidden layer summed out:
        log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta (vW + hb)_j).
        X_base : None - the uniform base (a = 0); an [N, n_visible] array - the base rates of that data,
        a_i = logit((sum_n X[n, i] + 1) / (N + 2)), which makes AIS usable on trained models; an [n_visible] array - `a` itself.
        Both layers are always sampled, dropout is not applied.  In a multi-GPU job every rank runs all chains."""
        values = self._on_device().ais(n_betas, n_runs, n_gibbs_steps, seed=self._graph_seed,
                                       base_bias=self._base_rate_bias(X_base))
        log_mean = log_mean_exp(values)
        log_std = log_std_exp(values, log_mean_exp_x=log_mean)
        log_high = log_sum_exp([log_std, log_mean])
        log_low = log_diff_exp([log_std, log_mean])[0]
        return log_mean, (log_low, log_high), values

    @single_joint_only
    @run_on_engine()
    def log_proba(self, X, log_Z):
        """Exact log p(x) = -F(x) - log_Z per row of X, F the free energy -x.vb - sum_j softplus((xW + hb)_j) of the model's
        own parameters (no dropout); `log_Z` e.g. from `log_Z()`.  Draws nothing: the model's state and seed streams stay
        as they are."""
        eng = self._on_device()
        X = np.ascontiguousarray(X, dtype=eng.dtype)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        Xd = self._to_device(X)
        F = np.empty(len(X))
        for start in range(0, len(X), self.batch_size):
            B = min(self.batch_size, len(X) - start)
            F[start:start + B] = eng.free_energy_rows(Xd, B, row=start)
        return -F - log_Z


class BernoulliRBM(BaseRBM):
    """RBM with Bernoulli visible and hidden units (reference rbm/rbm.py:10-22)."""

    def __init__(self, model_path='b_rbm_model/', *args, **kwargs):
        super(BernoulliRBM, self).__init__(model_path=model_path, *args, **kwargs)


class MultinomialRBM(BaseRBM):
    """RBM with Bernoulli visible and a single Multinomial hidden unit (= `n_samples` softmax units
    with tied weights; reference rbm/rbm.py:25-65, layers.py:54-70).

    Parameters
    ----------
    n_hidden : int
        Number of possible states of the multinomial unit.
    n_samples : int
        Number of softmax units with shared weights (= draws from one softmax unit).

    Hidden means are `n_samples * softmax(vW + hb)`, hidden states the counts of `n_samples`
    categorical draws; `transform` returns the means divided by `n_samples` (rbm.py:62-65).
    """

    _H_UNIT = _ffi.UNIT_MULTINOMIAL

    def __init__(self, n_samples=100, model_path='m_rbm_model/', *args, **kwargs):
        self.n_samples = n_samples
        super(MultinomialRBM, self).__init__(model_path=model_path, *args, **kwargs)

    def transform(self, *args, **kwargs):
        H = super(MultinomialRBM, self).transform(*args, **kwargs)
        H /= float(self.n_samples)
        return H


class GaussianRBM(BaseRBM):
    """RBM with Gaussian visible (fixed `sigma`) and Bernoulli hidden units
    (reference rbm/rbm.py:68-116)."""

    _V_UNIT = _ffi.UNIT_GAUSSIAN

    def __init__(self, learning_rate=1e-3, sigma=1., model_path='g_rbm_model/', *args, **kwargs):
        self.sigma = sigma
        super(GaussianRBM, self).__init__(learning_rate=learning_rate, model_path=model_path, *args, **kwargs)
        if hasattr(self.sigma, '__iter__'):
            self._sigma_tmp = self.sigma = np.asarray(self.sigma)
        else:
            self._sigma_tmp = np.repeat(self.sigma, self.n_visible)

    def _sigma_vector(self):
        return np.asarray(self._sigma_tmp, dtype=self._np_dtype)

    # ---- the model as one joint: AIS, log-density and parallel tempering (no counterpart in the reference) --------
    # With u = x / sigma and c = float32(vb / sigma) the free energy that `fit` reports, F(u) = 1/2 |u - c|^2 - sum_j softplus((uW + hb)_j),
    # and the prop-down x ~ N(vb + sigma (W h), sigma^2) are the conditionals of ONE joint,
    #     E(u, h) = 1/2 |u - c|^2 - u W h - hb.h,    h | u ~ Ber(sigmoid(uW + hb)),    u | h ~ N(c + W h, I),    x = sigma u.
    # The methods below evaluate and sample that model.  (`fit` keeps the reference's chain, which feeds unscaled samples back into
    # the prop-up - for sigma != 1 the Gibbs sampler of no joint; with sigma = 1 the two coincide.)  `log_Z`, `log_proba`, `sample_v`
    # and `set_negative_phase('tempered')` stay refused for this class.
    def _check_gauss_joint(self, what):
        name = '%s.%s' % (self.__class__.__name__, what)
        if self._H_UNIT == _ffi.UNIT_NRELU:
            raise ValueError('%s: not defined with noisy rectified-linear (NReLU) hidden units (the unit has no closed-form free '
                             'energy and real-valued hidden states)' % name)
        if np.dtype(self.dtype) != np.float32:
            raise NotImplementedError("%s: dtype='%s' models are not supported (float32 only)" % (name, np.dtype(self.dtype).name))
        if self.dbm_first or self.dbm_last:
            raise NotImplementedError('%s: a dbm_first / dbm_last model doubles one of its conditionals, which then belong to '
                                      'no single joint distribution' % name)

    def _base_mean(self, X_base):
        """the mean `a` of the AIS base model N(a, I) in the scaled variable u = x / sigma, float32 [V]: None (a = 0), data [N][V]
        -> mean(X / sigma), or a [V] vector - the base mean in data units -> float32(X_base / sigma)"""
        if X_base is None:
            return None
        sigma = self._sigma_vector().astype(np.float32)
        X = np.asarray(X_base, dtype=np.float32)
        if X.ndim == 2 and X.shape[1] == self.n_visible:
            return (X / sigma).astype(np.float64).mean(axis=0).astype(np.float32)
        if X.shape != (self.n_visible,):
            raise ValueError('`X_base` has invalid shape {0}: expected [N, {1}] or [{1}]'.format(X.shape, self.n_visible))
        return (X / sigma).astype(np.float32)

    def ais_log_Z(self, n_betas=100, n_runs=100, n_gibbs_steps=5, X_base=None):
        """AIS estimate of the log normaliser of exp(-F(x / sigma)) over x (data units: sum_i log sigma_i included), so that
        `log_density(X, log_Z)` integrates to one.  Returns log_mean, (log_low, log_high), values - as `BernoulliRBM.log_Z`.

        `n_runs` chains run from the base model p_0(u) = N(a, I), h uniform, through `n_betas` temperatures linspace(0, 1, n_betas)
        with `n_gibbs_steps` transitions each, the hidden layer summed out:
        log p*_beta(u) = -(1 - beta) 1/2 |u - a|^2 - beta 1/2 |u - c|^2 + sum_j softplus(beta (uW + hb)_j).
        X_base : None - a = 0; an [N, n_visible] array - a = mean(X / sigma), which makes AIS usable on trained models; an
        [n_visible] array - the base mean in data units.
        Both layers are always sampled, dropout is not applied.  One seed is drawn from the model's host stream; no parameter is
        changed.  In a multi-GPU job every rank runs all chains."""
        self._check_gauss_joint('ais_log_Z')
        n_betas, n_runs, n_gibbs_steps = int(n_betas), int(n_runs), int(n_gibbs_steps)
        if n_betas < 2 or n_runs < 1 or n_gibbs_steps < 1:
            raise ValueError('%s.ais_log_Z: n_betas must be >= 2, n_runs and n_gibbs_steps >= 1 (got %d, %d, %d)'
                             % (self.__class__.__name__, n_betas, n_runs, n_gibbs_steps))
        return self._ais_log_Z_checked(n_betas, n_runs, n_gibbs_steps, self._base_mean(X_base))

    @run_on_engine(update_seed=True)
    def _ais_log_Z_checked(self, n_betas, n_runs, n_gibbs_steps, a):
        values = self._on_device().gauss_ais(n_betas, n_runs, n_gibbs_steps, seed=self._graph_seed, base_mean=a)
        log_mean = log_mean_exp(values)
        log_std = log_std_exp(values, log_mean_exp_x=log_mean)
        log_high = log_sum_exp([log_std, log_mean])
        log_low = log_diff_exp([log_std, log_mean])[0]
        return log_mean, (log_low, log_high), values

    def free_energy(self, X):
        """F(x / sigma) = 1/2 |u - c|^2 - sum_j softplus((uW + hb)_j) per row of X [N, n_visible] (data units), float64 [N]: the free
        energy of the model's own parameters, no dropout.  Draws nothing: the model's state and seed streams stay as they are."""
        self._check_gauss_joint('free_energy')
        return self._free_energy_checked(X)

    @run_on_engine()
    def _free_energy_checked(self, X):
        eng = self._on_device()
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        Xd = self._to_device(X)
        F = np.empty(len(X))
        for start in range(0, len(X), self.batch_size):
            B = min(self.batch_size, len(X) - start)
            F[start:start + B] = eng.gauss_free_energy_rows(Xd, B, row=start)
        return F

    def log_density(self, X, log_Z):
        """log density of x per row of X: -F(x / sigma) - log_Z, `log_Z` e.g. from `ais_log_Z()`.  Draws nothing."""
        self._check_gauss_joint('log_density')
        return -self._free_energy_checked(X) - log_Z

    def sample_v_tempered(self, n_samples, n_gibbs_steps=1000, n_temperatures=10, betas=None, V_init=None, return_stats=False):
        """Unconditional samples of the visible units by parallel tempering (replica exchange), as `BernoulliRBM.sample_v`:
        `n_samples` independent chains, each with one replica per temperature of the ladder 0 < betas[0] < ... < betas[-1] = 1,
        run `n_gibbs_steps` steps of (h ~ Ber(sigmoid(beta (uW + hb))), exchange of neighbouring temperatures,
        u ~ N(c + W h, I / beta)) on the scaled variable u = x / sigma - the temperature widens the variance of the visible
        conditional and leaves its mean; the replica at beta = 1 of every chain is returned in data units, [n_samples, n_visible].

        betas : the ladder; None: float32(linspace(0, 1, n_temperatures + 1)[1:]).  `n_temperatures=1` is plain Gibbs on the joint.
        V_init : [n_samples, n_visible] start of every chain (all its replicas), in data units; None: u_0 ~ N(c, I / beta).
        With `return_stats` also the acceptance rate of every neighbouring pair of temperatures, [n_temperatures - 1].
        Both layers are always sampled, dropout is not applied.  One seed is drawn from the model's host stream; no parameter is
        changed.  In a multi-GPU job every rank runs all chains."""
        self._check_gauss_joint('sample_v_tempered')
        n_samples, n_gibbs_steps = int(n_samples), int(n_gibbs_steps)
        if n_samples < 1 or n_gibbs_steps < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        return self._sample_v_tempered_checked(n_samples, n_gibbs_steps, resolve_ladder(n_temperatures, betas), V_init, return_stats)

    @run_on_engine(update_seed=True)
    def _sample_v_tempered_checked(self, n_samples, n_gibbs_steps, ladder, V_init, return_stats):
        return run_tempered_sampler(self._on_device().gauss_pt, n_samples, n_gibbs_steps, ladder, V_init, self.n_visible, return_stats)


class NReLUHidden(object):
    """Noisy rectified-linear hidden units (NReLU; Nair & Hinton 2010), mixed in in front of an RBM class.

    With t = vW + hb: hidden means max(0, t), hidden states max(0, t + n * sqrt(sigmoid(t))), n ~ N(0, 1).  `fit`, `transform`,
    `sample_h`, `load_model`, checkpoints and `init_from` work as for the other classes; the update consumes the means and
    states exactly as the Bernoulli update does.  The unit has no closed-form free energy and real-valued hidden states, so
    everything built on either is refused with a ValueError before the engine is touched: the `pll` / `feg` metrics,
    `sparsity_cost`, `dropout`, `dbm_first` / `dbm_last`, dtype='float64', `set_negative_phase('tempered')`, `set_centering`,
    `set_classes`, `sample_v`, `sample_v_given`, `log_Z`, `log_proba`, BM355_DATA_PARALLEL jobs, and use as a layer of a `DBM`
    or a `StackClassifier`."""

    _H_UNIT = _ffi.UNIT_NRELU
    _UNIT_NAME = 'noisy rectified-linear (NReLU) hidden units'

    def _nrelu_refuse(self, what, why):
        raise ValueError('%s.%s: %s with %s' % (self.__class__.__name__, what, why, self._UNIT_NAME))

    def _check_nrelu_config(self, what):
        """the constructor keywords the unit does not combine with (set_params may change them: checked again before the
        engine is built)"""
        for m in ('pll', 'feg'):
            if self.metrics_config.get(m):
                self._nrelu_refuse(what, "metrics_config['%s'] needs a free energy in closed form, which does not exist" % m)
        if self.sparsity_cost != 0.:
            self._nrelu_refuse(what, 'the sparsity penalty (sparsity_cost=%r) targets a probability; it is not combined' % (self.sparsity_cost,))
        if self.dropout is not None:
            self._nrelu_refuse(what, 'dropout (dropout=%r) is not combined' % (self.dropout,))
        if self.dbm_first or self.dbm_last:
            self._nrelu_refuse(what, 'dbm_first / dbm_last (a doubled conditional, a DBM layer) is not defined')
        if np.dtype(self.dtype) != np.float32:
            self._nrelu_refuse(what, "dtype='%s' is not supported (float32 only)" % np.dtype(self.dtype).name)

    def __init__(self, *args, **kwargs):
        super(NReLUHidden, self).__init__(*args, **kwargs)
        self._check_nrelu_config('__init__')

    def _ensure_engine(self):
        if self._engine is None:
            self._check_nrelu_config('fit')
            if os.environ.get('BM355_DATA_PARALLEL', '0') == '1':
                self._nrelu_refuse('fit', 'data-parallel mode (BM355_DATA_PARALLEL) is not combined: the split step has no such form')
        return super(NReLUHidden, self)._ensure_engine()

    def set_negative_phase(self, kind='cd', *args, **kwargs):
        if kind != 'cd':
            self._nrelu_refuse('set_negative_phase', 'a %r negative phase (the tempered family needs an energy) is not defined' % (kind,))
        return super(NReLUHidden, self).set_negative_phase(kind, *args, **kwargs)

    def set_centering(self, enabled=True, *args, **kwargs):
        if enabled:
            self._nrelu_refuse('set_centering', 'centering is not combined')
        return super(NReLUHidden, self).set_centering(enabled, *args, **kwargs)

    def set_classes(self, n_classes, *args, **kwargs):
        if n_classes is not None:
            self._nrelu_refuse('set_classes', 'a class head (exact p(y|x) sums softplus terms over Bernoulli units) is not defined')
        return super(NReLUHidden, self).set_classes(n_classes, *args, **kwargs)

    def sample_v(self, *args, **kwargs):
        self._nrelu_refuse('sample_v', 'parallel tempering (it needs an energy) is not defined')

    def sample_v_given(self, *args, **kwargs):
        self._nrelu_refuse('sample_v_given', 'the clamped sweep is not built')

    def log_Z(self, *args, **kwargs):
        self._nrelu_refuse('log_Z', 'AIS (it needs a free energy in closed form) is not defined')

    def log_proba(self, *args, **kwargs):
        self._nrelu_refuse('log_proba', 'the likelihood (it needs a free energy in closed form) is not defined')


class ReLURBM(NReLUHidden, BaseRBM):
    """RBM with Bernoulli visible and noisy rectified-linear hidden units (Nair & Hinton 2010; no counterpart in the
    reference).  See `NReLUHidden` for the unit and for what is refused."""

    def __init__(self, model_path='relu_rbm_model/', *args, **kwargs):
        super(ReLURBM, self).__init__(model_path=model_path, *args, **kwargs)


class GaussianReLURBM(NReLUHidden, GaussianRBM):
    """RBM with Gaussian visible (fixed `sigma`) and noisy rectified-linear hidden units: the usual model for real-valued data
    (Nair & Hinton 2010; no counterpart in the reference).  See `NReLUHidden` for the unit and for what is refused."""

    def __init__(self, learning_rate=1e-4, model_path='g_relu_rbm_model/', *args, **kwargs):
        super(GaussianReLURBM, self).__init__(learning_rate=learning_rate, model_path=model_path, *args, **kwargs)


class SoftmaxVisible(object):
    """Softmax (categorical) visible units (Salakhutdinov, Mnih & Hinton 2007), mixed in in front of an RBM
    class: the visible layer is `n_groups` groups of `n_categories` mutually exclusive units, one-hot per group.

    p(v_{gK+k} = 1 | h) = softmax_k((hW^T + vb)_{gK..gK+K-1}) independently per group; the hidden conditional, the update and
    the free energy are the Bernoulli ones.  `fit`, `transform`, `sample_h`, `sample_v_from_h`, `log_proba`, `load_model`,
    checkpoints and `init_from` work as for the other classes.  What is not built for one-hot groups is refused with a
    ValueError before the engine is touched: the `pll` metric, `dropout`, `dbm_first` / `dbm_last`, dtype='float64',
    `set_negative_phase` other than 'cd', `set_centering`, `set_classes`, `sample_v_given`, `log_Z`, BM355_DATA_PARALLEL jobs,
    and use as a layer of a `DBM` or a `StackClassifier`.

    Incomplete rows: with `missing_values=True` a group of all zeros is a missing value - `fit` accepts rows
    whose groups are one-hot or empty and trains each row's observed units only.  `group_log_proba`, `predict_proba`, `predict`
    and `pseudo_log_likelihood` give the exact conditionals of the groups with the hidden layer summed out, and
    `sample_groups_given` draws the empty groups of a row given its observed ones; these work whatever `missing_values` says.

    Density evaluation: `ais_log_Z` estimates the log partition function of the model, or of the sub-model over
    one pattern of observed groups, by AIS from a categorical base model; `ais_log_Z_rows(X)` does so for every pattern of
    incomplete rows, so that `log_proba(X, ais_log_Z_rows(X))` is their log-likelihood."""

    _UNIT_NAME = 'softmax visible units'
    _PT_VIEW, _PT_SETTER = 'groups_pt', 'set_group_tempering()'      # (tempering_stats: the ensemble of `set_group_tempering`)

    @property
    def _V_GROUP_WIDTH(self):
        return int(self.n_categories)

    def _softmax_refuse(self, what, why):
        raise ValueError('%s.%s: %s with %s' % (self.__class__.__name__, what, why, self._UNIT_NAME))

    def _check_softmax_config(self, what):
        """the constructor keywords the unit does not combine with (set_params may change them: checked again before the
        engine is built)"""
        if int(self.n_groups) < 1 or int(self.n_categories) < 2:
            raise ValueError('%s.%s: n_groups must be >= 1 and n_categories >= 2 (got %r, %r)'
                             % (self.__class__.__name__, what, self.n_groups, self.n_categories))
        if self.n_visible != int(self.n_groups) * int(self.n_categories):
            raise ValueError('%s.%s: n_visible = %r is not n_groups x n_categories = %d x %d'
                             % (self.__class__.__name__, what, self.n_visible, self.n_groups, self.n_categories))
        if self.metrics_config.get('pll'):
            self._softmax_refuse(what, "metrics_config['pll'] flips single bits, which leaves the one-hot states; it is not defined")
        if self.dropout is not None:
            self._softmax_refuse(what, 'dropout (dropout=%r) is not combined' % (self.dropout,))
        if self.dbm_first or self.dbm_last:
            self._softmax_refuse(what, 'dbm_first / dbm_last (a doubled conditional, a DBM layer) is not built')
        if np.dtype(self.dtype) != np.float32:
            self._softmax_refuse(what, "dtype='%s' is not supported (float32 only)" % np.dtype(self.dtype).name)

    def __init__(self, *args, **kwargs):
        super(SoftmaxVisible, self).__init__(*args, **kwargs)
        self._check_softmax_config('__init__')

    def _ensure_engine(self):
        if self._engine is None:
            self._check_softmax_config('fit')
            if os.environ.get('BM355_DATA_PARALLEL', '0') == '1':
                self._softmax_refuse('fit', 'data-parallel mode (BM355_DATA_PARALLEL) is not combined: the split step is not built')
        out = super(SoftmaxVisible, self)._ensure_engine()
        if hasattr(self._engine, 'groups_set_missing'):       # incomplete rows: a property of the handle, read by every training chain
            self._engine.groups_set_missing(bool(self.missing_values))
        return out

    def set_negative_phase(self, kind='cd', *args, **kwargs):
        if kind != 'cd':
            self._softmax_refuse('set_negative_phase', 'a %r negative phase (the tempered sweep has no softmax pass) is not built' % (kind,))
        return super(SoftmaxVisible, self).set_negative_phase(kind, *args, **kwargs)

    def set_centering(self, enabled=True, *args, **kwargs):
        if enabled:
            self._softmax_refuse('set_centering', 'centering is not combined')
        return super(SoftmaxVisible, self).set_centering(enabled, *args, **kwargs)

    def set_classes(self, n_classes, *args, **kwargs):
        if n_classes is not None:
            self._softmax_refuse('set_classes', 'a class head is not built')
        return super(SoftmaxVisible, self).set_classes(n_classes, *args, **kwargs)

    def sample_v_given(self, *args, **kwargs):
        self._softmax_refuse('sample_v_given', 'the clamped sweep (clamped groups) is not built')

    def log_Z(self, *args, **kwargs):
        self._softmax_refuse('log_Z', 'AIS (its base model and its sweeps are Bernoulli) is not built; `ais_log_Z` is the estimator')

    # ---- AIS log Z and held-out log-likelihood
    def _base_group_logits(self, X_base):
        """the base logits `a` of the AIS base model p_0(v) = prod_g softmax(a_g)[v_g]: None (uniform), `a` itself [V], or data
        [N][V] of one-hot-or-empty groups -> a_{gK+k} = log((count_{g,k} + 1) / (N_g + K)), N_g the rows that observe g (Laplace
        smoothing; float64, handed over as float32)"""
        if X_base is None:
            return None
        X = np.asarray(X_base, dtype=np.float64)
        if X.ndim == 2 and X.shape[1] == self.n_visible:
            X, observed = self._groups_of(X, 'ais_log_Z')
            G, K = int(self.n_groups), int(self.n_categories)
            count = X.astype(np.float64).sum(axis=0).reshape(G, K)
            n_g = observed.sum(axis=0).astype(np.float64)
            return np.log((count + 1.) / (n_g[:, None] + K)).reshape(self.n_visible).astype(np.float32)
        if X.shape != (self.n_visible,):
            raise ValueError('`X_base` has invalid shape {0}: expected [N, {1}] or [{1}]'.format(X.shape, self.n_visible))
        return X.astype(np.float32)

    def _observed_pattern(self, observed, what):
        if observed is None:
            return None
        o = np.asarray(observed)
        if o.shape != (int(self.n_groups),) or o.dtype != np.bool_:
            raise ValueError('%s.%s: `observed` must be a boolean array of shape [%d] (got %s %r)'
                             % (self.__class__.__name__, what, self.n_groups, o.dtype, o.shape))
        if not o.any():
            raise ValueError('%s.%s: `observed` names no group (a model without visible units)' % (self.__class__.__name__, what))
        return o

    def ais_log_Z(self, n_betas=100, n_runs=100, n_gibbs_steps=5, X_base=None, observed=None):
        """AIS estimate of the log partition function of this model - or, with `observed`, of the sub-model that has the named
        groups only (the model of a row whose other groups are missing).  Returns log_mean, (log_low, log_high),
        values - as `BernoulliRBM.log_Z`.

        `n_runs` chains run from the base model p_0(v) = prod_g softmax(a_g)[v_g] through `n_betas` temperatures
        linspace(0, 1, n_betas) with `n_gibbs_steps` transitions each, the hidden layer summed out:
        log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta (vW + hb)_j).
        X_base : None - the uniform base (a = 0); an [N, n_visible] array of one-hot-or-empty groups - the smoothed base rates of
        that data, a_{gK+k} = log((count_{g,k} + 1) / (N_g + K)) with N_g the rows that observe group g; an [n_visible] array -
        the logits `a` themselves.
        observed : None - every group; a boolean [n_groups] array - the groups the model has.
        Both layers are always sampled.  One seed is drawn from the model's host stream; no parameter is changed."""
        n_betas, n_runs, n_gibbs_steps = int(n_betas), int(n_runs), int(n_gibbs_steps)
        if n_betas < 2 or n_runs < 1 or n_gibbs_steps < 1:
            raise ValueError('%s.ais_log_Z: n_betas must be >= 2, n_runs and n_gibbs_steps >= 1 (got %d, %d, %d)'
                             % (self.__class__.__name__, n_betas, n_runs, n_gibbs_steps))
        a = self._base_group_logits(X_base)
        o = self._observed_pattern(observed, 'ais_log_Z')
        return self._ais_log_Z_checked(n_betas, n_runs, n_gibbs_steps, a, o)

    @run_on_engine(update_seed=True)
    def _ais_log_Z_checked(self, n_betas, n_runs, n_gibbs_steps, a, o):
        values = self._on_device().groups_ais(n_betas, n_runs, n_gibbs_steps, seed=self._graph_seed, base_bias=a, observed=o)
        log_mean = log_mean_exp(values)
        log_std = log_std_exp(values, log_mean_exp_x=log_mean)
        log_high = log_sum_exp([log_std, log_mean])
        log_low = log_diff_exp([log_std, log_mean])[0]
        return log_mean, (log_low, log_high), values

    def observed_patterns(self, X):
        """(patterns [P, n_groups] bool, index [N] int64): the distinct patterns of observed groups among the rows of X (every
        group one-hot or empty) and, for every row, the position of its pattern - X's row n observes patterns[index[n]]"""
        _, observed = self._groups_of(X, 'observed_patterns')
        if not len(observed):
            return np.zeros((0, int(self.n_groups)), dtype=bool), np.zeros(0, dtype=np.int64)
        patterns, index = np.unique(observed, axis=0, return_inverse=True)
        return patterns.astype(bool), np.asarray(index, dtype=np.int64).reshape(len(observed))

    def ais_log_Z_rows(self, X, **ais_kwargs):
        """[N] float64: for every row of X (every group one-hot or empty) the AIS log Z of the sub-model over the row's observed
        groups, so that `log_proba(X, ais_log_Z_rows(X))` is the log-likelihood of incomplete rows.  One `ais_log_Z` run per
        DISTINCT pattern of X, its log_mean scattered to the rows of that pattern: the cost is P runs for P patterns (see
        `observed_patterns`), each drawing one seed from the model's host stream.  A row with no observed group is refused
        (ValueError): it belongs to no model.  `ais_kwargs`: n_betas, n_runs, n_gibbs_steps, X_base."""
        if 'observed' in ais_kwargs:
            raise ValueError('%s.ais_log_Z_rows: the patterns come from `X`; `observed` is not an argument' % self.__class__.__name__)
        patterns, index = self.observed_patterns(X)
        empty = ~patterns.any(axis=1)
        if empty.any():
            raise ValueError('%s.ais_log_Z_rows: row %d observes no group' % (self.__class__.__name__, int(np.argmax(empty[index]))))
        per_pattern = np.array([self.ais_log_Z(observed=p, **ais_kwargs)[0] for p in patterns], dtype=np.float64)
        return per_pattern[index] if len(index) else np.zeros(0)

    # ---- one-hot coding
    def encode(self, C, missing=None):
        """integer categories [N, n_groups] with entries in [0, n_categories) -> one-hot float32 [N, n_groups * n_categories];
        entries equal to `missing` (when one is given, e.g. -1) become empty - all-zero - groups"""
        C = np.asarray(C)
        if C.ndim != 2 or C.shape[1] != self.n_groups:
            raise ValueError('`C` has invalid shape {0}: expected [N, {1}]'.format(C.shape, self.n_groups))
        gone = np.zeros(C.shape, dtype=bool) if missing is None else (C == missing)
        Ci = np.where(gone, 0, C).astype(np.int64)
        if C.size and (np.any(Ci != np.where(gone, 0, C)) or Ci.min() < 0 or Ci.max() >= self.n_categories):
            raise ValueError('`C` has entries outside the categories 0 .. {0}'.format(self.n_categories - 1))
        X = np.zeros((len(C), self.n_groups, self.n_categories), dtype=np.float32)
        np.put_along_axis(X, Ci[:, :, None], 1.0, axis=2)
        X[gone] = 0.0
        return X.reshape(len(C), self.n_visible)

    def decode(self, X, missing=None):
        """[N, n_groups * n_categories] (states or means) -> the argmax per group, int64 [N, n_groups]; with `missing` given,
        empty - all-zero - groups decode to it"""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        X3 = X.reshape(len(X), self.n_groups, self.n_categories)
        C = X3.argmax(axis=2)
        if missing is not None:
            C = np.where(np.any(X3 != 0, axis=2), C, missing)
        return C

    # ---- incomplete rows, clamped groups, exact group conditionals
    def _groups_of(self, X, what):
        """X as float32 [N, n_visible], every group of every row one-hot or empty (else ValueError) -> (X, observed [N, n_groups])"""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        X3 = X.reshape(len(X), self.n_groups, self.n_categories)
        ones, total = (X3 == 1).sum(axis=2), (X3 != 0).sum(axis=2)
        if np.any((total > 1) | (ones != total)):
            b, g = np.argwhere((total > 1) | (ones != total))[0]
            raise ValueError('%s.%s: group %d of row %d is neither one-hot nor empty (all zeros: a missing value)'
                             % (self.__class__.__name__, what, g, b))
        return X, total == 1

    def fit(self, X, X_val=None, *args, **kwargs):
        if self.missing_values:
            self._groups_of(X, 'fit')
            if X_val is not None:
                self._groups_of(X_val, 'fit')
        return super(SoftmaxVisible, self).fit(X, X_val, *args, **kwargs)

    @run_on_engine()
    def group_log_proba(self, X):
        """log p(v_g = k | v_-g) for every row, group and category, [N, n_groups, n_categories] float64, the hidden layer summed
        out exactly.  X : [N, n_visible], every group one-hot or empty.  For an observed group the conditioning set is every
        other observed group of the row (the term of the pseudo-likelihood over groups); for an empty group it is every
        observed group, the other empty groups being absent from the row's model: the exact prediction of a missing value.
        Draws nothing, changes nothing."""
        eng = self._on_device()
        X, _ = self._groups_of(X, 'group_log_proba')
        if not len(X):
            return np.zeros((0, self.n_groups, self.n_categories))
        S = eng.groups_scores(self._to_device(X), len(X)).reshape(len(X), self.n_groups, self.n_categories)
        S = S - S.max(axis=2, keepdims=True)
        return S - np.log(np.exp(S).sum(axis=2, keepdims=True))

    def predict_proba(self, X):
        """exp(group_log_proba(X)): [N, n_groups, n_categories]"""
        return np.exp(self.group_log_proba(X))

    def predict(self, X):
        """categories [N, n_groups] int64: an observed group keeps its category, an empty group takes the most probable one
        given the row's observed groups"""
        X, observed = self._groups_of(X, 'predict')
        X3 = X.reshape(len(X), self.n_groups, self.n_categories)
        return np.where(observed, X3.argmax(axis=2), self.group_log_proba(X).argmax(axis=2)).astype(np.int64)

    def pseudo_log_likelihood(self, X):
        """[N] float64: the sum over a row's observed groups of log p(v_g | v_-g), the pseudo-likelihood over groups"""
        X, _ = self._groups_of(X, 'pseudo_log_likelihood')
        X3 = X.reshape(len(X), self.n_groups, self.n_categories)
        return (self.group_log_proba(X) * X3).sum(axis=(1, 2))

    @run_on_engine(update_seed=True)
    def sample_groups_given(self, X, n_gibbs_steps=1000, return_means=False):
        """Conditional sampling over groups: the empty groups of every row of X are drawn jointly from p(v_free | v_observed)
        by block-Gibbs with the observed groups clamped (imputation of missing values).

        X : [N, n_visible], every group one-hot (observed) or empty (to be drawn).  The free groups start at uniform
        categories drawn under the call's seed.  Returns one-hot rows [N, n_visible] after `n_gibbs_steps` sweeps (with
        `return_means`: a pair, states and the means of the last visible pass); observed groups hold X in both.  Both layers
        are always sampled.  The rows are processed in slices of at most `batch_size`, every row drawing from its own position
        of the call's random stream: the result does not depend on the slicing.  One seed is drawn from the model's host
        stream; no parameter is changed."""
        eng = self._on_device()
        X, observed = self._groups_of(X, 'sample_groups_given')
        k = int(n_gibbs_steps)
        if k < 1:
            raise ValueError('`n_gibbs_steps` must be >= 1 (got {0})'.format(k))
        N = len(X)
        start_cats = np.random.RandomState(self._graph_seed).randint(0, self.n_categories, (N, self.n_groups))
        obs_units = np.repeat(observed, self.n_categories, axis=1)
        V0 = np.where(obs_units, X, self.encode(start_cats))
        Vd, Cd = self._to_device(V0), self._to_device(X)
        Md = self._to_device(obs_units.astype(np.float32))
        Hd = _ffi.DeviceArray((N, self.n_hidden), np.float32)
        Pd = _ffi.DeviceArray((N, self.n_visible), np.float32) if return_means else None
        try:
            for start in range(0, N, self.batch_size):
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.groups_gibbs_clamped(Vd, Hd, min(self.batch_size, N - start), k, Cd, Md, Pd, row=start)
            eng.sync()
        finally:
            eng.set_row_offset(0)
        return (Vd.numpy(), Pd.numpy()) if return_means else Vd.numpy()

    @run_on_engine(update_seed=True)
    def sample_v(self, n_samples, n_gibbs_steps=1000, V_init=None):
        """Unconditional samples of the visible units by single-temperature block-Gibbs: `n_samples` independent chains run
        `n_gibbs_steps` steps of (v ~ p(v|h), h ~ p(h|v)) from h ~ p(h | v_0); the one-hot states of the last step are returned,
        [n_samples, n_visible].

        V_init : [n_samples, n_visible] one-hot start of every chain; None: uniform categories drawn under the call's seed.
        Both layers are always sampled (`sample_v_states` / `sample_h_states` do not apply): every pass is a
        `bm_rbm_sample_v_from_h` / `bm_rbm_sample_h` call, which draw whatever the flags say, where `bm_rbm_gibbs` would follow
        them.  The rows are processed in slices of at most `batch_size`, every row drawing from its own position of the call's
        random stream: the result does not depend on the slicing.  One seed is drawn from the model's host stream; no
        parameter is changed."""
        eng = self._on_device()
        n_samples, n_gibbs_steps = int(n_samples), int(n_gibbs_steps)
        if n_samples < 1 or n_gibbs_steps < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        if V_init is None:
            V0 = self.encode(np.random.RandomState(self._graph_seed).randint(0, self.n_categories, (n_samples, self.n_groups)))
        else:
            V0 = np.ascontiguousarray(V_init, dtype=np.float32)
            if V0.shape != (n_samples, self.n_visible):
                raise ValueError('`V_init` has invalid shape {0}: expected [{1}, {2}]'.format(V0.shape, n_samples, self.n_visible))
        Vd = self._to_device(V0)
        Hd = _ffi.DeviceArray((n_samples, self.n_hidden), np.float32)
        try:
            for start in range(0, n_samples, self.batch_size):
                B = min(self.batch_size, n_samples - start)
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.sample_h(Vd, B, None, Hd, row=start, out_row=start)
                for _ in range(n_gibbs_steps):
                    eng.sample_v_from_h(Hd, B, None, Vd, row=start, out_row=start)
                    eng.sample_h(Vd, B, None, Hd, row=start, out_row=start)
            eng.sync()
        finally:
            eng.set_row_offset(0)
        return Vd.numpy()

    # ---- parallel tempering and the tempered negative phase
    def sample_v_tempered(self, n_samples, n_gibbs_steps=1000, n_temperatures=10, betas=None, V_init=None, return_stats=False):
        """Unconditional samples of the visible units by parallel tempering (replica exchange), as `BernoulliRBM.sample_v`:
        `n_samples` independent chains, each with one replica per temperature of the ladder 0 < betas[0] < ... < betas[-1] = 1,
        run `n_gibbs_steps` steps of (h ~ p_beta(h|v), exchange of neighbouring temperatures, v_g ~ softmax(beta (hW^T + vb)_g)
        per group); the replica at beta = 1 of every chain is returned as one-hot rows [n_samples, n_visible].  The hot replicas
        cross between modes the single-temperature `sample_v` stays in.

        betas : the ladder; None: float32(linspace(0, 1, n_temperatures + 1)[1:]).  `n_temperatures=1` is plain Gibbs.
        V_init : [n_samples, n_visible] complete one-hot start of every chain (all its replicas); None: uniform categories
        drawn on the device under the call's seed.
        With `return_stats` also the acceptance rate of every neighbouring pair of temperatures, [n_temperatures - 1].
        Both layers are always sampled; `missing_values` does not apply (every row of the ensemble is complete).  One seed is
        drawn from the model's host stream; no parameter is changed.  It replaces the ensemble of `set_group_tempering`, which
        the next `fit` builds again."""
        n_samples, n_gibbs_steps = int(n_samples), int(n_gibbs_steps)
        if n_samples < 1 or n_gibbs_steps < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        ladder = resolve_ladder(n_temperatures, betas)
        if V_init is not None:
            V_init = np.ascontiguousarray(V_init, dtype=np.float32)
            if V_init.shape != (n_samples, self.n_visible):
                raise ValueError('`V_init` has invalid shape {0}: expected [{1}, {2}]'.format(V_init.shape, n_samples, self.n_visible))
            _, observed = self._groups_of(V_init, 'sample_v_tempered')
            if not observed.all():
                b, g = np.argwhere(~observed)[0]
                raise ValueError('%s.sample_v_tempered: group %d of row %d of `V_init` is empty (the rows of a tempered ensemble '
                                 'are complete one-hot rows)' % (self.__class__.__name__, g, b))
        return self._sample_v_tempered_checked(n_samples, n_gibbs_steps, ladder, V_init, return_stats)

    @run_on_engine(update_seed=True)
    def _sample_v_tempered_checked(self, n_samples, n_gibbs_steps, ladder, V_init, return_stats):
        eng = self._on_device()
        try:
            eng.groups_set_missing(False)             # (the ensemble's rows are complete whatever `missing_values` says)
            return run_tempered_sampler(eng.groups_pt, n_samples, n_gibbs_steps, ladder, V_init, self.n_visible, return_stats)
        finally:
            eng.groups_set_missing(bool(self.missing_values))

    def _check_tempered_setting(self, what):
        if self.missing_values:
            self._softmax_refuse(what, 'a tempered negative phase with missing_values=True (a row of the tempered ensemble has no '
                                       'pattern of observed groups) is not built')
        return super(SoftmaxVisible, self)._check_tempered_setting(what)

    def set_group_tempering(self, enabled=True, n_temperatures=10, betas=None, n_chains=None):
        """Where the negative particles of `fit` come from: `enabled=True` - the beta = 1 replicas of a persistent tempered
        ensemble of `n_chains` chains (None: `batch_size`; at least `batch_size`) over the ladder `betas` (None:
        float32(linspace(0, 1, n_temperatures + 1)[1:])), every update sweeping all of it for `n_gibbs_steps` tempered steps -
        `BernoulliRBM.set_negative_phase('tempered')` with the softmax prop-down of `sample_v_tempered`; `enabled=False` - CD-k
        from the batch again.  The ensemble starts at uniform categories at the first update of every `fit()` call and again
        whenever the ladder or `n_chains` changed; `tempering_stats()` reports its swap acceptance.  Neither the ensemble nor
        this setting is written to checkpoints.  Refused with `missing_values=True` (ValueError, before the engine is touched),
        and wherever `BernoulliRBM.set_negative_phase('tempered')` is (BM355_DATA_PARALLEL).  `set_negative_phase('tempered')`
        itself stays refused for this class.  Returns self."""
        self._fast_weights = None
        if not enabled:
            self._neg_phase = None
            return self
        self._check_tempered_setting('set_group_tempering')
        self._set_negative_phase('tempered', n_temperatures, betas, n_chains)
        return self

    def _train_epoch_tempered(self, eng, *args, **kwargs):
        # (the ensemble and its updates live under the engine's groups prefix; everything else the epoch calls is the engine's)
        return super(SoftmaxVisible, self)._train_epoch_tempered(eng.groups_pt, *args, **kwargs)


class CategoricalRBM(SoftmaxVisible, BaseRBM):
    """RBM with softmax (categorical) visible units and Bernoulli hidden units: `n_groups` one-hot groups of `n_categories`
    units each, n_visible = n_groups * n_categories (no counterpart in the reference).  The model for ratings, quantised pixels,
    characters, categorical table columns.  See `SoftmaxVisible` for the unit and for what is refused."""

    def __init__(self, n_groups=1, n_categories=2, n_hidden=256, model_path='c_rbm_model/', *args, missing_values=False, **kwargs):
        self.n_groups, self.n_categories = n_groups, n_categories
        # incomplete rows: an all-zero group of a training row is a missing value, absent from the row's model
        self.missing_values = missing_values
        n_visible = kwargs.pop('n_visible', None)          # (params.json carries it: load_model hands it back)
        if n_visible is not None and int(n_visible) != int(n_groups) * int(n_categories):
            raise ValueError('CategoricalRBM: n_visible = %r is not n_groups x n_categories = %r x %r' % (n_visible, n_groups, n_categories))
        super(CategoricalRBM, self).__init__(n_visible=int(n_groups) * int(n_categories), n_hidden=n_hidden, model_path=model_path,
                                             *args, **kwargs)


class ReplicatedSoftmaxVisible(object):
    """Replicated softmax visible units (Salakhutdinov & Hinton 2009), mixed in in front of an RBM class: the
    visible layer is ONE softmax over the whole vocabulary of `n_visible` words, drawn D times per document and summed into a
    count vector; the hidden bias is scaled by the document length D.  The RBM for bag-of-words data.

    Rows of X are count vectors: non-negative integers whose sum D = X.sum(axis=1) lies in [1, max_length].
    p(h_j = 1 | v) = sigmoid(D hb_j + (vW)_j);  v | h ~ Multinomial(D, softmax(vb + W h)), means D * softmax;
    F(v) = -v.vb - sum_j softplus(D hb_j + (vW)_j).  The update is the Bernoulli one with the hidden-bias gradient
    (1/N) sum_b D_b (h0_b - hk_b).  `fit`, `transform`, `sample_h`, checkpoints, `load_model` and `init_from` work as for the
    other classes; `sample_v_from_h` and `sample_v` take the documents' lengths; `free_energy` gives F per row; `encode` turns
    lists of token ids into count rows; `ais_log_Z` / `ais_log_Z_rows` estimate log Z per document length by AIS, and
    `log_likelihood` / `perplexity` score held-out documents with it; `sample_v_tempered` samples documents by
    parallel tempering and `set_count_tempering` makes `fit` take its negative particles from a tempered ensemble (DESIGN.md
    3.31).  What is not built for word counts is refused with a ValueError before the engine is
    touched: the `pll` and `feg` metrics, `dropout`, a non-zero `sparsity_cost`, `dbm_first` / `dbm_last`, dtype='float64',
    `set_negative_phase` other than 'cd', `set_centering`, `set_classes`, `sample_v_given`, `log_Z` / `log_proba`,
    BM355_DATA_PARALLEL jobs, and use as a layer of a `DBM` or a `StackClassifier`."""

    _UNIT_NAME = 'replicated softmax visible units'
    _PT_VIEW, _PT_SETTER = 'rsm_pt', 'set_count_tempering()'         # (tempering_stats: the ensemble of `set_count_tempering`)
    _MAX_VISIBLE = 16384         # csrc/bm_rsm.h: RSM_MAX_V

    @property
    def _RSM_MAX_LENGTH(self):
        return int(self.max_length)

    def _rsm_refuse(self, what, why):
        raise ValueError('%s.%s: %s with %s' % (self.__class__.__name__, what, why, self._UNIT_NAME))

    def _check_rsm_config(self, what):
        """the constructor keywords the unit does not combine with (set_params may change them: checked again before the
        engine is built)"""
        name = self.__class__.__name__
        if not 1 <= int(self.max_length) < (1 << 24):
            raise ValueError('%s.%s: max_length must be in [1, 2^24) for %s (got %r)' % (name, what, self._UNIT_NAME, self.max_length))
        if not 2 <= int(self.n_visible) <= self._MAX_VISIBLE:
            raise ValueError('%s.%s: n_visible must be in [2, %d] for %s (got %r)' % (name, what, self._MAX_VISIBLE, self._UNIT_NAME,
                                                                                   self.n_visible))
        if self.metrics_config.get('pll'):
            self._rsm_refuse(what, "metrics_config['pll'] flips single bits, which leaves the count vectors; it is not defined")
        if self.metrics_config.get('feg'):
            self._rsm_refuse(what, "metrics_config['feg'] (the batch free energy has no length-scaled bias) is not built; "
                                   "`free_energy` gives the rows' free energies")
        if self.dropout is not None:
            self._rsm_refuse(what, 'dropout (dropout=%r) is not combined' % (self.dropout,))
        if self.sparsity_cost != 0:
            self._rsm_refuse(what, 'a sparsity penalty (sparsity_cost=%r) is not combined' % (self.sparsity_cost,))
        if self.dbm_first or self.dbm_last:
            self._rsm_refuse(what, 'dbm_first / dbm_last (a doubled conditional, a DBM layer) is not built')
        if np.dtype(self.dtype) != np.float32:
            self._rsm_refuse(what, "dtype='%s' is not supported (float32 only)" % np.dtype(self.dtype).name)

    def __init__(self, *args, **kwargs):
        super(ReplicatedSoftmaxVisible, self).__init__(*args, **kwargs)
        self._check_rsm_config('__init__')

    def _ensure_engine(self):
        if self._engine is None:
            self._check_rsm_config('fit')
            if os.environ.get('BM355_DATA_PARALLEL', '0') == '1':
                self._rsm_refuse('fit', 'data-parallel mode (BM355_DATA_PARALLEL) is not combined: the split step is not built')
        return super(ReplicatedSoftmaxVisible, self)._ensure_engine()

    def set_negative_phase(self, kind='cd', *args, **kwargs):
        if kind != 'cd':
            self._rsm_refuse('set_negative_phase', 'a %r negative phase (the tempered sweep has no count sampler) is not built' % (kind,))
        return super(ReplicatedSoftmaxVisible, self).set_negative_phase(kind, *args, **kwargs)

    def set_centering(self, enabled=True, *args, **kwargs):
        if enabled:
            self._rsm_refuse('set_centering', 'centering is not combined')
        return super(ReplicatedSoftmaxVisible, self).set_centering(enabled, *args, **kwargs)

    def set_classes(self, n_classes, *args, **kwargs):
        if n_classes is not None:
            self._rsm_refuse('set_classes', 'a class head is not built')
        return super(ReplicatedSoftmaxVisible, self).set_classes(n_classes, *args, **kwargs)

    def sample_v_given(self, *args, **kwargs):
        self._rsm_refuse('sample_v_given', 'the clamped sweep is not built')

    def log_Z(self, *args, **kwargs):
        self._rsm_refuse('log_Z', 'AIS (its base model and its sweeps are Bernoulli) is not built; log Z depends on the document '
                                  'length here: `ais_log_Z` / `ais_log_Z_rows` are the estimators')

    def log_proba(self, *args, **kwargs):
        self._rsm_refuse('log_proba', 'the log-likelihood (it needs log Z per document length) is not built; `log_likelihood` and '
                                      '`perplexity` take the rows\' log Z from `ais_log_Z_rows`')

    # ---- AIS log Z per document length, log-likelihood, perplexity
    _AIS_MAX_ROWS = 1 << 16      # chains of one engine call; longer runs go through chain0 in chunks (the slice property)

    def _base_logits(self, X_base):
        """the logits `a` of the AIS base model p_0(v) = Multinomial(D, softmax(a)): None (uniform), `a` itself [V], or count
        rows [N][V] -> the smoothed unigram a_i = log((sum_n X[n,i] + 1) / (sum_n D_n + V)) (float64, handed over as float32)"""
        if X_base is None:
            return None
        X = np.asarray(X_base, dtype=np.float64)
        if X.ndim == 2 and X.shape[1] == self.n_visible:
            X, D = self._counts_of(X, 'ais_log_Z')
            count = X.astype(np.float64).sum(axis=0)
            return np.log((count + 1.) / (float(D.sum()) + self.n_visible)).astype(np.float32)
        if X.shape != (self.n_visible,) or not np.all(np.isfinite(X)):
            raise ValueError('`X_base` has invalid shape {0} or entries: expected count rows [N, {1}] or finite logits [{1}]'
                             .format(X.shape, self.n_visible))
        return X.astype(np.float32)

    def _ais_lengths(self, lengths, what):
        """(lengths as int64 [L], scalar?) - integers in [1, max_length], a scalar or a 1-D array"""
        D = np.asarray(lengths)
        scalar = D.ndim == 0
        D = D.reshape(1) if scalar else D
        ok = D.ndim == 1 and len(D) >= 1 and D.dtype.kind in 'iuf'
        ok = ok and bool(np.all(np.isfinite(D)) and np.all(D == np.trunc(D)) and np.all(D >= 1) and np.all(D <= int(self.max_length)))
        if not ok:
            raise ValueError('%s.%s: `lengths` must be an integer or a 1-D array of integers in [1, max_length = %d]'
                             % (self.__class__.__name__, what, int(self.max_length)))
        return D.astype(np.int64), scalar

    def ais_log_Z(self, lengths, n_betas=100, n_runs=100, n_gibbs_steps=5, X_base=None):
        """AIS estimates of log Z_D, the log partition function over the count vectors of D tokens, for every D in `lengths`:
        Z_D = sum_h exp(D h.hb) (sum_i exp(vb_i + (W h)_i))^D depends on the document length, so a held-out set needs one
        estimate per distinct length.  All of them come from ONE run whose chains have different lengths.

        lengths : an integer or a 1-D array of L integers in [1, max_length]; duplicates get chains of their own.
        Returns log_mean, (log_low, log_high), values - per length what `BernoulliRBM.log_Z` returns - of shapes [L], ([L], [L])
        and [L, n_runs]; a scalar `lengths` gives scalars and [n_runs].
        `n_runs` chains per length run from the base model p_0(v) = Multinomial(D, softmax(a)) through `n_betas` temperatures
        linspace(0, 1, n_betas) with `n_gibbs_steps` transitions each, the hidden layer summed out:
        log p*_beta(v) = log(D!/prod v_i!) + (1 - beta) a.v + beta vb.v + sum_j softplus(beta (D hb + vW)_j).
        X_base : None - the uniform base (a = 0); [N, n_visible] count rows - their smoothed unigram,
        a_i = log((sum_n X[n,i] + 1) / (sum_n D_n + n_visible)); an [n_visible] array - the logits `a` themselves.
        The chain of length lengths[l] and run r has index l * n_runs + r in the call's random streams, whatever the chunking.
        Both layers are always sampled.  One seed is drawn from the model's host stream; no parameter is changed."""
        n_betas, n_runs, n_gibbs_steps = int(n_betas), int(n_runs), int(n_gibbs_steps)
        if n_betas < 2 or n_runs < 1 or n_gibbs_steps < 1:
            raise ValueError('%s.ais_log_Z: n_betas must be >= 2, n_runs and n_gibbs_steps >= 1 (got %d, %d, %d)'
                             % (self.__class__.__name__, n_betas, n_runs, n_gibbs_steps))
        D, scalar = self._ais_lengths(lengths, 'ais_log_Z')
        a = self._base_logits(X_base)
        values = self._rsm_ais_checked(n_betas, np.repeat(D, n_runs), n_gibbs_steps, a).reshape(len(D), n_runs)
        log_mean, log_low, log_high = (np.zeros(len(D)) for _ in range(3))
        for l in range(len(D)):
            log_mean[l] = log_mean_exp(values[l])
            log_std = log_std_exp(values[l], log_mean_exp_x=log_mean[l])
            log_high[l] = log_sum_exp([log_std, log_mean[l]])
            log_low[l] = log_diff_exp([log_std, log_mean[l]])[0]
        if scalar:
            return log_mean[0], (log_low[0], log_high[0]), values[0]
        return log_mean, (log_low, log_high), values

    @run_on_engine(update_seed=True)
    def _rsm_ais_checked(self, n_betas, D_rows, n_gibbs_steps, a):
        """[len(D_rows)] float32: chain c has length D_rows[c]; chunks of at most _AIS_MAX_ROWS chains through chain0"""
        eng = self._on_device()
        out = np.empty(len(D_rows), dtype=np.float32)
        for c0 in range(0, len(D_rows), self._AIS_MAX_ROWS):
            c1 = min(len(D_rows), c0 + self._AIS_MAX_ROWS)
            out[c0:c1] = eng.rsm_ais(n_betas, D_rows[c0:c1], n_gibbs_steps, seed=self._graph_seed, chain0=c0, base_logits=a)
        return out

    def ais_log_Z_rows(self, X, **ais_kwargs):
        """[N] float64: for every count row of X the AIS log Z of its length, so that `log_likelihood(X, ais_log_Z_rows(X))` is
        the held-out log-likelihood.  The DISTINCT lengths of X go through one `ais_log_Z` call - one run, one seed - and every
        row gets the log_mean of its length.  `ais_kwargs`: n_betas, n_runs, n_gibbs_steps, X_base."""
        if 'lengths' in ais_kwargs:
            raise ValueError('%s.ais_log_Z_rows: the lengths come from `X`; `lengths` is not an argument' % self.__class__.__name__)
        _, D = self._counts_of(X, 'ais_log_Z_rows')
        if not len(D):
            return np.zeros(0)
        distinct, index = np.unique(D, return_inverse=True)
        return np.asarray(self.ais_log_Z(distinct, **ais_kwargs)[0], dtype=np.float64)[index.reshape(-1)]

    @staticmethod
    def _log_coefficient(X):
        """log(D! / prod_i v_i!) per count row, float64"""
        from math import lgamma
        Xi = np.asarray(X).astype(np.int64)
        D = Xi.sum(axis=1)
        vals = np.unique(np.concatenate([Xi.reshape(-1), D]))          # lgamma once per distinct integer
        lg = np.array([lgamma(v + 1.) for v in vals], dtype=np.float64)
        return lg[np.searchsorted(vals, D)] - lg[np.searchsorted(vals, Xi)].sum(axis=1)

    def log_likelihood(self, X, log_Z_rows, ordered=False):
        """[N] float64 log-probabilities of the count rows of X given the log partition function of every row's length
        (`ais_log_Z_rows(X)`, or exact values).
        ordered=False : log p(v) = log(D!/prod_i v_i!) - F(v) - log Z_D, the probability of the COUNT VECTOR (these sum to one over
        the count vectors of a length); the coefficient is computed in float64 on the host.
        ordered=True : -F(v) - log Z_D, the probability of ONE token sequence with those counts (the coefficient left out)."""
        X, D = self._counts_of(X, 'log_likelihood')
        lz = np.asarray(log_Z_rows, dtype=np.float64)
        if lz.shape != (len(X),):
            raise ValueError('`log_Z_rows` has invalid shape {0}: expected [{1}], one value per row'.format(lz.shape, len(X)))
        if not len(X):
            return np.zeros(0)
        lp = -np.asarray(self.free_energy(X), dtype=np.float64) - lz
        return lp if ordered else lp + self._log_coefficient(X)

    def perplexity(self, X, log_Z_rows):
        """exp(-mean_n(log p_ordered(v_n) / D_n)): the per-word perplexity of Salakhutdinov & Hinton (2009), from the probability
        of a document as a token SEQUENCE (`log_likelihood(..., ordered=True)`: no multinomial coefficient), so that it compares
        with a unigram model's exp(-mean_n (1/D_n) sum_i v_ni log q_i) and with the uniform model's n_visible."""
        X, D = self._counts_of(X, 'perplexity')
        if not len(X):
            raise ValueError('`X` has no rows')
        return float(np.exp(-np.mean(self.log_likelihood(X, log_Z_rows, ordered=True) / D.astype(np.float64))))

    # ---- count rows
    def _counts_of(self, X, what):
        """X as float32 [N, n_visible] with its lengths [N] int64; ValueError names the condition a row fails"""
        name = self.__class__.__name__
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`X` has invalid shape {0}: expected [N, {1}]'.format(X.shape, self.n_visible))
        if not np.all(np.isfinite(X)) or np.any(X != np.trunc(X)):
            b = int(np.argwhere(~(np.isfinite(X) & (X == np.trunc(X))))[0][0])
            raise ValueError('%s.%s: row %d is not integer-valued (%s take word counts)' % (name, what, b, self._UNIT_NAME))
        if np.any(X < 0):
            raise ValueError('%s.%s: row %d has a negative entry (%s take word counts)'
                             % (name, what, int(np.argwhere(X < 0)[0][0]), self._UNIT_NAME))
        D = X.astype(np.float64).sum(axis=1)
        if np.any(D < 1):
            raise ValueError('%s.%s: row %d is empty (length 0; %s need at least one token)'
                             % (name, what, int(np.argwhere(D < 1)[0][0]), self._UNIT_NAME))
        if np.any(D > int(self.max_length)):
            b = int(np.argwhere(D > int(self.max_length))[0][0])
            raise ValueError('%s.%s: row %d has length %d > max_length = %d (%s)' % (name, what, b, int(D[b]), int(self.max_length),
                                                                                  self._UNIT_NAME))
        return X, D.astype(np.int64)

    def lengths(self, X):
        """document lengths D = X.sum(axis=1), [N] int64, of count rows X (validated as `fit` validates them)"""
        return self._counts_of(X, 'lengths')[1]

    def encode(self, docs):
        """documents (sequences of token ids in [0, n_visible)) -> count rows [N, n_visible] float32"""
        X = np.zeros((len(docs), self.n_visible), dtype=np.float32)
        for b, doc in enumerate(docs):
            ids = np.asarray(doc, dtype=np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= self.n_visible):
                raise ValueError('%s.encode: document %d has a token id outside [0, %d)' % (self.__class__.__name__, b, self.n_visible))
            np.add.at(X[b], ids, 1.0)
        return X

    def _lengths_arg(self, lengths, N, what):
        D = np.asarray(lengths)
        D = np.repeat(D.reshape(1), N) if D.ndim == 0 else D.reshape(-1)
        if len(D) != N or np.any(D != np.trunc(D)) or np.any(D < 1) or np.any(D > int(self.max_length)):
            raise ValueError('%s.%s: `lengths` must be one integer in [1, max_length = %d] per row (%d rows)'
                             % (self.__class__.__name__, what, int(self.max_length), N))
        return np.ascontiguousarray(D, dtype=np.float32)

    def fit(self, X, X_val=None, *args, **kwargs):
        self._fit_lengths = self._counts_of(X, 'fit')[1]       # (set_count_tempering: the chains' lengths come from these)
        if X_val is not None:
            self._counts_of(X_val, 'fit')
        return super(ReplicatedSoftmaxVisible, self).fit(X, X_val, *args, **kwargs)

    @run_on_engine()
    def free_energy(self, X):
        """F(v) = -v.vb - sum_j softplus(D hb_j + (vW)_j) of every count row of X, [N] float32.  Draws nothing, changes nothing."""
        eng = self._on_device()
        X, _ = self._counts_of(X, 'free_energy')
        if not len(X):
            return np.zeros(0, dtype=np.float32)
        return eng.free_energy_rows(self._to_device(X), len(X))

    @run_on_engine(update_seed=True)
    def sample_v_from_h(self, H, lengths, return_means=False):
        """One draw of the count vectors given H, v ~ Multinomial(D, softmax(vb + W h)), by a single prop-down.

        H : [N, n_hidden], taken as given; lengths : the documents' lengths D, one integer or [N].  Returns the counts
        [N, n_visible] (with `return_means`: a pair, counts and the expected counts D * softmax); every row sums to its D.  The
        rows are processed in slices of at most `batch_size`; draw d of row r reads position r * max_length + d of the call's
        random stream: the result does not depend on the slicing.  One seed is drawn from the model's host stream; no parameter
        is changed."""
        eng = self._on_device()
        H = np.ascontiguousarray(H, dtype=np.float32)
        if H.ndim != 2 or H.shape[1] != self.n_hidden:
            raise ValueError('`H` has invalid shape {0}: expected [N, {1}]'.format(H.shape, self.n_hidden))
        N = len(H)
        Dd = self._to_device(self._lengths_arg(lengths, N, 'sample_v_from_h'))
        Hd = self._to_device(H)
        Sd = _ffi.DeviceArray((N, self.n_visible), np.float32)
        Md = _ffi.DeviceArray((N, self.n_visible), np.float32) if return_means else None
        try:
            for start in range(0, N, self.batch_size):
                B = min(self.batch_size, N - start)
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.set_row_lengths(Dd, B, row=start)
                eng.sample_v_from_h(Hd, B, Md, Sd, row=start, out_row=start)
            eng.sync()
        finally:
            eng.set_row_offset(0)
        return (Sd.numpy(), Md.numpy()) if return_means else Sd.numpy()

    @run_on_engine(update_seed=True)
    def sample_v(self, n_samples, lengths, n_gibbs_steps=1000, V_init=None):
        """Unconditional documents of given lengths by single-temperature block-Gibbs: `n_samples` independent chains run
        `n_gibbs_steps` steps of (v ~ p(v|h), h ~ p(h|v)) from h ~ p(h | v_0); the count rows of the last step are returned,
        [n_samples, n_visible].

        lengths : the documents' lengths D, one integer or [n_samples]; every step draws exactly D tokens per row.
        V_init : [n_samples, n_visible] count rows of those lengths; None: D tokens drawn uniformly over the vocabulary under
        the call's seed.  Both layers are always sampled.  The rows are processed in slices of at most `batch_size`, every row
        drawing from its own position of the call's random stream: the result does not depend on the slicing.  One seed is
        drawn from the model's host stream; no parameter is changed."""
        eng = self._on_device()
        n_samples, n_gibbs_steps = int(n_samples), int(n_gibbs_steps)
        if n_samples < 1 or n_gibbs_steps < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        D = self._lengths_arg(lengths, n_samples, 'sample_v')
        if V_init is None:
            rng = np.random.RandomState(self._graph_seed)
            V0 = self.encode([rng.randint(0, self.n_visible, int(d)) for d in D])
        else:
            V0, D0 = self._counts_of(V_init, 'sample_v')
            if V0.shape != (n_samples, self.n_visible) or np.any(D0 != D):
                raise ValueError('`V_init` must be [{0}, {1}] count rows of the given lengths'.format(n_samples, self.n_visible))
        Vd, Dd = self._to_device(V0), self._to_device(D)
        Hd = _ffi.DeviceArray((n_samples, self.n_hidden), np.float32)
        try:
            for start in range(0, n_samples, self.batch_size):
                B = min(self.batch_size, n_samples - start)
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.set_row_lengths(Dd, B, row=start)
                eng.sample_h(Vd, B, None, Hd, row=start, out_row=start)
                for _ in range(n_gibbs_steps):
                    eng.sample_v_from_h(Hd, B, None, Vd, row=start, out_row=start)
                    eng.sample_h(Vd, B, None, Hd, row=start, out_row=start)
            eng.sync()
        finally:
            eng.set_row_offset(0)
        return Vd.numpy()

    # ---- parallel tempering and the tempered negative phase
    def sample_v_tempered(self, n_samples, lengths, n_gibbs_steps=1000, n_temperatures=10, betas=None, V_init=None, return_stats=False):
        """Unconditional documents of given lengths by parallel tempering (replica exchange), as `BernoulliRBM.sample_v`:
        `n_samples` independent chains, each with one replica per temperature of the ladder 0 < betas[0] < ... < betas[-1] = 1,
        run `n_gibbs_steps` steps of (h ~ Ber(sigmoid(beta (D hb + vW))), exchange of neighbouring temperatures,
        v ~ Multinomial(D, softmax(beta (vb + W h)))); the replica at beta = 1 of every chain is returned as count rows
        [n_samples, n_visible], every row summing to its length.  The multinomial coefficient is the base measure and is not
        tempered; all replicas of a chain share its length.  The hot replicas cross between the topic mixtures the
        single-temperature `sample_v` stays in.

        lengths : the documents' lengths D, one integer or [n_samples] integers in [1, max_length].
        betas : the ladder; None: float32(linspace(0, 1, n_temperatures + 1)[1:]).  `n_temperatures=1` is plain Gibbs.
        V_init : [n_samples, n_visible] count rows of those lengths, the start of every chain (all its replicas); None: D tokens
        drawn uniformly over the vocabulary on the device under the call's seed.
        With `return_stats` also the acceptance rate of every neighbouring pair of temperatures, [n_temperatures - 1].
        Both layers are always sampled.  One seed is drawn from the model's host stream; no parameter is changed.  It replaces
        the ensemble of `set_count_tempering`, which the next `fit` builds again."""
        n_samples, n_gibbs_steps = int(n_samples), int(n_gibbs_steps)
        if n_samples < 1 or n_gibbs_steps < 1:
            raise ValueError('`n_samples` and `n_gibbs_steps` must be >= 1 (got {0}, {1})'.format(n_samples, n_gibbs_steps))
        D, scalar = self._ais_lengths(lengths, 'sample_v_tempered')
        D = np.repeat(D, n_samples) if scalar else D
        if len(D) != n_samples:
            raise ValueError('%s.sample_v_tempered: `lengths` must be one integer or one per sample (%d for %d samples)'
                             % (self.__class__.__name__, len(D), n_samples))
        ladder = resolve_ladder(n_temperatures, betas)
        if V_init is not None:
            V_init, D0 = self._counts_of(V_init, 'sample_v_tempered')
            if V_init.shape != (n_samples, self.n_visible) or np.any(D0 != D):
                raise ValueError('`V_init` must be [{0}, {1}] count rows of the given lengths'.format(n_samples, self.n_visible))
        return self._sample_v_tempered_checked(n_samples, D, n_gibbs_steps, ladder, V_init, return_stats)

    @run_on_engine(update_seed=True)
    def _sample_v_tempered_checked(self, n_samples, D, n_gibbs_steps, ladder, V_init, return_stats):
        return run_tempered_sampler(self._on_device().rsm_pt, n_samples, n_gibbs_steps, ladder, V_init, self.n_visible, return_stats,
                                    lengths=D)

    def _check_tempered_setting(self, what):
        self._check_rsm_config(what)
        if os.environ.get('BM355_DATA_PARALLEL', '0') == '1':
            self._rsm_refuse(what, 'a tempered negative phase in data-parallel mode (BM355_DATA_PARALLEL: chains are not sharded '
                                   'over ranks) is not built')

    def set_count_tempering(self, enabled=True, n_temperatures=10, betas=None, n_chains=None, chain_lengths=None):
        """Where the negative particles of `fit` come from: `enabled=True` - the beta = 1 replicas of a persistent tempered
        ensemble of `n_chains` chains (None: `batch_size`; at least `batch_size`) over the ladder `betas` (None:
        float32(linspace(0, 1, n_temperatures + 1)[1:])), every update sweeping all of it for `n_gibbs_steps` tempered steps -
        `BernoulliRBM.set_negative_phase('tempered')` with the count sampler of `sample_v_tempered`; `enabled=False` - CD-k from
        the batch again.

        chain_lengths : [n_chains] integers in [1, max_length], the document length of every chain, fixed for the life of the
        ensemble; None: the lengths of the first `n_chains` rows of the `X` of the `fit` call, cycled.  The chains' lengths STAND
        FOR THE CORPUS'S LENGTH DISTRIBUTION in the negative term: negative particle b of an update is a document of chain b's
        length, not of batch row b's, and its hidden-bias statistic is weighted by that length (D_b h0_b - Dn_b hk_b).  Take
        them from the corpus (the default) unless there is a reason not to.

        The ensemble starts at uniform tokens at the first update of every `fit()` call and again whenever the ladder, `n_chains`
        or the chains' lengths changed; no extra seed is drawn; `tempering_stats()` reports its swap acceptance.  Neither the
        ensemble nor this setting is written to checkpoints.  `set_negative_phase('tempered')` itself stays refused for this
        class.  Returns self."""
        self._fast_weights = None
        if not enabled:
            self._neg_phase = None
            self._count_chain_lengths = None
            return self
        self._check_tempered_setting('set_count_tempering')
        if chain_lengths is not None:
            D, scalar = self._ais_lengths(chain_lengths, 'set_count_tempering')
            want = int(self.batch_size if n_chains is None else n_chains)
            if scalar or len(D) != want:
                raise ValueError('%s.set_count_tempering: `chain_lengths` must hold one length per chain (%d chains)'
                                 % (self.__class__.__name__, want))
            chain_lengths = tuple(int(d) for d in D)
        self._set_negative_phase('tempered', n_temperatures, betas, n_chains)
        self._count_chain_lengths = chain_lengths
        return self

    def _train_chain_lengths(self):
        n_chains = self._neg_phase[1]
        given = getattr(self, '_count_chain_lengths', None)
        if given is not None:
            return tuple(given)
        D = getattr(self, '_fit_lengths', None)
        if D is None or not len(D):
            raise RuntimeError('set_count_tempering: no chain lengths (fit() takes them from its X)')
        return tuple(int(d) for d in np.resize(D, n_chains))

    def _ensure_train_ensemble(self, eng):
        """`eng` is the engine's rsm_pt view; a change of the chains' lengths builds the ensemble again"""
        D = self._train_chain_lengths()
        if getattr(eng, '_train_len_key', None) != D:
            self._pt_fresh = True
        eng.train_lengths, eng._train_len_key = np.asarray(D, dtype=np.float32), D
        return super(ReplicatedSoftmaxVisible, self)._ensure_train_ensemble(eng)

    def _train_epoch_tempered(self, eng, *args, **kwargs):
        # (the ensemble and its updates live under the engine's rsm prefix; everything else the epoch calls is the engine's)
        return super(ReplicatedSoftmaxVisible, self)._train_epoch_tempered(eng.rsm_pt, *args, **kwargs)


class ReplicatedSoftmaxRBM(ReplicatedSoftmaxVisible, BaseRBM):
    """RBM with a replicated softmax (word-count) visible layer and Bernoulli hidden units: `n_visible` is the vocabulary size,
    `max_length` the longest document the model will see (no counterpart in the reference).  The model for bag-of-words data.
    See `ReplicatedSoftmaxVisible` for the unit and for what is refused."""

    def __init__(self, n_visible=2000, n_hidden=256, max_length=1000, model_path='rs_rbm_model/', *args, **kwargs):
        self.max_length = max_length
        super(ReplicatedSoftmaxRBM, self).__init__(n_visible=n_visible, n_hidden=n_hidden, model_path=model_path, *args, **kwargs)


def logit_mean(X):
    """log(p / (1 - p)) of the per-feature mean, clipped (reference rbm/rbm.py:119-123)."""
    p = np.mean(X, axis=0)
    p = np.clip(p, 1e-7, 1. - 1e-7)
    q = np.log(p / (1. - p))
    return q
