"""Class head of a BernoulliRBM: the Python side.

Larochelle & Bengio 2008, "Classification using discriminative restricted Boltzmann machines".  A head of C classes on the
hidden layer - U [C, H], yb [C] beside the RBM's own W, hb, vb - gives the exact class posterior

    z = x W + hb,   s_c = yb_c + sum_i softplus(z_i + U[c, i]),   log p(c|x) = s_c - logsumexp_c' s_c'

and `fit_discriminative` ascends the batch mean of log p(t|x) with the exact gradient (no sampling), through the update rules
of `fit` (bm_rbm_set_classes / bm_rbm_class_*, include/bm355.h).  The workflow: `fit(X)` unsupervised, `set_classes(C)`,
`fit_discriminative(X, y)`, `predict(X)`.  `fit_joint(X, y)` trains the joint p(x, y) of the same model with CD-k instead (or,
with `discriminative_weight`, both objectives in one update) and `sample_v_given_class(y)` draws x given a class (DESIGN.md
3.19; bm_rbm_class_joint_* / bm_rbm_class_gibbs); `fit_semi_supervised(X, y, X_unlabelled)` interleaves it with updates on unlabelled
rows, which train the same parameters through log p(x) = log sum_y p(x, y) (bm_rbm_class_unsup_* /
bm_rbm_class_semi_train_epoch).  The head is model state like the momentum buffers: U, yb, dU, dyb go into model.npz
(`class_U`, `class_yb`, `class_dU`, `class_dyb`) and `n_classes` into params.json only while a head is attached; a model
without a head is saved exactly as before.
"""
import os

import numpy as np

from .base import run_on_engine
from .utils import make_list_from, write_during_training

_CLASS_VARS = ('U', 'yb', 'dU', 'dyb')
_PREDICT_ROWS = 4096          # rows per engine call of predict_log_proba (bounds the workspaces, not the input)


def validate_labels(y, n_rows, n_classes):
    """labels for `n_rows` rows of a head of `n_classes` classes -> contiguous int32 [n_rows]; ValueError for anything that is not
    a one-dimensional integer array of that length with every entry in [0, n_classes)"""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError('`y` has invalid shape {0}: expected [{1}]'.format(y.shape, n_rows))
    if len(y) != n_rows:
        raise ValueError('`y` has {0} labels for {1} rows of `X`'.format(len(y), n_rows))
    if not (np.issubdtype(y.dtype, np.integer) or y.dtype == np.bool_):
        raise ValueError('`y` must hold integer class labels (got dtype {0})'.format(y.dtype))
    if len(y) and (y.min() < 0 or y.max() >= n_classes):
        bad = y[(y < 0) | (y >= n_classes)][0]
        raise ValueError('`y` holds the label {0} outside [0, n_classes={1})'.format(int(bad), n_classes))
    return np.ascontiguousarray(y, dtype=np.int32)


class ClassHead(object):
    """`self._class_head` is None (no head) or dict(C=n_classes, pending=None | {name: array}): `pending` holds the head's
    variables while no engine has them (before the engine is built, across a rebuild, after load_model).  `n_classes` is an
    INSTANCE attribute only while a head is attached, so that params.json of a model without one keeps its schema."""
    _class_head = None
    n_classes = None

    # ---- checks that need no device
    def _check_class_head(self, what, train=False):
        name = '%s.%s' % (self.__class__.__name__, what)
        from . import _ffi
        if self._V_UNIT != _ffi.UNIT_BERNOULLI:
            raise ValueError('%s: a class head needs Bernoulli visible units (Gaussian visible units are not supported)' % name)
        if self._H_UNIT != _ffi.UNIT_BERNOULLI:
            raise ValueError('%s: a class head needs Bernoulli hidden units (Multinomial hidden units are not supported)' % name)
        if np.dtype(self.dtype) != np.float32:
            raise ValueError("%s: the class head runs in float32 only (dtype=%r)" % (name, self.dtype))
        if self.dbm_first or self.dbm_last:
            raise ValueError('%s: a dbm_first / dbm_last model (one conditional doubled) takes no class head' % name)
        if what != 'set_classes' and self._class_head is None:
            raise ValueError('%s: no class head is attached; call set_classes(n_classes) first' % name)
        if train:
            if self.dropout is not None:
                raise ValueError('%s is not combined with dropout (dropout=%r)' % (name, self.dropout))
            if self.sparsity_cost != 0.:
                raise ValueError('%s is not combined with the sparsity penalty (sparsity_cost=%r)' % (name, self.sparsity_cost))
            if self._centering is not None:
                raise ValueError('%s is not combined with centering; call set_centering(False) first' % name)
            if os.environ.get('BM355_DATA_PARALLEL', '0') == '1' or getattr(self, '_dp', None) is not None:
                raise ValueError('%s is not combined with data parallelism (BM355_DATA_PARALLEL)' % name)
        return name

    def _check_class_X(self, X, name='X'):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.n_visible:
            raise ValueError('`{0}` has invalid shape {1}: expected [N, {2}]'.format(name, X.shape, self.n_visible))
        return X

    # ---- the head
    def set_classes(self, n_classes, U=None, yb=None, U_std=0.01):
        """Attach a head of `n_classes` >= 2 classes to this BernoulliRBM, or detach it (`n_classes=None`).

        U : [n_classes, n_hidden] class weights; None: a normal draw of standard deviation `U_std` from the model's seeded host
            stream (the stream `make_random_seed` draws from).  yb : [n_classes] class biases; None: zeros.  The momentum
        buffers start at zero.  An attached head is replaced.  BernoulliRBM in float32 only: GaussianRBM, MultinomialRBM,
        float64 and `dbm_first` / `dbm_last` models raise ValueError.  Nothing else about the model changes.  Returns self."""
        if n_classes is None:
            was, self._class_head = self._class_head, None
            self.__dict__.pop('n_classes', None)
            if was is not None and self._engine is not None and was['pending'] is None:
                self._engine.set_classes(0)
            return self
        self._check_class_head('set_classes')
        C, H = int(n_classes), self.n_hidden
        if C != n_classes or C < 2:
            raise ValueError('set_classes: n_classes must be an integer >= 2 or None (got {0!r})'.format(n_classes))
        if U is None:
            U = self._rng.normal(0., float(U_std), (C, H))
        U = np.ascontiguousarray(U, dtype=np.float32)
        yb = np.zeros(C, dtype=np.float32) if yb is None else np.ascontiguousarray(yb, dtype=np.float32)
        if U.shape != (C, H):
            raise ValueError('`U` has invalid shape {0} != {1}'.format(U.shape, (C, H)))
        if yb.shape != (C,):
            raise ValueError('`yb` has invalid shape {0} != {1}'.format(yb.shape, (C,)))
        self.n_classes = C
        self._class_head = dict(C=C, pending=dict(U=U, yb=yb, dU=np.zeros_like(U), dyb=np.zeros_like(yb)))
        if self._engine is not None:
            self._apply_class_head()
        return self

    def _apply_class_head(self):
        """the engine exists: attach the head to it and hand over the variables that wait for it"""
        c = self._class_head
        if c is None or c['pending'] is None:
            return
        self._check_class_head('fit')
        self._engine.set_classes(c['C'])
        for name in _CLASS_VARS:
            self._engine.set(name, c['pending'][name])
        c['pending'] = None

    def _class_detach(self):
        """the engine is about to be closed (a rebuild after set_params): the head's variables wait on the host"""
        c = self._class_head
        if c is not None and c['pending'] is None and self._engine is not None:
            c['pending'] = {name: np.array(self._engine.get(name), dtype=np.float32) for name in _CLASS_VARS}

    def class_variables(self):
        """dict(U, yb, dU, dyb) of float32 arrays; None without a head"""
        c = self._class_head
        if c is None:
            return None
        if c['pending'] is not None:
            return {name: np.array(c['pending'][name], dtype=np.float32) for name in _CLASS_VARS}
        return {name: np.array(self._engine.get(name), dtype=np.float32) for name in _CLASS_VARS}

    # ---- checkpoints
    def _class_variables(self):
        """what model.npz additionally holds while a head is attached"""
        v = self.class_variables()
        return {} if v is None else {'class_' + name: v[name] for name in _CLASS_VARS}

    def _class_restore(self, d):
        """load_model only: takes the class_* arrays out of `d` and re-attaches the head they describe"""
        taken = {k: d.pop(k) for k in [k for k in d if k.startswith('class_')]}
        self.__dict__.pop('n_classes', None)
        if 'class_U' not in taken:
            return
        U = np.ascontiguousarray(taken['class_U'], dtype=np.float32)
        self.set_classes(U.shape[0], U=U, yb=taken['class_yb'])
        for name in ('dU', 'dyb'):
            self._class_head['pending'][name] = np.ascontiguousarray(taken['class_' + name], dtype=np.float32)

    # ---- discriminative training
    def fit_discriminative(self, X, y, X_val=None, y_val=None, n_epochs=10, learning_rate=0.1, momentum=0.5, batch_size=None,
                           verbose=None):
        """Ascend the mean of log p(y|x) over (X, y) with the exact gradient: W, hb, U, yb move, vb sees a zero gradient.

        y : integer labels in [0, n_classes), one per row of X (checked on the host before anything is uploaded).
        learning_rate, momentum : a number or one value per epoch (the last one repeats), like the schedules of `fit`; `l2` is
        the model's.  batch_size : None = the model's; at most the model's.  Batches are consecutive rows, the last one may be
        short.  X_val, y_val : evaluated after every epoch.  Returns dict(log_proba=[..], accuracy=[..]) with one entry per
        epoch - the mean log p(y|x) and the accuracy over the epoch's rows, each batch's taken before its update - plus
        val_log_proba / val_accuracy when validation data is given.  Touches neither `epoch_` / `iter_`, the schedules of
        `fit`, the RNG streams nor the persistent chains.  Not combined with dropout, a sparsity penalty, centering or data
        parallelism (ValueError)."""
        self._check_class_head('fit_discriminative', train=True)
        X = self._check_class_X(X)
        y = validate_labels(y, len(X), self._class_head['C'])
        if (X_val is None) != (y_val is None):
            raise ValueError('fit_discriminative: `X_val` and `y_val` go together')
        if X_val is not None:
            X_val = self._check_class_X(X_val, 'X_val')
            y_val = validate_labels(y_val, len(X_val), self._class_head['C'])
        bs = self.batch_size if batch_size is None else int(batch_size)
        if not 1 <= bs <= self.batch_size:
            raise ValueError('fit_discriminative: batch_size {0} outside [1, the model\'s batch_size = {1}]'.format(bs, self.batch_size))
        if len(X) < 1 or int(n_epochs) < 0:
            raise ValueError('fit_discriminative: needs at least one row and n_epochs >= 0')
        return self._fit_discriminative(X, y, X_val, y_val, int(n_epochs), make_list_from(learning_rate), make_list_from(momentum),
                                        bs, self.verbose if verbose is None else verbose)

    @run_on_engine(check_initialized=False)
    def _fit_discriminative(self, X, y, X_val, y_val, n_epochs, lrs, moms, bs, verbose):
        from . import _ffi
        self.initialized_ = True
        eng = self._on_device()
        Xd = self._to_device(X, 'fit_X')
        yd = _ffi.DeviceArray.from_numpy(y, np.int32)
        names = ['log_proba', 'accuracy'] + (['val_log_proba', 'val_accuracy'] if X_val is not None else [])
        out = {name: [] for name in names}
        for epoch in range(n_epochs):
            lr, mom = float(lrs[min(epoch, len(lrs) - 1)]), float(moms[min(epoch, len(moms) - 1)])
            lp, acc = eng.class_train_epoch(Xd, yd, len(X), bs, lr, mom)
            out['log_proba'].append(lp)
            out['accuracy'].append(acc)
            if X_val is not None:
                L = self._class_log_proba(X_val)
                out['val_log_proba'].append(float(L[np.arange(len(y_val)), y_val].astype(np.float64).mean()))
                out['val_accuracy'].append(float((L.argmax(axis=1) == y_val).mean()))
            if verbose:
                parts = ['epoch: %*d/%d' % (len(str(n_epochs)), epoch + 1, n_epochs)]
                parts += ['%s: %s' % (m.replace('val_', 'val.'), format(out[m][-1], '.4f')) for m in names]
                write_during_training('; '.join(parts))
        eng.sync()
        self._save_model()
        return out

    # ---- joint training of p(x, y)
    def fit_joint(self, X, y, X_val=None, y_val=None, n_epochs=10, n_gibbs_steps=1, learning_rate=0.05, momentum=0.5,
                  discriminative_weight=0., batch_size=None, verbose=None):
        """Train the classification RBM over (x, one-hot y) with CD-k on the joint: h0 from (x, y), every Gibbs step draws v and
        y from the hidden layer, W, hb, vb, U, yb all move.  `discriminative_weight` > 0 adds that multiple of the gradient of
        log p(y|x) (`fit_discriminative`'s objective) in the same update: the hybrid objective of Larochelle & Bengio 2008,
        L_disc + alpha L_gen, with discriminative_weight = 1 / alpha folded into the learning rate.

        Labels, schedules, batches, validation data and the returned dict are those of `fit_discriminative` (the epoch's
        log_proba / accuracy are taken before each update).  n_gibbs_steps : the k of CD-k, >= 1.  One seed is drawn from the
        model's host stream, as by every stochastic public call.  Touches neither `epoch_` / `iter_`, the schedules of `fit`
        nor the persistent chains.  Not combined with dropout, a sparsity penalty, centering or data parallelism (ValueError)."""
        self._check_class_head('fit_joint', train=True)
        X = self._check_class_X(X)
        y = validate_labels(y, len(X), self._class_head['C'])
        if (X_val is None) != (y_val is None):
            raise ValueError('fit_joint: `X_val` and `y_val` go together')
        if X_val is not None:
            X_val = self._check_class_X(X_val, 'X_val')
            y_val = validate_labels(y_val, len(X_val), self._class_head['C'])
        bs = self.batch_size if batch_size is None else int(batch_size)
        if not 1 <= bs <= self.batch_size:
            raise ValueError('fit_joint: batch_size {0} outside [1, the model\'s batch_size = {1}]'.format(bs, self.batch_size))
        if len(X) < 1 or int(n_epochs) < 0:
            raise ValueError('fit_joint: needs at least one row and n_epochs >= 0')
        if int(n_gibbs_steps) != n_gibbs_steps or int(n_gibbs_steps) < 1:
            raise ValueError('fit_joint: `n_gibbs_steps` must be an integer >= 1 (got {0!r})'.format(n_gibbs_steps))
        if not float(discriminative_weight) >= 0.:
            raise ValueError('fit_joint: `discriminative_weight` must be >= 0 (got {0!r})'.format(discriminative_weight))
        return self._fit_joint(X, y, X_val, y_val, int(n_epochs), int(n_gibbs_steps), make_list_from(learning_rate),
                               make_list_from(momentum), float(discriminative_weight), bs, self.verbose if verbose is None else verbose)

    @run_on_engine(check_initialized=False, update_seed=True)
    def _fit_joint(self, X, y, X_val, y_val, n_epochs, k, lrs, moms, gamma, bs, verbose):
        from . import _ffi
        self.initialized_ = True
        eng = self._on_device()
        Xd = self._to_device(X, 'fit_X')
        yd = _ffi.DeviceArray.from_numpy(y, np.int32)
        names = ['log_proba', 'accuracy'] + (['val_log_proba', 'val_accuracy'] if X_val is not None else [])
        out = {name: [] for name in names}
        for epoch in range(n_epochs):
            lr, mom = float(lrs[min(epoch, len(lrs) - 1)]), float(moms[min(epoch, len(moms) - 1)])
            lp, acc = eng.class_joint_train_epoch(Xd, yd, len(X), bs, k, lr, mom, gamma)
            out['log_proba'].append(lp)
            out['accuracy'].append(acc)
            if X_val is not None:
                L = self._class_log_proba(X_val)
                out['val_log_proba'].append(float(L[np.arange(len(y_val)), y_val].astype(np.float64).mean()))
                out['val_accuracy'].append(float((L.argmax(axis=1) == y_val).mean()))
            if verbose:
                parts = ['epoch: %*d/%d' % (len(str(n_epochs)), epoch + 1, n_epochs)]
                parts += ['%s: %s' % (m.replace('val_', 'val.'), format(out[m][-1], '.4f')) for m in names]
                write_during_training('; '.join(parts))
        eng.sync()
        self._save_model()
        return out

    # ---- semi-supervised training
    def fit_semi_supervised(self, X, y, X_unlabelled, X_val=None, y_val=None, n_epochs=10, n_gibbs_steps=1, learning_rate=0.05,
                            momentum=0.5, discriminative_weight=0., unlabelled_weight=1., batch_size=None, verbose=None):
        """`fit_joint` on the labelled rows (X, y) with the unlabelled rows `X_unlabelled` training the same W, U, hb, vb, yb
        through log p(x) = log sum_y p(x, y): behind every labelled batch's update one update on the next batch of unlabelled
        rows - its positive phase over y exact (the class posterior of `predict_proba`), its negative phase the CD-k chain of
        `fit_joint` started at a class drawn from that posterior - with the learning rate `learning_rate * unlabelled_weight`.
        That is stochastic gradient ascent on L_sup + unlabelled_weight * L_unsup with alternating minibatches (Larochelle &
        Bengio 2008, section 6); `unlabelled_weight = 0` is `fit_joint`.

        The unlabelled rows are taken as consecutive batches of `batch_size` rows (a short last one), cyclically; the cursor
        carries over from epoch to epoch within the call and starts at the first batch.  Everything else - labels, schedules,
        validation data, `discriminative_weight`, the seed drawn from the model's host stream, the saved model - is
        `fit_joint`'s.  The returned dict adds `unlabelled_entropy` and `unlabelled_confidence` per epoch: the mean entropy of
        p(.|x) and the mean max_c p(c|x) over the epoch's unlabelled rows, each batch's taken before its update (nan for an
        epoch without unlabelled updates).  Touches neither `epoch_` / `iter_`, the schedules of `fit` nor the persistent
        chains.  Not combined with dropout, a sparsity penalty, centering or data parallelism (ValueError)."""
        self._check_class_head('fit_semi_supervised', train=True)
        X = self._check_class_X(X)
        y = validate_labels(y, len(X), self._class_head['C'])
        if not float(unlabelled_weight) >= 0.:
            raise ValueError('fit_semi_supervised: `unlabelled_weight` must be >= 0 (got {0!r})'.format(unlabelled_weight))
        X_unlabelled = self._check_class_X(X_unlabelled, 'X_unlabelled')
        if len(X_unlabelled) < 1:
            raise ValueError('fit_semi_supervised: `X_unlabelled` has no rows')
        if (X_val is None) != (y_val is None):
            raise ValueError('fit_semi_supervised: `X_val` and `y_val` go together')
        if X_val is not None:
            X_val = self._check_class_X(X_val, 'X_val')
            y_val = validate_labels(y_val, len(X_val), self._class_head['C'])
        bs = self.batch_size if batch_size is None else int(batch_size)
        if not 1 <= bs <= self.batch_size:
            raise ValueError('fit_semi_supervised: batch_size {0} outside [1, the model\'s batch_size = {1}]'.format(bs, self.batch_size))
        if len(X) < 1 or int(n_epochs) < 0:
            raise ValueError('fit_semi_supervised: needs at least one row and n_epochs >= 0')
        if int(n_gibbs_steps) != n_gibbs_steps or int(n_gibbs_steps) < 1:
            raise ValueError('fit_semi_supervised: `n_gibbs_steps` must be an integer >= 1 (got {0!r})'.format(n_gibbs_steps))
        if not float(discriminative_weight) >= 0.:
            raise ValueError('fit_semi_supervised: `discriminative_weight` must be >= 0 (got {0!r})'.format(discriminative_weight))
        return self._fit_semi_supervised(X, y, X_unlabelled, X_val, y_val, int(n_epochs), int(n_gibbs_steps), make_list_from(learning_rate),
                                         make_list_from(momentum), float(discriminative_weight), float(unlabelled_weight), bs,
                                         self.verbose if verbose is None else verbose)

    @run_on_engine(check_initialized=False, update_seed=True)
    def _fit_semi_supervised(self, X, y, Xu, X_val, y_val, n_epochs, k, lrs, moms, gamma, beta, bs, verbose):
        from . import _ffi
        self.initialized_ = True
        eng = self._on_device()
        Xd = self._to_device(X, 'fit_X')
        Xud = self._to_device(Xu, 'fit_X_unlabelled')
        yd = _ffi.DeviceArray.from_numpy(y, np.int32)
        names = ['log_proba', 'accuracy', 'unlabelled_entropy', 'unlabelled_confidence']
        names += ['val_log_proba', 'val_accuracy'] if X_val is not None else []
        out = {name: [] for name in names}
        n_batches, n_slices, cursor = (len(X) + bs - 1) // bs, (len(Xu) + bs - 1) // bs, 0
        for epoch in range(n_epochs):
            lr, mom = float(lrs[min(epoch, len(lrs) - 1)]), float(moms[min(epoch, len(moms) - 1)])
            lp, acc, ent, conf = eng.class_semi_train_epoch(Xd, yd, len(X), Xud, len(Xu), cursor, bs, k, lr, mom, gamma, beta)
            if beta > 0.:
                cursor = (cursor + n_batches) % n_slices
            else:
                ent = conf = float('nan')
            for name, v in zip(names, (lp, acc, ent, conf)):
                out[name].append(v)
            if X_val is not None:
                L = self._class_log_proba(X_val)
                out['val_log_proba'].append(float(L[np.arange(len(y_val)), y_val].astype(np.float64).mean()))
                out['val_accuracy'].append(float((L.argmax(axis=1) == y_val).mean()))
            if verbose:
                parts = ['epoch: %*d/%d' % (len(str(n_epochs)), epoch + 1, n_epochs)]
                parts += ['%s: %s' % (m.replace('val_', 'val.'), format(out[m][-1], '.4f')) for m in names]
                write_during_training('; '.join(parts))
        eng.sync()
        self._save_model()
        return out

    def sample_v_given_class(self, y, n_gibbs_steps=None, V_init=None, return_means=False):
        """Class-conditional sampling ("show me a 7"): one chain per entry of `y`, block-Gibbs h ~ p(h | v, y), v ~ p(v | h) with
        the class clamped.

        y : [N] integer labels in [0, n_classes).  n_gibbs_steps : sweeps; None: the model's `n_gibbs_steps` of the current
        epoch.  V_init : [N, n_visible] start of the chains; None: v_0 ~ Ber(1/2).  Returns the visible states [N, n_visible]
        after the last sweep (with `return_means`: a pair, states and the means of the last visible pass).
        Both layers are always sampled.  The rows are processed in slices of at most `batch_size`, every row drawing from its
        own position of the call's random stream: the result does not depend on the slicing.  One seed is drawn from the
        model's host stream; no parameter is changed."""
        self._check_class_head('sample_v_given_class')
        y = np.asarray(y)
        y = validate_labels(y, len(y) if y.ndim == 1 else -1, self._class_head['C'])
        if len(y) < 1:
            raise ValueError('sample_v_given_class: `y` is empty')
        if V_init is not None:
            V_init = self._check_class_X(V_init, 'V_init')
            if len(V_init) != len(y):
                raise ValueError('`V_init` has {0} rows for {1} labels'.format(len(V_init), len(y)))
        if n_gibbs_steps is not None and int(n_gibbs_steps) < 1:
            raise ValueError('`n_gibbs_steps` must be >= 1 (got {0})'.format(n_gibbs_steps))
        return self._sample_v_given_class(y, n_gibbs_steps, V_init, return_means)

    @run_on_engine(update_seed=True)
    def _sample_v_given_class(self, y, n_gibbs_steps, V_init, return_means):
        from . import _ffi
        eng = self._on_device()
        k = int(n_gibbs_steps) if n_gibbs_steps is not None else self._feed()[2]
        if k < 1:
            raise ValueError('`n_gibbs_steps` must be >= 1 (got {0})'.format(k))
        N = len(y)
        yd = _ffi.DeviceArray.from_numpy(y, np.int32)
        V0 = self._to_device(V_init) if V_init is not None else None
        Vd = _ffi.DeviceArray((N, self.n_visible), np.float32)
        Pd = _ffi.DeviceArray((N, self.n_visible), np.float32) if return_means else None
        try:
            for start in range(0, N, self.batch_size):
                # every slice at call 0 of the call's seed and at its own rows of the stream: a row's draws depend on its index alone
                eng.seed(self._graph_seed)
                eng.set_row_offset(start)
                eng.class_gibbs(V0, yd, min(self.batch_size, N - start), k, Vd, Pd, row=start)
            eng.sync()
        finally:
            eng.set_row_offset(0)
        return (Vd.numpy(), Pd.numpy()) if return_means else Vd.numpy()

    # ---- prediction
    def _class_log_proba(self, X):
        eng = self._on_device()
        Xd = self._to_device(X)
        L = np.empty((len(X), self._class_head['C']), dtype=np.float32)
        for start in range(0, len(X), _PREDICT_ROWS):
            B = min(_PREDICT_ROWS, len(X) - start)
            L[start:start + B] = eng.class_log_proba(Xd, B, row=start)
        return L

    def predict_log_proba(self, X):
        """[N, n_classes] float32: the exact log p(c|x) per row of X.  Draws nothing."""
        self._check_class_head('predict_log_proba')
        return self._predict_log_proba(self._check_class_X(X))

    @run_on_engine()
    def _predict_log_proba(self, X):
        return self._class_log_proba(X)

    def predict_proba(self, X):
        """[N, n_classes]: p(c|x) per row of X"""
        return np.exp(self.predict_log_proba(X))

    def predict(self, X):
        """[N] int64: argmax_c p(c|x) per row of X (the lowest class among equals)"""
        return self.predict_log_proba(X).argmax(axis=1)

    def score(self, X, y):
        """the accuracy of `predict(X)` against the labels `y`"""
        self._check_class_head('score')
        X = self._check_class_X(X)
        y = validate_labels(y, len(X), self._class_head['C'])
        return float((self.predict(X) == y).mean())
