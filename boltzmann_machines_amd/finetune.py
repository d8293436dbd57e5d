"""Fine-tuning a stack of pre-trained layers below a class head by back-propagation: the Python side.

The reference's pipeline ends in a classifier: pre-train RBMs or a DBM, unroll the stack into a sigmoid network, fine-tune it on
labels.  `StackClassifier` is that last step on the engine: D >= 0 feature layers under a classification RBM,

    a_0 = x,   a_l = sigmoid(a_{l-1} W_l + hb_l),   log p(c|x) = the class head's exact posterior (3.18) of the top RBM on a_D

and `fit` ascends the batch mean of log p(y|x) through every layer (bm_rbm_class_stack_*, include/bm355.h).  Every layer is a
`BernoulliRBM` of its own; its W, hb, momentum buffers, `l2` and update rule are the model's own, its vb takes part in nothing.
The models' parameters are trained in place.

    stack = StackClassifier.from_rbms([rbm1, rbm2], n_classes=10, learning_rate=[0.01, 0.05])
    stack.fit(X, y).predict(X_test)
    stack = StackClassifier.from_dbm(dbm, n_classes=10)          # W of every layer but the top doubled
"""
import json
import os

import numpy as np

from .classification import validate_labels
from .utils import RNG, write_during_training

_PREDICT_ROWS = 4096          # rows per engine call of predict_log_proba / transform (bounds the device copies, not the input)
_STACK_JSON = 'stack.json'


class StackClassifier(object):
    """layers : list of BernoulliRBM models, bottom first; the last one is the top and gets a head of `n_classes` classes if it
        has none (U ~ N(0, 0.01^2) from `random_seed`, zero class biases).
    learning_rate : a number or one value per layer, the top's last.  momentum : a number.
    batch_size : None = the smallest `batch_size` among the layers; at most that.
    Batches are consecutive rows in order (the last one may be short), as in `fit_discriminative`.
    Only float32 Bernoulli-Bernoulli layers without dropout, sparsity penalty, centering, `dbm_first` / `dbm_last` and data
    parallelism; anything else raises ValueError before any device work."""

    def __init__(self, layers, n_classes=None, learning_rate=0.05, momentum=0.5, batch_size=None, max_epoch=10, random_seed=None,
                 model_path='stack_model/', verbose=False):
        self.layers = list(layers) if layers is not None else []
        self.learning_rate = learning_rate
        self.momentum = float(momentum)
        self.max_epoch = int(max_epoch)
        self.random_seed = random_seed
        self.model_path = model_path if model_path.endswith('/') else model_path + '/'
        self.verbose = verbose
        self.history_ = {}
        self._check_layers()
        top = self.layers[-1]
        if top._class_head is None:
            if n_classes is None:
                raise ValueError('StackClassifier: the top layer has no class head; pass `n_classes`')
            C = int(n_classes)
            U = RNG(seed=random_seed).normal(0., 0.01, (C, top.n_hidden)) if C == n_classes and C >= 2 else None
            top.set_classes(n_classes, U=U)
        elif n_classes is not None and int(n_classes) != top._class_head['C']:
            raise ValueError('StackClassifier: the top layer has a head of {0} classes, `n_classes` is {1}'.format(
                top._class_head['C'], n_classes))
        self.n_classes = top._class_head['C']
        smallest = min(m.batch_size for m in self.layers)
        self.batch_size = smallest if batch_size is None else int(batch_size)
        if not 1 <= self.batch_size <= smallest:
            raise ValueError('StackClassifier: batch_size {0} outside [1, {1}] (max_batch: the smallest batch_size among the '
                             'layers)'.format(self.batch_size, smallest))
        self._lrs()

    # ---- checks that need no device
    def _check_layers(self):
        from . import _ffi
        from .rbm import BaseRBM
        if not self.layers:
            raise ValueError('StackClassifier: `layers` is empty')
        for i, m in enumerate(self.layers):
            name = 'StackClassifier: layer %d' % i
            if not isinstance(m, BaseRBM):
                raise ValueError('%s is no RBM model (%r)' % (name, type(m).__name__))
            if any(m is o for o in self.layers[:i]):
                raise ValueError('%s is the same model as an earlier layer (the same handle twice)' % name)
            if m._V_UNIT != _ffi.UNIT_BERNOULLI:
                raise ValueError('%s has Gaussian visible units; a stack takes Bernoulli layers only' % name)
            if getattr(m, '_V_GROUP_WIDTH', 0):
                raise ValueError('%s (%s) has softmax visible units; a stack (from_rbms) takes Bernoulli layers only'
                                 % (name, type(m).__name__))
            if getattr(m, '_RSM_MAX_LENGTH', 0):
                raise ValueError('%s (%s) has replicated softmax visible units; a stack (from_rbms) takes Bernoulli layers only'
                                 % (name, type(m).__name__))
            if m._H_UNIT == _ffi.UNIT_NRELU:
                raise ValueError('%s (%s) has noisy rectified-linear (NReLU) hidden units; a stack (from_rbms) takes Bernoulli layers '
                                 'only' % (name, type(m).__name__))
            if m._H_UNIT != _ffi.UNIT_BERNOULLI:
                raise ValueError('%s has Multinomial hidden units; a stack takes Bernoulli layers only' % name)
            if np.dtype(m.dtype) != np.float32:
                raise ValueError("%s: back-propagation runs in float32 only (dtype=%r; float64 is not supported)" % (name, m.dtype))
            if m.dbm_first or m.dbm_last:
                raise ValueError('%s is a dbm_first / dbm_last model (one conditional doubled)' % name)
            if m.dropout is not None:
                raise ValueError('%s: not combined with dropout (dropout=%r)' % (name, m.dropout))
            if m.sparsity_cost != 0.:
                raise ValueError('%s: not combined with the sparsity penalty (sparsity_cost=%r)' % (name, m.sparsity_cost))
            if m._centering is not None:
                raise ValueError('%s: not combined with centering; call set_centering(False) first' % name)
            if os.environ.get('BM355_DATA_PARALLEL', '0') == '1' or getattr(m, '_dp', None) is not None:
                raise ValueError('%s: not combined with data parallelism (BM355_DATA_PARALLEL)' % name)
            if i and self.layers[i - 1].n_hidden != m.n_visible:
                raise ValueError('StackClassifier: the widths do not chain (layer {0} has {1} hidden units, layer {2} {3} visible)'.format(
                    i - 1, self.layers[i - 1].n_hidden, i, m.n_visible))

    def _lrs(self):
        lr = self.learning_rate
        lr = [float(lr)] * len(self.layers) if not hasattr(lr, '__iter__') else [float(v) for v in lr]
        if len(lr) != len(self.layers):
            raise ValueError('StackClassifier: `learning_rate` needs one value per layer, the top last ({0} values for {1} '
                             'layers)'.format(len(lr), len(self.layers)))
        return lr

    def _check_X(self, X, name='X'):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.layers[0].n_visible:
            raise ValueError('`{0}` has invalid shape {1}: expected [N, {2}]'.format(name, X.shape, self.layers[0].n_visible))
        return X

    # ---- the engines
    def _stack_engine(self):
        from .engine import RbmEngine, StackEngine
        self._check_layers()
        engines = []
        for m in self.layers:
            m._graph_seed = None
            if not m.initialized_:
                m._on_graph_build()
            m._ensure_engine()
            m.initialized_ = True
            if not isinstance(m._engine, RbmEngine):
                raise ValueError('StackClassifier: a layer has no float32 engine')
            engines.append(m._engine)
        return StackEngine(engines)

    @staticmethod
    def _device(a, dt=np.float32):
        from ._ffi import DeviceArray
        return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dt), dt)

    # ---- training
    def fit(self, X, y, X_val=None, y_val=None):
        """`max_epoch` epochs of consecutive batches over (X, y); `history_` holds log_proba / accuracy per epoch (each batch's
        taken before its update) and, with validation data, val_log_proba / val_accuracy.  Saves the stack.  Returns self."""
        self._check_layers()
        lrs = self._lrs()
        X = self._check_X(X)
        y = validate_labels(y, len(X), self.n_classes)
        if (X_val is None) != (y_val is None):
            raise ValueError('StackClassifier.fit: `X_val` and `y_val` go together')
        if X_val is not None:
            X_val = self._check_X(X_val, 'X_val')
            y_val = validate_labels(y_val, len(X_val), self.n_classes)
        if len(X) < 1:
            raise ValueError('StackClassifier.fit: needs at least one row')
        eng = self._stack_engine()
        Xd, yd = self._device(X), self._device(y, np.int32)
        names = ['log_proba', 'accuracy'] + (['val_log_proba', 'val_accuracy'] if X_val is not None else [])
        out = {name: [] for name in names}
        for epoch in range(self.max_epoch):
            lp, acc = eng.train_epoch(Xd, yd, len(X), self.batch_size, lrs, self.momentum)
            out['log_proba'].append(lp)
            out['accuracy'].append(acc)
            if X_val is not None:
                L = self._log_proba(eng, X_val)
                out['val_log_proba'].append(float(L[np.arange(len(y_val)), y_val].astype(np.float64).mean()))
                out['val_accuracy'].append(float((L.argmax(axis=1) == y_val).mean()))
            if self.verbose:
                parts = ['epoch: %*d/%d' % (len(str(self.max_epoch)), epoch + 1, self.max_epoch)]
                parts += ['%s: %s' % (m.replace('val_', 'val.'), format(out[m][-1], '.4f')) for m in names]
                write_during_training('; '.join(parts))
        eng.sync()
        self.history_ = out
        self.save()
        return self

    # ---- prediction
    def _log_proba(self, eng, X):
        Xd = self._device(X)
        L = np.empty((len(X), self.n_classes), dtype=np.float32)
        for start in range(0, len(X), _PREDICT_ROWS):
            B = min(_PREDICT_ROWS, len(X) - start)
            L[start:start + B] = eng.log_proba(Xd, B, row=start)
        return L

    def predict_log_proba(self, X):
        """[N, n_classes] float32: the exact log p(c|x) per row of X.  Draws nothing."""
        X = self._check_X(X)
        return self._log_proba(self._stack_engine(), X)

    def predict_proba(self, X):
        return np.exp(self.predict_log_proba(X))

    def predict(self, X):
        """[N] int64: argmax_c p(c|x) per row of X (the lowest class among equals)"""
        return self.predict_log_proba(X).argmax(axis=1)

    def score(self, X, y):
        """the accuracy of `predict(X)` against the labels `y`"""
        X = self._check_X(X)
        y = validate_labels(y, len(X), self.n_classes)
        return float((self.predict(X) == y).mean())

    def transform(self, X):
        """[N, n_visible of the top] float32: a_D, the deterministic features the head sees (x itself without layers below)"""
        X = self._check_X(X)
        if len(self.layers) == 1:
            return X.copy()
        from ._ffi import DeviceArray
        eng = self._stack_engine()
        Xd = self._device(X)
        Ad = DeviceArray((len(X), self.layers[-1].n_visible), np.float32)
        eng.transform(Xd, len(X), Ad)
        return Ad.numpy()

    # ---- persistence: each layer through its own model directory, plus a small JSON of the stack
    def save(self):
        """layer i goes to `<model_path>/layer_<i>/` (the layer's working paths are moved there), the stack to
        `<model_path>/stack.json`"""
        if not os.path.isdir(self.model_path):
            os.makedirs(self.model_path)
        dirs = []
        for i, m in enumerate(self.layers):
            d = os.path.join(self.model_path, 'layer_%d/' % i)
            m.update_working_paths(model_path=d)
            if m._engine is None:
                self._stack_engine()
            m._save_model()
            m._join_save()
            dirs.append('layer_%d/' % i)
        lr = self.learning_rate
        meta = dict(layers=dirs, classes=[type(m).__name__ for m in self.layers], n_classes=self.n_classes,
                    learning_rate=[float(v) for v in lr] if hasattr(lr, '__iter__') else float(lr), momentum=self.momentum,
                    batch_size=self.batch_size, max_epoch=self.max_epoch, random_seed=self.random_seed, verbose=bool(self.verbose))
        tmp = os.path.join(self.model_path, _STACK_JSON + '.tmp')
        with open(tmp, 'w') as f:
            json.dump(meta, f, indent=4, sort_keys=True)
        os.replace(tmp, os.path.join(self.model_path, _STACK_JSON))

    @classmethod
    def load_model(cls, model_path):
        from . import rbm as _rbm
        model_path = model_path if model_path.endswith('/') else model_path + '/'
        with open(os.path.join(model_path, _STACK_JSON)) as f:
            meta = json.load(f)
        layers = [getattr(_rbm, c).load_model(os.path.join(model_path, d)) for c, d in zip(meta['classes'], meta['layers'])]
        return cls(layers, n_classes=meta['n_classes'], learning_rate=meta['learning_rate'], momentum=meta['momentum'],
                   batch_size=meta['batch_size'], max_epoch=meta['max_epoch'], random_seed=meta['random_seed'], model_path=model_path,
                   verbose=meta['verbose'])

    # ---- builders
    @classmethod
    def from_rbms(cls, rbms, n_classes, **kw):
        """a stack of pre-trained RBMs as it is, bottom first"""
        return cls(list(rbms), n_classes=n_classes, **kw)

    @classmethod
    def from_dbm(cls, dbm, n_classes, bottom_up_scale=2.0, **kw):
        """fresh BernoulliRBMs from a DBM's W, W_1, ..., hb, hb_1, ... (a fitted `DBM`, or a dict of those arrays with `vb`
        optional).  The weights of every layer but the top are multiplied by `bottom_up_scale`: in a single bottom-up pass the
        doubled input stands in for the missing top-down term.  Layer i > 0 takes the hidden bias below it as its (unused)
        visible bias.  Stacks of Bernoulli layers only; the DBM is not modified."""
        from . import _ffi
        from .rbm import BernoulliRBM
        if isinstance(dbm, dict):
            params = dbm
        else:
            if any(int(u) == _ffi.UNIT_NRELU for u in dbm.h_units_):
                raise ValueError('StackClassifier.from_dbm: a layer with noisy rectified-linear (NReLU) hidden units; stacks of '
                                 'Bernoulli layers only')
            if dbm.v_unit_ != _ffi.UNIT_BERNOULLI or any(int(u) != _ffi.UNIT_BERNOULLI for u in dbm.h_units_):
                raise ValueError('StackClassifier.from_dbm: stacks of Bernoulli layers only (this DBM has Gaussian or Multinomial units)')
            if np.dtype(dbm.dtype) != np.float32:
                raise ValueError('StackClassifier.from_dbm: float32 only (dtype=%r; float64 is not supported)' % dbm.dtype)
            params = dbm.get_tf_params(scope='weights')
        sfx = lambda i: '_%d' % i if i else ''
        n = 0
        while 'W' + sfx(n) in params:
            n += 1
        if n < 1:
            raise ValueError('StackClassifier.from_dbm: no weights `W` among the parameters')
        model_path = kw.get('model_path', 'stack_model/')
        model_path = model_path if model_path.endswith('/') else model_path + '/'
        batch = int(kw.get('batch_size') or getattr(dbm, 'batch_size', 10))
        l2 = kw.pop('l2', 1e-4)                  # (the fresh layers' weight decay; no keyword of the constructor)
        layers = []
        for i in range(n):
            W = np.array(params['W' + sfx(i)], dtype=np.float32)
            if i + 1 < n:
                W = W * np.float32(bottom_up_scale)
            hb = np.array(params['hb' + sfx(i)], dtype=np.float32)
            vb = params.get('vb') if i == 0 else params['hb' + sfx(i - 1)]
            vb = np.zeros(W.shape[0], np.float32) if vb is None else np.array(vb, dtype=np.float32)
            if W.ndim != 2 or hb.shape != (W.shape[1],) or vb.shape != (W.shape[0],):
                raise ValueError('StackClassifier.from_dbm: layer {0} has W {1}, hb {2}, vb {3}'.format(i, W.shape, hb.shape, vb.shape))
            layers.append(BernoulliRBM(n_visible=W.shape[0], n_hidden=W.shape[1], W_init=W, vb_init=vb, hb_init=hb, batch_size=batch,
                                       l2=l2, random_seed=kw.get('random_seed'), verbose=False,
                                       model_path=os.path.join(model_path, 'layer_%d/' % i)))
        return cls(layers, n_classes=n_classes, **kw)
