"""Thin object wrappers over the C-ABI handles (include/bm355.h).

`RbmEngine` plays the role the TF session plays in the reference: it owns the
variables of one model in HBM and executes the fetch sites of
boltzmann_machines/rbm/base_rbm.py (`session.run(train_op)` :566, metric
fetches :554-564,:578, `transform_op.eval` :697, free energy :605,:612).
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import DeviceArray, check

RBM_VARS = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'sigma')


def as_device(X):
    """host ndarray -> DeviceArray (float32, C order); DeviceArray passes through."""
    if isinstance(X, DeviceArray):
        return X
    return DeviceArray.from_numpy(np.asarray(X), np.float32)


class _PtCalls(object):
    """Parallel tempering (bm355.h: bm_rbm_pt_* / bm_dbm_pt_*): the three calls on the handle's tempered ensemble, the same for
    both engines but for the symbol prefix and the hidden state matrices pt_read hands out."""
    _pt_prefix = None                             # 'bm_rbm' / 'bm_dbm'
    _pt_n_hidden = 0                              # hidden state matrices pt_read accepts: 1 (Hd) / 2 (H1d, H2d)

    def _pt_call(self, name):
        return getattr(self.lib, '%s_pt_%s' % (self._pt_prefix, name))

    def pt_init(self, n_chains, betas, V0_d=None, chain0=0):
        """build the tempered ensemble of n_chains x len(betas) replicas in the handle; V0_d [n_chains, V] (DeviceArray): every
        chain's replicas start there, None: v_0 ~ Ber(1/2); a DBM's h2_0 ~ Ber(1/2) either way"""
        b = np.ascontiguousarray(betas, dtype=np.float32).ravel()
        check(self._pt_call('init')(self._h, int(n_chains), len(b), b.ctypes.data_as(C.c_void_p),
                                    V0_d.ptr if V0_d is not None else None, int(chain0)))
        self._pt_shape = (int(n_chains), len(b))
        self._pt_train_key = None                 # (whoever builds the ensemble for training records its ladder: tempering.py)

    def pt_sweep(self, n_steps):
        """n_steps on the whole ensemble, each the tempered passes of one Gibbs sweep with the replica exchange after the first
        (RBM: prop-up, exchange, prop-down; DBM: h1, exchange, h2, v)"""
        check(self._pt_call('sweep')(self._h, int(n_steps)))

    def pt_read(self, Vd=None, *Hd):
        """beta = 1 rows -> Vd [n_chains, V] and the hidden states (RBM: Hd [n_chains, H]; DBM: H1d [n_chains, n_1], H2d
        [n_chains, n_2]), all DeviceArrays, all optional; returns (swaps [2, R-1] int64: attempts and accepts per ladder pair,
        ladder_idx [n_chains, R] int32: the ladder index of every row)"""
        if len(Hd) > self._pt_n_hidden:
            raise TypeError('pt_read() takes at most %d hidden state matrices (%d given)' % (self._pt_n_hidden, len(Hd)))
        mats = (Vd,) + Hd + (None,) * (self._pt_n_hidden - len(Hd))
        M, R = getattr(self, '_pt_shape', (0, 1))
        swaps = np.zeros((2, max(R - 1, 0)), dtype=np.int64)
        idx = np.zeros((M, R), dtype=np.int32)
        check(self._pt_call('read')(self._h, *[d.ptr if d is not None else None for d in mats],
                                    swaps.ctypes.data_as(C.c_void_p) if swaps.size else None,
                                    idx.ctypes.data_as(C.c_void_p) if idx.size else None))
        return swaps, idx

    # tempered negative phase (bm355.h: <prefix>_train_step_pt / _train_epoch_pt); the ensemble of pt_init supplies the particles
    def train_step_pt(self, Xd, B, lr, momentum, k, row=0):
        check(getattr(self.lib, self._pt_prefix + '_train_step_pt')(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k))

    def train_epoch_pt(self, Xd, N, batch, lr, momentum, k, row=0):
        """N rows starting at `row`, consecutive batches of `batch` rows, one tempered update each, driven from C"""
        check(getattr(self.lib, self._pt_prefix + '_train_epoch_pt')(self._h, Xd.offset_ptr(row * self.V), N, batch, lr, momentum, k))


class _RbmPtView(_PtCalls):
    """The tempered ensemble of an RbmEngine whose visible unit has entries of its own, under their prefix, on the engine's handle.
    Every other attribute is the engine's, so that the tempered sampler and the tempered epoch of tempering.py / rbm.py run on a
    view as they run on an engine."""
    _pt_n_hidden = 1
    _pt_param = 'pt_'                             # the bm_rbm_get_param names of the ensemble: 'pt_*' / 'gpt_*'

    def __init__(self, engine):
        self._engine = engine
        self.lib, self.V = engine.lib, engine.V

    @property
    def _h(self):
        return self._engine._h

    def __getattr__(self, name):                  # (only what this object does not define itself)
        if name == '_engine':
            raise AttributeError(name)
        return getattr(self._engine, name)

    def _pt_shapes(self, rows):
        eng = self._engine
        return dict(v=(rows, eng.V), h=(rows, eng.H), part_v=((eng.V + 15) // 16, rows), part_h=((eng.H + 15) // 16, rows), mult=(rows,))

    def pt_state(self):
        """the whole ensemble as NumPy arrays (tests, tools): v [M R, V], h [M R, H], part_v [ceil(V/16), M R], part_h
        [ceil(H/16), M R], mult [M R], idx [M R] int32, swaps [2, R - 1] int64 (bm_rbm_get_param and pt_read); waits for the
        device.  Counts: part_v [2, M R] (the float32 pair hi, lo of the double v.vb) and len [M R] besides.  Gaussian: v is the
        scaled variable u, part_v the slots of -1/2 (u - c)^2"""
        M, R = self._pt_shape
        out = {}
        for name, shape in self._pt_shapes(M * R).items():
            a = np.empty(shape, dtype=np.float32)
            check(self.lib.bm_rbm_get_param(self._h, (self._pt_param + name).encode(), a.ctypes.data_as(C.c_void_p), a.size))
            out[name] = a
        swaps, idx = self.pt_read()
        out.update(idx=idx.reshape(-1), swaps=swaps)
        return out


class RbmGroupsPt(_RbmPtView):
    """The tempered ensemble of an RbmEngine with visible groups (bm355.h: bm_rbm_groups_pt_* / _train_step_pt / _train_epoch_pt;
    DESIGN.md 3.29): pt_init / pt_sweep / pt_read and the two tempered updates under the prefix 'bm_rbm_groups'."""
    _pt_prefix = 'bm_rbm_groups'


class RbmRsmPt(_RbmPtView):
    """The tempered ensemble of an RbmEngine with replicated softmax visible units (bm355.h: bm_rbm_rsm_pt_* / _train_step_pt /
    _train_epoch_pt): pt_init / pt_sweep / pt_read and the two tempered updates under the prefix 'bm_rbm_rsm'.
    pt_init takes the chains' document lengths; `train_lengths` holds those of the ensemble that the next tempered `fit` builds
    (rbm.py: set_count_tempering)."""
    _pt_prefix = 'bm_rbm_rsm'
    train_lengths = None

    def pt_init(self, n_chains, betas, V0_d=None, chain0=0, lengths=None):
        """build the tempered ensemble of n_chains x len(betas) replicas; lengths [n_chains]: the chains' document lengths
        (None: `train_lengths`); V0_d [n_chains, V] count rows of those lengths, None: v_0 ~ Multinomial(D_c, uniform)"""
        b = np.ascontiguousarray(betas, dtype=np.float32).ravel()
        D = self.train_lengths if lengths is None else lengths
        if D is None:
            raise ValueError('pt_init: the chains of a count ensemble need their document lengths')
        D = np.ascontiguousarray(D, dtype=np.float32).ravel()
        if len(D) != int(n_chains):
            raise ValueError('pt_init: %d lengths for %d chains' % (len(D), int(n_chains)))
        check(self.lib.bm_rbm_rsm_pt_init(self._h, int(n_chains), len(b), b.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p),
                                          V0_d.ptr if V0_d is not None else None, int(chain0)))
        self._pt_shape = (int(n_chains), len(b))
        self._pt_train_key = None

    def _pt_shapes(self, rows):
        return dict(super(RbmRsmPt, self)._pt_shapes(rows), part_v=(2, rows), len=(rows,))


class RbmGaussPt(_RbmPtView):
    """The tempered ensemble of an RbmEngine with Gaussian visible units (bm355.h: bm_rbm_gauss_pt_*): pt_init /
    pt_sweep / pt_read under the prefix 'bm_rbm_gauss' (the unit has no tempered update).  V0_d of pt_init and the rows pt_read
    hands out are in data units; the ensemble itself lives in the scaled variable u = x / sigma."""
    _pt_prefix, _pt_param = 'bm_rbm_gauss', 'gpt_'


class RbmEngine(_PtCalls):
    dtype = np.float32
    _pt_prefix, _pt_n_hidden = 'bm_rbm', 1

    def __init__(self, n_visible, n_hidden, v_unit=_ffi.UNIT_BERNOULLI, sample_v_states=False,
                 sample_h_states=True, dbm_first=False, dbm_last=False, max_batch=10, l2=1e-4,
                 sparsity_target=0.1, sparsity_cost=0., sparsity_damping=0.9, dropout=None,
                 h_unit=_ffi.UNIT_BERNOULLI, n_samples=0, v_groups=0, rsm_max_length=0):
        self.lib = _ffi.load()
        self.V, self.H, self.max_batch = int(n_visible), int(n_hidden), int(max_batch)
        cfg = _ffi.RbmConfig(self.V, self.H, int(v_unit), int(bool(sample_v_states)),
                             int(bool(sample_h_states)), int(bool(dbm_first)), int(bool(dbm_last)),
                             self.max_batch, float(l2), float(sparsity_target), float(sparsity_cost),
                             float(sparsity_damping), -1.0 if dropout is None else float(dropout),
                             int(h_unit), int(n_samples))
        self._h = C.c_void_p()
        check(self.lib.bm_rbm_create(C.byref(cfg), C.byref(self._h)))
        if v_groups:          # softmax visible units: n_visible / v_groups one-hot groups (bm_rbm_set_visible_groups)
            try:
                self.set_visible_groups(v_groups)
            except Exception:
                self.close()
                raise
        if rsm_max_length:    # replicated softmax visible units: one softmax over the layer, drawn D times per row
            try:
                self.set_replicated_softmax(rsm_max_length)
            except Exception:
                self.close()
                raise

    # -- lifetime
    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.bm_rbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- variables
    def _size(self, name):
        C_ = getattr(self, 'n_classes', 0)
        return {'W': self.V * self.H, 'dW': self.V * self.H, 'vb': self.V, 'dvb': self.V, 'sigma': self.V,
                'hb': self.H, 'dhb': self.H, 'q_means': self.H, 'ov': self.V, 'oh': self.H,
                'W_fast': self.V * self.H, 'W_eff': self.V * self.H, 'vb_fast': self.V, 'vb_eff': self.V,
                'hb_fast': self.H, 'hb_eff': self.H,
                'grad': self.V * self.H + self.V + 2 * self.H,
                'U': C_ * self.H, 'dU': C_ * self.H, 'yb': C_, 'dyb': C_}[name]

    def _shape(self, name):
        if name in ('U', 'dU'):          # the class head's weights (set_classes)
            return (getattr(self, 'n_classes', 0), self.H)
        return (self.V, self.H) if name in ('W', 'dW', 'W_fast', 'W_eff') else (self._size(name),)

    def set(self, name, value):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float32), self._shape(name)))
        check(self.lib.bm_rbm_set_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def get(self, name):
        a = np.empty(self._shape(name), dtype=np.float32)
        check(self.lib.bm_rbm_get_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def stage(self, slot):
        """snapshot of every variable into device-side slot 0 | 1, in stream order, without a host wait (bm_rbm_stage)"""
        check(self.lib.bm_rbm_stage(self._h, int(slot)))

    def get_staged(self, slot, name):
        """one variable of a staged snapshot; waits for the staged copies only, callable from another thread"""
        a = np.empty(self._shape(name), dtype=np.float32)
        check(self.lib.bm_rbm_get_staged(self._h, int(slot), name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def set_fast_binary(self, on, everywhere=False):
        """opt-in exact-product bf16 x 3 mode of the sampling sweep (bm_rbm_set_fast_binary): where it pays (>= 8M weights);
        everywhere=True: wherever legal (tests, measurements)"""
        check(self.lib.bm_rbm_set_fast_binary(self._h, (2 if everywhere else 1) if on else 0))

    def set_centering(self, on, nu_v=0.01, nu_h=0.01):
        """centred update (bm_rbm_set_centering): while on, every fused update entry of this handle takes it; the offsets are
        the variables 'ov' / 'oh'"""
        check(self.lib.bm_rbm_set_centering(self._h, int(bool(on)), float(nu_v), float(nu_h)))

    def set_fast_weights(self, on, fast_learning_rate=0.0, fast_decay=0.95):
        """fast-weights PCD (bm_rbm_set_fast_weights): while on, train_step_pt / train_epoch_pt run their negative phase under
        W + W_fast, vb + vb_fast, hb + hb_fast and move the fast set with every update; off -> on starts from a zero fast set,
        on -> on changes the two scalars only, off releases the set.  Variables while on: 'W_fast', 'vb_fast', 'hb_fast'
        (get / set), 'W_eff', 'vb_eff', 'hb_eff' (get)"""
        check(self.lib.bm_rbm_set_fast_weights(self._h, int(bool(on)), float(fast_learning_rate), float(fast_decay)))

    def set_from_device(self, name, darr):
        """variable <- dense DeviceArray, asynchronously on the engine's stream (bm_rbm_set_param_dev)"""
        check(self.lib.bm_rbm_set_param_dev(self._h, name.encode(), darr.ptr, int(np.prod(darr.shape))))

    def device_view(self, name):
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.bm_rbm_dev_ptr(self._h, name.encode(), C.byref(p), C.byref(n)))
        return DeviceArray((n.value,), np.float32, ptr=p.value, owner=self)

    # -- control
    def seed(self, seed):
        check(self.lib.bm_rbm_seed(self._h, int(seed)))

    def set_row_offset(self, row0):
        check(self.lib.bm_rbm_set_row_offset(self._h, int(row0)))

    def sync(self):
        check(self.lib.bm_rbm_sync(self._h))

    # -- fetch sites
    def train_step(self, Xd, B, lr, momentum, k, row=0):
        check(self.lib.bm_rbm_train_step(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k))

    def train_step_metrics(self, Xd, B, lr, momentum, k, row=0):
        out = (C.c_float * 4)()
        check(self.lib.bm_rbm_train_step_metrics(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k, out))
        return np.array(out[:], dtype=np.float32)

    MAX_PENDING_METRICS = 4096

    def train_step_metrics_async(self, Xd, B, lr, momentum, k, row=0):
        """train_step_metrics without the host wait: the values arrive with the next collect_metrics()"""
        check(self.lib.bm_rbm_train_step_metrics_async(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k))

    def collect_metrics(self):
        """[n, 4] float32: the pending asynchronous fetches, oldest first (ONE stream synchronisation)"""
        out = np.empty((self.MAX_PENDING_METRICS, 4), dtype=np.float32)
        n = C.c_int32(0)
        check(self.lib.bm_rbm_collect_metrics(self._h, out.ctypes.data_as(C.POINTER(C.c_float)),
                                              self.MAX_PENDING_METRICS, C.byref(n)))
        return out[:n.value].copy()

    def train_epoch(self, Xd, N, batch, lr, momentum, k, row=0):
        """N rows starting at `row`, consecutive batches of `batch` rows, driven from C (no Python per batch)"""
        check(self.lib.bm_rbm_train_epoch(self._h, Xd.offset_ptr(row * self.V), N, batch, lr, momentum, k))

    def grad_step(self, Xd, B, k, row=0):
        check(self.lib.bm_rbm_grad_step(self._h, Xd.offset_ptr(row * self.V), B, k))

    def apply_step(self, B_global, lr, momentum):
        check(self.lib.bm_rbm_apply_step(self._h, B_global, lr, momentum))

    # delayed-gradient data parallelism (bm355.h: bm_rbm_set_grad_slot / _allreduce_grads_async / _wait_grads)
    def set_grad_slot(self, slot):
        check(self.lib.bm_rbm_set_grad_slot(self._h, slot))

    def allreduce_grads_async(self, comm):
        check(self.lib.bm_rbm_allreduce_grads_async(self._h, comm._c))

    def wait_grads(self, slot):
        check(self.lib.bm_rbm_wait_grads(self._h, slot))

    def transform(self, Xd, B, k, Hd, row=0, out_row=0):
        check(self.lib.bm_rbm_transform(self._h, Xd.offset_ptr(row * self.V), B, k, Hd.offset_ptr(out_row * self.H)))

    def sample_h(self, Xd, B, Hmean_d=None, Hstate_d=None, row=0, out_row=0):
        """one prop-up of the handle's own hidden conditional from rows [row, row + B) of Xd, the input taken as given
        (bm_rbm_sample_h): means and / or states into rows [out_row, out_row + B) of the dense DeviceArrays"""
        check(self.lib.bm_rbm_sample_h(self._h, Xd.offset_ptr(row * self.V), B,
                                       Hmean_d.offset_ptr(out_row * self.H) if Hmean_d is not None else None,
                                       Hstate_d.offset_ptr(out_row * self.H) if Hstate_d is not None else None))

    def sample_v_from_h(self, Hd, B, Vmean_d=None, Vstate_d=None, row=0, out_row=0):
        """one prop-down of the handle's own visible conditional from rows [row, row + B) of Hd, taken as given
        (bm_rbm_sample_v_from_h): means and / or states into rows [out_row, out_row + B) of the dense DeviceArrays"""
        check(self.lib.bm_rbm_sample_v_from_h(self._h, Hd.offset_ptr(row * self.H), B,
                                              Vmean_d.offset_ptr(out_row * self.V) if Vmean_d is not None else None,
                                              Vstate_d.offset_ptr(out_row * self.V) if Vstate_d is not None else None))

    def set_visible_groups(self, K):
        """softmax visible units (bm_rbm_set_visible_groups): n_visible / K one-hot groups of K units; 0: Bernoulli units again"""
        check(self.lib.bm_rbm_set_visible_groups(self._h, int(K)))
        self.v_groups = int(K)

    def set_replicated_softmax(self, max_length):
        """replicated softmax visible units (bm_rbm_set_replicated_softmax): rows are count vectors of 1 .. max_length tokens;
        0: Bernoulli units again"""
        check(self.lib.bm_rbm_set_replicated_softmax(self._h, int(max_length)))
        self.rsm_max_length = int(max_length)

    def set_row_lengths(self, Dd, B, row=0):
        """the lengths of the B rows that the next sample_v_from_h / gibbs calls run on: entries [row, row + B) of the float32
        DeviceArray Dd (bm_rbm_set_row_lengths)"""
        check(self.lib.bm_rbm_set_row_lengths(self._h, Dd.offset_ptr(row), B))

    # softmax visible units: incomplete rows, clamped groups, exact group conditionals (bm355.h: bm_rbm_groups_*)
    def groups_set_missing(self, on):
        """while on, an all-zero group of a training row is a missing group, held at zero by every prop-down of the chain"""
        check(self.lib.bm_rbm_groups_set_missing(self._h, int(bool(on))))

    def groups_gibbs_clamped(self, Vd, Hd, B, n_steps, clamp_val_d, clamp_mask_d, Vmean_d=None, row=0):
        """gibbs_clamped for a handle with visible groups; the mask must be constant within every group
        (bm_rbm_groups_gibbs_clamped)"""
        ov, oh = row * self.V, row * self.H
        check(self.lib.bm_rbm_groups_gibbs_clamped(self._h, Vd.offset_ptr(ov), Hd.offset_ptr(oh),
                                                   Vmean_d.offset_ptr(ov) if Vmean_d is not None else None, B, n_steps,
                                                   clamp_val_d.offset_ptr(ov), clamp_mask_d.offset_ptr(ov)))

    def groups_scores(self, Xd, B, row=0):
        """[B, V] float64: S of rows [row, row + B) of Xd (bm_rbm_groups_scores); B is not bounded by max_batch"""
        out = np.empty((B, self.V), dtype=np.float64)
        check(self.lib.bm_rbm_groups_scores(self._h, Xd.offset_ptr(row * self.V), B, out.ctypes.data_as(C.c_void_p)))
        return out

    def groups_ais(self, n_betas, n_runs, k, seed, chain0=0, base_bias=None, observed=None):
        """[n_runs] float32 per-chain AIS estimates of log Z of a handle with visible groups (bm_rbm_groups_ais);
        base_bias [V]: the base logits `a`, None: the uniform base; observed [n_groups] bool: the groups the model has, None: all"""
        out = np.empty(n_runs, dtype=np.float32)
        a = o = None
        if base_bias is not None:
            a = np.ascontiguousarray(base_bias, dtype=np.float32)
            if a.shape != (self.V,):
                raise ValueError('base_bias has shape %r, expected (%d,)' % (a.shape, self.V))
        if observed is not None:
            o = np.ascontiguousarray(np.asarray(observed) != 0, dtype=np.uint8)
            K = getattr(self, 'v_groups', 0)
            if K and o.shape != (self.V // K,):
                raise ValueError('observed has shape %r, expected (%d,)' % (o.shape, self.V // K))
        check(self.lib.bm_rbm_groups_ais(self._h, n_betas, n_runs, k, a.ctypes.data_as(C.c_void_p) if a is not None else None,
                                         o.ctypes.data_as(C.c_void_p) if o is not None else None, int(seed), int(chain0),
                                         out.ctypes.data_as(C.c_void_p)))
        return out

    @property
    def groups_pt(self):
        """the tempered ensemble of a handle with visible groups and its calls (RbmGroupsPt), one object per engine"""
        view = self.__dict__.get('_groups_pt')
        if view is None:
            view = self.__dict__['_groups_pt'] = RbmGroupsPt(self)
        return view

    @property
    def rsm_pt(self):
        """the tempered ensemble of a handle with replicated softmax visible units and its calls (RbmRsmPt), one object per engine"""
        view = self.__dict__.get('_rsm_pt')
        if view is None:
            view = self.__dict__['_rsm_pt'] = RbmRsmPt(self)
        return view

    def debug_rsm_up(self, Vd, J, Dd, beta, per_row, Hd, part_d=None):
        """launch-level probe (tests; bm_debug_rsm_up): the tempered prop-up of the J count rows of Vd with lengths Dd into Hd at
        site 4 of the current call - per_row: the DB + RT pass with every row at `beta` (its energy partials into part_d
        [ceil(H/16), J]), else the existing DB pass at mult == bmult == beta; the call counter does not advance"""
        check(self.lib.bm_debug_rsm_up(self._h, Vd.ptr, int(J), Dd.ptr, float(beta), int(bool(per_row)), Hd.ptr,
                                       part_d.ptr if part_d is not None else None))

    def rsm_ais(self, n_betas, lengths, k, seed, chain0=0, base_logits=None):
        """[len(lengths)] float32 per-chain AIS estimates of log Z_D of a handle with replicated softmax visible units, chain r
        over count vectors of lengths[r] tokens (bm_rbm_rsm_ais); base_logits [V]: the base logits `a`, None: the
        uniform base"""
        D = np.ascontiguousarray(lengths, dtype=np.float32).reshape(-1)
        out = np.empty(len(D), dtype=np.float32)
        a = None
        if base_logits is not None:
            a = np.ascontiguousarray(base_logits, dtype=np.float32)
            if a.shape != (self.V,):
                raise ValueError('base_logits has shape %r, expected (%d,)' % (a.shape, self.V))
        check(self.lib.bm_rbm_rsm_ais(self._h, n_betas, len(D), k, a.ctypes.data_as(C.c_void_p) if a is not None else None,
                                      D.ctypes.data_as(C.c_void_p), int(seed), int(chain0), out.ctypes.data_as(C.c_void_p)))
        return out

    def metrics(self, Xd, B, k, row=0):
        out = (C.c_float * 4)()
        check(self.lib.bm_rbm_metrics(self._h, Xd.offset_ptr(row * self.V), B, k, out))
        return np.array(out[:], dtype=np.float32)

    def free_energy(self, Xd, B, row=0):
        out = C.c_float()
        check(self.lib.bm_rbm_free_energy(self._h, Xd.offset_ptr(row * self.V), B, C.byref(out)))
        return float(out.value)

    def free_energy_rows(self, Xd, B, row=0):
        """[B] float32: F(x) of rows [row, row + B) of Xd under the RBM's own parameters (bm_rbm_free_energy_rows)"""
        out = np.empty(B, dtype=np.float32)
        check(self.lib.bm_rbm_free_energy_rows(self._h, Xd.offset_ptr(row * self.V), B, out.ctypes.data_as(C.c_void_p)))
        return out

    # class head (bm355.h: bm_rbm_set_classes / _class_log_proba / _class_train_step / _class_train_epoch)
    n_classes = 0

    def set_classes(self, n_classes):
        """attach a head of n_classes >= 2 classes (the variables 'U' [C, H], 'yb' [C], 'dU', 'dyb', all zero), or detach it (0)"""
        check(self.lib.bm_rbm_set_classes(self._h, int(n_classes)))
        self.n_classes = int(n_classes)

    def class_log_proba(self, Xd, B, row=0):
        """[B, C] float32: log p(c|x) of rows [row, row + B) of Xd (any B)"""
        out = np.empty((B, self.n_classes), dtype=np.float32)
        check(self.lib.bm_rbm_class_log_proba(self._h, Xd.offset_ptr(row * self.V), B, out.ctypes.data_as(C.c_void_p)))
        return out

    def class_train_step(self, Xd, yd, B, lr, momentum, row=0, fetch=True):
        """one discriminative update from rows [row, row + B) of Xd and of the int32 labels yd; fetch: returns the batch's
        (mean log p(t|x), accuracy) of the forward pass before the update, else only queues and returns None"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_train_step(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), B, lr, momentum,
                                               out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def class_train_epoch(self, Xd, yd, N, batch, lr, momentum, row=0, fetch=True):
        """N rows starting at `row` as consecutive batches of `batch` rows, driven from C; fetch: (mean log p(t|x), accuracy)
        over the N rows, each batch's taken before its update"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_train_epoch(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), N, batch, lr, momentum,
                                                out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    # back-propagation below a class head (bm355.h: bm_rbm_backprop_down / bm_rbm_delta_update; StackEngine drives whole stacks)
    def backprop_down(self, Dd, B, Od, Ad=None, lda=None, ldo=None):
        """Od [B, V] (pitch ldo, default V) = (Dd [B, H] W^T) * Ad * (1 - Ad), Ad [B, V] (pitch lda, default V) an activation
        matrix; Ad=None: Dd W^T itself.  Queues only"""
        check(self.lib.bm_rbm_backprop_down(self._h, Dd.ptr, B, Ad.ptr if Ad is not None else None,
                                            self.V if lda is None else int(lda), Od.ptr, self.V if ldo is None else int(ldo)))

    def delta_update(self, Xd, Dd, B, lr, momentum):
        """W, W^T, hb from the input Xd [B, V] and the delta Dd [B, H] through the fused update (dvb = 0).  Queues only"""
        check(self.lib.bm_rbm_delta_update(self._h, Xd.ptr, Dd.ptr, B, lr, momentum))

    # joint training of p(x, y) and sampling by class (bm355.h: bm_rbm_class_joint_* / bm_rbm_class_gibbs)
    def class_joint_train_step(self, Xd, yd, B, k, lr, momentum, disc_weight=0., row=0, fetch=True):
        """one update of L_gen + disc_weight * L_disc (CD-k on (x, y)) from rows [row, row + B) of Xd and of the int32 labels yd;
        fetch: the batch's (mean log p(t|x), accuracy) before the update, else only queues and returns None"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_joint_train_step(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), B, k, lr, momentum,
                                                     disc_weight, out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def class_joint_train_epoch(self, Xd, yd, N, batch, k, lr, momentum, disc_weight=0., row=0, fetch=True):
        """N rows starting at `row` as consecutive batches of `batch` rows, driven from C; fetch as class_train_epoch"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_joint_train_epoch(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), N, batch, k, lr,
                                                      momentum, disc_weight, out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def class_joint_chain(self, Xd, yd, B, k, row=0):
        """the chain of one joint update without the update: dict(h0m, h0s, vk, yk, hk) of host arrays"""
        out = dict(h0m=np.empty((B, self.H), np.float32), h0s=np.empty((B, self.H), np.float32), vk=np.empty((B, self.V), np.float32),
                   yk=np.empty(B, np.int32), hk=np.empty((B, self.H), np.float32))
        check(self.lib.bm_rbm_class_joint_chain(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), B, k,
                                                *[out[n].ctypes.data_as(C.c_void_p) for n in ('h0m', 'h0s', 'vk', 'yk', 'hk')]))
        return out

    # semi-supervised training (bm355.h: bm_rbm_class_unsup_* / bm_rbm_class_semi_train_epoch)
    def class_unsup_train_step(self, Xd, B, k, lr, momentum, row=0, fetch=True):
        """one update on the unlabelled rows [row, row + B) of Xd (exact positive phase over y, CD-k from y0 ~ p(y | x)); fetch:
        the batch's (mean posterior entropy, mean max_c p(c|x)) before the update, else only queues and returns None"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_unsup_train_step(self._h, Xd.offset_ptr(row * self.V), B, k, lr, momentum, out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def class_unsup_chain(self, Xd, B, k, row=0):
        """the chain and the positive operand of one unlabelled update without the update: dict(y0, em, h0s, vk, yk, hk)"""
        out = dict(y0=np.empty(B, np.int32), em=np.empty((B, self.H), np.float32), h0s=np.empty((B, self.H), np.float32),
                   vk=np.empty((B, self.V), np.float32), yk=np.empty(B, np.int32), hk=np.empty((B, self.H), np.float32))
        check(self.lib.bm_rbm_class_unsup_chain(self._h, Xd.offset_ptr(row * self.V), B, k,
                                                *[out[n].ctypes.data_as(C.c_void_p) for n in ('y0', 'em', 'h0s', 'vk', 'yk', 'hk')]))
        return out

    def class_semi_train_epoch(self, Xd, yd, N, Xud, Nu, u_slice, batch, k, lr, momentum, disc_weight=0., unl_weight=1., row=0, fetch=True):
        """N labelled rows starting at `row` as consecutive batches, one unlabelled update with lr * unl_weight behind each on the
        next slice of `batch` rows of Xud [Nu, V] (cyclic, from slice u_slice; Xud may be None while unl_weight == 0); fetch:
        (mean log p(t|x), accuracy, mean posterior entropy, mean max_c p(c|x)), each over its own rows and before its update"""
        out = (C.c_float * 4)()
        check(self.lib.bm_rbm_class_semi_train_epoch(self._h, Xd.offset_ptr(row * self.V), yd.offset_ptr(row), N,
                                                     Xud.ptr if Xud is not None else None, Nu, u_slice, batch, k, lr, momentum,
                                                     disc_weight, unl_weight, out if fetch else None))
        return tuple(float(v) for v in out) if fetch else None

    def class_gibbs(self, Vd, yd, B, n_steps, out_v, out_vmeans=None, row=0):
        """n_steps of h ~ p(h | v, y), v ~ p(v | h) for rows [row, row + B): from Vd (None: Ber(1/2)) into out_v / out_vmeans"""
        check(self.lib.bm_rbm_class_gibbs(self._h, Vd.offset_ptr(row * self.V) if Vd is not None else None, yd.offset_ptr(row), B,
                                          n_steps, out_v.offset_ptr(row * self.V),
                                          out_vmeans.offset_ptr(row * self.V) if out_vmeans is not None else None))

    def ais(self, n_betas, n_runs, k, seed, chain0=0, base_bias=None):
        """[n_runs] float32 per-chain AIS estimates of the RBM's log Z (bm_rbm_ais); base_bias [V]: the bias `a` of the
        base model p_0(v) ~ exp(a.v), None: the uniform base"""
        out = np.empty(n_runs, dtype=np.float32)
        a = None
        if base_bias is not None:
            a = np.ascontiguousarray(base_bias, dtype=np.float32)
            if a.shape != (self.V,):
                raise ValueError('base_bias has shape %r, expected (%d,)' % (a.shape, self.V))
        check(self.lib.bm_rbm_ais(self._h, n_betas, n_runs, k, a.ctypes.data_as(C.c_void_p) if a is not None else None,
                                  int(seed), int(chain0), out.ctypes.data_as(C.c_void_p)))
        return out

    # Gaussian visible units as one joint model (bm355.h: bm_rbm_gauss_*)
    def gauss_ais(self, n_betas, n_runs, k, seed, chain0=0, base_mean=None):
        """[n_runs] float32 per-chain AIS estimates of the log normaliser of exp(-F(x / sigma)) over x of a handle with Gaussian
        visible units (bm_rbm_gauss_ais); base_mean [V]: the mean `a` of the base model N(a, I) in the SCALED variable u = x / sigma,
        None: a = 0"""
        out = np.empty(n_runs, dtype=np.float32)
        a = None
        if base_mean is not None:
            a = np.ascontiguousarray(base_mean, dtype=np.float32)
            if a.shape != (self.V,):
                raise ValueError('base_mean has shape %r, expected (%d,)' % (a.shape, self.V))
        check(self.lib.bm_rbm_gauss_ais(self._h, n_betas, n_runs, k, a.ctypes.data_as(C.c_void_p) if a is not None else None,
                                        int(seed), int(chain0), out.ctypes.data_as(C.c_void_p)))
        return out

    def ais_state(self, n_runs):
        """(v [n_runs, V], h [n_runs, H]): the chain states the last AIS entry left in the handle (tests)"""
        v, h = np.empty((n_runs, self.V), np.float32), np.empty((n_runs, self.H), np.float32)
        for name, a in (('ais_v', v), ('ais_h', h)):
            check(self.lib.bm_rbm_get_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return v, h

    def gauss_free_energy_rows(self, Xd, B, row=0):
        """[B] float64: F(x / sigma) = 1/2 |u - c|^2 - sum_j softplus((u W + hb)_j) of rows [row, row + B) of Xd (data units;
        bm_rbm_gauss_free_energy_rows); B is not bounded by max_batch"""
        out = np.empty(B, dtype=np.float64)
        check(self.lib.bm_rbm_gauss_free_energy_rows(self._h, Xd.offset_ptr(row * self.V), B, out.ctypes.data_as(C.c_void_p)))
        return out

    @property
    def gauss_pt(self):
        """the tempered ensemble of a handle with Gaussian visible units and its calls (RbmGaussPt), one object per engine"""
        view = self.__dict__.get('_gauss_pt')
        if view is None:
            view = self.__dict__['_gauss_pt'] = RbmGaussPt(self)
        return view

    def gauss_pt_init(self, n_chains, betas, V0_d=None, chain0=0):
        return self.gauss_pt.pt_init(n_chains, betas, V0_d, chain0)

    def gauss_pt_sweep(self, n_steps):
        return self.gauss_pt.pt_sweep(n_steps)

    def gauss_pt_read(self, Vd=None, *Hd):
        return self.gauss_pt.pt_read(Vd, *Hd)

    def gibbs(self, Hd, Vd, B, n_steps):
        check(self.lib.bm_rbm_gibbs(self._h, Hd.ptr, Vd.ptr, B, n_steps))

    def gibbs_clamped(self, Vd, Hd, B, n_steps, clamp_val_d, clamp_mask_d, Vmean_d=None, row=0):
        """n_steps of v -> h -> v from the visible states in Vd [B, V] (in/out) with the entries where clamp_mask_d is
        non-zero held at clamp_val_d (both dense [B, V]); Hd [B, H] and Vmean_d (optional) receive the last hidden states
        and visible means (bm_rbm_gibbs_clamped).  row: the B rows start at this row of every array"""
        ov, oh = row * self.V, row * self.H
        check(self.lib.bm_rbm_gibbs_clamped(self._h, Vd.offset_ptr(ov), Hd.offset_ptr(oh),
                                            Vmean_d.offset_ptr(ov) if Vmean_d is not None else None, B, n_steps,
                                            clamp_val_d.offset_ptr(ov), clamp_mask_d.offset_ptr(ov)))

    def stream(self):
        p = C.c_void_p()
        check(self.lib.bm_rbm_stream(self._h, C.byref(p)))
        return p.value

    def chain_stats(self):
        """(chained launches issued, tiles they must compute, BM355_DEBUG=chain=.. mode) - csrc/bm_chain.h"""
        out = (C.c_int64 * 3)()
        check(self.lib.bm_rbm_chain_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def profile(self, enable):
        check(self.lib.bm_rbm_profile(self._h, int(bool(enable))))

    def kernel_times(self):
        ms, n = (C.c_float * 6)(), (C.c_int32 * 6)()
        check(self.lib.bm_rbm_kernel_times(self._h, ms, n))
        names = ('act_up', 'act_down', 'grad', 'colsum', 'bias', 'other')
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def timer_start(self):
        check(self.lib.bm_rbm_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.bm_rbm_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    def timer_mark(self):
        check(self.lib.bm_rbm_timer_mark(self._h))

    def timer_elapsed(self):
        ms = C.c_float()
        check(self.lib.bm_rbm_timer_elapsed(self._h, C.byref(ms)))
        return float(ms.value)


class StackEngine(object):
    """A stack of RbmEngine handles, bottom first, the last one carrying a class head: the bm_rbm_class_stack_* entries
    (include/bm355.h).  Owns nothing: the engines stay their owners'."""

    def __init__(self, engines):
        engines = list(engines)
        if not engines:
            raise ValueError('StackEngine needs at least one engine (the top)')
        self.engines, self.top, self.below = engines, engines[-1], engines[:-1]
        self.lib = self.top.lib
        self.n_below = len(self.below)
        self._below = (C.c_void_p * self.n_below)(*[e._h.value for e in self.below]) if self.n_below else None
        self.V = engines[0].V

    def _lrs(self, lr):
        lr = [float(lr)] * len(self.engines) if np.isscalar(lr) else [float(v) for v in lr]
        if len(lr) != len(self.engines):
            raise ValueError('one learning rate per layer, the top last: %d values for %d layers' % (len(lr), len(self.engines)))
        return (C.c_float * len(lr))(*lr)

    def train_step(self, Xd, yd, B, lr, momentum, row=0, fetch=True):
        """one update of the whole stack from rows [row, row + B); lr: a number or one value per layer, the top last; fetch as
        RbmEngine.class_train_step (without it the call only queues: sync() before reading variables)"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_stack_train_step(self.top._h, self._below, self.n_below, Xd.offset_ptr(row * self.V),
                                                     yd.offset_ptr(row), B, self._lrs(lr), momentum, out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def train_epoch(self, Xd, yd, N, batch, lr, momentum, row=0, fetch=True):
        """N rows starting at `row` as consecutive batches of `batch` rows, driven from C"""
        out = (C.c_float * 2)()
        check(self.lib.bm_rbm_class_stack_train_epoch(self.top._h, self._below, self.n_below, Xd.offset_ptr(row * self.V),
                                                      yd.offset_ptr(row), N, batch, self._lrs(lr), momentum, out if fetch else None))
        return (float(out[0]), float(out[1])) if fetch else None

    def log_proba(self, Xd, B, row=0):
        """[B, C] float32: log p(c|x) of rows [row, row + B) of Xd through the stack (any B)"""
        out = np.empty((B, self.top.n_classes), dtype=np.float32)
        check(self.lib.bm_rbm_class_stack_log_proba(self.top._h, self._below, self.n_below, Xd.offset_ptr(row * self.V), B,
                                                    out.ctypes.data_as(C.c_void_p)))
        return out

    def transform(self, Xd, B, Ad, row=0):
        """a_D of rows [row, row + B) of Xd into the DeviceArray Ad [B, V of the top] (a stack without layers below: a copy)"""
        if not self.n_below:
            raise ValueError('a stack without layers below the top has a_D = x')
        check(self.lib.bm_rbm_stack_transform(self._below, self.n_below, Xd.offset_ptr(row * self.V), B, Ad.ptr))

    def sync(self):
        """every layer's stream; the top last (it reports a label outside [0, C))"""
        for e in self.engines:
            e.sync()


class RbmEngine64(object):
    """float64 RBM handle (bm_rbm64_*, include/bm355.h): same method names as RbmEngine, float64
    device arrays and scalars.  Compatibility path for dtype='float64' models (base/mixin.py:15)."""

    dtype = np.float64

    def __init__(self, n_visible, n_hidden, v_unit=_ffi.UNIT_BERNOULLI, sample_v_states=False,
                 sample_h_states=True, dbm_first=False, dbm_last=False, max_batch=10, l2=1e-4,
                 sparsity_target=0.1, sparsity_cost=0., sparsity_damping=0.9, dropout=None,
                 h_unit=_ffi.UNIT_BERNOULLI, n_samples=0):
        self.lib = _ffi.load()
        self.V, self.H, self.max_batch = int(n_visible), int(n_hidden), int(max_batch)
        drop = -1.0 if dropout is None else float(dropout)
        cfg = _ffi.RbmConfig(self.V, self.H, int(v_unit), int(bool(sample_v_states)),
                             int(bool(sample_h_states)), int(bool(dbm_first)), int(bool(dbm_last)),
                             self.max_batch, float(l2), float(sparsity_target), float(sparsity_cost),
                             float(sparsity_damping), drop, int(h_unit), int(n_samples))
        hyper = (C.c_double * 5)(float(l2), float(sparsity_target), float(sparsity_cost), float(sparsity_damping), drop)
        self._h = C.c_void_p()
        check(self.lib.bm_rbm64_create(C.byref(cfg), hyper, C.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.bm_rbm64_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, name):
        if name in ('W', 'dW'):
            return (self.V, self.H)
        return (self.V,) if name in ('vb', 'dvb', 'sigma') else (self.H,)

    def set(self, name, value):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), self._shape(name)))
        check(self.lib.bm_rbm64_set_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def get(self, name):
        a = np.empty(self._shape(name), dtype=np.float64)
        check(self.lib.bm_rbm64_get_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def seed(self, seed):
        check(self.lib.bm_rbm64_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_row_offset(self, row0):
        check(self.lib.bm_rbm64_set_row_offset(self._h, int(row0)))

    def sync(self):
        check(self.lib.bm_rbm64_sync(self._h))

    def train_step(self, Xd, B, lr, momentum, k, row=0):
        check(self.lib.bm_rbm64_train_step(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k))

    def train_step_metrics(self, Xd, B, lr, momentum, k, row=0):
        out = (C.c_double * 4)()
        check(self.lib.bm_rbm64_train_step_metrics(self._h, Xd.offset_ptr(row * self.V), B, lr, momentum, k, out))
        return np.array(out[:], dtype=np.float64)

    def transform(self, Xd, B, k, Hd, row=0, out_row=0):
        check(self.lib.bm_rbm64_transform(self._h, Xd.offset_ptr(row * self.V), B, k, Hd.offset_ptr(out_row * self.H)))

    def metrics(self, Xd, B, k, row=0):
        out = (C.c_double * 4)()
        check(self.lib.bm_rbm64_metrics(self._h, Xd.offset_ptr(row * self.V), B, k, out))
        return np.array(out[:], dtype=np.float64)

    def free_energy(self, Xd, B, row=0):
        out = C.c_double()
        check(self.lib.bm_rbm64_free_energy(self._h, Xd.offset_ptr(row * self.V), B, C.byref(out)))
        return float(out.value)


class DbmEngine(_PtCalls):
    """One bm_dbm handle: the variables, variational parameters and fantasy particles
    of a DBM in HBM + the fetch sites of boltzmann_machines/dbm.py (`session.run` at
    :798,:805,:813,:869,:882,:893,:930,:954)."""
    _pt_prefix, _pt_n_hidden = 'bm_dbm', 2

    def __init__(self, n_visible, n_hiddens, v_unit=_ffi.UNIT_BERNOULLI, sample_v_states=True,
                 sample_h_states=None, n_particles=100, batch_size=100, max_mf_updates=10, mf_tol=1e-7,
                 l2=0., max_norm=np.inf, sparsity_target=0.1, sparsity_cost=0., sparsity_damping=0.9,
                 h_units=None, n_samples=None):
        self.lib = _ffi.load()
        self.V = int(n_visible)
        self.n_hiddens = [int(x) for x in n_hiddens]
        self.L = len(self.n_hiddens)
        self.N, self.M = int(batch_size), int(n_particles)
        cfg = _ffi.DbmConfig()
        cfg.n_layers, cfg.n_visible, cfg.v_unit = self.L, self.V, int(v_unit)
        cfg.sample_v_states = int(bool(sample_v_states))
        sh = sample_h_states or [True] * self.L
        st = sparsity_target if hasattr(sparsity_target, '__iter__') else [sparsity_target] * self.L
        sc = sparsity_cost if hasattr(sparsity_cost, '__iter__') else [sparsity_cost] * self.L
        for i in range(self.L):
            cfg.n_hiddens[i] = self.n_hiddens[i]
            cfg.sample_h_states[i] = int(bool(sh[i]))
            cfg.sparsity_target[i] = float(st[i])
            cfg.sparsity_cost[i] = float(sc[i])
            cfg.h_unit[i] = int((h_units or [_ffi.UNIT_BERNOULLI] * self.L)[i])      # layers.py:39-70
            cfg.n_samples[i] = int((n_samples or [0] * self.L)[i])
        cfg.n_particles, cfg.batch_size, cfg.max_mf_updates = self.M, self.N, int(max_mf_updates)
        cfg.mf_tol, cfg.l2, cfg.max_norm = float(mf_tol), float(l2), float(max_norm)
        cfg.sparsity_damping = float(sparsity_damping)
        self._h = C.c_void_p()
        self._create(cfg, (float(mf_tol), float(l2), float(max_norm), float(sparsity_damping),
                           [float(x) for x in st], [float(x) for x in sc]))

    dtype = np.float32

    def _create(self, cfg, hyper):
        check(self.lib.bm_dbm_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            (self.lib.bm_dbm64_destroy if self.dtype == np.float64 else self.lib.bm_dbm_destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- variables ("W", "W_1", "hb", "hb_1", "mu_1", "h", "h_1", "v", ...)
    def shape(self, name):
        base, idx = name, 0
        if '_' in name and name.rsplit('_', 1)[1].isdigit():
            base, idx = name.rsplit('_', 1)[0], int(name.rsplit('_', 1)[1])
        n = [self.V] + self.n_hiddens
        if base in ('W', 'dW'):
            return (n[idx], n[idx + 1])
        if base in ('mu', 'mu_new'):
            return (self.N, n[idx + 1])
        if base in ('h', 'h_new'):
            return (self.M, n[idx + 1])
        if base in ('v', 'v_new'):
            return (self.M, self.V)
        if base in ('hb', 'dhb', 'q_means', 'mu_means', 'W_norm'):
            return (n[idx + 1],)
        if base in ('vb', 'dvb', 'sigma', 'ov'):
            return (self.V,)
        if base == 'oh':
            return (n[idx + 1],)
        raise KeyError(name)

    def set(self, name, value):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float32), self.shape(name)))
        check(self.lib.bm_dbm_set_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def get(self, name):
        a = np.empty(self.shape(name), dtype=np.float32)
        check(self.lib.bm_dbm_get_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def seed(self, seed):
        check(self.lib.bm_dbm_seed(self._h, int(seed)))

    def set_row_offset(self, row0, particle0):
        check(self.lib.bm_dbm_set_row_offset(self._h, int(row0), int(particle0)))

    def sync(self):
        check(self.lib.bm_dbm_sync(self._h))

    def train_step(self, Xd, lr, momentum, k, row=0, want_msre=False):
        nmf, msre = C.c_int32(), C.c_float()
        check(self.lib.bm_dbm_train_step(self._h, Xd.offset_ptr(row * self.V), lr, momentum, k, C.byref(nmf),
                                         C.byref(msre) if want_msre else None))
        return int(nmf.value), (float(msre.value) if want_msre else None)

    def metrics(self, Xd, k, row=0):
        """validation fetch (dbm.py:813): mean-field + k PCD sweeps + reconstruction msre, no update"""
        nmf, msre = C.c_int32(), C.c_float()
        check(self.lib.bm_dbm_metrics(self._h, Xd.offset_ptr(row * self.V), k, C.byref(nmf), C.byref(msre)))
        return int(nmf.value), float(msre.value)

    def grad_step(self, Xd, k, row=0):
        nmf = C.c_int32()
        check(self.lib.bm_dbm_grad_step(self._h, Xd.offset_ptr(row * self.V), k, C.byref(nmf)))
        return int(nmf.value)

    def apply_step(self, N_global, M_global, lr, momentum):
        check(self.lib.bm_dbm_apply_step(self._h, N_global, M_global, lr, momentum))

    def set_comm(self, comm):
        """install (or, with None, remove) the library-owned RCCL communicator: the mean-field residual is then
        all-reduced (max) on the device per sweep (bm_dbm_set_comm)"""
        self._comm = comm
        check(self.lib.bm_dbm_set_comm(self._h, comm._c if comm is not None else None))

    def set_fast_binary(self, on, everywhere=False):
        """opt-in exact-product bf16 x 3 mode (bm_dbm_set_fast_binary): AIS, and the particle sweeps where they gain (>= 8M
        weights in the bottom layer); everywhere=True: wherever legal (tests, measurements)"""
        check(self.lib.bm_dbm_set_fast_binary(self._h, (2 if everywhere else 1) if on else 0))

    def set_centering(self, on, nu=0.01):
        """centred update (bm_dbm_set_centering): while on, train_step and train_step_pt take it; nu: one sliding factor or
        one per layer (v, h_1, ...); the offsets are the variables 'ov', 'oh', 'oh_1', ..."""
        nus = [float(x) for x in nu] if hasattr(nu, '__iter__') else [float(nu)] * (self.L + 1)
        if len(nus) != self.L + 1:
            raise ValueError('centering: %d sliding factors for %d layers' % (len(nus), self.L + 1))
        check(self.lib.bm_dbm_set_centering(self._h, int(bool(on)), (C.c_float * (self.L + 1))(*nus)))

    def set_ais_literal(self, on):
        """AIS log-weights accumulated in float32 in the reference graph's order (bm_dbm_set_ais_literal)"""
        check(self.lib.bm_dbm_set_ais_literal(self._h, int(bool(on))))

    def set_sigmoid_literal(self, on):
        """every Bernoulli activation as the reference's float32 `1 / (1 + exp(-x))` (bm_dbm_set_sigmoid_literal)"""
        check(self.lib.bm_dbm_set_sigmoid_literal(self._h, int(bool(on))))

    def set_xchg(self, xchg):
        """like set_comm, with the per-sweep residual max over the direct peer-memory exchange (bm_dbm_set_xchg)"""
        self._xchg = xchg
        check(self.lib.bm_dbm_set_xchg(self._h, xchg._c if xchg is not None else None))

    def ais_sharded_direct(self, xchg, n_betas, n_runs_total, k, seed):
        """ais_sharded over the direct peer-memory exchange (parallel.DirectExchange of THIS engine) instead of the RCCL
        communicator: bm_dbm_ais_sharded_direct; returns all n_runs_total values, the owners' bits"""
        out = np.empty(n_runs_total, dtype=np.float32)
        check(self.lib.bm_dbm_ais_sharded_direct(self._h, xchg._c, n_betas, n_runs_total, k, int(seed),
                                                 out.ctypes.data_as(C.c_void_p)))
        return out

    def ais_sharded(self, comm, n_betas, n_runs_total, k, seed):
        """this rank's slice of the chains + ONE all-gather (bm_dbm_ais_sharded); returns all n_runs_total values"""
        out = np.empty(n_runs_total, dtype=np.float32)
        check(self.lib.bm_dbm_ais_sharded(self._h, comm._c, n_betas, n_runs_total, k, int(seed),
                                          out.ctypes.data_as(C.c_void_p)))
        return out

    def set_mf_allreduce(self, fn):
        """fn(local_max: float) -> global max over ranks (mean-field loop condition)"""
        self._mf_cb = _ffi.MF_REDUCE_FN(lambda x, ctx: float(fn(x))) if fn is not None else None
        check(self.lib.bm_dbm_set_mf_allreduce(self._h, C.cast(self._mf_cb, C.c_void_p) if self._mf_cb else None, None))

    def device_view(self, name):
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.bm_dbm_dev_ptr(self._h, name.encode(), C.byref(p), C.byref(n)))
        return DeviceArray((n.value,), np.float32, ptr=p.value, owner=self)

    def stream(self):
        p = C.c_void_p()
        check(self.lib.bm_dbm_stream(self._h, C.byref(p)))
        return p.value

    def mean_field(self, Xd, row=0, out=None, out_row=0):
        nmf = C.c_int32()
        p = out.offset_ptr(out_row * self.n_hiddens[-1]) if out is not None else None
        check(self.lib.bm_dbm_mean_field(self._h, Xd.offset_ptr(row * self.V), p, C.byref(nmf)))
        return int(nmf.value)

    def reconstruct(self, Xd, Rd, row=0, out_row=0):
        check(self.lib.bm_dbm_reconstruct(self._h, Xd.offset_ptr(row * self.V), Rd.offset_ptr(out_row * self.V)))

    def sample_v(self, k, Vd=None):
        check(self.lib.bm_dbm_sample_v(self._h, k, Vd.ptr if Vd is not None else None))

    def sample_v_clamped(self, k, clamp_val_d, clamp_mask_d, Vd=None):
        """sample_v with the visible units of the particles held at clamp_val_d where clamp_mask_d is non-zero (both dense
        [n_particles, V]; bm_dbm_sample_v_clamped)"""
        check(self.lib.bm_dbm_sample_v_clamped(self._h, k, clamp_val_d.ptr, clamp_mask_d.ptr, Vd.ptr if Vd is not None else None))

    # tempered negative phase (bm355.h: bm_dbm_train_step_pt); the ensemble of pt_init supplies the particles
    def train_step_pt(self, Xd, lr, momentum, k, row=0, want_msre=False):
        """train_step whose negative particles are the beta = 1 rows of the chains [0, n_particles) after k tempered steps of
        the whole ensemble; returns (n_mf, msre or None)"""
        nmf, msre = C.c_int32(), C.c_float()
        check(self.lib.bm_dbm_train_step_pt(self._h, Xd.offset_ptr(row * self.V), lr, momentum, k, C.byref(nmf),
                                            C.byref(msre) if want_msre else None))
        return int(nmf.value), (float(msre.value) if want_msre else None)

    def ais(self, n_betas, n_runs, k, seed, chain0=0):
        out = np.empty(n_runs, dtype=np.float32)
        check(self.lib.bm_dbm_ais(self._h, n_betas, n_runs, k, int(seed), int(chain0), out.ctypes.data_as(C.c_void_p)))
        return out

    def log_proba(self, Xd, row=0):
        out = np.empty(self.N, dtype=np.float32)
        check(self.lib.bm_dbm_log_proba(self._h, Xd.offset_ptr(row * self.V), out.ctypes.data_as(C.c_void_p)))
        return out

    def timer_start(self):
        check(self.lib.bm_dbm_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.bm_dbm_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    def timer_mark(self):
        check(self.lib.bm_dbm_timer_mark(self._h))

    def timer_elapsed(self):
        ms = C.c_float()
        check(self.lib.bm_dbm_timer_elapsed(self._h, C.byref(ms)))
        return float(ms.value)



class DbmEngine64(DbmEngine):
    """float64 DBM handle (bm_dbm64_*, include/bm355.h): the method names of DbmEngine with float64 device arrays and
    scalars.  Compatibility path for DBM(dtype='float64') (base/mixin.py:14-25): Bernoulli hidden layers, one process."""

    dtype = np.float64

    def _create(self, cfg, hyper):
        mf_tol, l2, max_norm, damping, st, sc = hyper
        if not np.isfinite(max_norm):
            max_norm = float(np.finfo(np.float64).max)
        pad = lambda v: list(v) + [0.0] * (4 - len(v))
        h12 = (C.c_double * 12)(mf_tol, l2, max_norm, damping, *(pad(st) + pad(sc)))
        check(self.lib.bm_dbm64_create(C.byref(cfg), h12, C.byref(self._h)))

    def set(self, name, value):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), self.shape(name)))
        check(self.lib.bm_dbm64_set_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def get(self, name):
        a = np.empty(self.shape(name), dtype=np.float64)
        check(self.lib.bm_dbm64_get_param(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def seed(self, seed):
        check(self.lib.bm_dbm64_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_row_offset(self, row0, particle0):
        check(self.lib.bm_dbm64_set_row_offset(self._h, int(row0), int(particle0)))

    def sync(self):
        check(self.lib.bm_dbm64_sync(self._h))

    def train_step(self, Xd, lr, momentum, k, row=0, want_msre=False):
        nmf, msre = C.c_int32(), C.c_double()
        check(self.lib.bm_dbm64_train_step(self._h, Xd.offset_ptr(row * self.V), lr, momentum, k, C.byref(nmf),
                                           C.byref(msre) if want_msre else None))
        return int(nmf.value), (float(msre.value) if want_msre else None)

    def metrics(self, Xd, k, row=0):
        nmf, msre = C.c_int32(), C.c_double()
        check(self.lib.bm_dbm64_metrics(self._h, Xd.offset_ptr(row * self.V), k, C.byref(nmf), C.byref(msre)))
        return int(nmf.value), float(msre.value)

    def mean_field(self, Xd, row=0, out=None, out_row=0):
        nmf = C.c_int32()
        p = out.offset_ptr(out_row * self.n_hiddens[-1]) if out is not None else None
        check(self.lib.bm_dbm64_mean_field(self._h, Xd.offset_ptr(row * self.V), p, C.byref(nmf)))
        return int(nmf.value)

    def reconstruct(self, Xd, Rd, row=0, out_row=0):
        check(self.lib.bm_dbm64_reconstruct(self._h, Xd.offset_ptr(row * self.V), Rd.offset_ptr(out_row * self.V)))

    def sample_v(self, k, Vd=None):
        check(self.lib.bm_dbm64_sample_v(self._h, k, Vd.ptr if Vd is not None else None))

    def ais(self, n_betas, n_runs, k, seed, chain0=0):
        out = np.empty(n_runs, dtype=np.float64)
        check(self.lib.bm_dbm64_ais(self._h, n_betas, n_runs, k, int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain0),
                                    out.ctypes.data_as(C.c_void_p)))
        return out

    def log_proba(self, Xd, row=0):
        out = np.empty(self.N, dtype=np.float64)
        check(self.lib.bm_dbm64_log_proba(self._h, Xd.offset_ptr(row * self.V), out.ctypes.data_as(C.c_void_p)))
        return out

    def _unsupported(self, *a, **kw):
        raise NotImplementedError('the float64 DBM path is a single-process compatibility path (csrc/bm_dbm64.hip)')

    grad_step = apply_step = set_comm = set_xchg = ais_sharded = ais_sharded_direct = set_mf_allreduce = _unsupported
    device_view = stream = timer_start = timer_stop = timer_mark = timer_elapsed = _unsupported

    def sample_v_clamped(self, *a, **kw):
        raise NotImplementedError('conditional sampling has no float64 entry (bm_dbm64_* has no clamped sample_v)')

    def set_centering(self, *a, **kw):
        raise NotImplementedError('centering has no float64 entry (bm_dbm64_* has no centred update)')

    def _no_pt(self, *a, **kw):
        raise NotImplementedError('parallel tempering has no float64 entry (bm_dbm64_* has no pt_init / pt_sweep / pt_read / '
                                  'train_step_pt)')

    pt_init = pt_sweep = pt_read = train_step_pt = _no_pt

    def set_fast_binary(self, on, everywhere=False):
        if on:
            self._unsupported()

    def set_ais_literal(self, on):
        pass                                    # float64 AIS accumulates in double: the model dtype IS the literal order's dtype

    def set_sigmoid_literal(self, on):
        if on:
            raise ValueError('the literal float32 tf.sigmoid is a float32 notion')
