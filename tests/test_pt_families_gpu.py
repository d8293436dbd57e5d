"""-m gpu: the four tempered families of one RBM handle (Bernoulli bm_rbm_pt_*, softmax groups bm_rbm_groups_pt_*, replicated
softmax bm_rbm_rsm_pt_*, Gaussian bm_rbm_gauss_pt_*) keep to their own ensembles: on a handle that
holds the ensemble of one family every other family's sweep, read and tempered update is refused with the words below and leaves
the ensemble as it was, bit for bit; turning a unit off and on again leaves no ensemble."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
V, H, K, ML, M, R = 20, 16, 4, 8, 2, 2
BETAS = [0.5, 1.0]
FAMILIES = ('bm_rbm', 'bm_rbm_groups', 'bm_rbm_rsm', 'bm_rbm_gauss')
# REFUSED[owner][other]: what bm_last_error says when an entry of `other` meets a handle whose ensemble is `owner`'s
GROUPS, RSM, GAUSS = 'needs a handle with visible groups', 'needs a handle with replicated softmax visible units', 'needs Gaussian visible units'
REFUSED = {
    'bm_rbm': {'bm_rbm_groups': GROUPS, 'bm_rbm_rsm': RSM, 'bm_rbm_gauss': GAUSS},
    'bm_rbm_groups': {'bm_rbm': 'is not available for softmax visible units', 'bm_rbm_rsm': RSM, 'bm_rbm_gauss': GAUSS},
    'bm_rbm_rsm': {'bm_rbm': 'is not available for replicated softmax visible units', 'bm_rbm_groups': GROUPS, 'bm_rbm_gauss': GAUSS},
    'bm_rbm_gauss': {'bm_rbm': 'no ensemble', 'bm_rbm_groups': GROUPS, 'bm_rbm_rsm': RSM},
}


def make_engine(family):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    kw = {'bm_rbm': {}, 'bm_rbm_groups': dict(v_groups=K), 'bm_rbm_rsm': dict(rsm_max_length=ML),
          'bm_rbm_gauss': dict(v_unit=_ffi.UNIT_GAUSSIAN)}[family]
    eng = RbmEngine(V, H, max_batch=4, **kw)
    rng = np.random.RandomState(7)
    eng.set('W', (0.3 * rng.randn(V, H)).astype(f32))
    eng.set('vb', (0.2 * rng.randn(V)).astype(f32))
    eng.set('hb', (0.2 * rng.randn(H)).astype(f32))
    eng.seed(11)
    return eng


def view_of(eng, family):
    return {'bm_rbm': eng, 'bm_rbm_groups': eng.groups_pt, 'bm_rbm_rsm': eng.rsm_pt, 'bm_rbm_gauss': eng.gauss_pt}[family]


def state_of(eng, family):
    """the whole ensemble of the owning family as bytes per array (the Bernoulli engine has no pt_state of its own: the same
    variables through bm_rbm_get_param and pt_read)"""
    if family != 'bm_rbm':
        st = view_of(eng, family).pt_state()
    else:
        rows = M * R
        st = {}
        for name, shape in dict(v=(rows, V), h=(rows, H), part_v=((V + 15) // 16, rows), part_h=((H + 15) // 16, rows), mult=(rows,)).items():
            a = np.empty(shape, f32)
            assert eng.lib.bm_rbm_get_param(eng._h, ('pt_' + name).encode(), a.ctypes.data_as(C.c_void_p), a.size) == 0
            st[name] = a
        swaps, idx = eng.pt_read()
        st.update(idx=idx.reshape(-1), swaps=swaps)
    return {n: (a.dtype.str, a.shape, a.tobytes()) for n, a in st.items()}


@pytest.mark.parametrize('owner', FAMILIES)
def test_other_families_are_refused_and_leave_the_ensemble(gpu_lib, owner):
    from boltzmann_machines_amd._ffi import Bm355Error
    from boltzmann_machines_amd.engine import as_device
    lib = gpu_lib
    eng = make_engine(owner)
    h = eng._h
    pt = view_of(eng, owner)
    if owner == 'bm_rbm_rsm':
        pt.pt_init(M, BETAS, lengths=[3, ML])
    else:
        pt.pt_init(M, BETAS)
    pt.pt_sweep(1)
    before = state_of(eng, owner)
    assert set(before) >= {'v', 'h', 'part_v', 'part_h', 'mult', 'idx', 'swaps'}
    Xd = as_device(np.zeros((2, V), f32))
    for other in FAMILIES:
        if other == owner:
            continue
        calls = [('_pt_sweep', lambda f: f(h, 1)), ('_pt_read', lambda f: f(h, None, None, None, None))]
        if other != 'bm_rbm_gauss':
            calls.append(('_train_step_pt', lambda f: f(h, Xd.ptr, 2, 0.05, 0.5, 1)))
        for suffix, call in calls:
            entry = other + suffix
            assert call(getattr(lib, entry)) != 0, '%s was accepted on a handle with the ensemble of %s_pt_init' % (entry, owner)
            msg = lib.bm_last_error().decode()
            assert REFUSED[owner][other] in msg, '%s on %s: %s' % (entry, owner, msg)
            assert state_of(eng, owner) == before, '%s changed the ensemble of %s' % (entry, owner)
    # the unit off and on again, where it can be: the ensemble went with it
    if owner == 'bm_rbm_groups':
        eng.set_visible_groups(0)
        eng.set_visible_groups(K)
    elif owner == 'bm_rbm_rsm':
        eng.set_replicated_softmax(0)
        eng.set_replicated_softmax(ML)
    if owner in ('bm_rbm_groups', 'bm_rbm_rsm'):
        with pytest.raises(Bm355Error, match='no ensemble'):
            pt.pt_sweep(1)
    else:
        pt.pt_sweep(1)                                # (no such switch: the ensemble is still this family's)
    eng.close()
