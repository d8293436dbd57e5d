"""Path model of the float64 engine (csrc/bm_rbm64.hip, csrc/bm_dbm64.hip) and the lattice of shapes that walks it.

A plain-Python restatement of the BRANCH PREDICATES of the device code - which tiles of which launch take the pipelined
fast path (t64_fast_segment), how many K chunks each path runs, which t64_fetch flavour loads the operands, how the bias
jobs are spread - written from the kernels, not from their results.  For a shape it returns a set of LABELS; the lattice
below is the smallest set of shapes whose labels cover REQUIRED.  tests/test_f64_lattice.py asserts that coverage (a
lattice row cannot be lost unnoticed) and cross-checks the oracle on every row; tests/test_f64_lattice_gpu.py runs every
row on the device, bit for bit against the oracle, and names the branch of a mismatch through this model.

Also here: the probe sets of the float64 sigmoid / softplus tests (shared by the CPU and the GPU file).
"""
import numpy as np

TI, TJ, BK = 64, 32, 32          # T64_TI, T64_TJ, T64_BK

# Two branches of the tile engine cannot be reached through the C ABI; nothing here tries to.
UNREACHABLE = {
    'misaligned-pointer': "the `((uintptr_t)p & 15) != 0` fallback of t64_fetch / t64_mainloop: every operand is an "
                          "allocation base, or a base plus `row * V` doubles (the row offset of the data matrix), and V is "
                          "even whenever the vector path is eligible (ld == V must be even), so the byte offset is a "
                          "multiple of 16",
    'even-ld-odd-ncols': "`vec` in t64_fetch with an even ld and an odd ncols: every caller passes ld == ncols (dense "
                         "matrices).  t64_fetch requires (ncols & 1) == 0 for the vector path since the clamp "
                         "min(col, (ncols - 2) & ~1) would otherwise select the wrong element of the last column; the "
                         "term changes no reachable launch",
}


# ---------------------------------------------------------------------------------------------------------- launches
def _launch(name, I, J, qkm, segs):
    """one contraction launch: out[j][i] = sum over segments of sum_k P[k][i] * Q(j, k); segs = [(K, ldp, ldq), ...]"""
    return dict(name=name, I=int(I), J=int(J), qkm=bool(qkm), segs=[tuple(int(x) for x in s) for s in segs])


def rbm_launches(V, H, B, k=1):
    """launch_act (up / down) and grad_kernel's two segments of one bm_rbm64 train step (run_chain + launch_update)"""
    up = _launch('up', H, B, False, [(V, H, V)])            # P = W [V][H], Q = input rows [B][V]
    down = _launch('down', V, B, False, [(H, V, H)])        # P = Wt [H][V], Q = hidden rows [B][H]
    grad = _launch('grad', H, V, True, [(B, H, V), (B, H, V)])   # P = h0m | hm [B][H], Q = X | vs [B][V] (k-major)
    return [up] + [down, up] * k + [grad]


def dbm_launches(V, nh, N, M):
    """every layer_update, both douter_kernel launches per layer and the reconstruction of one bm_dbm64 train step"""
    n = [V] + list(nh)
    L = len(nh)
    out = []
    for i in range(L):                                      # approximate-inference init: below only
        out.append(_launch('mf_init_%d' % i, n[i + 1], N, False, [(n[i], n[i + 1], n[i])]))

    def sweep(tag, J):
        for i in range(L):
            segs = [(n[i], n[i + 1], n[i])]
            if i + 1 < L:
                segs.append((n[i + 2], n[i + 1], n[i + 2]))     # P = Wt[i + 1] [n[i+2]][n[i+1]], Q = the layer above
            out.append(_launch('%s_%d' % (tag, i), n[i + 1], J, False, segs))
    sweep('mf_sweep', N)
    sweep('particles', M)
    out.append(_launch('particles_v', V, M, False, [(n[1], V, n[1])]))
    out.append(_launch('recon', V, N, False, [(n[1], V, n[1])]))
    for i in range(L):
        out.append(_launch('outer_pos_%d' % i, n[i + 1], n[i], True, [(N, n[i + 1], n[i])]))
        out.append(_launch('outer_neg_%d' % i, n[i + 1], n[i], True, [(M, n[i + 1], n[i])]))
    return out


# ---------------------------------------------------------------------------------------------------- branch predicates
def tile_path(launch, i0, j0):
    """per segment 'fast' / 'generic': the `fast && sg.K >= T64_BK` test of t64_mainloop (operands 16-byte aligned)"""
    interior = i0 + TI <= launch['I'] and j0 + TJ <= launch['J']
    return tuple('fast' if (interior and ((ldp | ldq) & 1) == 0 and K >= BK) else 'generic'
                 for K, ldp, ldq in launch['segs'])


def tiles(launch):
    return [(i0, j0) for j0 in range(0, launch['J'], TJ) for i0 in range(0, launch['I'], TI)]


def _nfull_class(nf):
    if nf <= 4:
        return str(nf)
    return 'odd>=5' if nf & 1 else 'even>=6'


def _fetch_labels(launch, seg, nch_generic):
    """t64_fetch flavours of a segment whose generic loop runs `nch_generic` chunks"""
    K, ldp, ldq = seg
    # P window: [K][I] rows of pitch ldp, ncols = I.  Q window: x-major [J][K] (ncols = K) or k-major [K][J] (ncols = J)
    pn, qn = launch['I'], (launch['J'] if launch['qkm'] else K)
    pvec = (ldp & 1) == 0 and (pn & 1) == 0 and pn >= 2
    qvec = (ldq & 1) == 0 and (qn & 1) == 0 and qn >= 2
    lab = {'fetch:P-vector' if pvec else 'fetch:P-scalar', 'fetch:Q-vector' if qvec else 'fetch:Q-scalar',
           'fetch:Q-k-major' if launch['qkm'] else 'fetch:Q-x-major'}
    if pvec != qvec:
        lab.add('fetch:P-vector&Q-scalar' if pvec else 'fetch:P-scalar&Q-vector')
    if pn == 1 or qn == 1:
        lab.add('fetch:ncols==1')
    if not (pvec and qvec) and nch_generic >= 3:
        lab.add('fetch:scalar&chunks>=3')       # the `cur` double-buffer parity of the generic loop under scalar loads
    return lab


def launch_labels(launch):
    I, J = launch['I'], launch['J']
    lab = set()
    paths = {t: tile_path(launch, *t) for t in tiles(launch)}
    n_fast_tiles = sum(1 for p in paths.values() if 'fast' in p)
    lab.add('launch:all-fast' if n_fast_tiles == len(paths) else ('launch:all-generic' if n_fast_tiles == 0 else 'launch:mixed'))
    has_interior = I >= TI and J >= TJ
    for s, seg in enumerate(launch['segs']):
        K, ldp, ldq = seg
        nch = (K + BK - 1) // BK
        kinds = set(p[s] for p in paths.values())
        if has_interior and ((ldp | ldq) & 1) == 0 and K < BK:
            lab.update(('launch:interior-tile-K<32', 'seg:nfull=0'))
        generic_chunks = set()
        if 'fast' in kinds:
            nf = K // BK
            lab.add('seg:nfull=' + _nfull_class(nf))
            lab.add('seg:tail=%d' % (nch - nf))
            if nch > nf:
                generic_chunks.add(nch - nf)
                lab.add('seg:nfull=%s&tail=1' % _nfull_class(nf))
        if 'generic' in kinds:
            generic_chunks.add(nch)
            lab.add('seg:generic-chunks=' + ('>=3' if nch >= 3 else str(nch)))
        if generic_chunks:                       # the last chunk runs in the generic loop: its `ksteps` rounding
            lab.add('seg:K%%4=%d' % (K % 4))
            lab |= _fetch_labels(launch, seg, max(generic_chunks))
    r = I % TI
    lab.add('edge:I%64=' + ('0' if r == 0 else '1..31' if r < 32 else '32' if r == 32 else '33..63'))
    r = J % TJ
    lab.add('edge:J%32=' + ('0' if r == 0 else '1..15' if r < 16 else '16' if r == 16 else '17..31'))
    if I < TI:
        lab.add('edge:I<64')
    if J < TJ:
        lab.add('edge:J<32')
    if len(launch['segs']) == 2:
        for p in set(paths.values()):
            lab.add('order:(%s,%s)' % p)
            if p[1] == 'fast' and launch['segs'][0][0] % BK != 0:
                lab.add('order:seg1-tail&seg2-fast')
    return lab


def bias_labels(V, H, B, fused):
    """launch_update: bias_wave jobs, separate (bias_kernel) or in extra grid rows of grad_kernel"""
    lab = {'bias:fused' if fused else 'bias:separate', 'bias:B%32==0' if B % 32 == 0 else 'bias:B%32!=0'}
    if B < 4:
        lab.add('bias:B<4')
    if B % 4:
        lab.add('bias:B%4!=0')
    if B >= 256:
        lab.add('bias:B>=256')
    if V % 16:
        lab.add('bias:V%16!=0')
    if H % 16:
        lab.add('bias:H%16!=0')
    nbias = (V + 15) // 16 + (H + 15) // 16
    if nbias % 4:
        lab.add('bias:nbias%4!=0')
    if fused:
        nx = (H + TI - 1) // TI
        extra = (nbias + 4 * nx - 1) // (4 * nx)
        if extra >= 2:
            lab.add('bias:extra>=2')
            if nbias % 4:
                lab.add('bias:extra>=2&nbias%4!=0')
    return lab


def rbm_labels(V, H, B, k=1, kw=None, gaussian=False, row=0):
    kw = kw or {}
    lab = set()
    for l in rbm_launches(V, H, B, k):
        lab |= launch_labels(l)
    lab |= bias_labels(V, H, B, fused=float(kw.get('sparsity_cost', 0.)) == 0.)
    lab.add('metrics:B<=256' if B <= 256 else 'metrics:B>256')      # reduce_fixed_kernel's strided loop, pll_index_kernel's grid
    if row:
        lab.add('rbm:row-offset')
    if gaussian:
        lab.add('rbm:gaussian')
    if k > 1:
        lab.add('rbm:k>1')
    if kw.get('dropout') is not None:
        lab.add('rbm:dropout')
        if row:
            lab.add('rbm:row-offset&dropout')            # prep_kernel's flat Philox index row0 * V + e
    if kw.get('sample_v_states'):
        lab.add('rbm:sampled-visibles')
        if row:
            lab.add('rbm:row-offset&sampled-visibles')   # the draw index (row0 + j) * I + i of the prop-down launch
    return lab


def dbm_labels(V, nh, N, M, expect=(), gaussian=False, row=0, particle0=0):
    """`expect`: labels that depend on the data, not on the shape ('dbm:mf-exit-tol', ...); the CPU test checks them on the
    oracle"""
    lab = set(expect)
    for l in dbm_launches(V, nh, N, M):
        lab |= launch_labels(l)
    lab.add('dbm:layers=%d' % len(nh))
    if gaussian:
        lab.add('dbm:gaussian')
    if row:
        lab.add('dbm:row-offset')                        # offset operand pointer of the data matrix
    if particle0:
        lab.add('dbm:particle-offset')                   # the Philox row index of the particle sweeps (dact_kernel)
    return lab


def locate(launch, j, i):
    """the tile (i0, j0) of output element (row j, column i) of a launch, its path per segment and the launch's labels"""
    i0, j0 = (i // TI) * TI, (j // TJ) * TJ
    return 'launch %s (I=%d J=%d segs=%s) tile (i0=%d, j0=%d) path %s; labels %s' % (
        launch['name'], launch['I'], launch['J'], launch['segs'], i0, j0, tile_path(launch, i0, j0),
        sorted(launch_labels(launch)))


REQUIRED = frozenset(
    ['launch:all-fast', 'launch:mixed', 'launch:all-generic', 'launch:interior-tile-K<32']
    + ['seg:nfull=' + c for c in ('0', '1', '2', '3', '4', 'odd>=5', 'even>=6')]
    + ['seg:tail=0', 'seg:tail=1', 'seg:nfull=1&tail=1', 'seg:nfull=odd>=5&tail=1']
    + ['seg:generic-chunks=' + c for c in ('1', '2', '>=3')]
    + ['seg:K%%4=%d' % r for r in range(4)]
    + ['fetch:P-vector', 'fetch:P-scalar', 'fetch:Q-vector', 'fetch:Q-scalar', 'fetch:P-vector&Q-scalar',
       'fetch:P-scalar&Q-vector', 'fetch:scalar&chunks>=3', 'fetch:ncols==1', 'fetch:Q-x-major', 'fetch:Q-k-major']
    + ['edge:I%64=' + c for c in ('0', '1..31', '32', '33..63')]
    + ['edge:J%32=' + c for c in ('0', '1..15', '16', '17..31')]
    + ['edge:I<64', 'edge:J<32']
    + ['order:(fast,fast)', 'order:(fast,generic)', 'order:(generic,fast)', 'order:(generic,generic)',
       'order:seg1-tail&seg2-fast']
    + ['bias:fused', 'bias:separate', 'bias:B<4', 'bias:B%4!=0', 'bias:B%32==0', 'bias:B%32!=0', 'bias:B>=256',
       'bias:V%16!=0', 'bias:H%16!=0', 'bias:extra>=2', 'bias:nbias%4!=0', 'bias:extra>=2&nbias%4!=0']
    + ['metrics:B<=256', 'metrics:B>256']
    + ['rbm:row-offset', 'rbm:gaussian', 'rbm:k>1', 'rbm:dropout', 'rbm:row-offset&dropout', 'rbm:sampled-visibles',
       'rbm:row-offset&sampled-visibles', 'dbm:row-offset', 'dbm:particle-offset']
    + ['dbm:maxnorm-clipped&unclipped', 'dbm:mf-exit-tol', 'dbm:mf-exit-cap', 'dbm:gaussian', 'dbm:layers=1',
       'dbm:layers=2', 'dbm:layers=3'])


# ------------------------------------------------------------------------------------------------------------ lattice
def _rbm(V, H, B, k=1, kw=None, gaussian=False, row=0, rows=None, why=''):
    return dict(V=V, H=H, B=B, k=k, kw=dict(kw or {}), gaussian=gaussian, row=row, rows=rows or B + row, why=why,
                id='%dx%dx%d%s' % (V, H, B, ''.join('-' + t for t in (
                    ['k%d' % k] * (k > 1) + ['gauss'] * gaussian + ['row%d' % row] * (row > 0) + sorted(kw or {})))))


RBM_LATTICE = [
    _rbm(64, 64, 32, why='every launch one interior tile, no tails; grad K = 32: nfull = 1'),
    _rbm(96, 128, 64, why='nfull 3, 4 and 2; I % 64 == 32'),
    _rbm(160, 66, 33, why='nfull 5; a 2-column and a 1-row edge tile; K = 66: two full chunks + tail, K % 4 == 2; grad '
                          'K = 33: nfull = 1 + tail with K % 4 == 1 in both segments; 15 bias jobs over two extra grid rows'),
    _rbm(35, 70, 67, kw=dict(sparsity_cost=1e-3, dropout=0.8),
         why='odd V: scalar Q with vector P and the reverse; three-chunk generic loops; K % 4 == 3; separate bias launch'),
    _rbm(70, 35, 100, kw=dict(dbm_first=True), why='the mirror of the previous row'),
    _rbm(64, 24, 32, why='interior tiles with K < 32'),
    _rbm(1, 1, 1, why='ncols == 1; B < 4'),
    _rbm(2, 1, 3, why='ncols == 1 on one operand only; B < 4'),
    _rbm(1, 2, 2, why='ncols == 1 on the other operand'),
    _rbm(130, 194, 300, kw=dict(sample_h_states=False), why='B > 256 (metrics, bias); grad K = 300: nfull = 9 + tail'),
    _rbm(64, 64, 32, row=5, rows=40, why='rows 5..36 of a 40-row device array, set_row_offset(5): offset operand '
                                         'pointer and Philox row index'),
    _rbm(96, 64, 40, gaussian=True, why='prep_kernel and the sigma epilogue on fast tiles; J % 32 == 8'),
    _rbm(96, 128, 64, k=3, kw=dict(dbm_last=True), why='chain continuation'),
    _rbm(120, 192, 48, why='J % 32 == 16 (batch) and J % 32 == 24 (grad); nfull = 6 without a tail; grad K = 48: nfull = 1 '
                           '+ a 16-row tail'),
    _rbm(66, 64, 32, row=3, rows=40, kw=dict(dropout=0.8, sample_v_states=True),
         why='row offset under dropout (prep_kernel draws at row0 * V + e) and under sampled visibles (the draw index of '
             'the prop-down launch)'),
]


def _dbm(V, nh, N, M, kw=None, gaussian=False, expect=(), row=0, particle0=0, why=''):
    return dict(V=V, nh=list(nh), N=N, M=M, kw=dict(kw or {}), gaussian=gaussian, expect=tuple(expect), why=why,
                row=row, rows=N + 2 * row, particle0=particle0,
                id='%d-%s-%d-%d%s%s' % (V, '_'.join(str(x) for x in nh), N, M, '-gauss' * gaussian,
                                        ('-row%d-p%d' % (row, particle0)) * bool(row or particle0)))


DBM_LATTICE = [
    _dbm(64, [64, 64], 32, 32, kw=dict(max_mf_updates=3, mf_tol=1e-7), expect=['dbm:mf-exit-cap'], why='all fast'),
    _dbm(96, [66, 35], 33, 65, kw=dict(max_mf_updates=30, mf_tol=1e-5, l2=1e-3), expect=['dbm:mf-exit-tol'],
         why='(fast, generic); an all-generic odd layer; outer products with K = 33 and K = 65'),
    _dbm(35, [130, 96, 40], 67, 34, kw=dict(max_mf_updates=4, mf_tol=1e-9, max_norm=0.5),
         expect=['dbm:maxnorm-clipped&unclipped', 'dbm:mf-exit-cap'],
         why='(generic, fast); (fast + tail, fast + tail); a narrow top layer; clipped and unclipped columns in W_1'),
    _dbm(166, [128], 64, 96, kw=dict(max_mf_updates=2), expect=['dbm:mf-exit-cap'],
         why='one layer; K = 166: nfull = 5 together with a K tail'),
    _dbm(64, [64, 32], 32, 32, kw=dict(max_mf_updates=5, mf_tol=1e-8, sample_v_states=False, l2=1e-3), gaussian=True,
         expect=['dbm:mf-exit-cap'], why='Gaussian DBM (means only) on fast tiles'),
    _dbm(20, [12, 16], 10, 10, kw=dict(max_mf_updates=3), expect=['dbm:mf-exit-cap'], row=3, particle0=7,
         why='rows 3..12 of a 16-row device array and set_row_offset(3, 7): offset data pointer, Philox row index of the '
             'particle sweeps'),
]


def rbm_case_labels(c):
    return rbm_labels(c['V'], c['H'], c['B'], c['k'], c['kw'], c['gaussian'], c['row'])


def dbm_case_labels(c):
    return dbm_labels(c['V'], c['nh'], c['N'], c['M'], c['expect'], c['gaussian'], c['row'], c['particle0'])


def lattice_labels(rbm=None, dbm=None):
    lab = set()
    for c in (RBM_LATTICE if rbm is None else rbm):
        lab |= rbm_case_labels(c)
    for c in (DBM_LATTICE if dbm is None else dbm):
        lab |= dbm_case_labels(c)
    return lab


# ---------------------------------------------------------------------------------- initialisation shared by CPU and GPU
SEED0 = 87654321


def rbm_params(V, H):
    """the initialisation of tests/test_rbm64_parity_gpu.py"""
    from oracle import oracle as orc
    W = (orc.normal(SEED0, 1337, 0, V * H).astype(np.float64) * 0.05).reshape(V, H)
    vb = (orc.uniform_d(SEED0, 1338, 0, V) - 0.5) * 0.2
    hb = (orc.uniform_d(SEED0, 1339, 0, H) - 0.5) * 0.2
    return dict(W=W, vb=vb, hb=hb)


def rbm_data(rows, V, s, gaussian=False):
    from oracle import oracle as orc
    if gaussian:
        return orc.normal(SEED0, 43 + s, 0, rows * V).astype(np.float64).reshape(rows, V)
    return (orc.uniform_d(SEED0, 42 + s, 0, rows * V).reshape(rows, V) < 0.1307).astype(np.float64)


def rbm_sigma(V):
    return np.linspace(0.5, 1.5, V)


RBM_SEED, RBM_LR, RBM_MOM = 1337, 0.05, 0.9
RBM_LR_GAUSS = 1e-3


def dbm_params(V, nh, M, seed=3):
    """the initialisation of tests/test_dbm64_parity_gpu.py"""
    from oracle import oracle as orc
    n = [V] + list(nh)
    P = {}
    for i in range(len(nh)):
        sfx = '' if i == 0 else '_%d' % i
        P['W' + sfx] = (orc.normal(SEED0, seed + i, 0, n[i] * n[i + 1]).astype(np.float64) * 0.1).reshape(n[i], n[i + 1])
        P['hb' + sfx] = (orc.uniform_d(SEED0, seed + 10 + i, 0, n[i + 1]) - 0.5) * 0.4
        P['h' + sfx] = (orc.uniform_d(SEED0, seed + 20 + i, 0, M * n[i + 1]) < 0.5).astype(np.float64).reshape(M, n[i + 1])
    P['vb'] = (orc.uniform_d(SEED0, seed + 30, 0, V) - 0.5) * 0.4
    P['v'] = (orc.uniform_d(SEED0, seed + 31, 0, M * V) < 0.3).astype(np.float64).reshape(M, V)
    return P


def dbm_data(N, V, s, gaussian=False):
    """N rows (a case with a row offset asks for its whole device array and takes rows row .. row + N - 1)"""
    from oracle import oracle as orc
    if gaussian:
        return orc.normal(SEED0, 77 + s, 0, N * V).astype(np.float64).reshape(N, V)
    return (orc.uniform_d(SEED0, 99 + s, 0, N * V) < 0.2).astype(np.float64).reshape(N, V)


def dbm_state_names(nh):
    names = ['vb', 'dvb', 'v']
    for i in range(len(nh)):
        sfx = '' if i == 0 else '_%d' % i
        names += [b + sfx for b in ('W', 'dW', 'hb', 'dhb', 'q_means', 'mu_means', 'mu', 'h')]
    return names


# ------------------------------------------------------------------------------------------------------ numeric probes
def _neighbours(x, n=3):
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def sigmoid_probes():
    """where exp_neg can break: the half-integer multiples of ln 2 where `rint` flips (n = 0..1010, the float64 nearest
    (n + 1/2) ln 2 and three neighbours on each side), the 700 clamp, the exponent-field add near n = -1010, the
    x >= 0 / e / d branch around zero; both signs"""
    ln2 = np.log(np.longdouble(2))
    pts = []
    for n in range(1011):
        pts += _neighbours(np.float64((np.longdouble(n) + np.longdouble(0.5)) * ln2))
    pts += [0.0, 5e-324, 2.0 ** -53, 2.0 ** -52, 36.7, 37.0, np.nextafter(700.0, -np.inf), np.nextafter(700.0, np.inf),
            700.0, 745.2, 800.0, 1e300]
    pts = np.array(pts, dtype=np.float64)
    return np.concatenate([pts, -pts])


def sigmoid_exact(x):
    """long-double value of the function the engine defines: the logistic of x clamped to [-700, 700] (the clamp is part
    of the definition: exp_neg takes arguments in [0, 700])"""
    xl = np.clip(np.asarray(x, dtype=np.float64), -700.0, 700.0).astype(np.longdouble)
    return np.longdouble(1) / (np.longdouble(1) + np.exp(-xl))


def ulp_error(got, exact):
    """|got - exact| in units of the spacing of float64 at the exact value (exact: long double)"""
    sp = np.spacing(np.abs(exact).astype(np.float64)).astype(np.longdouble)
    return np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - exact) / sp


def softplus_probes():
    """about 200 points spanning +-800: 0, a coarse sweep, the points where exp(-|x|) drops below 2**-53 (log1p(e) == e,
    then x + e == x), the edge of the subnormals (-708.4), the last non-zero value (-745.13) and beyond"""
    x0 = 53 * np.log(2.0)                                       # exp(-x0) == 2**-53
    pts = [0.0, 5e-324, 2.0 ** -53, 1e-8, 0.5, 1.0, 2.0, 10.0, 30.0, 36.0, 37.0, 38.0, 100.0, 500.0, 700.0, 708.0, 708.4,
           709.0, 740.0, 745.0, 745.13, 745.2, 750.0, 800.0]
    pts += _neighbours(x0, 3) + _neighbours(np.log(2.0), 2)
    pts += list(np.linspace(0.3, 44.0, 38)) + list(np.linspace(50.0, 790.0, 20))
    pts = np.array(pts, dtype=np.float64)
    return np.concatenate([pts, -pts[1:]])


def softplus_exact(x):
    xl = np.asarray(x, dtype=np.float64).astype(np.longdouble)
    return np.maximum(xl, np.longdouble(0)) + np.log1p(np.exp(-np.abs(xl)))


def softplus_host(x):
    """the device's formula under the host's libm"""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


TINY = 2.0 ** -1022                                             # smallest normal double


def softplus_host_error():
    """E: the largest error of softplus_host in ulps of the exact value, over the probes whose exact value is normal"""
    x = softplus_probes()
    ex = softplus_exact(x)
    ok = ex >= TINY
    return float(np.max(ulp_error(softplus_host(x)[ok], ex[ok])))


# ------------------------------------------------------------------------------------------------------ max-norm edges
MAXNORM_SHAPE = (20, [12, 16], 10, 10)
MAXNORM_LIMIT = 0.3


def maxnorm_edge_params():
    """DBM parameters whose weight matrices carry the edge columns of dmaxnorm_kernel: column 0 all zero (0 * 0 / 1e-8),
    column 1 all 1e-10 (norm below the 1e-8 floor), column 2 all 1.0 (clipped to the limit), the rest random"""
    V, nh, N, M = MAXNORM_SHAPE
    P = dbm_params(V, nh, M)
    for nm in ('W', 'W_1'):
        P[nm][:, 0], P[nm][:, 1], P[nm][:, 2] = 0.0, 1e-10, 1.0
    return P


def maxnorm_exact(W, limit=MAXNORM_LIMIT):
    """long double: column norms n and W * min(n, limit) / max(n, 1e-8) (dbm.py:511-513)"""
    Wl = W.astype(np.longdouble)
    n = np.sqrt(np.sum(Wl * Wl, axis=0))
    return n, Wl * np.minimum(n, np.longdouble(limit)) / np.maximum(n, np.longdouble(1e-8))
