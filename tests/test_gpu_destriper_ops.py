"""The destriper's operator kernels (csrc/destriper_cg.hip: k_ds_bin, k_ds_project,
k_ds_project_sell, the CG vector kernels) one call at a time against the sample-level reference
of tests/golden/destriper_ops_cases.py.

On the exact inputs (small integers, h a power of two or 0) every sum of the definition is exact
in float64 -- tests/test_destriper_ops_reference.py checks T < 2^53 -- so the device must equal
the reference bit for bit whatever the lane count, unroll, grid or summation order: every
comparison of (a), (b), (d), (e) is np.array_equal.  (c) compares real-valued inputs under
|device - long double| <= (n + 8) 2^-53 T per element, n the entries of the element's operator
row and T the sum of the absolute values of its sample terms: the check that would catch a
coefficient or an accumulator held in float32, which small integers cannot.

Every test that claims a kernel instantiation asserts, from ops.nnz(), the row statistic that
selects it.  The launch knobs (COMAP_DS_*) are read when the problem is created."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import destriper_ops_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE = ('mid8', 'mid16', 'dense', 'wide', 'skew')
KNOBS = ('COMAP_DS_BL', 'COMAP_DS_BU', 'COMAP_DS_PG', 'COMAP_DS_PB', 'COMAP_DS_SELL', 'COMAP_DS_CF', 'COMAP_DS_CGGRAPH',
         'COMAP_DS_WALK', 'COMAP_DS_HEAVY')
needs_long_double = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2e-19, reason='needs an 80-bit long double')


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def knobs(monkeypatch, **kw):
    for k, v in kw.items():
        monkeypatch.setenv('COMAP_DS_' + k, str(v))


# ---------------------------------------------------------------- device side
class Dev:
    """A DeviceOps of one set of inputs, with the moves between the caller's band-major arrays
    ([n_bands, n]) and the device's interleaved vectors ([n][nb], offsets in internal order)."""

    def __init__(self, inp, okey=None):
        import torch
        from comapreduce_amd.mapmaking.destriper import DeviceOps
        p = inp['prob']
        self.torch, self.inp = torch, inp
        key = None
        if okey is not None:
            key = (torch.from_numpy(np.asarray(okey[0], np.int32)).cuda(), int(okey[1]))
        self.ops = DeviceOps(p['pix'], inp['tod'], inp['w'], p['L'], p['npix'], keep=inp['keep'], okey=key)
        self.nb, self.n_bands = self.ops.nb, inp['n_bands']
        self.NO, self.npix = self.ops.n_offsets, p['npix']
        assert self.NO == p['n_off']
        k = torch.arange(self.NO, dtype=torch.float64, device=self.ops.dev).repeat_interleave(self.nb)
        self.pos = self.ops.natural(k).cpu().numpy().reshape(self.NO, self.nb)[:, 0].astype(np.int64)

    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(self.ops.dev)

    def offsets(self, v):
        a = np.zeros((self.NO, self.nb))
        a[self.pos, :self.n_bands] = np.asarray(v, np.float64).T
        return self._dev(a)

    def offsets_back(self, t):
        return t.cpu().numpy().reshape(self.NO, self.nb)[self.pos][:, :self.n_bands].T

    def maps(self, m):
        a = np.zeros((self.npix, self.nb))
        a[:, :self.n_bands] = np.asarray(m, np.float64).T
        return self._dev(a)

    def maps_back(self, t):
        return t.cpu().numpy().reshape(self.npix, self.nb)[:, :self.n_bands].T

    def scalars(self, v):
        a = np.ones(self.nb)
        a[:self.n_bands] = v
        return self._dev(a)

    def nan(self, n):
        return self.torch.full((n * self.nb,), float('nan'), dtype=self.torch.float64, device=self.ops.dev)

    def selects(self):
        """(bin lanes, bin U, project G) the launchers choose at default dispatch, from the
        device's own entry counts."""
        nnz, nnzp = self.ops.nnz()
        U = dc.bin_unroll(nnz, self.npix)
        return dc.bin_lanes(nnzp, self.npix, U), U, dc.project_lanes(nnz, self.NO)

    def entry_form(self, form):
        want = 4 + self.nb if form == 'count' else 4 + 8 * self.nb
        assert self.ops.entry_bytes() == want, (self.ops.entry_bytes(), want)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ; first at {i}: '
                             f'device {got[i]!r}, reference {want[i]!r}')


# ---------------------------------------------------------------- shared references (computed once)
_REF = {}


def ref_of(key, what):
    """Reference result `what` ('bin0', 'bin1', 'proj', 'rhs') of dc.inputs(*key), cached."""
    k = key + (what,)
    if k not in _REF:
        inp = dc.inputs(*key)
        ref = dc.reference(inp)
        if what in ('bin0', 'bin1'):
            _REF[k] = ref.bin(inp['x'], int(what[-1]))
        elif what == 'proj':
            _REF[k] = ref.project(inp['xs'], inp['num'], inp['h'])
        else:
            _REF[k] = ref.project(None, inp['num'], inp['h'])
        assert ref.exact_ok
    return _REF[k]


def check_bin(dev, key):
    inp = dc.inputs(*key)
    x = dev.offsets(inp['x'])
    for mode in (0, 1):
        out = dev.nan(dev.npix)                      # every pixel row must be written, the empty ones too
        dev.ops.bin(x, mode, out)
        same(dev.maps_back(out), ref_of(key, f'bin{mode}')[0], f'bin mode {mode} {key}')


def check_project(dev, key):
    inp = dc.inputs(*key)
    num, h = dev.maps(inp['num']), dev.maps(inp['h'])
    y, dot = dev.nan(dev.NO), dev.nan(1)
    dev.ops.project(dev.offsets(inp['xs']), num, h, y, dot)
    r = ref_of(key, 'proj')
    same(dev.offsets_back(y), r['y'], f'project {key}')
    same(dot.cpu().numpy()[:dev.n_bands], r['dot'], f'project dot {key}')
    y = dev.nan(dev.NO)
    dev.ops.project(None, num, h, y)
    same(dev.offsets_back(y), ref_of(key, 'rhs')['y'], f'project(None) {key}')


def check_within_bound(dev, key):
    """(c): the same calls on real-valued inputs, each element within (n + 8) 2^-53 T with n the
    entries of the element's operator row (the terms the kernel sums).  Returns the largest
    error / bound, and for the record the same with n = the definition's sample terms."""
    inp = dc.inputs(*key)
    worst = 0.0
    model = dc.entry_model(inp['prob'], inp['w'])
    by_samples = [0.0]

    def ratio(got, want, n, T, what):
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        bnd = dc.bound(model['prow' if what.startswith('bin') else 'orow'][None, :], T)
        assert np.all(np.isfinite(got)), what
        over = err > bnd
        assert not np.any(over), (f'{what} {key}: {int(over.sum())} elements over the bound, largest error / bound '
                                  f'{np.max(err[over] / bnd[over]):.3g}')
        ns = dc.bound(n, T)
        by_samples[0] = max(by_samples[0], float(np.max(err[ns > 0] / ns[ns > 0])))
        return float(np.max(err[bnd > 0] / bnd[bnd > 0]))

    x = dev.offsets(inp['x'])
    for mode in (0, 1):
        out = dev.nan(dev.npix)
        dev.ops.bin(x, mode, out)
        num, n, T = ref_of(key, f'bin{mode}')
        worst = max(worst, ratio(dev.maps_back(out), num, n, T, f'bin mode {mode}'))
    num, h = dev.maps(inp['num']), dev.maps(inp['h'])
    y, dot = dev.nan(dev.NO), dev.nan(1)
    dev.ops.project(dev.offsets(inp['xs']), num, h, y, dot)
    r = ref_of(key, 'proj')
    worst = max(worst, ratio(dev.offsets_back(y), r['y'], r['n'], r['T'], 'project'))
    # y . x: each y_o within its bound, then an n_off-term sum of the products
    xa = np.abs(inp['xs'])
    dbound = np.sum(dc.bound(model['orow'][None, :], r['T']) * xa, axis=1) + (dev.NO + 1) * dc.EPS * r['Tdot'].astype(np.float64)
    derr = np.abs(dot.cpu().numpy()[:dev.n_bands].astype(np.longdouble) - r['dot']).astype(np.float64)
    assert np.all(derr <= dbound), (derr / dbound)
    y = dev.nan(dev.NO)
    dev.ops.project(None, num, h, y)
    r = ref_of(key, 'rhs')
    worst = max(worst, ratio(dev.offsets_back(y), r['y'], r['n'], r['T'], 'project(None)'))
    return worst, by_samples[0]


# ---------------------------------------------------------------- (a) bin, (b) projection: default dispatch
@pytest.mark.parametrize('form', ['count', 'full'])
@pytest.mark.parametrize('n_bands', [1, 4])
@pytest.mark.parametrize('name', FIVE)
def test_default_dispatch_bit_for_bit(name, n_bands, form):
    """Each problem selects its own instantiations (asserted from the device's entry counts); 4
    bands: different weights, tod and vectors per band, and a keep mask that drops different
    offsets per band."""
    key = (name, form, n_bands, True, n_bands == 4)
    dev = Dev(dc.inputs(*key))
    dev.entry_form(form)
    assert dev.selects() == dc.SELECTS[name], (dev.ops.nnz(), dev.NO, dev.npix)
    assert dev.ops.sell_entries() == -1
    check_bin(dev, key)
    check_project(dev, key)


@pytest.mark.parametrize('form', ['count', 'full'])
@pytest.mark.parametrize('n_bands', [2, 3])
@pytest.mark.parametrize('name', ['mid16', 'dense'])
def test_two_and_three_bands_bit_for_bit(name, n_bands, form):
    """2 bands, and 3 padded to 4 with an empty band."""
    key = (name, form, n_bands, True, False)
    dev = Dev(dc.inputs(*key))
    dev.entry_form(form)
    assert dev.nb == (2 if n_bands == 2 else 4)
    assert dev.selects() == dc.SELECTS[name]
    check_bin(dev, key)
    check_project(dev, key)


@pytest.mark.parametrize('name', ['mid8', 'dense'])
def test_full_form_forced_on_count_weights(monkeypatch, name):
    """COMAP_DS_CF=0: uniform weights stored as f64 entry sums."""
    knobs(monkeypatch, CF=0)
    key = (name, 'count', 2, True, False)
    dev = Dev(dc.inputs(*key))
    dev.entry_form('full')
    check_bin(dev, key)
    check_project(dev, key)


# ---------------------------------------------------------------- (a) bin: every lane count and unroll
@pytest.mark.parametrize('BU', [4, 8])
@pytest.mark.parametrize('BL', [4, 8, 16, 32, 64])
@pytest.mark.parametrize('name', ['dense', 'skew'])
def test_bin_lanes_and_unroll_bit_for_bit(monkeypatch, name, BL, BU):
    """Rows of thousands of entries (dense) and of 0 .. a few (skew) under every
    k_ds_bin<lanes, NB, CF, U>: count form at 1 band, full form at 4."""
    knobs(monkeypatch, BL=BL, BU=BU)
    for key in ((name, 'count', 1, True, False), (name, 'full', 4, True, True), (name, 'count', 2, True, False)):
        dev = Dev(dc.inputs(*key))
        dev.entry_form(key[1])
        check_bin(dev, key)


@pytest.mark.parametrize('n_bands', [1, 4])
def test_bin_grid_wraps_at_64_lanes(monkeypatch, n_bands):
    """npix = 270 000 at 64 lanes per row: 67 500 blocks' worth of rows on the 65 536-block grid."""
    knobs(monkeypatch, BL=64)
    key = ('skew_big', 'count', n_bands, True, False)
    dev = Dev(dc.inputs(*key))
    assert (dev.npix * 64 + 255) // 256 > 65536
    check_bin(dev, key)
    # k_div_map over npix nb values (4 bands: beyond its 4096-block grid)
    inp = dc.inputs(*key)
    out = dev.nan(dev.npix)
    dev.ops.div_map(dev.maps(inp['num']), dev.maps(inp['h']), out)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.where(inp['h'] != 0, inp['num'] / inp['h'], inp['num'])
    same(dev.maps_back(out), want, 'div_map')


# ---------------------------------------------------------------- (b) projection: CSR paths
def test_project_prefetch_path_g64(monkeypatch):
    """wide at G = 64 on 256 blocks: 275 sweeps of 4 offsets, so the next sweep's prefetched
    pass and the loop's wrap condition run."""
    knobs(monkeypatch, PG=64, PB=256, SELL=0)
    for key in (('wide', 'count', 1, True, False), ('wide', 'full', 4, True, True)):
        dev = Dev(dc.inputs(*key))
        assert dev.selects()[2] == 64 and -(-dev.NO // (256 // 64)) > 256
        check_project(dev, key)


@pytest.mark.parametrize('PG', [4, 8, 16, 32, 64])
def test_project_lane_groups_on_skew(monkeypatch, PG):
    """Rows of ~245 entries among rows of ~10 under every G: the long-rows loop runs
    ceil(245 / 4 G) - 1 passes (15 at G = 4, none at G = 64)."""
    knobs(monkeypatch, PG=PG, SELL=0)
    if PG <= 8:
        knobs(monkeypatch, PB=256)
    for key in (('skew', 'count', 4, True, True), ('skew', 'full', 1, True, False), ('skew', 'count', 2, True, False)):
        dev = Dev(dc.inputs(*key))
        assert dev.ops.nnz()[0] > 24 * 200          # the 24 wide offsets' rows are there
        check_project(dev, key)


def test_project_grid_wraps_at_g16(monkeypatch):
    """mid16's pointing at 4200 offsets, G = 16 on 256 blocks: 263 sweeps."""
    knobs(monkeypatch, PG=16, PB=256, SELL=0)
    for key in (('mid16_long', 'count', 1, True, False), ('mid16_long', 'full', 2, True, False)):
        dev = Dev(dc.inputs(*key))
        assert dev.selects()[2] == 16 and dev.NO > 256 * 16
        check_project(dev, key)


# ---------------------------------------------------------------- (b) projection: sliced-ELLPACK
@pytest.mark.parametrize('name', ['skew', 'wide', 'mid8'])
def test_project_sell_bit_for_bit(monkeypatch, name):
    """Offset counts that are no multiple of 64 (a partly filled last chunk), rows of 0 .. 250
    entries inside one chunk."""
    knobs(monkeypatch, SELL=1)
    for key in ((name, 'count', 1, True, False), (name, 'full', 4, True, True), (name, 'count', 4, True, True),
                (name, 'full', 2, True, False)):
        dev = Dev(dc.inputs(*key))
        assert dev.NO % 64 and dev.ops.sell_entries() >= dev.ops.nnz()[0]
        check_project(dev, key)
        check_bin(dev, key)


@pytest.mark.parametrize('n_bands', [1, 4])
def test_project_sell_more_chunks_than_waves(monkeypatch, n_bands):
    """70 001 offsets of L = 4 on 256 blocks: 1094 chunks for 1024 waves."""
    knobs(monkeypatch, SELL=1, PB=256)
    key = ('short', 'count' if n_bands == 1 else 'full', n_bands, True, False)
    dev = Dev(dc.inputs(*key))
    assert dev.ops.sell_entries() > 0 and (dev.NO + 63) // 64 > 256 * 4
    check_project(dev, key)


# ---------------------------------------------------------------- an arbitrary internal order
@pytest.mark.parametrize('sell', [0, 1])
def test_caller_keyed_offset_order(monkeypatch, sell):
    """okey: seeded random keys instead of the first on-map pixel."""
    knobs(monkeypatch, SELL=sell)
    key = ('mid8', 'count', 4, True, True)
    inp = dc.inputs(*key)
    okey = np.random.default_rng(77).integers(0, 1000, size=inp['prob']['n_off']).astype(np.int32)
    dev = Dev(inp, okey=(okey, 1000))
    same(dev.pos, dc.reference(inp).offset_order(okey), 'internal order')
    check_bin(dev, key)
    check_project(dev, key)


# ---------------------------------------------------------------- (c) real-valued inputs
@needs_long_double
@pytest.mark.parametrize('sell', [0, 1])
@pytest.mark.parametrize('form', ['count', 'full'])
@pytest.mark.parametrize('n_bands', [1, 4])
@pytest.mark.parametrize('name', ['skew', 'dense'])
def test_real_inputs_within_derived_bound(monkeypatch, name, n_bands, form, sell):
    knobs(monkeypatch, SELL=sell)
    key = (name, form, n_bands, False, False)
    dev = Dev(dc.inputs(*key))
    dev.entry_form(form)
    worst, by_samples = check_within_bound(dev, key)
    print(f'\nratio {name} nb={n_bands} {form} {"sell" if sell else "csr"}: largest error / bound = {worst:.4f}'
          f' (with n = sample terms: {by_samples:.4f})')


# ---------------------------------------------------------------- (d) vector kernels
ALPHA = ((3.0, 12.0), (5.0, 40.0), (7.0, 14.0), (6.0, 3.0))       # rr / pq = 1/4, 1/8, 1/2, 2
BETA = ((12.0, 3.0), (5.0, 40.0), (7.0, 14.0), (3.0, 6.0))        # rr_new / rr = 4, 1/8, 1/2, 1/2


@pytest.mark.parametrize('n_bands', [1, 4])
@pytest.mark.parametrize('name', ['vector', 'pairs'])
def test_vector_kernels_bit_for_bit(name, n_bands):
    """1 100 003 offsets: the second grid-stride trip of every vector kernel (the 4096-block
    ones wrap above 1 048 576); 300 037: of the 1024-block update and the 256-block dot."""
    key = (name, 'count', n_bands, True, False)
    inp = dc.inputs(*key)
    dev = Dev(inp)
    ops, NO, nb = dev.ops, dev.NO, n_bands
    ref = dc.reference(inp)
    same(dev.pos, ref.offset_order(), 'natural: the internal order')
    rng = np.random.default_rng(5 + n_bands)
    x, r, p, q = (dc.integers(rng, (nb, NO), 1024) for _ in range(4))
    # natural: per-band values
    same(ops.natural(dev.offsets(x)).cpu().numpy().reshape(NO, dev.nb).T, x, 'natural')
    # dot
    out = dev.nan(1)
    ops.dot(dev.offsets(p), dev.offsets(q), out)
    same(out.cpu().numpy(), ref.dot(p, q)[0], 'dot')
    # update: x += a p, r -= a q, r.r
    rr, pq = (np.array(v[:nb]) for v in zip(*ALPHA))
    a = (rr / pq)[:, None]
    xd, rd, rrn = dev.offsets(x), dev.offsets(r), dev.nan(1)
    ops.cg_update(dev.scalars(rr), dev.scalars(pq), xd, rd, dev.offsets(p), dev.offsets(q), rrn)
    r1 = r - a * q
    same(dev.offsets_back(xd), x + a * p, 'cg_update x')
    same(dev.offsets_back(rd), r1, 'cg_update r')
    r8 = np.rint(8 * r1).astype(np.int64)
    assert np.array_equal(r8, 8 * r1)
    same(rrn.cpu().numpy(), np.sum(r8 * r8, axis=1) / 64.0, 'cg_update r.r')
    # direction: p = r + b p
    rn, ro = (np.array(v[:nb]) for v in zip(*BETA))
    pd = dev.offsets(p)
    ops.cg_direction(dev.scalars(rn), dev.scalars(ro), pd, dev.offsets(r))
    same(dev.offsets_back(pd), r + (rn / ro)[:, None] * p, 'cg_direction')
    # div_map with the dyadic h
    out = dev.nan(dev.npix)
    ops.div_map(dev.maps(inp['num']), dev.maps(inp['h']), out)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.where(inp['h'] != 0, inp['num'] / inp['h'], inp['num'])
    same(dev.maps_back(out), want, 'div_map')
    # the count form's wbar o x pre-scale (k_scale) through the bin, and the default SELL projection
    dev.entry_form('count')
    assert ops.sell_entries() > 0
    check_bin(dev, key)
    check_project(dev, key)


# ---------------------------------------------------------------- (e) the native loop's private paths
@pytest.mark.parametrize('sell', [0, 1])
@pytest.mark.parametrize('form', ['count', 'full'])
@pytest.mark.parametrize('n_bands', [1, 4])
@pytest.mark.parametrize('name', ['skew', 'dense', 'pairs'])
def test_native_loop_equals_per_piece_drivers(monkeypatch, name, n_bands, form, sell):
    """comap_destripe_solve (hit-row bin that divides by h, pre-scaled pt, fused update and
    direction; one replayed 16-iteration graph + 2 eager iterations) against cg_solve and
    cg_solve_batched over the per-piece calls checked above: x and the iteration counts equal."""
    from comapreduce_amd.mapmaking.destriper import cg_solve, cg_solve_batched
    knobs(monkeypatch, SELL=sell, CGGRAPH=1)
    dev = Dev(dc.inputs(name, form, n_bands, False, False))
    ops = dev.ops
    dev.entry_form(form)
    xn, itn, _ = ops.solve_native(0.0, 18)
    xn = xn.cpu().numpy()
    assert itn == [18] * n_bands and np.all(np.isfinite(xn)) and np.any(xn != 0)
    xb, itb, _, _ = cg_solve_batched(ops, lambda a: a, threshold=0.0, niter=18)
    assert itb == itn
    same(ops.natural(xb).cpu().numpy(), xn, 'cg_solve_batched x')
    if n_bands == 1:
        xc, itc, _, _ = cg_solve(ops, lambda a: a, threshold=0.0, niter=18)
        assert [itc] == itn
        same(ops.natural(xc).cpu().numpy(), xn, 'cg_solve x')
