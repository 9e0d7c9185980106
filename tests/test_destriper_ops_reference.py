"""The operator-kernel tests' own footing (tests/golden/destriper_ops_cases.py),
checked without a GPU: the exact inputs really make every sum exact in float64, the problem
generators produce the row statistics that select the kernel instantiations the GPU tests claim
(under the entry model: distinct (offset, pixel id) pairs among non-zero-weight samples), and the
sample-level reference agrees with the oracle's operator pieces (oracle.destriper.ShardOps)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import destriper_ops_cases as dc  # noqa: E402

FIVE = ('mid8', 'mid16', 'dense', 'wide', 'skew')
ALL = FIVE + ('vector', 'skew_big', 'mid16_long', 'short', 'pairs')


@pytest.mark.parametrize('form', ['count', 'full'])
@pytest.mark.parametrize('name', ALL)
def test_exact_inputs_keep_every_sum_below_2_53(name, form):
    """T = sum |terms| < 2^53 per element (checked on the int64 sums, the projection's in units
    of 1/4) for the bin, both projections and their dot products at 4 bands: the float64
    evaluation of the definition, in any order, then equals the int64 one bit for bit."""
    inp = dc.inputs(name, form, 4)
    ref = dc.reference(inp)
    worst = 0.0
    for mode in (0, 1):
        num, n, T = ref.bin(inp['x'], mode)
        assert num.dtype == np.float64 and np.all(num == np.rint(num))
        worst = max(worst, T.max())
    for x in (inp['xs'], None):
        r = ref.project(x, inp['num'], inp['h'])
        assert np.all(4 * r['y'] == np.rint(4 * r['y']))
        worst = max(worst, 4 * r['T'].max(), 0.0 if x is None else 4 * r['Tdot'].max())
    _, T = ref.dot(inp['x'], inp['tod'][:, :inp['x'].shape[1]])
    worst = max(worst, T.max())
    print(f'{name} {form}: largest T = 2^{np.log2(worst):.1f}')
    assert ref.exact_ok and worst < 2.0 ** 53


@pytest.mark.parametrize('n_bands', [1, 4])
@pytest.mark.parametrize('name', FIVE)
def test_generators_select_the_instantiations(name, n_bands):
    prob = dc.problem(name)
    for form in ('count', 'full'):
        w = dc.inputs(name, form, n_bands)['w']
        e = dc.entry_model(prob, w)
        lanes, U, G = dc.SELECTS[name]
        assert dc.bin_unroll(e['nnz'], prob['npix']) == U
        assert dc.bin_lanes(e['nnzp'], prob['npix'], U) == lanes, e['nnzp'] // prob['npix']
        assert dc.project_lanes(e['nnz'], prob['n_off']) == G, e['nnz'] / prob['n_off']
        # where G is what the problem is for, the mean must not sit on a threshold: 5 % of slack
        for nnz in (int(0.95 * e['nnz']), int(1.05 * e['nnz'])) if name != 'dense' else ():
            assert dc.project_lanes(nnz, prob['n_off']) == G
        assert np.all(e['orow'][prob['dead']] == 0) and np.sum(e['orow'] == 0) >= dc.N_DEAD      # empty offset rows
        tail = np.arange(prob['npix'] - dc.TAIL, prob['npix'])
        assert np.all(e['prow'][tail] == 0) and np.all(e['read'][tail] > 0)       # hit only through the wrap
        off = np.mean(prob['pix'] < 0)
        assert 0.02 < off < 0.04 and prob['pix'].min() >= -prob['npix'] and prob['pix'].dtype == np.int32
        assert 0.03 < np.mean(w == 0) < 0.08


def test_single_path_problems():
    """The variants' statistics: the long rows of skew, the grid wraps of the scaled problems."""
    e = dc.entry_model(dc.problem('skew'), dc.inputs('skew', 'count', 1)['w'])
    wide = e['orow'][::dc.WIDE_EVERY]
    assert wide[wide > 0].min() > 14 * 16 and wide.max() <= 250        # ~15 passes of 16 entries at G = 4
    assert np.sort(e['orow'])[len(e['orow']) // 2] <= 16
    e = dc.entry_model(dc.problem('wide'), dc.inputs('wide', 'count', 1)['w'])
    assert 225 < e['nnz'] / 1100 < 245
    e = dc.entry_model(dc.problem('dense'), dc.inputs('dense', 'count', 1)['w'])
    assert e['nnzp'] // 48 > 2000
    big = dc.problem('skew_big')
    assert (big['npix'] * 64 + 255) // 256 > 65536                      # k_ds_bin's grid wraps at 64 lanes
    long = dc.problem('mid16_long')
    e = dc.entry_model(long, dc.inputs('mid16_long', 'count', 1)['w'])
    assert dc.project_lanes(e['nnz'], long['n_off']) == 16 and long['n_off'] > 256 * 16
    assert (dc.problem('short')['n_off'] + 63) // 64 > 256 * 4           # more SELL chunks than waves at 256 blocks
    assert dc.problem('pairs')['n_off'] > 262_144 and dc.problem('vector')['n_off'] > 1_048_576
    assert dc.problem('skew')['n_off'] % 64 and dc.problem('wide')['n_off'] % 64 and dc.problem('mid8')['n_off'] % 64


def shard_ops(inp, b):
    import oracle.destriper as od
    p = inp['prob']
    return od.ShardOps(p['pix'].astype(np.int64), inp['tod'][b], inp['w'][b], p['L'], p['npix'])


@pytest.mark.parametrize('name,form', [('tiny', 'full'), ('mid8', 'count'), ('skew', 'full')])
def test_reference_equals_oracle_pieces_on_exact_inputs(name, form):
    inp = dc.inputs(name, form, 2)
    ref = dc.reference(inp)
    for b in range(2):
        so = shard_ops(inp, b)
        for mode in (0, 1):
            out = np.zeros(so.npix)
            so.bin(inp['x'][b], mode, out)
            assert np.array_equal(out, ref.bin(inp['x'], mode)[0][b])
        for x in (inp['xs'], None):
            y, d = np.zeros(so.n_offsets), np.zeros(1)
            so.project(None if x is None else x[b], inp['num'][b], inp['h'][b], y, None if x is None else d)
            r = ref.project(x, inp['num'], inp['h'])
            assert np.array_equal(y, r['y'][b])
            assert x is None or d[0] == r['dot'][b]


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2e-19, reason='needs an 80-bit long double')
@pytest.mark.parametrize('name,form', [('tiny', 'full'), ('mid8', 'count'), ('skew', 'full')])
def test_reference_agrees_with_oracle_pieces_on_real_inputs(name, form):
    """|oracle (float64) - reference (long double)| <= (n + 8) 2^-53 T per element."""
    inp = dc.inputs(name, form, 2, exact=False)
    ref = dc.reference(inp)
    worst = 0.0
    for b in range(2):
        so = shard_ops(inp, b)
        for mode in (0, 1):
            out = np.zeros(so.npix)
            so.bin(inp['x'][b], mode, out)
            num, n, T = ref.bin(inp['x'], mode)
            err, bnd = np.abs(out - num[b]).astype(float), dc.bound(n[b], T[b])
            assert np.all(err <= bnd)
            worst = max(worst, np.max(err[bnd > 0] / bnd[bnd > 0]))
        for x in (inp['xs'], None):
            y = np.zeros(so.n_offsets)
            so.project(None if x is None else x[b], inp['num'][b], inp['h'][b], y)
            r = ref.project(x, inp['num'], inp['h'])
            err, bnd = np.abs(y - r['y'][b]).astype(float), dc.bound(r['n'][b], r['T'][b])
            assert np.all(err <= bnd)
            worst = max(worst, np.max(err[bnd > 0] / bnd[bnd > 0]))
    print(f'{name} {form}: largest error / bound = {worst:.3f}')


def test_offset_order_is_the_stable_sort_by_first_on_map_pixel():
    inp = dc.inputs('tiny', 'full', 1)
    ref = dc.reference(inp)
    pos = ref.offset_order()
    assert np.array_equal(np.sort(pos), np.arange(ref.NO))
    p = inp['prob']['pix'].reshape(ref.NO, -1)
    key = np.array([next((v for v in row if v >= 0), inp['prob']['npix']) for row in p])
    inv = np.argsort(pos)
    assert np.all(np.diff(key[inv]) >= 0)
    same = np.diff(key[inv]) == 0
    assert np.all(np.diff(inv)[same] > 0)
