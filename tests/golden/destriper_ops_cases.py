"""Problems, inputs and the sample-level reference for the destriper's operator kernels
(tests/test_destriper_ops_reference.py, tests/test_gpu_destriper_ops.py).

A *problem* is the pointing of N = n_off L samples plus the cut pattern (the offsets whose
weights are all zero).  *Inputs* add per-band weights, tod and the vectors a test hands to the
operator.  In the exact inputs every value is a small integer (h: a power of two or 0), so
every sum of the operator's definition is exact in float64 in any order -- the device must
equal the reference bit for bit.  The real-valued inputs are compared under the bound
(n + 8) 2^-53 T per element, T the sum of the absolute values of the element's sample terms
and n the number of terms summed -- the entries of the element's operator row for the device
(entry_model), the row's non-zero-weight samples for a sample-by-sample evaluation such as the
oracle's; the reference then runs in np.longdouble.

The reference is the definition, sample by sample and band by band, in the caller's offset
order; it shares no code with oracle/destriper.py.
"""
import functools

import numpy as np

EPS = 2.0 ** -53
TAIL = 3            # the last TAIL pixels are never binned: only negative ids read them (numpy's wrap)
N_DEAD = 7          # offsets whose weights are all zero (empty offset rows)

#            L   offsets  npix  pointing     what the problem selects by itself
PROBLEMS = {
    'mid8':   dict(L=20, n_off=1100, npix=1500, kind='uniform', seed=101),     # bin 8 lanes, project G = 8
    'mid16':  dict(L=50, n_off=1100, npix=700, kind='uniform', seed=102),      # bin 16 lanes, project G = 16
    'dense':  dict(L=50, n_off=4500, npix=48, kind='uniform', seed=103),       # bin 32 lanes, U = 8
    'wide':   dict(L=250, n_off=1100, npix=5000, kind='wide', seed=104),       # project G = 64
    # (1 wide offset in 64: with 1 in 32 the off-map ids of the narrow offsets -- ~7 distinct
    # ones each -- bring the mean row to ~17 entries, i.e. G = 8)
    'skew':   dict(L=250, n_off=1500, npix=4096, kind='skew', seed=105),       # project G = 4, long rows
    'vector': dict(L=1, n_off=1_100_003, npix=4096, kind='uniform', seed=106),  # every grid-stride wrap
    # variants for single paths
    'skew_big':  dict(L=250, n_off=1500, npix=270_000, kind='skew', seed=107),   # bin grid wrap at 64 lanes
    'mid16_long': dict(L=50, n_off=4200, npix=700, kind='uniform', seed=108),   # project G = 16 grid wrap
    'short':  dict(L=4, n_off=70_001, npix=4096, kind='uniform', seed=109),     # more SELL chunks than waves
    'pairs':  dict(L=2, n_off=300_037, npix=4096, kind='uniform', seed=110),    # the 1024-block kernels' wrap
    'tiny':   dict(L=6, n_off=24, npix=144, kind='uniform', seed=111),          # 12 x 12 map: dense-matrix check
}
WIDE_EVERY = 64     # skew: one offset in WIDE_EVERY visits L distinct pixels, the rest 3


@functools.lru_cache(maxsize=None)
def problem(name):
    """{'pix' int32 [N], 'L', 'npix', 'n_off', 'dead' (the all-zero-weight offsets)}"""
    spec = PROBLEMS[name]
    L, NO, npix, kind = spec['L'], spec['n_off'], spec['npix'], spec['kind']
    rng = np.random.default_rng(spec['seed'])
    M = npix - TAIL                                   # binned ids stay below the tail
    if kind == 'uniform':
        pix = rng.integers(0, M, size=(NO, L))
    else:
        start = rng.integers(0, M, size=(NO, 1))
        run = (start + np.arange(L)[None, :]) % M        # L distinct pixels per offset
        run = rng.permuted(run, axis=1)
        if kind == 'skew':
            three = rng.integers(0, M, size=(NO, 3))
            narrow = np.take_along_axis(three, rng.integers(0, 3, size=(NO, L)), axis=1)
            wide = (np.arange(NO) % WIDE_EVERY == 0)[:, None]
            run = np.where(wide, run, narrow)
        pix = run
    pix = pix.reshape(-1).astype(np.int64)
    N = pix.size
    off = rng.random(N) < 0.03                           # unbinned samples: they read m[npix + p]
    pix[off] = rng.integers(-npix, 0, size=int(off.sum()))
    first = np.nonzero(off)[0][:TAIL]
    pix[first] = -1 - np.arange(first.size)              # the tail pixels are read through the wrap
    dead = np.sort(rng.choice(NO, size=min(N_DEAD, NO // 3), replace=False))
    return {'name': name, 'pix': pix.astype(np.int32), 'L': L, 'npix': npix, 'n_off': NO, 'dead': dead}


def band_weights(prob, form, n_bands, exact, seed=0, keep=False):
    """(w [n_bands, N], keep [n_bands, n_off] uint8 or None).  form 'count': one value per
    (offset, band) -- integers 1 .. 7 or uniform (0.5, 2) -- and 0 on ~5 % cut samples (the cut
    differs per band); 'full': per-sample integers 1 .. 15 or uniform (0.5, 2).  The problem's
    dead offsets are zero in every band; keep: every band also drops its own ~4 % of offsets."""
    L, NO = prob['L'], prob['n_off']
    N = NO * L
    rng = np.random.default_rng([seed, 17, n_bands, form == 'count', exact])
    if form == 'count':
        wb = rng.integers(1, 8, size=(n_bands, NO)).astype(float) if exact else rng.uniform(0.5, 2.0, (n_bands, NO))
        w = np.repeat(wb, L, axis=1)
    else:
        w = rng.integers(1, 16, size=(n_bands, N)).astype(float) if exact else rng.uniform(0.5, 2.0, (n_bands, N))
    w[rng.random((n_bands, N)) < 0.05] = 0.0
    live = np.ones((n_bands, NO), bool)
    live[:, prob['dead']] = False
    kp = None
    if keep:
        drop = rng.random((n_bands, NO)) < 0.04
        live &= ~drop
        kp = (~drop).astype(np.uint8)
    w *= np.repeat(live, L, axis=1)
    return w, kp


def integers(rng, shape, bound):
    return rng.integers(-bound, bound + 1, size=shape).astype(float)


@functools.lru_cache(maxsize=None)
def inputs(name, form, n_bands, exact=True, keep=False):
    """One problem's weights, tod and operator arguments (caller's offset order, band-major):
    x / xs [n_bands, n_off] (xs: |v| <= 64, for the calls whose output enters a dot product),
    num [n_bands, npix], h [n_bands, npix] (exact: from {0, 1/2, 1, 2, 4})."""
    prob = problem(name)
    NO, npix, N = prob['n_off'], prob['npix'], prob['n_off'] * prob['L']
    w, kp = band_weights(prob, form, n_bands, exact, keep=keep)
    rng = np.random.default_rng([PROBLEMS[name]['seed'], n_bands, form == 'count', exact, 5])
    if exact:
        tod = integers(rng, (n_bands, N), 1024)
        x = integers(rng, (n_bands, NO), 1024)
        xs = integers(rng, (n_bands, NO), 64)
        num = integers(rng, (n_bands, npix), 1024)
        h = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 4.0]), size=(n_bands, npix))
    else:
        tod = rng.standard_normal((n_bands, N))
        x = rng.standard_normal((n_bands, NO))
        xs = rng.standard_normal((n_bands, NO))
        num = rng.standard_normal((n_bands, npix))
        h = rng.uniform(0.5, 2.0, (n_bands, npix))
        h[rng.random((n_bands, npix)) < 0.1] = 0.0
    return {'prob': prob, 'form': form, 'n_bands': n_bands, 'exact': exact, 'w': w, 'keep': kp, 'tod': tod,
            'x': x, 'xs': xs, 'num': num, 'h': h}


# ---------------------------------------------------------------- the entry model
def entry_model(prob, w):
    """The operator's entries as the set-up forms them: the distinct (offset, pixel id) pairs
    among the samples whose weight is non-zero in some band.  {'nnz' (all), 'nnzp' (binned ids),
    'orow' [n_off] / 'prow' [npix] row lengths, 'read' [npix] entries reading the pixel through
    the wrap}."""
    L, NO, npix = prob['L'], prob['n_off'], prob['npix']
    pix = prob['pix'].astype(np.int64)
    on = np.any(np.atleast_2d(w) != 0, axis=0)
    o = (np.arange(pix.size) // L)[on]
    p = pix[on]
    key = np.unique(o * (2 * npix) + (p + npix))
    eo, ep = key // (2 * npix), key % (2 * npix) - npix
    binned = ep >= 0
    return {'nnz': int(key.size), 'nnzp': int(binned.sum()),
            'orow': np.bincount(eo, minlength=NO), 'prow': np.bincount(ep[binned], minlength=npix),
            'read': np.bincount(ep[~binned] + npix, minlength=npix)}


def bin_lanes(nnzp, npix, U):
    """launch_bin_u's choice of lanes per pixel row."""
    mean = nnzp // npix
    return 32 if (mean >= 256 and U == 8) else (16 if mean >= 24 else (8 if mean >= 10 else 4))


def bin_unroll(nnz, npix):
    return 8 if nnz >= 256 * npix else 4


def project_lanes(nnz, n_off):
    """project_lanes' choice of lanes per offset row: the fewest with 4 G >= ceil(nnz / NO)."""
    mean = -(-nnz // n_off)
    g = 4
    while g < 64 and 4 * g < mean:
        g *= 2
    return g


# what each problem selects at default dispatch: (bin lanes, bin U, project G)
SELECTS = {'mid8': (8, 4, 8), 'mid16': (16, 4, 16), 'dense': (32, 8, 8), 'wide': (16, 4, 64), 'skew': (4, 4, 4)}


# ---------------------------------------------------------------- the reference
def sum_by(idx, vals, n):
    out = np.zeros(n, dtype=vals.dtype)
    np.add.at(out, idx, vals)
    return out


class Reference:
    """bin and project from their definitions, one band at a time, one term per sample.

    exact: the inputs are integers (h a power of two or 0) and every sum runs in int64 (the
    projection in units of 1/4, which holds num / h for h in {1/2, 1, 2, 4}); otherwise in
    np.longdouble.  Every result comes with n (the terms of each element's sum: its
    non-zero-weight samples) and T (the sum of the terms' absolute values); exact results
    are float64 when T < 2^53 holds, which ``exact_ok`` reports."""

    def __init__(self, pix, w, tod, L, npix, exact):
        self.acc = np.int64 if exact else np.longdouble
        self.exact = exact
        self.L, self.npix = int(L), int(npix)
        self.pix = np.asarray(pix).astype(np.int64)
        self.N = self.pix.size
        self.NO = self.N // self.L
        self.w, self.tod = np.atleast_2d(w), np.atleast_2d(tod)
        self.nb = self.w.shape[0]
        self.off = np.arange(self.N) // self.L
        self.binned = self.pix >= 0
        self.read = np.where(self.binned, self.pix, self.npix + self.pix)      # m[pointing]'s wrap
        self.exact_ok = True

    def _a(self, v):
        """float64 input in the accumulation type (exact inputs are integers)."""
        if self.exact:
            i = np.asarray(v).astype(np.int64)
            assert np.array_equal(i, v), 'exact inputs must be integers'
            return i
        return np.asarray(v).astype(np.longdouble)

    def _out(self, s, T, scale=1):
        """The sums as the caller compares them: exact -> float64 (exact when T < 2^53)."""
        if not self.exact:
            return s, T
        if T.size and int(np.max(T)) >= 2 ** 53:
            self.exact_ok = False
        return s.astype(np.float64) / scale, T.astype(np.float64) / scale

    def bin(self, x, mode=0):
        """num_p = sum_{i: pix_i = p >= 0} w_i x_o(i); mode 1: sum w_i tod_i - num_p.
        Returns (num, n, T), each [nb, npix]."""
        out = []
        sel = self.binned
        p, o = self.pix[sel], self.off[sel]
        for b in range(self.nb):
            w = self._a(self.w[b][sel])
            t = w * self._a(x[b])[o]
            s, T = sum_by(p, t, self.npix), sum_by(p, np.abs(t), self.npix)
            if mode == 1:
                tt = w * self._a(self.tod[b][sel])
                s = sum_by(p, tt, self.npix) - s
                T = T + sum_by(p, np.abs(tt), self.npix)
            n = sum_by(p, (w != 0).astype(np.int64), self.npix)
            s, T = self._out(s, T)
            out.append((s, n, T))
        return tuple(np.stack(v) for v in zip(*out))

    def share(self, num, h, b):
        """m = num / h where h != 0, else num; exact: 4 m as int64."""
        hv = np.asarray(h[b], np.float64)
        if self.exact:
            assert np.all(np.isin(hv, [0.0, 0.5, 1.0, 2.0, 4.0]))
            fac = np.where(hv == 0, 4.0, 4.0 / np.where(hv == 0, 1.0, hv)).astype(np.int64)
            return self._a(num[b]) * fac
        nu, hl = self._a(num[b]), self._a(hv)
        return np.where(hl != 0, nu / np.where(hl != 0, hl, 1), nu)

    def project(self, x, num, h):
        """y_o = (sum_{i in o} w_i) x_o - sum_{i in o} w_i m[wrap(pix_i)] (x None: the first
        term is sum w_i tod_i), and the fused dot y . x per band.  Returns {'y', 'n', 'T'
        [nb, NO], 'dot', 'Tdot' [nb] (None without x)}."""
        scale = 4 if self.exact else 1
        ys, ns, Ts, dots, Tdots = [], [], [], [], []
        for b in range(self.nb):
            w = self._a(self.w[b])
            m = self.share(num, h, b)
            z = self._a(self.tod[b]) if x is None else self._a(x[b])[self.off]
            first, second = scale * w * z, w * m[self.read]
            y = sum_by(self.off, first - second, self.NO)
            T = sum_by(self.off, np.abs(first) + np.abs(second), self.NO)
            ns.append(sum_by(self.off, (w != 0).astype(np.int64), self.NO))
            if x is not None:
                yx = y * self._a(x[b])
                d, Td = np.sum(yx, keepdims=True), np.sum(np.abs(yx), keepdims=True)
                d, Td = self._out(d, Td, scale)
                dots.append(d[0])
                Tdots.append(Td[0])
            y, T = self._out(y, T, scale)
            ys.append(y)
            Ts.append(T)
        res = {'y': np.stack(ys), 'n': np.stack(ns), 'T': np.stack(Ts), 'dot': None, 'Tdot': None}
        if x is not None:
            res['dot'], res['Tdot'] = np.array(dots), np.array(Tdots)
        return res

    def dot(self, a, c):
        """(sum_o a_o c_o per band, sum |a_o c_o|)"""
        t = np.stack([self._a(a[b]) * self._a(c[b]) for b in range(self.nb)])
        s, T = self._out(np.sum(t, axis=1), np.sum(np.abs(t), axis=1))
        return s, T

    def offset_order(self, okey=None):
        """pos[o]: the internal position of the caller's offset o -- a stable sort by okey, or by
        the offset's first on-map pixel id (npix when it has none)."""
        if okey is None:
            p = self.pix.reshape(self.NO, self.L)
            on = p >= 0
            okey = np.where(on.any(axis=1), p[np.arange(self.NO), np.argmax(on, axis=1)], self.npix)
        order = np.argsort(np.asarray(okey), kind='stable')
        pos = np.empty(self.NO, np.int64)
        pos[order] = np.arange(self.NO)
        return pos


def reference(inp):
    return Reference(inp['prob']['pix'], inp['w'], inp['tod'], inp['prob']['L'], inp['prob']['npix'], inp['exact'])


def bound(n, T):
    """(n + 8) 2^-53 T: an n-term sum in any order, products fused or not, is within
    (n + 1) u T to first order; + 8 covers the count form's roundings of wbar o x and wbar g, the
    projection's m = num / h, and second order."""
    return (np.asarray(n, np.float64) + 8.0) * EPS * np.asarray(T, np.float64)
