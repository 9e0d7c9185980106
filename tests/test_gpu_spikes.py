"""Kernel-level parity of the Level-2 spike mask (comap_spikes, spikes_kernels.hip) with
oracle.spikes, bit for bit, on inputs that run every path of the three kernels: the LDS
nanmedian of a scan shorter than the window (odd and even count), the running-median
path at n == w, scans holding NaN / +-inf, an all-zero row (rms NaN), dilation clipped
at scan edges that touch the next scan, dilation wider than a 1024-sample tile, an empty
scan, a gap, T shorter than one tile, and five (window, step, threshold) sets.

The expected mask is built per (row, scan) from oracle.spikes.tod_auto_rms / fit_spikes /
median_filter with the case's own parameters (oracle.spikes.spike_mask fixes the defaults).
The device forms the rms in another summation order than NumPy, so the mask is only
defined where no sample sits on the threshold: the oracle-only conditions below assert a
relative distance of >= 1e-6 from it for every sample, and that the expected masks are
neither empty where they are meant to fire nor set where they are not.
"""
import warnings

import numpy as np
import pytest

import oracle.spikes as ospk

pytestmark = pytest.mark.gpu

T = 5000
# A: crosses two tile boundaries; B: n < w, even; C: n = w - 1, odd; D: n = w (running
# median); an empty scan; [2549, 2600) is in no scan; F; G ends at T
SCANS = {'A': (0, 2300), 'B': (2300, 2350), 'C': (2350, 2449), 'D': (2449, 2549), 'F': (2600, 3700),
         'G': (3700, 5000)}
EDGES = np.array([SCANS['A'], SCANS['B'], SCANS['C'], SCANS['D'], (2549, 2549), SCANS['F'], SCANS['G']],
                 dtype=np.int64)
GAP = (2549, 2600)
PARAMS = [(100, 100, 10.0), (101, 7, 5.0), (400, 100, 4.0), (1023, 1, 10.0), (100, 1100, 10.0)]   # (w, step, thr)
DEFAULT = PARAMS[0]
SPIKE = 0.05
SIGMA = 1e-3
MARGIN = 1e-6
PROBE = 2e-4      # the row-5 probes sit this far (relative) inside the default threshold
NAN_AT = 3200     # row 3, inside F
FIRING_ROWS = (0, 1, 3, 5, 7)
EMPTY_ROWS = (2, 4, 6)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with np.errstate(all='ignore'):
            return fn(*a, **k)


def _set_probes(row):
    """Two samples of scan B (even count) and two of scan C (odd count) of ``row`` at
    median +- thr rms (1 - PROBE) for the default threshold: none fires, and a scan
    median that is off by as little as half an order-statistic spacing makes one fire.
    The row's rms depends (weakly) on the probes, so they are placed by fixed-point
    iteration."""
    w, _, thr = DEFAULT
    spots = [(2310, 2330, SCANS['B']), (2380, 2420, SCANS['C'])]
    for _ in range(40):
        rms = ospk.tod_auto_rms(row)
        for hi, lo, (s, e) in spots:
            med = ospk.median_filter(row[s:e], w)[0]
            row[hi] = med + thr * rms * (1.0 - PROBE)
            row[lo] = med - thr * rms * (1.0 - PROBE)


def make_main():
    """Two feeds x four bands x T = 5000 (row = 4 feed + band), Gaussian noise of 1e-3."""
    rng = np.random.default_rng(20240607)
    tod = SIGMA * rng.standard_normal((8, T))
    # row 0: single spikes at the file's first and last sample, at a tile's last sample,
    # at A's last sample, and one inside each of B, C, D (and F, so that every scan fires)
    for t in (0, 1023, 2299, 4999, 2320, 2400, 2500, 3000):
        tod[0, t] += SPIKE
    # row 1: ~10 % exact zeros, an odd count of non-zeros, a spike beside a zero
    tod[1, rng.random(T) < 0.1] = 0.0
    tod[1, 1500] += SPIKE
    tod[1, 1501] = 0.0
    if np.count_nonzero(tod[1]) % 2 == 0:
        tod[1, 1503] = 0.0
    # row 2: all zero (rms NaN)
    tod[2] = 0.0
    # row 3: a constant on the whole row (the rms is of differences), one NaN inside F
    # (median_filter returns zeros: the whole scan exceeds the threshold), spikes in A and F
    tod[3] += 1.0
    tod[3, 700] += SPIKE
    tod[3, 2800] += SPIKE
    tod[3, NAN_AT] = np.nan
    # row 4: +inf and -inf inside F: a pair difference is infinite, the rms NaN, the mask empty
    tod[4, 3000] = np.inf
    tod[4, 3101] = -np.inf
    # row 5: a tile's first sample; two spikes 150 apart (their dilations merge at step 100);
    # one 10 samples before A's end (must not leak into B); a 3-sample run; one 5 samples
    # after G's start (must not leak back into F); the threshold probes in B and C
    for t in (1024, 2900, 3050, 2290, 4200, 4201, 4202, 3705):
        tod[5, t] += SPIKE
    _set_probes(tod[5])
    # row 6: no spike.  Its own draw: about two draws in three have a 4-sigma sample that
    # fires at threshold 4; this one has none (asserted on the oracle below)
    tod[6] = SIGMA * np.random.default_rng(609).standard_normal(T)
    # row 7: first and last sample of every non-empty scan
    for s, e in SCANS.values():
        tod[7, s] += SPIKE
        tod[7, e - 1] -= SPIKE
    return tod.reshape(2, 4, T)


def make_small():
    """T = 300 < one tile: one feed x one band, two scans of 150 (>= w = 100)."""
    rng = np.random.default_rng(77)
    tod = SIGMA * rng.standard_normal((1, 1, 300))
    # two spikes in 150 difference pairs carry the row's rms (0.033): they are 12 rms high;
    # each sits near an edge of its scan, so that part of either scan stays unmasked
    for t in (10, 290):
        tod[0, 0, t] += 0.4
    return tod, np.array([(0, 150), (150, 300)], dtype=np.int64)


def expected_mask(tod, edges, w, step, thr):
    F, B, n = tod.shape
    out = np.zeros((F, B, n), dtype=bool)
    for f in range(F):
        for b in range(B):
            rms = _quiet(ospk.tod_auto_rms, tod[f, b])
            for s, e in edges:
                if e > s:
                    out[f, b, s:e] = _quiet(ospk.fit_spikes, tod[f, b, s:e], rms, w, thr, step)
    return out


def threshold_margin(tod, edges, w, thr):
    """min over finite-rms rows, scans and samples of | |tod - mf| - thr rms | / (thr rms)."""
    worst = np.inf
    for row in tod.reshape(-1, tod.shape[-1]):
        rms = _quiet(ospk.tod_auto_rms, row)
        if not np.isfinite(rms):
            continue
        for s, e in edges:
            if e > s:
                clean = row[s:e] - ospk.median_filter(row[s:e], w)
                worst = min(worst, np.nanmin(np.abs(np.abs(clean) - thr * rms)) / (thr * rms))
    return worst


@pytest.fixture(scope='module')
def main_tod():
    return make_main()


@pytest.fixture(scope='module')
def main_expected(main_tod):
    return {p: expected_mask(main_tod, EDGES, *p) for p in PARAMS}


def _rows(mask):
    return mask.reshape(-1, mask.shape[-1])


# ---------------------------------------------------------------- conditions on the oracle alone
def test_input_is_what_the_cases_need(main_tod):
    rows = _rows(main_tod)
    assert np.count_nonzero(rows[1]) % 2 == 1 and 0.05 < np.mean(rows[1] == 0) < 0.15
    assert rows[1, 1501] == 0 and rows[1, 1500] > 0.04
    assert not rows[2].any()
    rms = [_quiet(ospk.tod_auto_rms, r) for r in rows]
    assert [bool(np.isfinite(x)) for x in rms] == [True, True, False, True, False, True, True, True]
    # the constant of row 3 cancels in the pair differences
    assert 0.5 * SIGMA < rms[3] < 3 * SIGMA
    assert [int(e - s) for s, e in EDGES] == [2300, 50, 99, 100, 0, 1100, 1300]


@pytest.mark.parametrize('p', PARAMS)
def test_no_sample_on_the_threshold(main_tod, p):
    w, step, thr = p
    assert threshold_margin(main_tod, EDGES, w, thr) >= MARGIN


@pytest.mark.parametrize('p', PARAMS)
def test_expected_masks_fire_where_meant(main_expected, p):
    m = _rows(main_expected[p])
    for r in FIRING_ROWS:
        assert m[r].any(), r
    for r in EMPTY_ROWS:
        assert not m[r].any(), r
    assert not m[:, GAP[0]:GAP[1]].any()
    # row 3: the scan with the NaN is masked whole, the other scans are not
    s, e = SCANS['F']
    assert m[3, s:e].all()
    for k in 'ABCDG':
        s, e = SCANS[k]
        assert not m[3, s:e].all(), k
    if p == DEFAULT:
        for r in (0, 7):
            for k, (s, e) in SCANS.items():
                assert m[r, s:e].any(), (r, k)
        # row 5: the spike 10 samples before A's end masks up to A's end and not B (where
        # the probes stay below the threshold); the one after G's start not F's end
        assert m[5, 2190:2300].all() and not m[5, 2300:2449].any()
        assert not m[5, 3600:3700].any() and m[5, 3700:3800].all()
        # two spikes 150 apart: one merged run
        assert m[5, 2900 - 101:3050 + 100].all() and not m[5, 3050 + 100]


def test_expected_mask_feels_the_short_scan_median(main_tod, main_expected, monkeypatch):
    """The probes of row 5 turn a short-scan median that is off by one order statistic
    (odd count) or that takes only one of the two middle values (even count) into a
    different mask, in either direction."""
    orig = ospk.median_filter
    w, step, thr = DEFAULT
    for shift in (-1, 1):
        def perturbed(tod, w, shift=shift):
            if np.isfinite(tod).all() and tod.size < w:
                v = np.sort(tod)
                n = tod.size
                k = n // 2 + shift if n & 1 else (n // 2 - 1 if shift < 0 else n // 2)
                return np.zeros(n) + v[k]
            return orig(tod, w)
        monkeypatch.setattr(ospk, 'median_filter', perturbed)
        got = _rows(expected_mask(main_tod, EDGES, w, step, thr))
        monkeypatch.setattr(ospk, 'median_filter', orig)
        ref = _rows(main_expected[DEFAULT])
        for k in 'BC':
            s, e = SCANS[k]
            assert not np.array_equal(got[5, s:e], ref[5, s:e]), (shift, k)


# ---------------------------------------------------------------- the device
@pytest.mark.parametrize('p', PARAMS)
def test_spike_mask_bit_exact(main_tod, main_expected, p):
    from comapreduce_amd.stages.statistics import spike_mask
    w, step, thr = p
    got = spike_mask(main_tod, EDGES, medfilt_window=w, step=step, threshold=thr).cpu().numpy()
    ref = main_expected[p]
    assert got.shape == ref.shape and got.dtype == np.bool_
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (p, len(bad), bad[:8].tolist())
    inscan = np.zeros(T, dtype=bool)
    for s, e in EDGES:
        inscan[s:e] = True
    assert not got[..., ~inscan].any()


def test_spike_mask_partial_tile():
    """T = 300: a grid of one partial tile."""
    from comapreduce_amd.stages.statistics import spike_mask
    tod, edges = make_small()
    w, step, thr = DEFAULT
    assert threshold_margin(tod, edges, w, thr) >= MARGIN
    ref = expected_mask(tod, edges, w, step, thr)
    assert ref[0, 0, :150].any() and ref[0, 0, 150:].any() and not ref.all()
    got = spike_mask(tod, edges, medfilt_window=w, step=step, threshold=thr).cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8].tolist()


@pytest.mark.parametrize('kw,edges', [
    (dict(medfilt_window=0), [(0, 150), (150, 300)]),
    (dict(medfilt_window=1024), [(0, 150), (150, 300)]),
    (dict(step=0), [(0, 150), (150, 300)]),
    (dict(), [(0, 150), (150, 301)]),       # an edge beyond T
    (dict(), [(0, 150), (200, 150)]),       # e < s
])
def test_spike_mask_abi_refusals(kw, edges):
    from comapreduce_amd import _native as N
    from comapreduce_amd.stages.statistics import spike_mask
    tod, _ = make_small()
    with pytest.raises(N.NativeError):
        spike_mask(tod, np.array(edges, dtype=np.int64), **kw)
