"""The regression without pass C, as an identity in NumPy.

Level1AveragingGainCorrection.median_filter regresses every median channel on
[1, mf] (Level1Averaging.py:701-705).  The per-channel solution x_c reaches the
Level-2 outputs only as sum_c k_c x_c for three channel weightings k, and x_c
is linear in sum_t d_ct mf_t, so those constants follow from the dot of mf with
the per-sample band sum S_K,t = sum_c kappa_c d_ct (kappa = k alpha) that pass B
accumulates anyway.  This test states the device's phase-1 formulas in NumPy on
f32 data like the synthetic generator's and compares them with sum_c k_c x_c
taken from the per-channel np.linalg.solve of oracle.l1.median_filter itself.

What is compared are the band constants the outputs are formed from (k_coef_d's
dsum): -(sum kappa o + sum k x0), -sum kappa a and -sum k x1 per weighting.  The
intercepts x0_c are residual means, ~1e-6 of alpha o, so sum k x0 on its own is
a rounding-level quantity of the constant it enters; it is printed, not bounded.
"""
import numpy as np
import pytest

import oracle.l1 as ol1
from comapreduce_amd import synthetic

C, N = 1024, 12_288            # one band; n >= 2 w so the median filter runs
RTOL = 1e-12


@pytest.fixture(scope='module')
def band():
    """f32 band d[c, t] as synthetic.generate_feed forms it, its airmass, and the
    coefficients the reduction subtracts and scales with (o, a, alpha = 1 / rms)."""
    rng = np.random.default_rng(20241)
    tsys = rng.uniform(35.0, 45.0, C)
    gain = 1e6 * rng.uniform(0.9, 1.1, C)
    _, _, _, el = synthetic.pointing(N, 3)
    A = ol1.airmass(el)
    mult = 1.0 + synthetic.gain_drift(rng, N)
    noise = rng.standard_normal((C, N), dtype=np.float32) * np.float32(synthetic.WHITE_SIGMA)
    sig = (tsys[:, None] + 8.0 * (A - 1.4)[None, :]) * mult[None, :]
    d = (gain[:, None] * sig * (1.0 + noise)).astype(np.float32)
    o, a = ol1.fit_atmosphere(A, d)
    idx = ol1.median_index()
    clean = d[idx].astype(np.float64) - (o[idx, None] + a[idx, None] * A[None, :])
    y, rms = ol1.normalise_data(clean)
    return dict(d=d, A=A, o=o[idx], a=a[idx], alpha=1.0 / rms[:, 0], y=y, idx=idx, tsys=tsys[idx], gain=gain[idx],
                rms=rms[:, 0])


@pytest.fixture(scope='module')
def oracle_solution(band):
    """(x [2, n_idx], mf [n]) of oracle.l1.median_filter's own np.linalg.solve call."""
    full = np.zeros((1, C, N))
    full[0, band['idx']] = band['y']
    seen = []
    solve = np.linalg.solve

    def capture(a, b):
        x = solve(a, b)
        seen.append(x)
        return x
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(np.linalg, 'solve', capture)
        _, mf = ol1.median_filter(full)
    finally:
        mp.undo()
    assert len(seen) == 1 and seen[0].shape == (2, band['idx'].size)
    assert np.isfinite(mf[0]).all()
    return seen[0], mf[0]


def weightings(band):
    """Three channel weightings shaped like the device's: a signed gain-template
    weight, W nf / g and W Tsys with the band-average mask (zeros included)."""
    idx = band['idx']
    v = np.linspace(-1.0, 1.0, C)[idx]
    kg = (1.0 - 0.5 * v) / band['tsys'] / idx.size
    kg[(idx < 20) | (idx >= 1004)] = 0.0
    W = 1.0 / band['tsys'] ** 2
    W[(idx < 50) | (idx >= 974)] = 0.0
    return kg, W * band['rms'] / band['gain'], W * band['tsys']


def fused_constants(band, mf, k):
    """(dsum[3j], dsum[3j+1], dsum[3j+2], sum k x0) the way k_coef_d phase 1 forms them."""
    A, o, a = band['A'], band['o'], band['a']
    d = band['d'][band['idx']].astype(np.float64)
    n = float(N)
    SA = A.sum()
    Smf, Smm, SAm = mf.sum(), mf @ mf, A @ mf
    det = n * Smm - Smf * Smf
    kappa = k * band['alpha']
    live = kappa != 0.0
    S = kappa[live] @ d[live]                       # pass B: per-sample band sum
    P = mf @ S                                      # k_series_sums: the dot
    sko = (kappa * o)[live].sum()
    ska = (kappa * a)[live].sum()
    ksy = (kappa * (d.sum(axis=1) - n * o - a * SA))[live].sum()
    ksym = P - Smf * sko - SAm * ska
    kx0, kx1 = (Smm * ksy - Smf * ksym) / det, (n * ksym - Smf * ksy) / det
    return -(sko + kx0), -ska, -kx1, kx0


def test_band_constants_equal_per_channel_solve(band, oracle_solution):
    x, mf = oracle_solution
    for name, k in zip(('kg', 'kr', 'ko'), weightings(band)):
        assert (k == 0.0).any() and (k != 0.0).any()
        # the per-channel path: fb = -(alpha o + x0), fg = -alpha a, fd = -x1, summed with k
        ref = (-(k @ (band['alpha'] * band['o'] + x[0])), -(k @ (band['alpha'] * band['a'])), -(k @ x[1]))
        got = fused_constants(band, mf, k)
        err = [abs(g - r) / abs(r) for g, r in zip(got, ref)]
        print(f'{name}: constants {ref[0]:.6e} {ref[1]:.6e} {ref[2]:.6e} rel err {err[0]:.2e} {err[1]:.2e} '
              f'{err[2]:.2e}; sum k x0 {k @ x[0]:.3e} vs {got[3]:.3e}')
        assert max(err) < RTOL, (name, err)
