"""The residual pass's lane-tree summation order as NumPy states it (destriper.lane_tree_sum)
against a hand-written 64-lane loop, its distance from the exact sum, and the driver's new options:
the [Inputs] keys and the refusal of residuals together with the ground template.  No GPU."""
import math

import numpy as np
import pytest

from comapreduce_amd.mapmaking.destriper import lane_tree_sum

SIZES = (0, 1, 63, 64, 65, 250, 1000)


def by_lanes(v):
    """The order, lane by lane: lane l adds v[l], v[l + 64], ... from +0.0; then a[l] += a[l ^ s]
    for s = 32 .. 1 (every lane at once, from the values before the step); lane 0's result."""
    a = [0.0] * 64
    for lane in range(64):
        for i in range(lane, len(v), 64):
            a[lane] = a[lane] + float(v[i])
    for s in (32, 16, 8, 4, 2, 1):
        a = [a[lane] + a[lane ^ s] for lane in range(64)]
    return a[0]


@pytest.mark.parametrize('n', SIZES)
def test_lane_tree_sum_is_the_lane_loop(n):
    rng = np.random.default_rng(n)
    for v in (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n), rng.random(n)):
        got = lane_tree_sum(v)
        assert isinstance(got, float)
        assert np.float64(got).tobytes() == np.float64(by_lanes(v)).tobytes()
    assert lane_tree_sum(np.zeros(n)) == 0.0 and not np.signbit(lane_tree_sum(np.zeros(n)))


@pytest.mark.parametrize('n', SIZES)
def test_lane_tree_sum_is_close_to_the_exact_sum(n):
    """Non-negative terms: every partial sum is at most the total, and a term passes through at
    most ceil(n / 64) + 5 additions, which is <= n from n = 7 on, so the error is within n 2^-53
    of the total there; the smaller sizes here (0 and 1) are exact."""
    v = np.random.default_rng(100 + n).random(n) ** 4 * 1e3
    exact = math.fsum(v)
    assert abs(lane_tree_sum(v) - exact) <= n * 2.0 ** -53 * exact


def test_nan_and_inf_are_not_hidden():
    v = np.ones(100)
    v[70] = np.nan
    assert np.isnan(lane_tree_sum(v))
    v[70] = np.inf
    assert lane_tree_sum(v) == np.inf


def test_main_refuses_residuals_with_ground_before_reading(tmp_path):
    from comapreduce_amd.mapmaking.run_destriper import main
    missing = str(tmp_path / 'no_such_filelist.txt')
    for kw in (dict(residuals=True), dict(residual_cut=5.0)):
        with pytest.raises(NotImplementedError):
            main(missing, ground=True, device=0, **kw)


def test_ini_keys(tmp_path):
    from comapreduce_amd.mapmaking.run_destriper import residual_params
    from comapreduce_amd.tools.parser import Parser

    def parse(lines):
        f = tmp_path / 'p.ini'
        f.write_text('[Inputs]\nprefix : fg9\n' + lines)
        return residual_params(Parser(str(f))['Inputs'])

    assert parse('') == (False, None)                                   # existing files: off
    assert parse('residual_chi2 : True\n') == (True, None)
    assert parse('residual_chi2 : False\nresidual_cut : None\n') == (False, None)
    assert parse('residual_cut : 5\n') == (False, 5.0)
    assert parse('residual_chi2 = True\nresidual_cut = 2.5  # per (observation, feed)\n') == (True, 2.5)
    for bad in ('residual_cut : yes\n', 'residual_cut : 1, 2\n', 'residual_chi2 : 3\n', 'residual_cut : True\n'):
        with pytest.raises(ValueError):
            parse(bad)
