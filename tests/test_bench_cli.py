"""bench.py's command line and --dump-outputs writer (host arrays; no GPU)."""
import os
import sys

import numpy as np
import pytest


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'somewhere')
    assert a.full is True and a.dump_outputs == 'somewhere'
    with pytest.raises(SystemExit):
        _parse(monkeypatch, '--steps', '0')


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    from comapreduce_amd.pipeline.datahandling import COMAPLevel2
    rng = np.random.default_rng(5)
    n_big = bench.DUMP_WHOLE_BYTES // 8 + bench.DUMP_SAMPLE          # above the whole-array limit
    level2 = COMAPLevel2(filename='/nonexistent/level2.hd5')
    level2['vane/system_temperature'] = rng.standard_normal((2, 3, 4))
    level2['averaged_tod/tod'] = rng.standard_normal(n_big).astype(np.float32).reshape(2, -1)
    level2['averaged_tod/weights'] = rng.standard_normal(n_big).reshape(2, -1)
    level2['averaged_tod/scan_edges'] = np.array([[0, 10], [12, 40]], dtype=np.int64)
    level2['averaged_tod/absent'] = None
    level2['averaged_tod/frequency_power_spectra'] = np.zeros((2, 3, 4, 15, 2))     # placeholder, not computed
    out = [tmp_path / 'a', tmp_path / 'b']
    for d in out:
        bench.dump_outputs(level2, str(d))
    names = sorted(os.listdir(out[0]))
    assert names == ['averaged_tod__scan_edges.npy', 'averaged_tod__tod.npy', 'averaged_tod__weights.npy',
                     'vane__system_temperature.npy']
    got = {n: np.load(out[0] / n) for n in names}
    for n in names:                                                   # the same bytes from run to run
        assert np.array_equal(got[n], np.load(out[1] / n))
    assert np.array_equal(got['vane__system_temperature.npy'], level2['vane/system_temperature'])
    edges = got['averaged_tod__scan_edges.npy']
    assert edges.dtype == np.float64 and np.array_equal(edges, level2['averaged_tod/scan_edges'])
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n_big, bench.DUMP_SAMPLE, replace=False))
    tod, w = got['averaged_tod__tod.npy'], got['averaged_tod__weights.npy']
    assert tod.dtype == np.float32 and w.dtype == np.float64
    assert np.array_equal(tod, level2['averaged_tod/tod'].reshape(-1)[idx])
    assert np.array_equal(w, level2['averaged_tod/weights'].reshape(-1)[idx])
    assert sum(a.nbytes for a in got.values()) <= 64 << 20


def test_dump_outputs_writes_finite_files(tmp_path):
    """NaN / +-inf elements (channels without a fit) are written as 0 and their positions as
    a code array beside the dataset; datasets without any get no such file."""
    import bench
    from comapreduce_amd.pipeline.datahandling import COMAPLevel2
    fit = np.random.default_rng(9).standard_normal((3, 2, 4, 16, 2))
    fit[:, :, :, :2] = np.nan
    fit[1, 0, 2, 5, 0] = np.inf
    fit[2, 1, 3, 7, 1] = -np.inf
    level2 = COMAPLevel2(filename='/nonexistent/level2.hd5')
    level2['atmosphere/fit_values'] = fit
    level2['vane/system_gain'] = np.ones((1, 2, 4, 16), np.float32)
    bench.dump_outputs(level2, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['atmosphere__fit_values.npy', 'atmosphere__fit_values__nonfinite.npy',
                                            'vane__system_gain.npy']
    val, code = np.load(tmp_path / 'atmosphere__fit_values.npy'), np.load(tmp_path / 'atmosphere__fit_values__nonfinite.npy')
    assert val.dtype == np.float64 and code.dtype == np.float32 and val.shape == code.shape == fit.shape
    assert np.isfinite(val).all()
    fin = np.isfinite(fit)
    assert np.array_equal(code == 0, fin) and np.array_equal(val[fin], fit[fin]) and not val[~fin].any()
    assert np.array_equal(code == 1, np.isnan(fit))
    assert code[1, 0, 2, 5, 0] == 2 and code[2, 1, 3, 7, 1] == 3
