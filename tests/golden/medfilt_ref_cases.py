"""Seeded inputs of the running-median comparisons against the reference's compiled
filter(), shared by tests/test_oracle_golden.py and tests/golden/make_medfilt_ref.py
(which stores the reference's answers in golden_medfilt_ref.npz).  Each generator
yields (key, x, w); the draws and their order are part of the fixture."""
import numpy as np


def ties():
    """Rounded normal series (many ties), even and odd windows."""
    rng = np.random.default_rng(5)
    for n, w in [(3000, 6), (2500, 401), (1000, 3), (7000, 2000)]:
        yield f'ties_{n}_{w}', np.round(rng.standard_normal(n), 1), w


def infinities():
    """+-inf samples: scattered, a run making window medians +inf, a run whose windows'
    middle pair is -inf / +inf."""
    rng = np.random.default_rng(31)
    for n, w in [(5000, 400), (4000, 401), (3000, 6), (9000, 6000), (2000, 1)]:
        x = np.round(rng.standard_normal(n), 1)
        x[rng.random(n) < 0.03] = np.inf
        x[rng.random(n) < 0.03] = -np.inf
        a = n // 3
        x[a:a + 300] = np.inf
        x[a + 300:a + 600] = -np.inf
        yield f'inf_{n}_{w}', x, w


def twoheap_random():
    """Random NaN / +-inf / n < w series."""
    rng = np.random.default_rng(77)
    for i in range(150):
        n = int(rng.integers(1, 2500))
        w = int(rng.integers(1, 700))
        if n < w // 2 + w % 2:
            continue
        x = np.round(rng.standard_normal(n), 1)
        x[rng.random(n) < rng.choice([0.0, 0.01, 0.2])] = np.nan
        x[rng.random(n) < 0.01] = rng.choice([np.inf, -np.inf])
        yield f'rand{i:03d}_{n}_{w}', x, w
