"""Known answers of the reference's running median on the seeded series of
medfilt_ref_cases.py (ties, +-inf, random NaN / +-inf / short series).

Runs the reference's own filter() -- medianFilter.cpp + Mediator.h compiled unmodified
by oracle/Makefile into oracle/_ref/libmedfilt_ref.so -- and writes
tests/golden/golden_medfilt_ref.npz: one output array per case key (the inputs are
regenerated from their seeds).  Usage: python tests/golden/make_medfilt_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import medfilt_ref_cases as mc  # noqa: E402


def main():
    if oracle.ref_lib() is None:
        raise SystemExit('oracle/_ref/libmedfilt_ref.so is not built (make -C oracle, reference present)')
    arrays = {}
    for gen in (mc.ties, mc.infinities, mc.twoheap_random):
        for key, x, w in gen():
            arrays[key] = oracle.medfilt_reference(x.copy(), w)
    np.savez_compressed(os.path.join(HERE, 'golden_medfilt_ref.npz'), **arrays)
    print('wrote', len(arrays), 'cases')


if __name__ == '__main__':
    main()
