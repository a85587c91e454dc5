#!/usr/bin/env python
"""
Generate tests/golden/holo_frames.npz with the REAL Python reference's `libertem.utils.generate.hologram_frame`
(LiberTEM, /root/reference/src), through the same third-party stand-ins as generate_golden.py
(`tests/golden/refshim/`).  The inputs are fixed here and stored next to the results: amplitude and phase of
(12, 16), the default parameters, every deterministic parameter set to another value, and the `gaussian_noise` blur
(scipy).  The Poisson path draws from NumPy's global generator and is not stored: tests/test_holo_cpu.py checks it
against the formula under `np.random.seed`.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_holo_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'

if not os.path.isdir(REF):
    print("reference not present, nothing to do")
    sys.exit(0)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'refshim'))

import numpy as np  # noqa: E402

from libertem.utils.generate import hologram_frame  # noqa: E402

SHAPE = (12, 16)
PARAMS = dict(counts=250., sampling=3.5, visibility=0.6, f_angle=-50.)
GAUSS = dict(counts=1000., sampling=4., gaussian_noise=1.5)


def main():
    rng = np.random.default_rng(20081016)
    yy, xx = np.mgrid[:SHAPE[0], :SHAPE[1]]
    amp = 0.5 + 0.5 * rng.random(SHAPE)
    phi = 2 * np.pi * (yy / SHAPE[0] - 0.5 * xx / SHAPE[1]) + rng.normal(0., 0.2, SHAPE)
    out = {
        'amp': amp, 'phi': phi,
        'default': hologram_frame(amp, phi),
        'params': hologram_frame(amp, phi, **PARAMS),
        'gauss': hologram_frame(amp, phi, **GAUSS),
        'params__kwargs': np.array([PARAMS[k] for k in ('counts', 'sampling', 'visibility', 'f_angle')]),
        'gauss__kwargs': np.array([GAUSS[k] for k in ('counts', 'sampling', 'gaussian_noise')]),
    }
    path = os.path.join(HERE, 'holo_frames.npz')
    np.savez_compressed(path, **out)
    print({k: (v.dtype.str, v.shape) for k, v in out.items()})
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
