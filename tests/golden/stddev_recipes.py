"""Seeded inputs of the StdDevUDF golden cases (tests/golden/stddev.npz, generate_stddev_golden.py)."""
import numpy as np

STDDEV_CASES = [
    dict(name='u16', nav=(6, 7), sig=(16, 17), dtype='uint16', num_partitions=3, seed=901),
    dict(name='i32', nav=(5, 6), sig=(12, 13), dtype='int32', num_partitions=3, seed=902),
    dict(name='f32', nav=(6, 5), sig=(16, 19), dtype='float32', num_partitions=3, seed=903),
    dict(name='c64', nav=(4, 6), sig=(10, 11), dtype='complex64', num_partitions=3, seed=904),
    dict(name='c128', nav=(4, 5), sig=(9, 12), dtype='complex128', num_partitions=2, seed=905),
    dict(name='u16_base_f32', nav=(6, 7), sig=(16, 17), dtype='uint16', num_partitions=3, seed=906,
         udf_kwargs=dict(dtype='float32')),
    dict(name='f32_roi', nav=(8, 6), sig=(16, 16), dtype='float32', num_partitions=3, seed=907,
         roi_seed=17),
    dict(name='u16_partial_width', nav=(5, 6), sig=(16, 20), dtype='uint16', num_partitions=2, seed=908,
         tileshape=(4, 6, 7)),
    dict(name='f32_parts1', nav=(7, 7), sig=(12, 12), dtype='float32', num_partitions=1, seed=909),
    dict(name='f32_parts7', nav=(7, 7), sig=(12, 12), dtype='float32', num_partitions=7, seed=909),
    dict(name='u16_sync_p3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=910,
         sync_offset=3),
    dict(name='u16_sync_m3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=910,
         sync_offset=-3),
    dict(name='f32_corrections', nav=(5, 6), sig=(16, 16), dtype='float32', num_partitions=2, seed=911,
         corrections=True),
]


def make_stddev_case(case):
    """-> (data, roi or None, (dark, gain) or None)"""
    rng = np.random.default_rng(case['seed'])
    shape = tuple(case['nav']) + tuple(case['sig'])
    dt = np.dtype(case['dtype'])
    if dt.kind == 'u':
        data = rng.integers(0, 4000, shape).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(-70000, 70000, shape).astype(dt)
    elif dt.kind == 'c':
        data = (rng.normal(3., 1., shape) + 1j * rng.normal(-1., 2., shape)).astype(dt)
    else:
        data = (100. + rng.normal(0., 5., shape)).astype(dt)
    roi = None
    if 'roi_seed' in case:
        roi = np.random.default_rng(case['roi_seed']).random(tuple(case['nav'])) > 0.4
    corr = None
    if case.get('corrections'):
        sig = tuple(case['sig'])
        dark = rng.normal(2., 0.5, sig).astype(np.float32)
        gain = rng.uniform(0.8, 1.2, sig).astype(np.float32)
        corr = (dark, gain)
    return data, roi, corr
