"""Seeded inputs of the FEMUDF / LogsumUDF golden cases (tests/golden/framestats.npz,
generate_framestats_golden.py)."""
import numpy as np

FEM_CASES = [
    dict(name='fem_u16', nav=(6, 7), sig=(24, 24), dtype='uint16', num_partitions=3, seed=1001,
         center=(12, 12), rad_in=3, rad_out=9),
    dict(name='fem_i32', nav=(5, 6), sig=(20, 20), dtype='int32', num_partitions=3, seed=1002,
         center=(10, 9), rad_in=2, rad_out=8),
    dict(name='fem_f32', nav=(6, 5), sig=(24, 24), dtype='float32', num_partitions=3, seed=1003,
         center=(11.5, 12.25), rad_in=4.5, rad_out=10.),
    dict(name='fem_c64', nav=(4, 6), sig=(16, 16), dtype='complex64', num_partitions=3, seed=1004,
         center=(8, 8), rad_in=2, rad_out=6),
    # non-square frame, off-centre float center: center[0] is the row
    dict(name='fem_nonsquare', nav=(5, 5), sig=(18, 30), dtype='float32', num_partitions=2, seed=1005,
         center=(5.3, 20.7), rad_in=2.5, rad_out=7.2),
    dict(name='fem_partly_outside', nav=(5, 6), sig=(20, 20), dtype='uint16', num_partitions=2, seed=1006,
         center=(2, 17), rad_in=3, rad_out=9),
    dict(name='fem_rad_in0', nav=(5, 6), sig=(16, 16), dtype='uint16', num_partitions=2, seed=1007,
         center=(8, 8), rad_in=0, rad_out=5),
    dict(name='fem_empty', nav=(4, 5), sig=(16, 16), dtype='float32', num_partitions=2, seed=1008,
         center=(8, 8), rad_in=6, rad_out=4),
    dict(name='fem_nan', nav=(5, 6), sig=(20, 20), dtype='float32', num_partitions=2, seed=1009,
         center=(10, 10), rad_in=2, rad_out=6, nan=True),
    dict(name='fem_roi', nav=(8, 6), sig=(16, 16), dtype='float32', num_partitions=3, seed=1010,
         center=(8, 7), rad_in=2, rad_out=7, roi_seed=21),
    dict(name='fem_sync_p3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1011,
         center=(8, 8), rad_in=2, rad_out=6, sync_offset=3),
    dict(name='fem_sync_m3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1011,
         center=(8, 8), rad_in=2, rad_out=6, sync_offset=-3),
    dict(name='fem_parts1', nav=(7, 7), sig=(16, 16), dtype='float32', num_partitions=1, seed=1012,
         center=(8, 8), rad_in=3, rad_out=7),
    dict(name='fem_parts7', nav=(7, 7), sig=(16, 16), dtype='float32', num_partitions=7, seed=1012,
         center=(8, 8), rad_in=3, rad_out=7),
    dict(name='fem_corrections', nav=(5, 6), sig=(16, 16), dtype='float32', num_partitions=2, seed=1013,
         center=(8, 8), rad_in=2, rad_out=7, corrections=True),
]

LOGSUM_CASES = [
    dict(name='log_u8_full', nav=(6, 7), sig=(16, 17), dtype='uint8', num_partitions=3, seed=1101, full=True),
    dict(name='log_i8_full', nav=(6, 7), sig=(16, 17), dtype='int8', num_partitions=3, seed=1102, full=True),
    dict(name='log_u16_full', nav=(5, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1103, full=True),
    dict(name='log_i16', nav=(5, 6), sig=(16, 16), dtype='int16', num_partitions=3, seed=1104),
    dict(name='log_i32', nav=(5, 6), sig=(12, 13), dtype='int32', num_partitions=3, seed=1105),
    dict(name='log_f32_neg', nav=(6, 5), sig=(16, 19), dtype='float32', num_partitions=3, seed=1106),
    dict(name='log_f64', nav=(4, 5), sig=(9, 12), dtype='float64', num_partitions=2, seed=1107),
    dict(name='log_nan', nav=(5, 6), sig=(16, 16), dtype='float32', num_partitions=2, seed=1108, nan=True),
    dict(name='log_roi', nav=(8, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1109, roi_seed=23),
    dict(name='log_sync_p3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1110,
         sync_offset=3),
    dict(name='log_sync_m3', nav=(6, 6), sig=(16, 16), dtype='uint16', num_partitions=3, seed=1110,
         sync_offset=-3),
    dict(name='log_corrections', nav=(5, 6), sig=(16, 16), dtype='float32', num_partitions=2, seed=1111,
         corrections=True),
    dict(name='log_parts1', nav=(7, 7), sig=(12, 12), dtype='float32', num_partitions=1, seed=1112),
    dict(name='log_parts7', nav=(7, 7), sig=(12, 12), dtype='float32', num_partitions=7, seed=1112),
]


def make_case(case):
    """-> (data, roi or None, (dark, gain) or None)"""
    rng = np.random.default_rng(case['seed'])
    shape = tuple(case['nav']) + tuple(case['sig'])
    dt = np.dtype(case['dtype'])
    if dt.kind in 'ui' and case.get('full'):
        info = np.iinfo(dt)
        data = rng.integers(int(info.min), int(info.max) + 1, shape, endpoint=False).astype(dt)
        # every frame holds both ends of the range: native integer arithmetic would wrap
        flat = data.reshape((-1,) + tuple(case['sig']))
        flat[:, 0, 0] = info.min
        flat[:, -1, -1] = info.max
    elif dt.kind == 'u':
        data = rng.integers(0, 4000, shape).astype(dt)
    elif dt.kind == 'i':
        lim = 30000 if dt.itemsize == 2 else 70000
        data = rng.integers(-lim, lim, shape).astype(dt)
    elif dt.kind == 'c':
        data = (rng.normal(3., 1., shape) + 1j * rng.normal(-1., 2., shape)).astype(dt)
    else:
        data = (rng.normal(-20., 50., shape)).astype(dt)
    if case.get('nan'):
        flat = data.reshape((-1,) + tuple(case['sig']))
        flat[1, 0, 0] = np.nan                                  # outside any ring of the cases
        if 'center' in case:
            cy, cx = int(case['center'][0]), int(case['center'][1])
            flat[3, cy + int(case['rad_in']) + 1, cx] = np.nan  # inside the ring
            flat[4, cy + int(case['rad_in']) + 1, cx] = np.inf  # inside the ring
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
