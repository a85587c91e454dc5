"""
Seeded inputs of the golden vectors of RecordUDF, the transposed-data converter and NPYDataSet
(tests/golden/record.npz).  Imported by generate_record_golden.py (which runs the reference's RecordUDF,
ConvertTransposedDatasetUDF and NPYDataSet on them) and by the tests (which run this package on the same arrays and
files); only shapes, dtypes, checksums, image counts and the names of exception classes are stored.

Integer pixel values are <= 4095 and at most a few thousand are summed, so every sum of them is a whole number below
2**24 and exact in float32: the stored checksums of such sums are independent of the order of summation.
"""
import os

import numpy as np

# RecordUDF: a MemoryDataSet of `shape` with `sig_dims` signal dimensions in `num_partitions` partitions
RECORD = [
    dict(name='REC_u16_p2', shape=(5, 7, 9, 13), dtype='<u2', sig_dims=2, num_partitions=2, seed=11),
    dict(name='REC_u16_p3', shape=(5, 7, 9, 13), dtype='<u2', sig_dims=2, num_partitions=3, seed=11),
    dict(name='REC_f4_sig1', shape=(35, 6), dtype='<f4', sig_dims=1, num_partitions=2, seed=12),
]

# the converter: the MemoryDataSet is the (sig, nav) storage, so its nav axes are the S detector pixels and its sig
# axes the N scan positions.  S = 65, N = 42; S = 129, N = 135 (4 partitions do not divide 129; item sizes 1, 4, 8,
# 16); S = 130, N = 33
CONVERT = [
    dict(name='CONV_u16', shape=(5, 13, 6, 7), dtype='<u2', sig_dims=2, num_partitions=2, seed=21),
    dict(name='CONV_u8', shape=(3, 43, 9, 15), dtype='|u1', sig_dims=2, num_partitions=4, seed=22),
    dict(name='CONV_f4', shape=(3, 43, 9, 15), dtype='<f4', sig_dims=2, num_partitions=4, seed=23),
    dict(name='CONV_c8', shape=(3, 43, 9, 15), dtype='<c8', sig_dims=2, num_partitions=4, seed=24),
    dict(name='CONV_c16', shape=(3, 43, 9, 15), dtype='<c16', sig_dims=2, num_partitions=4, seed=25),
    dict(name='CONV_3d', shape=(130, 3, 11), dtype='<u2', sig_dims=2, num_partitions=3, seed=26),
]

# the .npy files that are loaded
NPY_FILES = {
    'u2': dict(shape=(4, 5, 6, 7), dtype='<u2', order='C', seed=31),
    'be': dict(shape=(4, 5, 6, 7), dtype='>u2', order='C', seed=32),
    'f4': dict(shape=(3, 4, 10), dtype='<f4', order='C', seed=33),
    'fortran': dict(shape=(4, 5, 6, 7), dtype='<u2', order='F', seed=34),
}

NPY_ROI = np.zeros((4, 5), dtype=bool)
NPY_ROI[0, 1] = NPY_ROI[1, 4] = NPY_ROI[2, 0] = NPY_ROI[2, 1] = NPY_ROI[3, 3] = NPY_ROI[3, 4] = True

# the loads: `kwargs` go to the dataset class next to `path`; `error`: the load must fail
NPY = [
    dict(name='NPY_plain', file='u2', kwargs=dict(num_partitions=2)),
    dict(name='NPY_be', file='be', kwargs=dict(num_partitions=2)),
    dict(name='NPY_f4_sig1', file='f4', kwargs=dict(sig_dims=1, num_partitions=2)),
    dict(name='NPY_nav', file='u2', kwargs=dict(nav_shape=(3, 4), num_partitions=2)),
    dict(name='NPY_sig', file='u2', kwargs=dict(sig_shape=(3, 14), num_partitions=2)),
    dict(name='NPY_p3_1', file='u2', kwargs=dict(sync_offset=3, num_partitions=1)),
    dict(name='NPY_p3_3', file='u2', kwargs=dict(sync_offset=3, num_partitions=3)),
    dict(name='NPY_m4_1', file='u2', kwargs=dict(sync_offset=-4, num_partitions=1)),
    dict(name='NPY_m4_3', file='u2', kwargs=dict(sync_offset=-4, num_partitions=3)),
    dict(name='NPY_roi', file='u2', kwargs=dict(num_partitions=2), roi=NPY_ROI),
    dict(name='NPY_fortran', file='fortran', kwargs=dict(), error=True),
    dict(name='NPY_mismatch', file='u2', kwargs=dict(sig_shape=(42,), sig_dims=2), error=True),
]


def case(name):
    return next(c for c in RECORD + CONVERT + NPY if c['name'] == name)


def make_data(recipe):
    """the seeded array of a RECORD / CONVERT recipe or of an entry of NPY_FILES, native byte order, C order"""
    rng = np.random.default_rng(recipe['seed'])
    dt = np.dtype(recipe['dtype']).newbyteorder('=')
    shape = tuple(recipe['shape'])
    if dt.kind == 'u':
        return rng.integers(0, 256 if dt.itemsize == 1 else 4096, shape).astype(dt)
    if dt.kind == 'f':
        return (rng.random(shape) * 100 - 30).astype(dt)
    return (rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5)).astype(dt)


def write_npy(key, dirpath):
    """write the file `key` of NPY_FILES -> its path"""
    f = NPY_FILES[key]
    data = make_data(f).astype(np.dtype(f['dtype']))
    if f['order'] == 'F':
        data = np.asfortranarray(data)
    path = os.path.join(str(dirpath), f'{key}.npy')
    np.save(path, data)
    return path
