"""
Seeded inputs of the raw_csr golden vectors (tests/golden/raw_csr.npz): small CSR triples, their sidecar
files and mask stacks.  Imported by generate_raw_csr_golden.py (which runs the reference on them) and by
the tests (which run this package on the same inputs); only results and input checksums are stored.
"""
import os

import numpy as np

NAV = (5, 7)
SIG = (9, 13)


def _case(name, dtype='<u2', idx='<i4', sync_offset=0, roi=False, num_partitions=2, n_masks=3,
          mask_dtype='float32', nan=False, seed=0):
    return dict(name=name, dtype=dtype, indptr_dtype=idx, indices_dtype=idx, sync_offset=sync_offset,
                roi=roi, num_partitions=num_partitions, n_masks=n_masks, mask_dtype=mask_dtype, nan=nan,
                seed=seed)


CASES = (
    [_case(f'dtype_{dt.strip("<")}', dtype=dt, idx=('<i4', '<i8')[i % 2], seed=10 + i)
     for i, dt in enumerate(('u1', '<u2', '<i2', '<u4', '<i4', '<f4'))]
    + [_case('sync_p3', sync_offset=3, seed=20),
       _case('sync_p3_roi', sync_offset=3, roi=True, num_partitions=3, idx='<i8', seed=21),
       _case('sync_m4', sync_offset=-4, num_partitions=1, seed=22),
       _case('sync_m4_roi', sync_offset=-4, roi=True, num_partitions=3, seed=23),
       _case('roi', roi=True, num_partitions=1, seed=24),
       _case('parts3', num_partitions=3, idx='<i8', seed=25)]
    + [_case(f'masks_{m}', n_masks=m, seed=30 + m) for m in (1, 16, 17)]
    + [_case('masks_f64', n_masks=3, mask_dtype='float64', seed=40),
       _case('nan_f4', dtype='<f4', nan=True, seed=41)]
)


def make_case(case):
    """-> dict(indptr int64, indices int64, data (the case's dtype, native), masks, roi | None); rows canonical"""
    rng = np.random.default_rng(case['seed'])
    n_nav, n_px = int(np.prod(NAV)), int(np.prod(SIG))
    dt = np.dtype(case['dtype']).newbyteorder('=')
    counts = rng.integers(0, 24, n_nav)
    counts[3] = 0                                           # an empty frame
    counts[n_nav - 1] = n_px                                # every pixel set
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_px, int(c), replace=False)) for c in counts]).astype(np.int64)
    if dt.kind == 'f':
        data = (rng.random(len(indices)) * 8 - 2).astype(dt)
    else:
        lo = -50 if dt.kind == 'i' else 1
        data = rng.integers(lo, 120, len(indices)).astype(dt)
    if case['nan']:
        data[int(indptr[5])] = np.nan                       # a stored NaN in frame 5
    masks = (rng.random((case['n_masks'],) + SIG) - 0.25).astype(case['mask_dtype'])
    masks[0, 0, :4] = 0                                     # weights that are exactly zero
    roi = None
    if case['roi']:
        roi = rng.random(NAV) < 0.6
        roi[0, 0] = roi[-1, -1] = True
    return dict(indptr=indptr, indices=indices, data=data, masks=masks, roi=roi)


def dense_frames(inp):
    """(n_frames, *SIG) of the stored frames (no sync_offset applied)"""
    import scipy.sparse as sp
    n_px = int(np.prod(SIG))
    m = sp.csr_matrix((inp['data'], inp['indices'], inp['indptr']), shape=(len(inp['indptr']) - 1, n_px))
    return m.toarray().reshape((-1,) + SIG)


def write_files(case, inp, dirpath, name='ds', filetype='raw_csr', indptr=None, indices=None, data=None):
    """the sidecar and the three flat files of a case (the arrays can be replaced) -> path of the TOML file"""
    arrays = dict(indptr=(inp['indptr'] if indptr is None else indptr, case['indptr_dtype']),
                  indices=(inp['indices'] if indices is None else indices, case['indices_dtype']),
                  data=(inp['data'] if data is None else data, case['dtype']))
    lines = ['[params]', f'filetype = "{filetype}"', f'nav_shape = [{NAV[0]}, {NAV[1]}]',
             f'sig_shape = [{SIG[0]}, {SIG[1]}]', '', f'[{filetype}]']
    for key, (arr, dt) in arrays.items():
        fn = f'{name}_{key}.bin'
        np.asarray(arr).astype(np.dtype(dt)).tofile(os.path.join(dirpath, fn))
        lines += [f'{key}_file = "{fn}"', f'{key}_dtype = "{dt}"']
    path = os.path.join(dirpath, f'{name}.toml')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return path
