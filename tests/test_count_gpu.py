"""
Electron counting on the MI355X (Context.make_with('hip')) against its own NumPy branch on the inline executor:
EventCountUDF on uint16 and float32 scans with several tiles per partition, three partitions and a sync offset;
`count_events` writing the same bytes on both executors; the planted events of an `electron_frames` scan given back;
the written dataset loaded as raw_csr on the device and run through ApplyMasksUDF; detector corrections applied by
`run_udf` in front of the UDF.  Counts, indices and values are compared for equality.
"""
import numpy as np
import pytest

import count_ref as cr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAV, SIG = (16, 16), (64, 64)
KEYS = ('indptr', 'indices', 'data')


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def cpu():
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def scan():
    from libertem_amd.utils.generate import electron_frames
    return electron_frames(NAV[0] * NAV[1], SIG, 0.05, 21, xrays=2)


def files(tmp_path, stem):
    out = {}
    for key in KEYS + ('toml',):
        with open(str(tmp_path / f'{stem}.{key}'), 'rb') as f:
            out[key] = f.read()
    return out


@pytest.mark.parametrize('dtype', ('uint16', 'float32'))
@pytest.mark.parametrize('sync_offset', (0, 5, -5))
def test_event_count_udf_vs_numpy_branch(ctx, cpu, scan, dtype, sync_offset):
    from libertem_amd.udf import EventCountUDF
    frames, dark, _ = scan
    data = frames.astype(dtype).reshape(NAV + SIG)
    if dtype == 'float32':
        data = data * np.float32(1.25)
    gain = np.linspace(0.9, 1.1, SIG[0] * SIG[1], dtype=np.float32).reshape(SIG)
    udf = EventCountUDF(10, 1000, dark=dark, gain=gain)
    # a tileshape of 7 frames: several tiles per partition, the last of them ragged
    kw = dict(num_partitions=3, sig_dims=2, sync_offset=sync_offset, tileshape=(7,) + SIG)
    dev = ctx.run_udf(dataset=ctx.load('memory', data=data, **kw), udf=udf)['n_events'].data
    host = cpu.run_udf(dataset=cpu.load('memory', data=data, **kw), udf=udf)['n_events'].data
    assert dev.dtype == np.int32 and dev.shape == NAV
    assert np.array_equal(dev, host) and host.sum() > 500
    empty = np.zeros(NAV[0] * NAV[1], bool)
    if sync_offset > 0:
        empty[-sync_offset:] = True
    elif sync_offset < 0:
        empty[:-sync_offset] = True
    assert np.all(dev.reshape(-1)[empty] == 0)


@pytest.mark.parametrize('values', ('count', 'intensity'))
def test_count_events_writes_the_cpu_executors_bytes(ctx, cpu, scan, tmp_path, values):
    from libertem_amd.udf import count_events
    frames, dark, (indptr, indices) = scan
    data = frames.reshape(NAV + SIG)
    kw = dict(num_partitions=3, sig_dims=2, sync_offset=2)
    on_cpu = count_events(cpu, cpu.load('memory', data=data, **kw), str(tmp_path / 'cpu.toml'), 10, 1000, dark=dark,
                          values=values)
    on_dev = count_events(ctx, ctx.load('memory', data=data, **kw), str(tmp_path / 'dev.toml'), 10, 1000, dark=dark,
                          values=values)
    want = files(tmp_path, 'cpu')
    got = files(tmp_path, 'dev')
    for key in KEYS:
        assert got[key] == want[key], key
    assert got['toml'] == want['toml'].replace(b'cpu.', b'dev.')
    assert on_dev['nnz'] == on_cpu['nnz'] and np.array_equal(on_dev['n_events'], on_cpu['n_events'])
    # position i holds frame i + 2: the planted events of the frames 2 .. 255
    assert np.frombuffer(want['indices'], '<i4').tobytes() == indices[indptr[2]:].tobytes()
    assert np.array_equal(np.frombuffer(want['indptr'], '<i8')[:-2], indptr[2:] - indptr[2])


def test_planted_events_come_back_and_feed_the_mask_kernels(ctx, scan, tmp_path):
    from libertem_amd.udf import count_events
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.common.hiparray import HipArray
    frames, dark, (indptr, indices) = scan
    # (the frames resident in HBM, as the benchmark holds them)
    ds = ctx.load('memory', data=HipArray.from_numpy(frames.reshape(NAV + SIG), 0), num_partitions=3, sig_dims=2)
    path = str(tmp_path / 'planted.toml')
    res = count_events(ctx, ds, path, 10, 1000, dark=dark)
    got = files(tmp_path, 'planted')
    assert got['indptr'] == indptr.astype('<i8').tobytes()
    assert got['indices'] == indices.astype('<i4').tobytes()
    assert got['data'] == b'\x01' * len(indices) and res['nnz'] == len(indices) > 500
    counted = ctx.load('raw_csr', path=path)
    assert tuple(counted.shape) == NAV + SIG and counted.dtype == np.uint8
    rng = np.random.default_rng(3)
    masks = (rng.random((2,) + SIG) - 0.3).astype(np.float32)
    udf = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=2, mask_dtype=np.float32)
    sparse = ctx.run_udf(dataset=counted, udf=udf)['intensity'].data
    kernels = [h.last_kernel() for h in udf.masks._handle_cache.values()]
    assert kernels and all(k.startswith('k_apply_csr<') for k in kernels), kernels
    images = cr.dense_event_images(indptr, indices, np.ones(len(indices), np.uint8), SIG)
    dense_ds = ctx.load('memory', data=images.reshape(NAV + SIG), num_partitions=3, sig_dims=2)
    udf2 = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=2, mask_dtype=np.float32)
    dense = ctx.run_udf(dataset=dense_ds, udf=udf2)['intensity'].data
    x = images.reshape((len(images), -1)).astype(np.float64)
    w = masks.reshape((2, -1)).astype(np.float64)
    bound = (1e-5 * (np.abs(x) @ np.abs(w).T)).reshape(NAV + (2,))   # the bound of tests/test_raw_csr_gpu.py
    assert sparse.shape == dense.shape == NAV + (2,)
    assert np.all(np.abs(sparse.astype(np.float64) - dense) <= bound)
    assert np.all(np.abs(sparse - (x @ w.T).reshape(NAV + (2,))) <= bound)


def test_corrections_in_front_of_the_udf(ctx, scan):
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf import EventCountUDF
    frames, dark, (indptr, _) = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=3, sig_dims=2)
    got = ctx.run_udf(dataset=ds, udf=EventCountUDF(10, 1000), corrections=CorrectionSet(dark=dark))['n_events'].data
    assert got.dtype == np.int32 and got.shape == NAV
    # (the corrected tiles are float32(float64(pixel) - dark): exact for these values, but nothing is claimed for
    #  the fused path in general)
    assert got.sum() > 500


def test_errors_on_device(ctx, scan):
    from libertem_amd.udf import EventCountUDF
    frames, dark, _ = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='dark of shape'):
        ctx.run_udf(dataset=ds, udf=EventCountUDF(10, dark=dark[:5]))
    ds64 = ctx.load('memory', data=frames.reshape(NAV + SIG).astype(np.float64), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='float64'):
        ctx.run_udf(dataset=ds64, udf=EventCountUDF(10))
