"""
RawCSRDataSet: frames stored sparse, in compressed sparse row format (`ctx.load("raw_csr", path=...)`,
reference io/dataset/raw_csr.py:105-346).  A TOML sidecar names three flat files -- `indptr`, `indices`
(flat pixel numbers) and `data` -- of a CSR matrix whose rows are the flattened frames; event-counting
detectors write it.  Same parameters, sidecar layout and errors as the reference; what differs is where the
frames live: the reference maps the three files and hands scipy.sparse tiles to the UDFs
(raw_csr.py:481-648); here `initialize()` uploads this process's part of the triple ONCE, checks it on the
device (`ltmi_csr_check`) and keeps it in HBM.  Tiles are `HipCSRArray` views of it: `ApplyMasksUDF` multiplies
the stored entries in place (`ltmi_apply_masks_csr`), `SumSigUDF` and `SumUDF` sum them in place
(`ltmi_csr_sum_sig`, `ltmi_csr_sum_frames`), every other UDF is handed the frames densified into one window of HBM
that the tiles of a partition share (`ltmi_csr_densify`).

On a CPU executor the tiles are slices of the memory-mapped triple, densified on the host: a convenience
for NumPy UDFs, not a hot path.
"""
import os

import numpy as np

from libertem_amd.common.math import prod
from libertem_amd.common.shape import Shape
from libertem_amd.common.slice import Slice
from libertem_amd.common.hiparray import HipArray, HipCSRArray, torch_dtype_for
from .base import DataSetException, DataSetMeta, DataTile
from .memory import MemoryDataSet, MemPartition


class TOMLError(Exception):
    """a sidecar that is not valid TOML (reference raw_csr.py:27-47)"""


def load_toml(path):
    try:
        import tomllib as toml
    except ImportError:
        import tomli as toml
    try:
        with open(path, "rb") as f:
            return toml.load(f)
    except toml.TOMLDecodeError as e:
        msg = str(e)
    raise TOMLError(msg)


#: dtypes the three files may carry (little-endian)
INDEX_DTYPES = tuple(np.dtype(t) for t in ('<i4', '<u4', '<i8', '<u8'))
DATA_DTYPES = tuple(np.dtype(t) for t in ('u1', '<u2', '<i2', '<u4', '<i4', '<f4'))


def _checked_dtype(name, what, allowed):
    try:
        dt = np.dtype(name)
    except TypeError:
        raise DataSetException(f"{what} dtype {name!r} is not a dtype")
    if dt not in allowed:
        raise DataSetException(
            f"{what} dtype {name!r} is not supported: one of {[d.str for d in allowed]}")
    return dt


def get_descriptor(path):
    """file names and dtypes from the sidecar (reference raw_csr.py:445-466)"""
    conf = load_toml(path)
    if conf['params']['filetype'].lower() != 'raw_csr':
        raise ValueError(f"Filetype is not CSR, found {conf['params']['filetype']}")
    base_path = os.path.dirname(path)
    csr_conf = conf[conf['params']['filetype']]
    return {
        'indptr_file': os.path.join(base_path, csr_conf['indptr_file']),
        'indptr_dtype': _checked_dtype(csr_conf['indptr_dtype'], 'indptr', INDEX_DTYPES),
        'indices_file': os.path.join(base_path, csr_conf['indices_file']),
        'indices_dtype': _checked_dtype(csr_conf['indices_dtype'], 'indices', INDEX_DTYPES),
        'data_file': os.path.join(base_path, csr_conf['data_file']),
        'data_dtype': _checked_dtype(csr_conf['data_dtype'], 'data', DATA_DTYPES),
    }


def get_triple(descriptor):
    """(indptr, indices, data) memory-mapped (reference raw_csr.py:410-431)"""
    def mapped(key):
        fn = descriptor[f'{key}_file']
        if os.path.getsize(fn) == 0:                  # (an empty file cannot be mapped)
            return np.zeros(0, dtype=descriptor[f'{key}_dtype'])
        return np.memmap(fn, dtype=descriptor[f'{key}_dtype'], mode='r')
    return mapped('indptr'), mapped('indices'), mapped('data')


def get_nav_size(descriptor):
    return os.path.getsize(descriptor['indptr_file']) // descriptor['indptr_dtype'].itemsize - 1


class _NoDenseFrames(HipArray):
    """What a device-resident raw_csr dataset gives MemoryDataSet as its array: the shape, dtype and device of the
    frames and no memory -- every way to their bytes raises instead of handing out a pointer."""
    __slots__ = ('_device',)

    def __init__(self, shape, dtype, device):
        super().__init__(None, shape, dtype)
        self._device = int(device)

    @property
    def device(self):
        return self._device

    def _refuse(self, *args, **kwargs):
        raise DataSetException("a raw_csr dataset has no dense array of its frames: run UDFs over it")

    data_ptr = rows = reshape = cpu = _refuse
    torch = property(_refuse)


class RawCSRDataSet(MemoryDataSet):
    """
    Parameters (reference raw_csr.py:138-166)
    ----------
    path : str
        the TOML file:

            [params]
            filetype = "raw_csr"
            nav_shape = [512, 512]
            sig_shape = [516, 516]

            [raw_csr]
            indptr_file = "rowind.dat"
            indptr_dtype = "<i4"
            indices_file = "coords.dat"
            indices_dtype = "<i4"
            data_file = "values.dat"
            data_dtype = "<i4"

    nav_shape, sig_shape : tuple of int, optional
        override the sidecar's (sig_shape: the same number of pixels)
    sync_offset : int
        > 0: frames to skip at the start; < 0: blank frames inserted at the start
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: upload and hold only this rank's block of the first nav axis
    """
    #: bytes of the triple this process may keep in HBM (None: what is free)
    MAX_RESIDENT_BYTES = None
    #: dense frames a tile may stand for: the window of HBM that `HipCSRArray.materialize()` fills
    DENSE_WINDOW_BYTES = 2 << 30

    def __init__(self, path, nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None,
                 num_partitions=None, shard=None):
        if io_backend is not None:
            raise NotImplementedError("alternative I/O backends are not part of this build")
        self._path = str(path)
        self._nav_arg = tuple(nav_shape) if nav_shape is not None else None
        self._sig_arg = tuple(sig_shape) if sig_shape is not None else None
        self._sync_offset_arg = int(sync_offset)
        self._num_partitions_arg = num_partitions
        self._shard_arg = shard
        self._conf = None
        self._descriptor = None
        self._image_count = None
        self._csr = None                   # device: dict(indptr, indices, values) of this rank's rows
        self._window = None
        self.canonicalised = False         # the files held unsorted rows or duplicates

    # --- the triple ---------------------------------------------------------------------------------
    def _local_triple(self, p0, p1, so):
        """scan positions [p0, p1) -> (indptr int64 rebased to 0, slice of the stored entries); positions
        without a frame become empty rows"""
        indptr_f, _, _ = self._triple
        g0 = min(max(p0 + so, 0), self._image_count)
        g1 = min(max(p1 + so, g0), self._image_count)
        lead = min(p1 - p0, max(0, g0 - (p0 + so)))
        stored = np.asarray(indptr_f[g0:g1 + 1]).astype(np.int64)
        if len(stored) and (np.any(np.diff(stored) < 0) or stored[0] < 0 or stored[-1] > self._nnz_file):
            raise DataSetException(f"{self._descriptor['indptr_file']}: indptr is not a non-decreasing "
                                   f"sequence inside [0, {self._nnz_file}]")
        indptr = np.zeros(p1 - p0 + 1, dtype=np.int64)
        n_src = g1 - g0
        if n_src > 0:
            indptr[lead:lead + n_src + 1] = stored - stored[0]
            indptr[lead + n_src + 1:] = indptr[lead + n_src]
            lo, hi = int(stored[0]), int(stored[-1])
        else:
            lo = hi = 0
        return indptr, lo, hi

    def _indices32(self, indices, n_px):
        """stored pixel numbers as int32; anything outside [0, n_px) cannot be represented and is refused"""
        if indices.dtype == np.dtype('int32'):
            return np.ascontiguousarray(indices)             # (checked on the device)
        if len(indices) and (int(indices.min()) < 0 or int(indices.max()) >= n_px):
            raise DataSetException(
                f"{self._descriptor['indices_file']}: pixel index outside [0, {n_px}) "
                f"(min {int(indices.min())}, max {int(indices.max())})")
        return np.ascontiguousarray(indices, dtype=np.int32)

    def _upload(self, device, executor, p0, p1, so, n_px):
        import torch
        from libertem_amd import hip
        if getattr(executor, '_make_current', None) is not None:
            executor._make_current()
        _, indices_f, data_f = self._triple
        indptr, lo, hi = self._local_triple(p0, p1, so)
        nnz = hi - lo
        dtype = np.dtype(self._descriptor['data_dtype']).newbyteorder('=')
        # (the triple, and the window of dense frames that the first UDF without a sparse kernel allocates)
        window = min(self.DENSE_WINDOW_BYTES, (p1 - p0) * n_px * dtype.itemsize)
        need = indptr.nbytes + nnz * (4 + dtype.itemsize) + window
        free_bytes, _ = torch.cuda.mem_get_info(device)
        limit = free_bytes if self.MAX_RESIDENT_BYTES is None else min(free_bytes, self.MAX_RESIDENT_BYTES)
        if need > limit:
            raise DataSetException(
                f"{p1 - p0} sparse frames with {nnz} stored entries need {need / 2**30:.1f} GiB of HBM "
                f"({window / 2**30:.1f} GiB of it for densified tiles), "
                f"{limit / 2**30:.1f} GiB are free on GPU {device}: a part of the scan "
                "(nav_shape + sync_offset) or a shard per GPU (shard=(rank, world))")
        indices = self._indices32(np.asarray(indices_f[lo:hi]), n_px)
        values = np.ascontiguousarray(np.asarray(data_f[lo:hi]).astype(dtype, copy=False))

        def to_device(indptr, indices, values):
            dev = f'cuda:{device}'
            vt = HipArray.from_numpy(values, device)._t if len(values) else \
                torch.empty(0, dtype=torch_dtype_for(dtype), device=dev)
            return dict(indptr=torch.from_numpy(indptr).to(dev),
                        indices=torch.from_numpy(indices).to(dev) if len(indices) else
                        torch.empty(0, dtype=torch.int32, device=dev), values=vt)

        def flags_of(csr):
            return hip.csr_check(device, csr['indptr'].data_ptr(), csr['indices'].data_ptr(), p1 - p0, n_px,
                                 nnz_now)

        nnz_now = nnz
        csr = to_device(indptr, indices, values)
        flags = flags_of(csr)
        if flags & 1:
            raise DataSetException(
                f"{self._path}: the CSR data cannot be used: a pixel index outside [0, {n_px}) or an indptr "
                "that does not describe the stored entries")
        if flags & 2:
            # rows that are merely unsorted or hold a pixel twice: canonical form on the host, once
            import scipy.sparse as sp
            # (copies: the arrays may be read-only views of the mapped files, and scipy works in place)
            m = sp.csr_matrix((values.copy(), indices.copy(), indptr.copy()), shape=(p1 - p0, n_px))
            m.sum_duplicates()
            m.sort_indices()
            indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(m.indices, dtype=np.int32)
            values = np.ascontiguousarray(m.data.astype(dtype, copy=False))
            nnz_now = int(indptr[-1])
            csr = None
            csr = to_device(indptr, indices, values)
            if flags_of(csr) != 0:
                raise DataSetException(f"{self._path}: the CSR rows could not be brought into canonical form")
            self.canonicalised = True
        torch.cuda.current_stream(device).synchronize()
        return csr

    def initialize(self, executor):
        self._conf = conf = load_toml(self._path)
        if conf['params']['filetype'].lower() != 'raw_csr':
            raise ValueError(f"Filetype is not CSR, found {conf['params']['filetype']}")
        nav_shape = self._nav_arg if self._nav_arg is not None else tuple(conf['params']['nav_shape'])
        toml_sig = tuple(conf['params']['sig_shape'])
        sig_shape = self._sig_arg
        if sig_shape is None:
            sig_shape = toml_sig
        elif prod(sig_shape) != prod(toml_sig):
            raise ValueError(f"Sig size mismatch between {sig_shape} and {toml_sig}.")
        nav_shape = tuple(int(n) for n in nav_shape)
        sig_shape = tuple(int(n) for n in sig_shape)
        self._descriptor = descriptor = get_descriptor(self._path)
        self._triple = get_triple(descriptor)
        if self._triple[1].shape != self._triple[2].shape:
            raise RuntimeError('Shape mismatch between data and indices.')
        self._nnz_file = int(self._triple[1].shape[0])
        self._image_count = image_count = get_nav_size(descriptor)
        n_nav, n_px = int(prod(nav_shape)), int(prod(sig_shape))
        so = self._sync_offset_arg
        if not (-max(image_count, 1) < so < max(image_count, 1)):
            raise DataSetException(
                f"offset should be in ({-image_count}, {image_count}), which is (-image_count, image_count)")
        local_nav, p0, p1 = nav_shape, 0, n_nav
        if self._shard_arg is not None:
            rank, world = int(self._shard_arg[0]), int(self._shard_arg[1])
            if nav_shape[0] % world:
                raise DataSetException(f"first nav axis {nav_shape[0]} does not split over {world} ranks")
            local_nav = (nav_shape[0] // world,) + tuple(nav_shape[1:])
            p0 = rank * int(prod(local_nav))
            p1 = p0 + int(prod(local_nav))
        dtype = np.dtype(descriptor['data_dtype']).newbyteorder('=')
        device = getattr(executor, 'gpu_id', None)
        full_local = tuple(local_nav) + sig_shape
        if device is not None:
            self._csr = self._upload(device, executor, p0, p1, so, n_px)
            self._window = {}
            MemoryDataSet.__init__(self, data=_NoDenseFrames(full_local, dtype, device), sig_dims=len(sig_shape),
                                   num_partitions=self._num_partitions_arg, shard=self._shard_arg)
        else:
            # host tiles are densified per tile: the dataset's "array" is a zero that is never read
            self._p0, self._so = p0, so
            MemoryDataSet.__init__(self, data=np.broadcast_to(np.zeros((), dtype=dtype), full_local),
                                   sig_dims=len(sig_shape), num_partitions=self._num_partitions_arg,
                                   shard=self._shard_arg)
        self._sync_offset = so
        lo = min(n_nav, max(0, -so))
        hi = max(lo, min(n_nav, image_count - so))
        self._valid_frames = None if (lo, hi) == (0, n_nav) else (lo, hi)
        self._meta = DataSetMeta(shape=self._shape, raw_dtype=dtype, sync_offset=so, image_count=image_count)
        return MemoryDataSet.initialize(self, executor)

    # --- frames -------------------------------------------------------------------------------------
    @property
    def stable_device_tiles(self):
        return False                    # (densified tiles share one window of HBM)

    @property
    def data(self):
        raise DataSetException("a raw_csr dataset has no dense array of its frames: run UDFs over it")

    @property
    def nnz(self):
        """stored entries this process holds"""
        if self._csr is not None:
            return int(self._csr['indices'].shape[0])
        return self._nnz_file

    def device_frames(self, local0, n):
        if self._csr is None:
            raise DataSetException("this raw_csr dataset was initialised on a CPU executor")
        c = self._csr
        return HipCSRArray(c['indptr'], c['indices'], c['values'], self.dtype, tuple(self._shape.sig),
                           row0=local0, n=n, window=self._window), 0

    def host_frames(self, local_positions):
        """dense frames (n, *sig) of local scan positions (ascending host integers), from the mapped files"""
        import scipy.sparse as sp
        indptr_f, indices_f, data_f = self._triple
        n_px = int(prod(self._shape.sig))
        pos = np.asarray(local_positions, dtype=np.int64)
        out = np.zeros((len(pos), n_px), dtype=self.dtype)
        g = pos + self._p0 + self._so
        ok = np.flatnonzero((g >= 0) & (g < self._image_count))
        if len(ok):
            g0, g1 = int(g[ok[0]]), int(g[ok[-1]]) + 1
            ptr = np.asarray(indptr_f[g0:g1 + 1]).astype(np.int64)
            lo, hi = int(ptr[0]), int(ptr[-1])
            m = sp.csr_matrix((np.asarray(data_f[lo:hi]), np.asarray(indices_f[lo:hi]).astype(np.int64),
                               ptr - ptr[0]), shape=(g1 - g0, n_px))
            out[ok] = m[g[ok] - g0].toarray()
        return out.reshape((len(pos),) + tuple(self._shape.sig))

    def get_partitions(self):
        if self._partitions is None:
            self._partitions = [
                RawCSRPartition(dataset=self, meta=self._meta, partition_slice=part_slice, idx=idx,
                                start_frame=start, num_frames=stop - start)
                for idx, (part_slice, start, stop) in enumerate(self.get_slices())]
        yield from self._partitions

    # --- the reference's descriptive surface --------------------------------------------------------
    @property
    def path(self):
        return self._path

    def supports_correction(self):
        return False

    def check_valid(self):
        return True

    def get_diagnostics(self):
        d = self._descriptor
        return [{"name": "data dtype", "value": str(d['data_dtype'])},
                {"name": "indptr dtype", "value": str(d['indptr_dtype'])},
                {"name": "indices dtype", "value": str(d['indices_dtype'])}]

    @classmethod
    def get_supported_extensions(cls):
        return {"toml"}

    @classmethod
    def get_supported_io_backends(cls):
        return []

    @classmethod
    def detect_params(cls, path, executor=None):
        try:
            _, extension = os.path.splitext(path)
            has_extension = extension.lstrip('.') in cls.get_supported_extensions()
            under_size_lim = os.stat(path).st_size < 2**20
            if not (has_extension or under_size_lim):
                return False
            conf = load_toml(path)
            if "params" not in conf or "filetype" not in conf["params"]:
                return False
            if conf["params"]["filetype"].lower() != "raw_csr":
                return False
            image_count = get_nav_size(get_descriptor(path))
            return {"parameters": {'path': path, "nav_shape": conf["params"]["nav_shape"],
                                   "sig_shape": conf["params"]["sig_shape"], "sync_offset": 0},
                    "info": {"image_count": image_count}}
        except (TypeError, UnicodeDecodeError, TOMLError, OSError):
            return False

    def get_cache_key(self):
        return {"path": self._path, "shape": tuple(self.shape), "sync_offset": self._sync_offset}

    def __getstate__(self):
        d = MemoryDataSet.__getstate__(self) if self._csr is None else None
        if d is None:
            raise TypeError("a device-resident RawCSRDataSet cannot be pickled")
        return d

    def __repr__(self):
        if self._descriptor is None or self._image_count is None:
            return f"<RawCSRDataSet {self._path} (not initialized)>"
        return f"<RawCSRDataSet of {self.dtype} shape={self.shape}>"


class RawCSRPartition(MemPartition):
    def set_corrections(self, corrections):
        if corrections is not None and corrections.have_corrections():
            raise NotImplementedError("corrections not implemented for raw CSR data set")

    def get_tiles(self, tiling_scheme, dest_dtype="float32", roi=None, array_backend=None, env=None,
                  corrections=None):
        self.set_corrections(corrections)
        from libertem_amd.common.udf import NUMPY, HIP
        from .base import TilingScheme
        ds = self._ds
        frame_bytes = max(1, prod(ds.shape.sig) * np.dtype(ds.dtype).itemsize)
        depth = max(1, ds.DENSE_WINDOW_BYTES // frame_bytes)
        if array_backend == HIP and tiling_scheme.intent != 'partition' and len(tiling_scheme) == 1 \
                and int(tiling_scheme.depth) > depth:
            # the tiles of a partition share one dense window (for the UDFs that take dense frames): bounded
            tiling_scheme = TilingScheme.make_for_shape(
                tileshape=Shape((depth,) + tuple(ds.shape.sig), sig_dims=ds.shape.sig.dims),
                dataset_shape=ds.shape, intent=tiling_scheme.intent, debug=tiling_scheme._debug)
        yield from MemPartition.get_tiles(self, tiling_scheme, dest_dtype=dest_dtype, roi=roi,
                                          array_backend=NUMPY if array_backend is None else array_backend,
                                          env=env, corrections=None)

    def _get_tiles_numpy(self, tiling_scheme, dest_dtype, roi, corrections=None):
        """host tiles: the frames of a group densified from the mapped triple, then cut into the scheme's
        sig slices (positions a sync_offset leaves without a frame are not delivered, as in MemPartition)"""
        ds = self._ds
        sig_dims = ds.shape.sig.dims
        idxs = self._roi_indices(roi)
        depth = int(tiling_scheme.depth)
        if idxs is None:
            n, compressed_origin = self._num_frames, self._start_frame
            idxs = np.arange(self._local0, self._local0 + n)
        else:
            n, compressed_origin = len(idxs), self.slice.adjust_for_roi(roi).origin[0]
        first, last = 0, n
        valid = getattr(ds, '_valid_frames', None)
        if valid is not None:
            lo, hi = valid[0] - ds.local_frame_range[0], valid[1] - ds.local_frame_range[0]
            first = int(np.searchsorted(idxs, lo, side='left'))
            last = int(np.searchsorted(idxs, hi, side='left'))
        for g0 in range(first, last, depth):
            g1 = min(last, g0 + depth)
            frames = ds.host_frames(idxs[g0:g1])
            for scheme_idx, sig_slice in tiling_scheme.slices:
                block = frames[(slice(None),) + sig_slice.get(sig_only=True)]
                block = np.ascontiguousarray(block.astype(dest_dtype, copy=False))
                tile_slice = Slice(
                    origin=(compressed_origin + g0,) + tuple(sig_slice.origin[-sig_dims:]),
                    shape=Shape((g1 - g0,) + tuple(sig_slice.shape.sig), sig_dims=sig_dims))
                yield DataTile(block, tile_slice, scheme_idx)
