"""
NPYDataSet: NumPy .npy files (`ctx.load("npy", path=...)`, reference io/dataset/npy.py:86-283) -- what RecordUDF and
`libertem_amd.contrib.convert_transposed` write.  Shape, dtype and the offset of the data are read from the file's
header; from there on the file is a flat binary file: it is memory-mapped from that offset and streamed to the GPU
like a `raw` dataset (RawFileDataSet, io/dataset/raw.py).
"""
import typing

from numpy.lib.format import open_memmap

from libertem_amd.common.math import prod
from libertem_amd.common.shape import Shape
from .base import DataSetException
from .raw import RawFileDataSet


class NPYInfo(typing.NamedTuple):
    dtype: str
    shape: typing.Tuple[int, ...]
    count: int
    offset: int


def read_npy_info(path) -> NPYInfo:
    """shape, dtype, number of elements and byte offset of the data of a C-ordered .npy file"""
    mmp = open_memmap(path, mode='r')
    try:
        shape, count, offset, dtype = mmp.shape, mmp.size, mmp.offset, mmp.dtype
        c_contiguous = mmp.flags['C_CONTIGUOUS']
    finally:
        # the file is closed before anything else happens
        mmp._mmap.close()
        del mmp
    if not c_contiguous:
        raise DataSetException('Unable to process NPY arrays that are not C_CONTIGUOUS, '
                               'consider converting with np.ascontiguousarray().')
    return NPYInfo(dtype=dtype, shape=tuple(shape), count=count, offset=offset)


def _reopen(kwargs):
    return NPYDataSet(**kwargs)


class NPYDataSet(RawFileDataSet):
    """
    Parameters (reference npy.py:96-123)
    ----------
    path : str
    sig_dims : int, optional, by default 2
        how many of the last dimensions of the file's shape are signal dimensions; None: as many as `sig_shape` has
    nav_shape, sig_shape : tuple of int, optional
        override the shape of the header: a reshaped block or a leading part of the file, frames and pixels in C
        order from the start of the data
    sync_offset : int
        as for `raw`
    num_partitions : int, optional

    The dtype is the file's own, little- or big-endian (reported in native order; big-endian integers are swapped
    on the device like those of a `raw` file).  Fortran-ordered files raise DataSetException.
    """

    def __init__(self, path, sig_dims=2, nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None,
                 num_partitions=None, shard=None):
        if io_backend is not None:
            raise ValueError("alternative I/O backends are not part of this build")
        nav_shape = tuple(nav_shape) if nav_shape else None
        sig_shape = tuple(sig_shape) if sig_shape else None
        if sig_shape is not None:
            if sig_dims is None:
                sig_dims = len(sig_shape)
            if len(sig_shape) != sig_dims:
                raise DataSetException(f'Mismatching sig_dims (= {sig_dims}) and sig_shape {sig_shape} arguments')
        if sig_dims is None or not isinstance(sig_dims, int):
            raise DataSetException('Must supply one of sig_dims or sig_shape to NPYDataSet')
        try:
            info = read_npy_info(path)
        except (OSError, ValueError) as e:
            raise DataSetException(f"could not read the .npy file {path}: {e}")
        if len(info.shape) <= sig_dims:
            raise DataSetException(f"the array of shape {info.shape} in {path} has no navigation dimension "
                                   f"with sig_dims = {sig_dims}")
        np_shape = Shape(info.shape, sig_dims=sig_dims)
        sig = sig_shape if sig_shape else tuple(np_shape.sig)
        nav = nav_shape if nav_shape else tuple(np_shape.nav)
        self._npy_info = info
        super().__init__(path=path, dtype=info.dtype, nav_shape=nav, sig_shape=sig, sync_offset=sync_offset,
                         num_partitions=num_partitions, shard=shard, _data_offset=info.offset)
        # the whole block of data read as frames of `sig` (reference npy.py:181-185)
        self._image_count = self._meta.image_count = int(info.count // prod(sig))
        self._ctor = dict(path=path, sig_dims=sig_dims, nav_shape=nav_shape, sig_shape=sig_shape,
                          sync_offset=sync_offset, num_partitions=num_partitions, shard=shard)

    def __reduce__(self):
        return (_reopen, (self._ctor,))

    @classmethod
    def detect_params(cls, path, executor=None):
        try:
            info = read_npy_info(path)
            # (assumption about the number of sig dims, as in the reference)
            shape = Shape(info.shape, sig_dims=2)
            return {
                "parameters": {"path": path, "nav_shape": tuple(shape.nav), "sig_shape": tuple(shape.sig)},
                "info": {"image_count": int(prod(shape.nav)), "native_sig_shape": tuple(shape.sig)},
            }
        except Exception:                                   # noqa: BLE001  (not a file this class reads)
            return False

    @classmethod
    def get_supported_extensions(cls):
        return {"npy"}

    def __repr__(self):
        return f"<NPYDataSet of {self.dtype} shape={tuple(self.shape)}>"
