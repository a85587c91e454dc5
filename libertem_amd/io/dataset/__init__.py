import pathlib

from .memory import MemoryDataSet
from .raw import RawFileDataSet
from .stream import StreamDataSet
from .mib import MIBDataSet
from .raw_csr import RawCSRDataSet
from .k2is import K2ISDataSet
from .frms6 import FRMS6DataSet
from .seq import SEQDataSet
from .empad import EMPADDataSet
from .blo import BloDataSet
from .npy import NPYDataSet
from .tvips import TVIPSDataSet
from .base import DataSet, DataSetException, Partition, DataTile, TilingScheme, Negotiator

#: the dataset types of this build, in the order the reference registers them ('stream' is this package's own)
filetypes = {
    "raw": RawFileDataSet,
    "raw_csr": RawCSRDataSet,
    "mib": MIBDataSet,
    "blo": BloDataSet,
    "k2is": K2ISDataSet,
    "frms6": FRMS6DataSet,
    "empad": EMPADDataSet,
    "seq": SEQDataSet,
    "tvips": TVIPSDataSet,
    "npy": NPYDataSet,
    "memory": MemoryDataSet,
    "stream": StreamDataSet,
}


def get_extensions():
    """the file extensions the types of this build name, lower case, without the dot"""
    return {ext.lower() for cls in filetypes.values() for ext in cls.get_supported_extensions()}


def get_search_order(path):
    """the keys of `filetypes` in the order detection tries them: the types registered for the suffix of `path`
    first (in their own order), then the rest"""
    order = list(filetypes)
    try:
        suffix = pathlib.Path(path).suffix.strip().lstrip('.').lower()
    except (TypeError, ValueError):
        return order
    first = [key for key in order if suffix in {e.lower() for e in filetypes[key].get_supported_extensions()}]
    return first + [key for key in order if key not in first]


def detect(path, executor=None):
    """-> {'parameters': ..., 'info': ..., 'type': key} of the first type that recognises `path`, or {}"""
    for key in get_search_order(path):
        try:
            params = filetypes[key].detect_params(path, executor)
        except Exception:                               # noqa: BLE001  (anything: not a file of this format)
            continue
        if params:
            return dict(params, type=key)
    return {}


def _auto_load(path=None, *args, **kwargs):
    if path is None:
        raise DataSetException("please specify the `path` argument to allow auto detection")
    detected = detect(path).get('type')
    if detected is None:
        raise DataSetException("could not determine DataSet type for file '%s'" % path)
    # (the caller's own arguments: what detection found out is not merged in, as in the reference)
    return load(detected, path, *args, **kwargs)


def load(filetype, *args, **kwargs):
    """In-memory arrays (host or HBM), flat binary files, NumPy .npy files, Merlin .mib files, Gatan K2 IS sector
    files, PNDetector FRMS6 sets, Norpix SEQ files, EMPAD scans, NanoMegas BLO files, TVIPS series, sparse frames in
    CSR files and frame streams of a running acquisition; 'auto' takes the type that `detect` finds for the path.
    The other file formats of the reference are out of scope of this build."""
    if filetype == 'auto':
        return _auto_load(*args, **kwargs)
    if filetype in ('memory', 'mem'):
        return MemoryDataSet(*args, **kwargs)
    if filetype == 'raw':
        return RawFileDataSet(*args, **kwargs)
    if filetype == 'mib':
        return MIBDataSet(*args, **kwargs)
    if filetype in ('k2is', 'K2IS'):
        return K2ISDataSet(*args, **kwargs)
    if filetype in ('frms6', 'FRMS6'):
        return FRMS6DataSet(*args, **kwargs)
    if filetype in ('seq', 'SEQ'):
        return SEQDataSet(*args, **kwargs)
    if filetype in ('empad', 'EMPAD'):
        return EMPADDataSet(*args, **kwargs)
    if filetype in ('blo', 'BLO'):
        return BloDataSet(*args, **kwargs)
    if filetype in ('tvips', 'TVIPS'):
        return TVIPSDataSet(*args, **kwargs)
    if filetype in ('npy', 'NPY'):
        return NPYDataSet(*args, **kwargs)
    if filetype == 'raw_csr':
        return RawCSRDataSet(*args, **kwargs)
    if filetype in ('stream', 'live'):
        return StreamDataSet(*args, **kwargs)
    raise DataSetException(
        f"dataset type {filetype!r} is not available: 'memory', 'raw', 'mib', 'k2is', 'frms6', 'seq', 'empad', 'blo', "
        "'tvips', 'npy', 'raw_csr' and 'stream' are in scope of this build")


__all__ = ['MemoryDataSet', 'RawFileDataSet', 'StreamDataSet', 'MIBDataSet', 'RawCSRDataSet', 'K2ISDataSet', 'FRMS6DataSet', 'SEQDataSet',
           'EMPADDataSet', 'BloDataSet', 'NPYDataSet', 'TVIPSDataSet', 'DataSet', 'DataSetException', 'Partition',
           'DataTile', 'TilingScheme', 'Negotiator', 'load', 'detect', 'filetypes', 'get_extensions',
           'get_search_order']
