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
from .base import DataSet, DataSetException, Partition, DataTile, TilingScheme, Negotiator


def load(filetype, *args, **kwargs):
    """In-memory arrays (host or HBM), flat binary files, NumPy .npy files, Merlin .mib files, Gatan K2 IS sector
    files, PNDetector FRMS6 sets, Norpix SEQ files, EMPAD scans, NanoMegas BLO files, sparse frames in CSR files and
    frame streams of a running acquisition; the other file formats of the reference are out of scope of this build."""
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
    if filetype in ('npy', 'NPY'):
        return NPYDataSet(*args, **kwargs)
    if filetype == 'raw_csr':
        return RawCSRDataSet(*args, **kwargs)
    if filetype in ('stream', 'live'):
        return StreamDataSet(*args, **kwargs)
    raise DataSetException(
        f"dataset type {filetype!r} is not available: 'memory', 'raw', 'mib', 'k2is', 'frms6', 'seq', 'empad', 'blo', "
        "'npy', 'raw_csr' and 'stream' are in scope of this build")


__all__ = ['MemoryDataSet', 'RawFileDataSet', 'StreamDataSet', 'MIBDataSet', 'RawCSRDataSet', 'K2ISDataSet', 'FRMS6DataSet', 'SEQDataSet',
           'EMPADDataSet', 'BloDataSet', 'NPYDataSet', 'DataSet', 'DataSetException', 'Partition', 'DataTile',
           'TilingScheme', 'Negotiator', 'load']
