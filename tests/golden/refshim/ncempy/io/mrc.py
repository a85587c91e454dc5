"""`mrcReader` for the dark and gain side files of the synthetic SEQ sets: the 1024-byte header's nx, ny, nz and
mode (int32 words 0-3), the length of the extended header (word 23), then the sections -> {'data': (nz, ny, nx)}.
Written apart from the package's reader (libertem_amd/io/dataset/seq.py); tests/test_records_cpu.py checks both
against the arrays the writer put into the files."""
import numpy as np

_MODES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16}


def mrcReader(fname, verbose=False):
    head = np.memmap(fname, dtype='<i4', mode='r', shape=(256,))
    nx, ny, nz, mode, ext = int(head[0]), int(head[1]), int(head[2]), int(head[3]), int(head[23])
    data = np.memmap(fname, dtype=np.dtype(_MODES[mode]).newbyteorder('<'), mode='r', offset=1024 + ext,
                     shape=(nz, ny, nx))
    return {'data': np.array(data), 'filename': fname}
