"""
RecordUDF -- the frames a run is handed, written into a NumPy .npy file of the dataset's shape.

Same contract as the reference's RecordUDF (src/libertem/udf/record.py:9-70): the file is created in `preprocess`
on the main process, every task maps it again and writes its tiles at `meta.slice`; there are no result buffers.
The frames are the ones every other UDF of the run sees: decoded (mib, k2is, frms6, seq, ...) and, with corrections
in force, corrected -- dtype and values.  A NumPy worker assigns the tile as the reference does; a HIP worker
copies the tile from HBM to the host (one D2H per tile, page-locked for large tiles) and assigns that.  Scan
positions that a `sync_offset` leaves without a frame stay zero in the file.

One process writes the file: a multi-rank run (`torchrun`) would have every rank create and map the same file and
is not supported.
"""
import numpy as np

from libertem_amd.common.buffers import reshaped_view
from libertem_amd.common.hiparray import HipArray
from libertem_amd.common.math import prod
from libertem_amd.udf.base import UDF


class RecordUDF(UDF):
    """
    Record input data as NumPy .npy file

    Parameters
    ----------
    filename : str or path-like
        Filename where to save. The file will be overwritten if it exists.
    _is_master : bool
        Internal flag, keep at default value.

    Runs in one process only: with several ranks (`torchrun`) all of them would write one file.
    """

    def __init__(self, filename, _is_master=True):
        self._is_master = _is_master
        super().__init__(filename=filename, _is_master=False)

    def get_backends(self):
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def get_preferred_input_dtype(self):
        return self.USE_NATIVE_DTYPE

    @property
    def _ds_shape(self):
        # only valid during run_udf hence _ property
        return self.meta.dataset_shape

    @property
    def _memmap_flat_shape(self):
        # only valid during run_udf hence _ property
        return (prod(self._ds_shape.nav), *self._ds_shape.sig)

    def preprocess(self):
        if self.meta.roi is not None:
            raise RuntimeError('Recording with ROI is not supported.')
        # create the file once in the preprocess method on the main process
        if self._is_master:
            np.lib.format.open_memmap(self.params.filename, mode='w+', dtype=self.meta.input_dtype,
                                      shape=tuple(self._ds_shape))

    def get_result_buffers(self):
        return {}

    def get_task_data(self):
        m = np.lib.format.open_memmap(self.params.filename, mode='r+', dtype=self.meta.input_dtype,
                                      shape=tuple(self._ds_shape))
        return {'memmap': reshaped_view(m, self._memmap_flat_shape)}

    def process_tile(self, tile):
        if isinstance(tile, HipArray):
            tile = tile.cpu()
        self.meta.slice.get(self.task_data.memmap)[:] = tile
