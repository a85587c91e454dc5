"""
A dataset stored as (sig, nav) -- all values of one detector pixel together, as Gatan K2 / K3 4D-STEM files are --
rewritten as a (nav, sig) .npy file (reference src/libertem/contrib/convert_transposed.py).

    ds = ctx.load('raw', path=..., dtype=..., nav_shape=(sig_y, sig_x), sig_shape=(nav_y, nav_x))
    convert_transposed(ctx, ds, 'out.npy')
    ctx.load('npy', path='out.npy')

The dataset is loaded as it is stored, so its "frames" are the maps of one detector pixel over the scan, and a
partition of n of them is an (n, N) block that lands at columns [o, o + n) of the (N, S) output.  The reference
assigns `partition.T` into the memory map: a scattered write of single elements on one CPU thread.  A HIP worker
transposes the partition in HBM (`ltmi_transpose2d`, csrc/ltmi_transpose.hip) into an (N, n) scratch array, copies
that to the host in one piece, and the host assigns N contiguous rows of n elements.  A NumPy worker runs the
reference's lines.

One process writes the file: multi-rank runs (`torchrun`) are not supported, see RecordUDF.
"""
import os
from typing import Optional

from libertem_amd import hip
from libertem_amd.common.hiparray import HipArray
from libertem_amd.common.math import prod
from libertem_amd.common.shape import Shape
from libertem_amd.io.dataset.base import DataSetException
from libertem_amd.udf.record import RecordUDF


class ConvertTransposedDatasetUDF(RecordUDF):
    """Writes the (sig, nav) dataset it runs on as a (nav, sig) .npy file.  Runs in one process only: with several
    ranks (`torchrun`) all of them would write one file."""

    def get_method(self):
        return self.UDF_METHOD.PARTITION

    @property
    def _ds_shape(self):
        nav_shape = self.meta.dataset_shape.sig.to_tuple()
        sig_shape = self.meta.dataset_shape.nav.to_tuple()
        return Shape(nav_shape + sig_shape, sig_dims=len(sig_shape))

    @property
    def _memmap_flat_shape(self):
        return (self._ds_shape.nav.size, self._ds_shape.sig.size)

    def get_task_data(self):
        data = super().get_task_data()
        data['scratch'] = None                  # (N, n) device array of the largest partition so far: grow-only
        return data

    def process_partition(self, partition):
        # partition will be of shape (n_sig_pix, *ds.shape.nav)
        n_sig_px = partition.shape[0]
        # the flat nav origin of the run is the sig origin in the memmap
        flat_sig_origin = self.meta.slice.origin[0]
        target = self.task_data.memmap[:, flat_sig_origin:flat_sig_origin + n_sig_px]
        if not isinstance(partition, HipArray):
            target[:] = partition.reshape((n_sig_px, -1)).T
            return
        n_nav = prod(partition.shape[1:])
        scratch = self.task_data.scratch
        if scratch is None or scratch.size < n_nav * n_sig_px or scratch.dtype != partition.dtype:
            scratch = HipArray.empty((n_nav * n_sig_px,), partition.dtype, partition.device)
            self.task_data.set_buffer('scratch', scratch)
        hip.transpose2d(partition.device, partition.data_ptr(), partition.ld, n_sig_px, n_nav,
                        partition.dtype.itemsize, scratch.data_ptr(), n_sig_px)
        target[:] = HipArray(scratch.torch, (n_nav, n_sig_px), partition.dtype).cpu()


def convert_transposed(ctx, ds, out_path: os.PathLike, **run_kwargs):
    """Write the dataset `ds`, stored as (sig, nav), to the .npy file `out_path` as (nav, sig): the file has the shape
    `ds.shape.sig + ds.shape.nav` and loads with `ctx.load('npy', path=out_path, sig_dims=len(ds.shape.nav))`.
    `run_kwargs` go to `ctx.run_udf` (`progress=...`).  One process only, no multi-rank runs."""
    ctx.run_udf(ds, ConvertTransposedDatasetUDF(out_path), **run_kwargs)


_convert_transposed_ds = convert_transposed


def convert_dm4_transposed(
    dm4_path: os.PathLike,
    out_path: os.PathLike,
    ctx=None,
    num_cpus: Optional[int] = None,
    dataset_index: Optional[int] = None,
    progress: bool = False,
):
    """The reference's convenience function for transposed Gatan Digital Micrograph (.dm4) files.  This build has no
    DM reader, so it raises DataSetException: load the file's data block as a `raw` (or `npy`) dataset of the
    file's (sig, nav) shape and call `convert_transposed`."""
    if ctx is not None and num_cpus is not None:
        raise ValueError('Either supply a Context or number of cpus to use in conversion')
    raise DataSetException(
        f"cannot read {dm4_path!r}: this build has no DM reader. Load the data block of the file with "
        "ctx.load('raw', path=..., dtype=..., nav_shape=<sig shape of the scan>, sig_shape=<nav shape of the scan>) "
        "(or as an 'npy' dataset of that (sig, nav) shape) and pass the dataset to "
        "libertem_amd.contrib.convert_transposed.convert_transposed(ctx, ds, out_path)")
