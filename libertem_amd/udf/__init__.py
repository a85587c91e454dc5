from .base import (
    UDF, UDFMeta, UDFRunner, UDFData, NoOpUDF, check_cast, UDFFrameMixin, UDFTileMixin, UDFPartitionMixin,
    UDFPostprocessMixin, UDFPreprocessMixin, UDFMergeAllMixin,
)
from libertem_amd.common.udf import UDFMethod
from libertem_amd.common.exceptions import UDFRunCancelled, UDFException
from .auto import AutoUDF
from .record import RecordUDF
from .correlation import CorrelationUDF, run_correlation
from .peakfind import PeakFindUDF, run_peakfind, find_peaks, find_in_maps
from .holography import HoloReconstructUDF, run_holo
from .cepstrum import CepstrumUDF, run_cepstrum, cepstrum_dataset, cepstrum_frames, hann_window
from .ssb import SSBUDF, run_ssb
from .wdd import WDDUDF, run_wdd
from .parallax import ParallaxUDF, run_parallax, parallax_bf, parallax_aberrations, fit_shifts
from .counting import EventCountUDF, EventStoreUDF, count_events, count_frames, estimate_thresholds
from .orientation import (
    OrientationMatchUDF, run_orientation_match, polar_table, polar_library, polar_frames, match_polar, rotation_angles,
)
from .lattice import LatticeRefineUDF, run_refine, fit_lattice, lattice_peaks, lattice_strain

__all__ = ['UDF', 'UDFFrameMixin', 'UDFTileMixin', 'UDFPartitionMixin', 'UDFPostprocessMixin', 'UDFPreprocessMixin',
           'UDFMergeAllMixin', 'UDFMeta', 'UDFRunner', 'UDFData', 'NoOpUDF', 'UDFMethod', 'check_cast', 'AutoUDF',
           'RecordUDF', 'CorrelationUDF', 'run_correlation', 'PeakFindUDF', 'run_peakfind', 'find_peaks', 'find_in_maps',
           'LatticeRefineUDF', 'run_refine', 'fit_lattice',
           'lattice_peaks', 'lattice_strain', 'HoloReconstructUDF', 'run_holo', 'CepstrumUDF', 'run_cepstrum',
           'cepstrum_dataset', 'cepstrum_frames', 'hann_window', 'SSBUDF', 'run_ssb', 'WDDUDF', 'run_wdd',
           'ParallaxUDF', 'run_parallax', 'parallax_bf', 'parallax_aberrations', 'fit_shifts',
           'EventCountUDF', 'EventStoreUDF', 'count_events', 'count_frames', 'estimate_thresholds',
           'OrientationMatchUDF', 'run_orientation_match', 'polar_table', 'polar_library', 'polar_frames',
           'match_polar', 'rotation_angles', 'UDFRunCancelled', 'UDFException']
