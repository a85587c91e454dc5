"""
EMPADDataSet: scans of the EMPAD detector (`ctx.load("empad", path=...)`, reference io/dataset/empad.py): a .raw
file of float32 frames and an .xml file that names it and holds the scan's shape.  The detector writes 130 rows
of 128 pixels per frame, of which the first 128 are the image: records of 130 x 128 x 4 bytes with a footer of
2 x 128 x 4, no headers.  The frames go to HBM through `RecordFileDataSet`.
"""
import os
import warnings

import numpy as np

from libertem_amd.common.math import prod
from .base import DataSetException
from .records import RecordFileDataSet

EMPAD_DETECTOR_SIZE = (128, 128)
EMPAD_DETECTOR_SIZE_RAW = (130, 128)
ITEMSIZE = 4
PAYLOAD_BYTES = int(prod(EMPAD_DETECTOR_SIZE)) * ITEMSIZE
RECORD_BYTES = int(prod(EMPAD_DETECTOR_SIZE_RAW)) * ITEMSIZE


def get_params_from_xml(path, scan_parameters_mode="acquire"):
    """-> (path of the .raw file, nav shape).  The .raw file is looked for next to the .xml, under the file name of
    `raw_file@filename`; the shape of a scan (`type` 'scan', or none) is (`scan_resolution_y`,
    `scan_resolution_x`) of the `scan_parameters` node of the given mode -- "acquire", or "search" for the files
    whose frames were recorded with the search settings --, that of a 'series' is (`count`,)."""
    try:
        from defusedxml import ElementTree
    except ImportError:                 # (the user's own local side file)
        from xml.etree import ElementTree
    root = ElementTree.parse(path).getroot()
    raw_name = os.path.basename(root.find("raw_file").attrib['filename'])
    path_raw = os.path.join(os.path.dirname(path), raw_name)
    kind = root.find("type")
    if kind is None or kind.text == 'scan':
        node = [n for n in root.findall("scan_parameters") if n.attrib["mode"] == scan_parameters_mode][0]
        nav_shape = (int(node.find("scan_resolution_y").text), int(node.find("scan_resolution_x").text))
    elif kind.text == 'series':
        nav_shape = (int(root.find("count").text),)
    else:
        raise ValueError(f"unknown type: {kind.text}")
    return path_raw, nav_shape


class EMPADDataSet(RecordFileDataSet):
    """
    Parameters (reference empad.py:113-158)
    ----------
    path : str
        the .xml file, or the .raw file together with `nav_shape`
    nav_shape : tuple of int, optional
        (y, x) of a scan or (frames,) of a series; read from the .xml file if that is the `path`
    sig_shape : tuple of int, optional
        same number of pixels as (128, 128)
    sync_offset : int
        > 0: frames to skip at the start; < 0: blank frames inserted at the start
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: load and hold only this rank's block of the first nav axis
    """
    KIND = "EMPAD file"

    def __init__(self, path, scan_size=None, nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None,
                 num_partitions=None, shard=None):
        if scan_size is not None:
            warnings.warn("scan_size argument is deprecated. please specify nav_shape instead", FutureWarning)
            if nav_shape is not None:
                raise ValueError("cannot specify both scan_size and nav_shape")
            nav_shape = scan_size
        RecordFileDataSet.__init__(self, path, nav_shape, sig_shape, sync_offset, io_backend, num_partitions, shard)
        self._path_raw = None
        self._filesize = None

    def _init_from_xml(self, mode):
        try:
            return get_params_from_xml(self._path, scan_parameters_mode=mode)
        except Exception as e:                          # noqa: BLE001
            raise DataSetException("could not initialize EMPAD file; error: %s" % (str(e)))

    def _scan_file(self):
        """-> FrameLayout, from the .xml file (if that is the path) and the size of the .raw file"""
        xml_nav = None
        lowpath = self._path.lower()
        if lowpath.endswith(".xml"):
            self._path_raw, xml_nav = self._init_from_xml("acquire")
        elif not lowpath.endswith(".raw"):
            raise DataSetException("path should either be .xml or .raw")
        elif self._nav_arg is None:
            raise DataSetException("need to set or detect nav_shape!")
        else:
            self._path_raw = self._path
        self._filesize = size = self._file_size(self._path_raw)
        if xml_nav is not None and size != RECORD_BYTES * int(prod(xml_nav)):
            # some files hold the frames of the "search" scan parameters
            _, other_nav = self._init_from_xml("search")
            expected, alternate = RECORD_BYTES * int(prod(xml_nav)), RECORD_BYTES * int(prod(other_nav))
            if size != alternate:
                raise ValueError(
                    f"RAW data file size mismatch; filesize={size} vs expected size {expected} for nav {xml_nav} "
                    f"or alternate {alternate} for nav {other_nav}.")
            xml_nav = other_nav
        in_file = size // RECORD_BYTES
        return self._record_layout(
            self._path_raw, file_header=0, frame_header=0, payload_bytes=PAYLOAD_BYTES,
            frame_footer=RECORD_BYTES - PAYLOAD_BYTES, storage=np.float32, native_shape=EMPAD_DETECTOR_SIZE,
            n_frames=in_file, nav_shape=self._nav_arg if self._nav_arg is not None else xml_nav,
            image_count=int(prod(xml_nav)) if xml_nav else in_file)

    def initialize(self, executor):
        self._gpu_of(executor)
        return self._load_records(executor, self._scan_file())

    def check_valid(self):
        try:
            if self._path_raw is None:
                self._scan_file()
            with open(self._path_raw, 'rb'):
                return True
        except (OSError, ValueError) as e:
            raise DataSetException("invalid dataset: %s" % e)

    def get_diagnostics(self):
        return [{"name": "Raw file", "value": str(self._path_raw)},
                {"name": "File size", "value": str(self._filesize)},
                {"name": "Frames", "value": str(self._image_count)}]

    @classmethod
    def get_supported_extensions(cls):
        return {"xml", "raw"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """an .xml file names the scan; a .raw file alone cannot be told from any other file (reference
        empad.py:280-304)"""
        try:
            ds = cls(path)
            layout = ds._scan_file()
            ds.check_valid()
        except Exception:                               # noqa: BLE001  (anything: not a set of this format)
            return False
        return {"parameters": {"path": path, "nav_shape": layout.nav_shape, "sig_shape": layout.sig_shape},
                "info": {"image_count": ds._image_count, "native_sig_shape": layout.sig_shape}}

    def get_cache_key(self):
        return {"path_raw": self._path_raw, "shape": tuple(self.shape), "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._layout is None:
            return f"<EMPADDataSet for {self._path} (not initialized)>"
        return f"<EMPADDataSet of {self.dtype} shape={tuple(self.shape)}>"
