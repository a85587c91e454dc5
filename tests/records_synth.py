"""
Synthetic record files for the tests (a helper, not a test): writers of Norpix `.seq` files with their side files
(`.seq.dark.mrc`, `.seq.gain.mrc`, `.seq.Config.Metadata.xml`, `.seq.metadata`), of EMPAD `.raw` + `.xml` pairs and
of NanoMegas `.blo` files, and a plain NumPy decoder that strips the framing -- the CPU yardstick of the record
tests, which tests/test_records_cpu.py pins to the reference's readers through tests/golden/records.npz.

All three are one file of fixed-size records behind a file header: [frame header | pixels | frame footer]
(DESIGN.md 4.11).  Headers and gaps are written as 0xFF bytes and footers as 0xEE, so that framing read as pixels
shows.
"""
import os
import struct

import numpy as np

HEAD_FILL, FOOT_FILL = 0xFF, 0xEE

# --- the decoder ---------------------------------------------------------------------------------------------


def strip(data, file_header, frame_header, payload_bytes, frame_footer, n_frames, dtype, frame_shape):
    """the bytes of a file -> frames (n_frames,) + frame_shape of `dtype`, read as stored (no byte swap); the last
    record may lack its footer"""
    data = np.asarray(data, dtype=np.uint8)
    stride = frame_header + payload_bytes + frame_footer
    out = np.empty((n_frames, payload_bytes), dtype=np.uint8)
    for i in range(n_frames):
        start = file_header + i * stride + frame_header
        out[i] = data[start:start + payload_bytes]
    return out.view(np.dtype(dtype)).reshape((n_frames,) + tuple(frame_shape))


def records(frames, frame_header, frame_footer, last_footer=True):
    """frames (n, ...) -> the bytes of n records, headers 0xFF and footers 0xEE"""
    frames = np.ascontiguousarray(frames)
    n = len(frames)
    payload = frames.reshape(n, -1).view(np.uint8)
    rec = np.empty((n, frame_header + payload.shape[1] + frame_footer), dtype=np.uint8)
    rec[:, :frame_header] = HEAD_FILL
    rec[:, frame_header:frame_header + payload.shape[1]] = payload
    rec[:, frame_header + payload.shape[1]:] = FOOT_FILL
    flat = rec.reshape(-1)
    return flat if last_footer or not frame_footer else flat[:-frame_footer]


def positioned(frames, n_nav, sync_offset):
    """frame g at scan position g - sync_offset, zero frames elsewhere -> (n_nav,) + frame shape"""
    out = np.zeros((n_nav,) + frames.shape[1:], dtype=frames.dtype)
    for p in range(n_nav):
        if 0 <= p + sync_offset < len(frames):
            out[p] = frames[p + sync_offset]
    return out


# --- Norpix .seq -------------------------------------------------------------------------------------------------
SEQ_FIELDS = (
    ('magic', 'L'), ('name', '24s'), ('version', 'l'), ('header_size', 'l'), ('description', '512s'),
    ('width', 'L'), ('height', 'L'), ('bit_depth', 'L'), ('bit_depth_real', 'L'), ('image_size_bytes', 'L'),
    ('image_format', 'L'), ('allocated_frames', 'L'), ('origin', 'L'), ('true_image_size', 'L'),
    ('suggested_frame_rate', 'd'), ('description_format', 'l'), ('reference_frame', 'L'), ('fixed_size', 'L'),
    ('flags', 'L'), ('bayer_pattern', 'l'), ('time_offset_us', 'l'), ('extended_header_size', 'l'),
    ('compression_format', 'L'), ('reference_time_s', 'l'), ('reference_time_ms', 'H'), ('reference_time_us', 'H'),
)


def seq_offset(version):
    return 8192 if version >= 5 else 1024


def seq_bytes(frames, footer, version=5, last_footer=True, **override):
    """the bytes of a .seq file of the frames (n, height, width), uint8 / uint16 / uint32; `override`: header
    fields to write differently (magic=..., compression_format=..., bit_depth=...)"""
    frames = np.asarray(frames)
    frames = frames.astype(frames.dtype.newbyteorder('<'))
    n, h, w = frames.shape
    payload = h * w * frames.dtype.itemsize
    fields = dict(
        magic=0xFEED, name='Norpix seq'.encode('utf-16-le'), version=version, header_size=1024,
        description='synthetic frames'.encode('utf-16-le'), width=w, height=h, bit_depth=8 * frames.dtype.itemsize,
        bit_depth_real=8 * frames.dtype.itemsize, image_size_bytes=payload, image_format=100, allocated_frames=n,
        origin=0, true_image_size=payload + footer, suggested_frame_rate=30.0, description_format=0,
        reference_frame=0, fixed_size=0, flags=0, bayer_pattern=0, time_offset_us=0, extended_header_size=0,
        compression_format=0, reference_time_s=0, reference_time_ms=0, reference_time_us=0)
    fields.update(override)
    head = np.full(seq_offset(version), HEAD_FILL, dtype=np.uint8)
    packed = b''.join(struct.pack('<' + code, fields[name]) for name, code in SEQ_FIELDS)
    head[:len(packed)] = np.frombuffer(packed, dtype=np.uint8)
    return np.concatenate([head, records(frames, 0, footer, last_footer)])


def write_seq(path, frames, footer, version=5, last_footer=True, **override):
    seq_bytes(frames, footer, version, last_footer, **override).tofile(path)
    return path


MRC_MODES = {np.dtype('int8'): 0, np.dtype('int16'): 1, np.dtype('float32'): 2, np.dtype('uint16'): 6}


def write_mrc(path, data, extended=0):
    """an MRC file of the sections data (nz, ny, nx); `extended`: bytes of extended header (0xFF) before the data"""
    data = np.ascontiguousarray(data)
    nz, ny, nx = data.shape
    words = np.zeros(256, dtype='<i4')
    words[:4] = nx, ny, nz, MRC_MODES[data.dtype]
    words[23] = extended
    words[52] = int.from_bytes(b'MAP ', 'little')
    with open(path, 'wb') as f:
        f.write(words.tobytes())
        f.write(bytes([HEAD_FILL]) * extended)
        f.write(data.astype(data.dtype.newbyteorder('<')).tobytes())
    return path


def read_mrc(path):
    """plain reader of what `write_mrc` wrote -> (nz, ny, nx)"""
    raw = np.fromfile(path, dtype=np.uint8)
    words = raw[:1024].view('<i4')
    nx, ny, nz, mode, extended = (int(words[i]) for i in (0, 1, 2, 3, 23))
    dtype = {v: k for k, v in MRC_MODES.items()}[mode]
    return raw[1024 + extended:].view(dtype.newbyteorder('<'))[:nx * ny * nz].reshape(nz, ny, nx)


def write_seq_metadata(path, frame_size_yx, offset_yx, binning=1):
    """`<base>.seq.metadata`: twelve values at byte 282, format 'iiiiiiiiiii?' (DEMetadataSize, DEMetadataVersion,
    UnbinnedFrameSizeX, UnbinnedFrameSizeY, OffsetX, OffsetY, HardwareBinning, Bitmode, FrameRate, RotationMode,
    FlipMode, OkraMode)"""
    values = (0, 1, frame_size_yx[1], frame_size_yx[0], offset_yx[1], offset_yx[0], binning, 16, 30, 0, 0, False)
    with open(path, 'wb') as f:
        f.write(bytes([HEAD_FILL]) * 282 + struct.pack('iiiiiiiiiii?', *values) + bytes([FOOT_FILL]) * 16)
    return path


def write_seq_xml(path, maps):
    """`<base>.seq.Config.Metadata.xml`; maps: [dict(columns, rows, binning (None: no attribute), defects)], a
    defect a dict of attributes: {'Rows': '1-2'}, {'Row': '3'}, {'Columns': '0-1'}, {'Column': '5'},
    {'Column': '2', 'Row': '4'}"""
    lines = ['<?xml version="1.0" encoding="utf-8"?>', '<Configuration>', ' <BadPixelMaps>']
    for m in maps:
        binning = '' if m.get('binning') is None else f' Binning="{m["binning"]}"'
        lines.append(f'  <BadPixelMap Columns="{m["columns"]}" Rows="{m["rows"]}"{binning}>')
        for defect in m['defects']:
            lines.append('   <Defect ' + ' '.join(f'{k}="{v}"' for k, v in defect.items()) + '/>')
        lines.append('  </BadPixelMap>')
    lines += [' </BadPixelMaps>', '</Configuration>']
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return path


# --- EMPAD ---------------------------------------------------------------------------------------------------------
EMPAD_SIZE, EMPAD_SIZE_RAW = (128, 128), (130, 128)


def write_empad_raw(path, frames, last_footer=True):
    """frames (n, 128, 128) float32 -> records of 130 x 128 x 4 bytes, the two extra rows 0xEE"""
    frames = np.asarray(frames, dtype='<f4')
    records(frames, 0, 2 * 128 * 4, last_footer).tofile(path)
    return path


def write_empad_xml(path, raw_name, acquire=None, search=None, series=None):
    """acquire / search: (y, x) of the `scan_parameters` node of that mode (None: no node); series: frame count
    (`type` is 'series' then, else 'scan').  `raw_file@filename` is written with a directory in front, as the
    acquisition computer does"""
    lines = ['<?xml version="1.0"?>', '<root>', f' <raw_file filename="/acquisition/data/{raw_name}"/>']
    if series is not None:
        lines += [' <type>series</type>', f' <count>{series}</count>']
    else:
        lines.append(' <type>scan</type>')
    for mode, shape in (('search', search), ('acquire', acquire)):
        if shape is not None:
            lines += [f' <scan_parameters mode="{mode}">', f'  <scan_resolution_x>{shape[1]}</scan_resolution_x>',
                      f'  <scan_resolution_y>{shape[0]}</scan_resolution_y>', ' </scan_parameters>']
    lines.append('</root>')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return path


# --- NanoMegas .blo --------------------------------------------------------------------------------------------------
BLO_FRAME_HEADER = 6
BLO_TEXT_START = 240


def blo_header_dtype(e):
    fields = [('ID', 'S6'), ('MAGIC', e + 'u2'), ('Data_offset_1', e + 'u4'), ('Data_offset_2', e + 'u4'),
              ('UNKNOWN1', e + 'u4'), ('DP_SZ', e + 'u2'), ('DP_rotation', e + 'u2'), ('NX', e + 'u2'),
              ('NY', e + 'u2'), ('Scan_rotation', e + 'u2'), ('SX', e + 'f8'), ('SY', e + 'f8'),
              ('Beam_energy', e + 'u4'), ('SDP', e + 'u2'), ('Camera_length', e + 'u4'),
              ('Acquisition_time', e + 'f8')]
    fields += [('Centering_N%d' % i, 'f8') for i in range(8)] + [('Distortion_N%02d' % i, 'f8') for i in range(14)]
    return np.dtype(fields)


def blo_bytes(frames, nav, endianess='<', magic=259, bit_depth_line=None, gap=0):
    """the bytes of a .blo file of the frames (n, DP_SZ, DP_SZ), uint8 or uint16, n = NY * NX of `nav`.  Header
    fields AND 16-bit pixels are written with `endianess`.  magic 259: a text block from byte 240 (with the line
    `bit_depth_line`, if any); then the virtual bright field image (NY * NX bytes of 0xEE) at Data_offset_1, `gap`
    bytes of 0xEE, and the patterns at Data_offset_2"""
    frames = np.asarray(frames)
    n, side, _ = frames.shape
    ny, nx = nav
    assert n == ny * nx
    text = b''
    if magic == 259:
        lines = ['Astar blockfile', 'Camera: synthetic'] + ([bit_depth_line] if bit_depth_line else []) + ['end']
        text = ('\r\n'.join(lines) + '\r\n').encode() + b'\x00' * 7
    offset_1 = BLO_TEXT_START + len(text)
    offset_2 = offset_1 + n + gap
    head = np.full(offset_2, FOOT_FILL, dtype=np.uint8)
    head[:BLO_TEXT_START] = HEAD_FILL
    dt = blo_header_dtype(endianess)
    fields = np.zeros(1, dtype=dt)
    fields['ID'], fields['MAGIC'] = b'IMGBLO', magic
    fields['Data_offset_1'], fields['Data_offset_2'] = offset_1, offset_2
    fields['DP_SZ'], fields['NX'], fields['NY'] = side, nx, ny
    fields['SX'] = fields['SY'] = 1.5
    fields['Beam_energy'], fields['SDP'], fields['Camera_length'] = 200000, 100, 1000
    head[:dt.itemsize] = fields.view(np.uint8)
    head[BLO_TEXT_START:offset_1] = np.frombuffer(text, dtype=np.uint8)
    stored = frames.astype(frames.dtype.newbyteorder(endianess)) if frames.dtype.itemsize > 1 else frames
    return np.concatenate([head, records(stored, BLO_FRAME_HEADER, 0)]), offset_2


def write_blo(path, frames, nav, endianess='<', magic=259, bit_depth_line=None, gap=0):
    data, offset_2 = blo_bytes(frames, nav, endianess, magic, bit_depth_line, gap)
    data.tofile(path)
    return path, offset_2
