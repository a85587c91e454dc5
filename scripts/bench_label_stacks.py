"""partition stacks (every pixel stored by at most one mask) on resident frames of 256 x 256: detector binning by 2 / 4 / 8
(masks.bin_masks), a 64 x 64 polar (r, theta) map and 128 hard rings, uint16 and float32 frames, each once with
LTMI_SPARSE_LABELS=0 (the gather kernel) and once with LTMI_SPARSE_LABELS=1 (the label image, k_labels), on 16 384 frames
and on 512 frames (the depth of a tile in a UDF run).  Per cell: 9 HIP event pairs around 3 launches each after 3 warm-up
launches; printed are the median and the minimum per launch.  The fraction is frame bytes / median time over 8 TB/s.
(A build without ltmi_labels.hip ignores the variable: both columns then show the same route.)"""
import os, sys
import numpy as np, torch
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip, masks as pm

N, SIG = 16384, (256, 256)
N_PX = SIG[0] * SIG[1]
PEAK = 8e12


def partition(label, weight=None):
    """(n_px, n_masks) CSR of a label image; label < 0: no mask stores the pixel"""
    label = label.ravel()
    px = np.flatnonzero(label >= 0)
    w = np.ones(px.size, dtype=np.float32) if weight is None else weight.ravel()[px].astype(np.float32)
    return sp.csr_matrix((w, (px, label[px])), shape=(label.size, int(label.max()) + 1))


def stacks():
    for b in (2, 4, 8):
        yield f"bin {b}", pm.bin_masks(SIG, b).T.tocsr()
    r, phi = pm.polar_map(128, 128, 256, 256)
    ri = np.floor(r / 2).astype(np.int64)
    ti = np.minimum(np.floor((phi + np.pi) / (2 * np.pi) * 64).astype(np.int64), 63)
    yield "polar 64x64", partition(np.where(ri < 64, ri * 64 + ti, -1))
    ri = np.floor(r).astype(np.int64)
    yield "128 hard rings", partition(np.where(ri < 128, ri, -1), 1.0 / np.maximum(r, 1.0))


def timed(h, tile, dt, out, n, n_masks, pairs=9, per_pair=3):
    """-> (median, minimum) ms per launch over `pairs` event pairs"""
    for _ in range(3):
        h.apply(tile.data_ptr(), dt, n, N_PX, out.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(pairs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_pair):
            h.apply(tile.data_ptr(), dt, n, N_PX, out.data_ptr(), n_masks, False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per_pair)
    return float(np.median(ms)), float(np.min(ms))


for dt in (np.dtype(np.uint16), np.dtype(np.float32)):
    if dt == np.uint16:
        tile = torch.randint(0, 4096, (N, N_PX), device='cuda', dtype=torch.int16)
    else:
        tile = torch.rand((N, N_PX), device='cuda')
    for name, csr in stacks():
        n_masks = csr.shape[1]
        out = torch.zeros((N, n_masks), device='cuda')
        for n in (N, 512):
            line = f"{dt.name:8s} {name:15s} {n_masks:6d} masks {n:6d} frames:"
            for switch in ('0', '1'):
                os.environ['LTMI_SPARSE_LABELS'] = switch
                h = hip.MaskHandle.csr(0, csr, np.float32)
                h.set_sig_shape(*SIG)
                med, low = timed(h, tile, dt, out, n, n_masks)
                line += (f"  [labels={switch}] median {med:7.3f} min {low:7.3f} ms"
                         f" {n * N_PX * dt.itemsize / (med * 1e-3) / PEAK:5.3f} of HBM  kind {h.kind()} {h.last_kernel()[:24]}")
                h.close()
            print(line, flush=True)
        del out
    del tile
