"""
Ground truth and the call helper of the crystallinity kernel tests (tests/test_kernels_gpu.py: the fused kernels of
csrc/ltmi_cryst.hip; tests/test_fft_route_kernels_gpu.py: the hipFFT route of csrc/ltmi_fft.hip).

    intensity[f] = sum( abs(rfft2(frame_f * real_mask)) * half_fourier_mask )

in float64 NumPy (udf/crystallinity.py:47-79 of the reference) through the oracle's mask construction, on frames that
`oracle.corrections.correct` has corrected where corrections apply.
"""
import numpy as np

F32_TOL = 1e-5             # the project's tolerance for float32 results against float64 (north star)
SAME_FRAMES_RTOL = 2e-6    # ... between two conversions of the same frames

# pixel values at the ends of a type's range and around 2^24, where float32 stops holding every integer: planted by
# the tests of the conversion kernels (k_fft_prepare here, k_corr_load in tests/correlation_ref.py)
EXTREMES = {
    'uint32': [2**32 - 1, 2**32 - 2, 2**32 - 129, 2**31, 2**31 + 1, 2**24 + 1, 2**24 + 3, 0],
    'int32': [2**31 - 1, 2**31 - 65, -2**31, -2**31 + 1, 2**24 + 1, -2**24 - 1, 2**30 + 1, -1],
    'float64': [16777217.0, 123456789.123, -98765432.1, 2.0**24 + 3, 1.0 + 2.0**-30, -16777219.0, 0.1, 3e7 + 0.5],
}


def _dev(arr):
    import torch
    if arr.dtype == np.uint16:
        return torch.from_numpy(arr.view(np.int16)).cuda()
    if arr.dtype == np.uint32:
        return torch.from_numpy(arr.view(np.int32)).cuda()
    return torch.from_numpy(arr).cuda()


def _cryst_reference(frames, rad_in, rad_out, real):
    """float64 restatement of udf/crystallinity.py:47-79 through the oracle's mask construction"""
    from libertem_amd.udf.crystallinity import crystallinity_masks
    sig = frames.shape[-2:]
    real_mask, half = crystallinity_masks(sig, rad_in, rad_out, real[0] if real else None,
                                          real[1] if real else None)
    out = np.zeros(len(frames))
    for i, fr in enumerate(frames.astype(np.float64)):
        out[i] = np.sum(abs(np.fft.rfft2(fr * real_mask if real_mask is not None else fr)) * half)
    return out, real_mask, half


def cryst_reference_many(frames, rad_in, rad_out, real, chunk=4096):
    """`_cryst_reference` for thousands of small frames: the same float64 expression, `chunk` frames per rfft2 call"""
    from libertem_amd.udf.crystallinity import crystallinity_masks
    sig = frames.shape[-2:]
    real_mask, half = crystallinity_masks(sig, rad_in, rad_out, real[0] if real else None,
                                          real[1] if real else None)
    out = np.zeros(len(frames))
    for i in range(0, len(frames), chunk):
        fr = frames[i:i + chunk].astype(np.float64)
        if real_mask is not None:
            fr = fr * real_mask
        out[i:i + chunk] = np.sum(np.abs(np.fft.rfft2(fr)) * half, axis=(1, 2))
    return out, real_mask, half


def _cryst_run(hip, frames, real_mask, half, accumulate_into=None, ld_pad=0, batch=64, offset_bytes=0, stream=None,
               tables=None, plan=None, sync=True):
    """One ltmi_crystallinity call on `frames` (n, h, w) -> (out float32 (n), label of the route).

    offset_bytes: the tile pointer is that many bytes past an allocation's (256-byte aligned) start.
    stream: a torch.cuda.Stream the call is enqueued on, after everything already on the current stream.
    tables: CorrectionSet.device_tables(...): the call goes to ltmi_crystallinity_corrected on these raw frames.
    plan: an existing hip.FFTPlan for (h, w), which stays open; without one a plan of `batch` frames lives for the call.
    sync=False: no synchronisation; `out` is then the device tensor (the caller synchronises before reading it)."""
    import torch
    from libertem_amd.udf.crystallinity import mask_box
    n, h, w = frames.shape
    own_plan = plan is None
    if own_plan:
        plan = hip.FFTPlan(0, h, w, batch)
    ld = h * w + ld_pad
    padded = np.zeros((n, ld), dtype=frames.dtype)
    padded[:, :h * w] = frames.reshape(n, -1)
    if offset_bytes:
        raw = np.zeros(padded.nbytes + offset_bytes, dtype=np.uint8)
        raw[offset_bytes:] = padded.reshape(-1).view(np.uint8)
        t = torch.from_numpy(raw).cuda()
        assert t.data_ptr() % 256 == 0
    else:
        t = _dev(padded)
    rm = None if real_mask is None else torch.from_numpy(
        np.ascontiguousarray(real_mask.astype(np.float32))).cuda()
    hm = torch.from_numpy(np.ascontiguousarray(half.astype(np.float32))).cuda()
    out = torch.full((n,), 7.0, dtype=torch.float32, device='cuda') if accumulate_into is None \
        else torch.from_numpy(accumulate_into.astype(np.float32)).cuda()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    args = (None if rm is None else rm.data_ptr(), hm.data_ptr(), mask_box(half), out.data_ptr(),
            accumulate_into is not None)
    if tables is None:
        plan.crystallinity(t.data_ptr() + offset_bytes, frames.dtype, n, ld, *args, stream=stream)
    else:
        plan.crystallinity_corrected(t.data_ptr() + offset_bytes, frames.dtype, n, ld, tables, *args, stream=stream)
    label = plan.last_kernel()
    if not sync:
        assert not own_plan, "sync=False needs a plan that outlives the call"
        return out, label, (t, rm, hm)              # (the inputs stay alive until the caller has synchronised)
    torch.cuda.synchronize()
    if own_plan:
        plan.close()
    return out.cpu().numpy(), label
