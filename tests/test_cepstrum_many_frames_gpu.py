"""
The cepstrum kernels at a frame count beyond what the 65535 rows of a grid hold: both kernels give a grid row four
frames to walk, so 270 000 frames in ONE launch leave 7860 rows a fifth frame, beyond 4 x 65535 = 262 140
(tests/test_cepstrum_kernels_gpu.py stays at 7 frames).

    a  ceps_store              270 000 half spectra (8, 5) -> (4, 4)     bit for bit against the NumPy float32 model
    b  ceps_load               270 000 x 64 and x 63 uint8 pixels         within 3 eps32 (1 + |z|) |window|, both paths
    c  CepstrumPlan.transform  270 000 x (8, 8) uint8 -> (4, 4), one batch within the bound of tests/cepstrum_ref.py

The tiles are drawn from a pool of 7 distinct members by a seeded index, so that the host side stays cheap: the
reference is computed for the pool once and indexed.  No frame is left out of the comparison.
"""
import numpy as np
import pytest

import cepstrum_ref as cr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N = 270000
ROWS = 65535
POOL = 7
CASE = ((8, 8), (4, 4))


@pytest.fixture(scope='module')
def index():
    idx = np.random.default_rng(70).integers(0, POOL, N)
    idx[[0, ROWS - 1, ROWS, ROWS + 1, 4 * ROWS - 1, 4 * ROWS, N - 1]] = (0, 1, 2, 3, 4, 5, 6)     # (around the limits)
    return idx


def test_a_store_every_round_of_the_frame_loop(index):
    from libertem_amd import hip
    (h, w), (oh, ow) = CASE
    rng = np.random.default_rng(71)
    pool = (rng.normal(size=(POOL, h, w // 2 + 1)) + 1j * rng.normal(size=(POOL, h, w // 2 + 1))).astype(np.complex64)
    scale_host = (rng.uniform(0.25, 1.0, (oh, ow)) / (h * w)).astype(np.float32)
    spec = torch.from_numpy(pool[index].view(np.float32).reshape(N, -1)).cuda()
    scale = torch.from_numpy(scale_host).cuda()
    out = torch.full((N, oh * ow), np.nan, dtype=torch.float32, device='cuda')
    hip.ceps_store(0, spec.data_ptr(), N, h, w, h * (w // 2 + 1), oh, ow, scale.data_ptr(), out.data_ptr(), oh * ow)
    torch.cuda.synchronize()
    ref = cr.store(pool, (h, w), (oh, ow), scale_host)[index]
    assert out.cpu().numpy().reshape(ref.shape).tobytes() == ref.tobytes()


@pytest.mark.parametrize('n_px', [64, 63], ids=['four-pixels-per-thread', 'one-pixel-per-thread'])
def test_b_load_every_round_of_the_frame_loop(index, n_px):
    from libertem_amd import hip
    rng = np.random.default_rng(72)
    pool = rng.integers(0, 255, (POOL, n_px), endpoint=True).astype(np.uint8)
    window_host = rng.uniform(0.25, 1.0, n_px).astype(np.float32)
    tile = torch.from_numpy(pool[index]).cuda()
    window = torch.from_numpy(window_host).cuda()
    out = torch.full((N, n_px), np.nan, dtype=torch.float32, device='cuda')
    hip.ceps_load(0, tile.data_ptr(), np.uint8, N, n_px, n_px, 0.5, window.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    z = cr.log_frames(pool, 0.5)
    ref = (z * window_host.astype(np.float64))[index]
    tol = (3 * cr.EPS32 * (1 + np.abs(z)) * window_host.astype(np.float64))[index]
    got = out.cpu().numpy()
    assert np.all(np.abs(got - ref) <= tol)
    # the frames of the later rounds of the loop are those of the pool, like the ones of the first round
    assert got[ROWS:].tobytes() == got[:ROWS][_first_of(index)][index[ROWS:]].tobytes()


def _first_of(index):
    """for every pool member, the first frame of the first round that holds it"""
    return np.array([int(np.flatnonzero(index[:ROWS] == m)[0]) for m in range(POOL)])


def test_c_plan_one_batch_of_270000(index):
    from libertem_amd import hip
    (h, w), (oh, ow) = CASE
    pool = cr.noise_frames((h, w), POOL, 'uint8', seed=73)
    window = cr.window_for(CASE)
    plan = hip.CepstrumPlan(0, h, w, oh, ow, N, 0.75, window, 1.5)
    tile = torch.from_numpy(pool[index].reshape(N, h * w)).cuda()
    out = torch.full((N, oh * ow), np.nan, dtype=torch.float32, device='cuda')
    plan.transform(tile.data_ptr(), np.uint8, N, h * w, out.data_ptr(), oh * ow)
    torch.cuda.synchronize()
    assert plan.last_kernel() == f'k_ceps_load<uint8> + hipfft_r2c + k_ceps_store batch={N}'
    plan.close()
    got = out.cpu().numpy().reshape((N, oh, ow))
    ref = cr.reference(pool, (oh, ow), 0.75, window, 1.5)
    bound = cr.bound(pool, 0.75, window)
    err = np.sqrt(((got.astype(np.float64) - ref[index]) ** 2).reshape((N, -1)).sum(axis=1))
    print(f"cepstrum 270000 frames: largest |dev - ref|_2 / bound = {(err / bound[index]).max():.5f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound[index])
