"""
`ltmi_wsum_workspace` and the argument checks of `ltmi_wsum_frames` that need no device: the refusals come before
the library touches a GPU.  The workspace cap of DESIGN.md section 4.6k is checked for the shapes the kernel tests
use and for the largest call the operator is specified for.
"""
import ctypes

import numpy as np
import pytest

from libertem_amd import hip

CAP = 256 << 20                       # bytes: or one slab, 4 k n_px, if that is more

# (n_frames, n_px, k) of tests/test_wsum_kernels_gpu.py
KERNEL_TEST_SHAPES = [(n, p, k) for n in (1, 7, 33, 1000, 8192) for p in (256, 3 * 515) for k in (1, 3, 16, 17, 64)]


@pytest.fixture(scope='module')
def lib():
    return hip.lib()


def test_workspace_is_whole_slabs_under_the_cap(lib):
    for n, p, k in KERNEL_TEST_SHAPES + [(65536, 65536, 64), (65536, 65536, 16), (100, 1 << 24, 64)]:
        nbytes = hip.wsum_workspace(n, p, k)
        slab = 4 * k * p
        assert nbytes > 0 and nbytes % slab == 0, (n, p, k)
        assert 1 <= nbytes // slab <= 256, (n, p, k)
        assert nbytes <= max(CAP, slab), (n, p, k)
    # the largest call of the specification: 64 components of 65 536 pixels over 65 536 frames
    assert hip.wsum_workspace(65536, 65536, 64) == CAP
    # one slab when even that is above the cap
    assert hip.wsum_workspace(100, 1 << 24, 64) == 4 * 64 * (1 << 24)


def test_workspace_slabs_keep_chains_short_and_partials_small(lib):
    # chains of at most 4096 frames while the cap allows: 65 536 frames of 256 pixels in 16 slabs or more
    assert hip.wsum_workspace(65536, 256, 16) // (4 * 16 * 256) >= 16
    # a slab holds at least max(32, 16 k) frames: the partials stay small next to the frames read
    for n, p, k in KERNEL_TEST_SHAPES:
        slabs = hip.wsum_workspace(n, p, k) // (4 * k * p)
        assert slabs == 1 or n // slabs >= max(32, 16 * k) - 4, (n, p, k)
    assert hip.wsum_workspace(1000, 1545, 17) // (4 * 17 * 1545) == 3
    assert hip.wsum_workspace(8192, 256, 1) // (4 * 256) == 256


def test_workspace_of_refused_shapes_is_zero(lib):
    for n, p, k in [(0, 256, 4), (-1, 256, 4), (8, 0, 4), (8, 256, 0), (8, 256, 65), (8, 256, -3)]:
        assert hip.wsum_workspace(n, p, k) == 0, (n, p, k)


def _call(lib, tile_dtype=np.uint16, n_frames=4, n_px=12, ld_tile=12, k=2, ld_w=2, cols=12, ld_out=12,
          comp_stride=12, tile=1, weights=1, out=1, workspace=1):
    """with fake non-null pointers: every call here must be refused (or be a no-op) before anything is read"""
    fake = ctypes.c_void_p(4096)
    ptr = lambda on: fake if on else None                              # noqa: E731
    return lib.ltmi_wsum_frames(0, ptr(tile), hip.dtype_code(tile_dtype), n_frames, n_px, ld_tile, ptr(weights), k,
                                ld_w, ptr(out), cols, ld_out, comp_stride, 0, ptr(workspace), None)


def test_argument_checks_without_a_device(lib):
    E_INVALID, E_DTYPE, E_SHAPE = -1, -2, -3
    for k in (0, 65, -1, 1000):
        assert _call(lib, k=k, ld_w=max(k, 1)) == E_SHAPE
        assert f"k = {k} " in lib.ltmi_last_error().decode()
    assert _call(lib, ld_w=1) == E_SHAPE                               # ld_w < k
    assert _call(lib, ld_tile=11) == E_SHAPE                           # ld_tile < n_px
    assert _call(lib, n_frames=-1) == E_SHAPE
    assert _call(lib, cols=5) == E_SHAPE                               # cols does not divide n_px
    assert _call(lib, cols=6, ld_out=5) == E_SHAPE                     # ld_out < cols
    assert _call(lib, cols=6, ld_out=8, comp_stride=13) == E_SHAPE     # two rows at stride 8 need 14 elements
    for dt in (np.float64, np.complex64, np.complex128, np.int64, np.uint64):
        assert _call(lib, tile_dtype=dt) == E_DTYPE
        assert str(np.dtype(dt)) in lib.ltmi_last_error().decode()
    for missing in ('tile', 'weights', 'out', 'workspace'):
        assert _call(lib, **{missing: 0}) == E_INVALID
    # no frames, no pixels: nothing to do, whatever the pointers
    assert _call(lib, n_frames=0, tile=0, weights=0, out=0, workspace=0) == 0
    assert _call(lib, n_px=0, ld_tile=0, cols=0, ld_out=0, comp_stride=0, tile=0, out=0) == 0


def test_python_binding_raises_value_error(lib):
    with pytest.raises(ValueError, match='k = 65'):
        hip.wsum_frames(0, 4096, np.uint16, 4, 12, 12, 4096, 65, 65, 4096, 12, False, 4096, stream=0)
    with pytest.raises(ValueError, match='float64'):
        hip.wsum_frames(0, 4096, np.float64, 4, 12, 12, 4096, 2, 2, 4096, 12, False, 4096, stream=0)
    assert hip.WSUM_MAX_K == 64
