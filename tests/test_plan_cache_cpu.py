"""
`libertem_amd.udf.plans` on fake plans (objects whose `close()` sets `_ptr = None`, as `hip._NativePlan.close` does):
one `make` per key; what a full cache does with its plans, by `owned`; `release` by device; `release_device_plans`
over the owned caches only; the caches of the real modules.  And the class declarations of the whole-frame UDFs.
"""
import numpy as np
import pytest

import parallax_ref as pr
import ssb_ref as sr
import wdd_ref as wr
from libertem_amd.udf import plans
from libertem_amd.udf.plans import PlanCache, array_digest, release_device_plans


class FakePlan:
    def __init__(self):
        self._ptr = 1

    def close(self):
        self._ptr = None


@pytest.fixture
def registry():
    """the caches made in a test leave the registry of owned caches again"""
    before = list(plans._OWNED)
    yield plans._OWNED
    plans._OWNED[:] = before


def test_get_or_make_calls_make_once_per_key(registry):
    cache = PlanCache(4, owned=False)
    made = []

    def make():
        made.append(FakePlan())
        return made[-1]

    a = cache.get_or_make((0, 8, 8), make)
    assert cache.get_or_make((0, 8, 8), make) is a and len(made) == 1
    b = cache.get_or_make((1, 8, 8), make)
    assert b is not a and len(made) == 2 and cache.get_or_make((1, 8, 8), make) is b and len(made) == 2
    assert isinstance(cache, dict) and len(cache) == 2 and list(cache.values()) == [a, b]
    assert [key[1:3] for key, _ in cache.items()] == [(8, 8), (8, 8)]


def test_a_full_cache_that_does_not_own_its_plans_drops_them_open(registry):
    cache = PlanCache(2, owned=False)
    held = [cache.get_or_make((0, i), FakePlan) for i in range(2)]
    assert len(cache) == 2
    third = cache.get_or_make((0, 2), FakePlan)
    assert list(cache.items()) == [((0, 2), third)]
    assert all(p._ptr is not None for p in held + [third])
    assert cache not in registry


def test_a_full_cache_that_owns_its_plans_closes_them(registry):
    cache = PlanCache(2, owned=True)
    held = [cache.get_or_make((0, i), FakePlan) for i in range(2)]
    assert cache.get_or_make((0, 1), FakePlan) is held[1] and all(p._ptr is not None for p in held)
    third = cache.get_or_make((1, 2), FakePlan)
    assert list(cache.items()) == [((1, 2), third)]
    assert all(p._ptr is None for p in held) and third._ptr is not None
    assert cache in registry


def test_release_closes_and_removes_the_plans_of_one_device(registry):
    cache = PlanCache(8, owned=True)
    on0 = [cache.get_or_make((0, i), FakePlan) for i in range(2)]
    on1 = [cache.get_or_make((1, i), FakePlan) for i in range(2)]
    cache.release(0)
    assert sorted(cache) == [(1, 0), (1, 1)]
    assert all(p._ptr is None for p in on0) and all(p._ptr is not None for p in on1)
    cache.release()
    assert not cache and all(p._ptr is None for p in on1)


def test_release_device_plans_reaches_the_owned_caches_only(registry):
    owned = [PlanCache(2, owned=True) for _ in range(2)]
    shared = PlanCache(8, owned=False)
    held = [[cache.get_or_make((d, 0), FakePlan) for d in (0, 1)] for cache in owned + [shared]]
    release_device_plans(0)
    for cache, (on0, on1) in zip(owned, held):
        assert list(cache) == [(1, 0)] and on0._ptr is None and on1._ptr is not None
    assert len(shared) == 2 and all(p._ptr is not None for p in held[2])


def test_array_digest_separates_and_skips():
    a, b = np.arange(4, dtype=np.float32), np.arange(4, 8, dtype=np.float32)
    assert array_digest(a, b) == array_digest(a.copy(), b.copy())
    assert array_digest(a, b) != array_digest(np.concatenate([a, b]))
    assert array_digest(a, b) != array_digest(b, a)
    assert array_digest(a, None) == array_digest(a) != array_digest(None, a)
    assert array_digest(a) != array_digest(a + 1)


def test_the_caches_of_the_modules():
    from libertem_amd.udf import cepstrum, correlation, crystallinity, holography, orientation, parallax, ssb, wdd
    frame = [m._PLANS for m in (crystallinity, correlation, holography, cepstrum, orientation)]
    scan = [m._PLANS for m in (ssb, wdd, parallax)]
    assert all(type(c) is PlanCache for c in frame + scan)
    assert [c.capacity for c in frame + scan] == [8, 8, 8, 8, 8, 2, 2, 2]
    assert [c.owned for c in frame + scan] == [False] * 5 + [True] * 3
    assert all(any(c is o for o in plans._OWNED) for c in scan)
    assert not any(c is o for c in frame for o in plans._OWNED)
    assert correlation.CORR_WORKSPACE_BYTES is plans.CORR_WORKSPACE_BYTES == 512 * 2**20


def _udfs():
    from libertem_amd.udf import (
        CepstrumUDF, CorrelationUDF, EventCountUDF, HoloReconstructUDF, LatticeRefineUDF, OrientationMatchUDF,
        ParallaxUDF, PeakFindUDF, SSBUDF, WDDUDF,
    )
    from libertem_amd.udf.counting import _CountingUDF
    from libertem_amd.udf.ssb import ScanPixelsUDF
    template = np.ones((8, 8), np.float32)
    return [
        CorrelationUDF(peaks=[[4, 4]], template=template, crop_radius=1),
        LatticeRefineUDF(indices=[[0, 0]], zero=(4, 4), a=(2, 0), b=(0, 2), template=template, crop_radius=1),
        PeakFindUDF(template=template, num_peaks=1, min_distance=1),
        HoloReconstructUDF(out_shape=(4, 4), sb_position=(2, 2), sb_size=1.0),
        CepstrumUDF(out_shape=(4, 4)),
        OrientationMatchUDF(library=None, center=(4., 4.), n_r=2, n_phi=4),
        _CountingUDF(),
        EventCountUDF(background_threshold=1.0),
        ScanPixelsUDF(),
        SSBUDF(**sr.GENERIC),
        WDDUDF(window=wr.WINDOWS[0], epsilon=wr.GENERIC_EPSILON, **wr.GENERIC),
        ParallaxUDF(**pr.PARAMS),
    ]


@pytest.mark.parametrize('udf', _udfs(), ids=lambda u: type(u).__name__)
def test_whole_frame_declarations(udf):
    from libertem_amd.udf.device import WholeFrameUDF
    assert isinstance(udf, WholeFrameUDF)
    assert udf.REUSE_TASK_INSTANCES is True and udf.VALID_FRAMES_ONLY is True and udf.WHOLE_FRAME_TILES is True
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert type(udf).process_tile is WholeFrameUDF.process_tile or type(udf).__name__ in ('CorrelationUDF',
                                                                                         'LatticeRefineUDF')


def test_the_scan_udfs_are_siblings():
    from libertem_amd.udf import ParallaxUDF, SSBUDF, WDDUDF
    from libertem_amd.udf.ssb import ScanPixelsUDF
    for cls in (SSBUDF, WDDUDF, ParallaxUDF):
        assert issubclass(cls, ScanPixelsUDF) and cls.__init__ is not ScanPixelsUDF.__init__
    assert not issubclass(WDDUDF, SSBUDF) and not issubclass(ParallaxUDF, SSBUDF)
