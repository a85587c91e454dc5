"""
The executor of a device releases the plans of every scan UDF when it closes (`plans.release_device_plans`): one
context, `run_ssb`, `run_wdd` and `run_parallax` on a 12 x 10 scan each (the fixtures and parameters of
tests/ssb_ref.py, tests/wdd_ref.py and tests/parallax_ref.py), then `close()` -- the three caches are empty and every
plan they held is destroyed.
"""
import numpy as np
import pytest

import parallax_ref as pr
import ssb_ref as sr
import wdd_ref as wr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


def test_executor_close_releases_the_plans_of_every_scan_udf():
    from libertem_amd.api import Context
    from libertem_amd.udf import parallax, run_parallax, run_ssb, run_wdd, ssb, wdd
    assert torch.cuda.is_available()
    nav = (12, 10)
    assert sr.GENERIC_NAV == nav
    caches = (ssb._PLANS, wdd._PLANS, parallax._PLANS)
    c = Context.make_with('hip', gpus=0)
    try:
        generic = c.load('memory', data=sr.generic_frames(), num_partitions=2, sig_dims=2)
        run_ssb(c, generic, **sr.GENERIC)
        run_wdd(c, generic, window=wr.WINDOWS[0], epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)
        run_parallax(c, c.load('memory', data=np.array(pr.counted(nav)), num_partitions=2, sig_dims=2), **pr.PARAMS)
        assert all(len(cache) >= 1 for cache in caches)
        plans = [plan for cache in caches for plan in cache.values()]
        assert all(plan._ptr is not None for plan in plans)
    finally:
        c.close()
    assert not any(caches) and all(plan._ptr is None for plan in plans)
