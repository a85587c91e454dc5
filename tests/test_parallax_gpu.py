"""
ParallaxUDF on the MI355X (Context.make_with('hip')) against the index-by-index float64 restatement
(tests/parallax_ref.py): both scans of the fixture (12 x 10 and 9 x 16, integer frames at 150 counts) through
`run_parallax`, a plain `run_udf` (the bright-field pixels come to the host, NumPy reconstructs) and
`result_where='device'` (the native plan); uint16, uint8 and float32 datasets, host and device-resident; 1 and 3
partitions; `regularize` on and off; the bright-field pixels kept on the device; a second run on the cached plan;
`release_plans`; the parameter errors on the device.

Tolerance of the device against the restatement.  The device transforms in float32, the restatement is float64
throughout.  Measured once on the MI355X on these fixtures (MEASURED, the largest over both scans, the three routes
to the plan, and `regularize` on and off): shifts 1.98e-7 scan pixels, matrix 1.09e-8, offset 2.96e-8, image 6.55e-8
and bright field 6.71e-8 of the largest value (the last two are the cast of the result to float32).  Every dataset
dtype, resident or streamed, and every partition count gave the same figures.  The bounds are 4 x these figures, which
leaves room for other seeds and hipFFT versions; the integer part of every shift is the restatement's (the fixture has
no near-ties: tests/test_parallax_cpu.py).  The NumPy route is float64 and is held to 1e-9, as on the CPU.
"""
import numpy as np
import pytest

import parallax_ref as pr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAV_IDS = ['12x10', '9x16']
FLOAT = ('shifts', 'matrix', 'offset')
IMAGES = ('image', 'bright_field')
# the largest deviation of the plan from the restatement seen on the MI355X (module docstring)
MEASURED = {'shifts': 1.98e-7, 'matrix': 1.09e-8, 'offset': 2.96e-8, 'image': 6.55e-8, 'bright_field': 6.71e-8}


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


def arrays(res):
    return {k: np.asarray(res[k].data if hasattr(res[k], 'data') and not isinstance(res[k], np.ndarray) else res[k])
            for k in FLOAT + IMAGES}


def check(res, ref, what, regularize=False, float64=False):
    """a dict of result arrays (or buffers) against the restatement"""
    a = arrays(res)
    assert all(a[k].dtype == np.float64 for k in FLOAT) and all(a[k].dtype == np.float32 for k in IMAGES)
    assert a['shifts'].shape == (pr.N_BF, 2) and a['matrix'].shape == (2, 2) and a['offset'].shape == (2,)
    err = pr.errors(a, ref)
    print(f"{what}: " + ' '.join(f"{k} {v:.3e}" for k, v in err.items()))
    if not regularize:
        assert pr.same_integer_parts(a, ref), what
    for name, e in err.items():
        if float64 and name in FLOAT:
            assert e <= 1e-9 * np.abs(ref[name]).max(), (what, name, e)
        elif float64:
            assert e <= 1e-7, (what, name, e)                      # (the cast of the images to float32)
        else:
            assert e <= 4 * MEASURED[name], (what, name, e)
    return err


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8', 'float32'])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_run_parallax(ctx, nav, dtype, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_parallax
    frames = pr.counted(nav)
    data = frames.astype(dtype)
    assert np.array_equal(data.astype(np.uint16), frames)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=3, sig_dims=2)
    out = run_parallax(ctx, ds, **pr.PARAMS)
    assert set(out) == set(FLOAT + IMAGES)
    assert out['image'].shape == nav and out['bright_field'].shape == nav
    check(out, pr.reference_of('counted', nav), f"run_parallax {nav} {dtype}")


@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_regularize_and_keep_bf(ctx, nav):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_parallax
    from libertem_amd.udf.ssb import bf_pixels
    frames = np.array(pr.counted(nav))
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    out = run_parallax(ctx, ds, regularize=True, keep_bf=True, **pr.PARAMS)
    assert isinstance(out['bf'], HipArray) and out['bf'].dtype == np.float32
    idx = bf_pixels(pr.SIG, pr.SEMICONV_PIX, pr.CY, pr.CX)
    n = nav[0] * nav[1]
    assert np.array_equal(out['bf'].cpu().reshape(n, pr.N_BF), frames.reshape(n, -1)[:, idx].astype(np.float32))
    check(out, pr.reference_of('counted', nav, True), f"run_parallax {nav} regularize", regularize=True)
    # the regularized shifts are their own affine fit
    offsets = np.array([(y - pr.CY, x - pr.CX) for y, x in pr.pixels()])
    assert np.abs(out['shifts'] - (offsets @ out['matrix'].T + out['offset'])).max() < 1e-12


@pytest.mark.parametrize('num_partitions', [1, 3])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_plain_run_udf_and_result_on_device(ctx, nav, num_partitions):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import ParallaxUDF
    from libertem_amd.udf import parallax
    frames = np.array(pr.counted(nav))
    ref = pr.reference_of('counted', nav)
    ds = ctx.load('memory', data=frames, num_partitions=num_partitions, sig_dims=2)
    udf = ParallaxUDF(**pr.PARAMS)
    host = ctx.run_udf(dataset=ds, udf=udf)                    # bf comes to the host, NumPy reconstructs
    check(host, ref, f"run_udf {nav}", float64=True)
    direct = parallax.parallax_bf(host['bf'].data.reshape(nav[0] * nav[1], pr.N_BF), nav, pr.SIG, **pr.PARAMS)
    assert host['shifts'].data.tobytes() == direct['shifts'].tobytes()
    assert host['image'].data.tobytes() == direct['image'].tobytes()
    dev = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert isinstance(dev['bf'].device_data, HipArray)
    check(dev, ref, f"result_where='device' {nav}")
    # the same UDF again: the cached plan, the same bytes
    n_plans = len(parallax._PLANS)
    again = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert len(parallax._PLANS) == n_plans
    for name in FLOAT + IMAGES:
        assert again[name].data.tobytes() == dev[name].data.tobytes(), name
    plans = [p for key, p in parallax._PLANS.items() if key[1:3] == nav]
    assert plans and all(p.last_kernel() == 'k_plx_ramps + k_plx_sum + k_plx_herm' for p in plans)
    assert all(p.max_batch == pr.N_BF and p.max_shift == pr.MAX_SHIFT for p in plans)
    # the plans go with their executor (HipJobExecutor.close calls this); the next run makes a new one
    parallax.release_plans(0)
    assert not parallax._PLANS and all(p._ptr is None for p in plans)
    fresh = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert fresh['shifts'].data.tobytes() == dev['shifts'].data.tobytes() and len(parallax._PLANS) == 1
    assert fresh['image'].data.tobytes() == dev['image'].data.tobytes()


def test_regularize_on_device_matches_the_restatement(ctx):
    from libertem_amd.udf import ParallaxUDF
    nav = (9, 16)
    ds = ctx.load('memory', data=np.array(pr.counted(nav)), num_partitions=3, sig_dims=2)
    udf = ParallaxUDF(regularize=True, **pr.PARAMS)
    ref = pr.reference_of('counted', nav, True)
    check(ctx.run_udf(dataset=ds, udf=udf), ref, 'regularize run_udf', regularize=True, float64=True)
    check(ctx.run_udf(dataset=ds, udf=udf, result_where='device'), ref, 'regularize device', regularize=True)


def test_executor_close_releases_the_plans():
    from libertem_amd.api import Context
    from libertem_amd.udf import parallax, run_parallax
    nav = (12, 10)
    c = Context.make_with('hip', gpus=0)
    try:
        run_parallax(c, c.load('memory', data=np.array(pr.counted(nav)), num_partitions=1, sig_dims=2), **pr.PARAMS)
        plans = list(parallax._PLANS.values())
        assert plans
    finally:
        c.close()
    assert not parallax._PLANS and all(p._ptr is None for p in plans)


def test_errors_on_device(ctx):
    from libertem_amd.udf import ParallaxUDF, run_parallax
    nav = (12, 10)
    frames = np.array(pr.counted(nav))
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    roi = np.zeros(nav, bool)
    roi[1] = True
    with pytest.raises(ValueError, match='roi'):
        ctx.run_udf(dataset=ds, udf=ParallaxUDF(**pr.PARAMS), roi=roi)
    with pytest.raises(ValueError, match='P = 0'):
        run_parallax(ctx, ds, **dict(pr.PARAMS, cx=-30.))
    with pytest.raises(ValueError, match=r'2 \* max_shift \+ 1 = 11'):
        run_parallax(ctx, ds, **dict(pr.PARAMS, max_shift=5))
    with pytest.raises(ValueError, match='max_shift 0'):
        run_parallax(ctx, ds, **dict(pr.PARAMS, max_shift=0))
    with pytest.raises(ValueError, match='iterations'):
        run_parallax(ctx, ds, **dict(pr.PARAMS, iterations=0))
    sliced = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, tileshape=(7, 4, 14))
    with pytest.raises(ValueError, match='whole frames'):
        run_parallax(ctx, sliced, **pr.PARAMS)
    # the context still works
    check(run_parallax(ctx, ds, **pr.PARAMS), pr.reference_of('counted', nav), 'after the errors')
