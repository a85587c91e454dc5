"""
The arithmetic that the datasets decoded on the GPU share (libertem_amd/io/dataset/decoded.py), without a GPU:
which scan positions a shard holds, which frames of the files land on a block of positions, which positions hold
a frame at all, and the window and partition count of a streamed block -- each against brute force over small
cases.
"""
import itertools

import pytest

from libertem_amd.io.dataset.base import DataSetException
from libertem_amd.io.dataset.decoded import shard_block, source_range, valid_range, stream_window

NAV_SHAPES = [(n,) for n in range(1, 7)] + [(2, 3), (3, 2)]


def n_positions(nav_shape):
    n = 1
    for k in nav_shape:
        n *= k
    return n


def shards_of(nav_shape):
    """(shard argument, positions of the block) of every shard of worlds 1, 2 and 3 that divide the first axis, and
    of no shard at all: rank r of w holds the rows [r * rows / w, (r + 1) * rows / w) of the first axis"""
    positions = list(range(n_positions(nav_shape)))
    per_row = len(positions) // nav_shape[0]
    out = [(None, positions)]
    for world in (1, 2, 3):
        if nav_shape[0] % world == 0:
            rows = nav_shape[0] // world
            for rank in range(world):
                out.append(((rank, world), positions[rank * rows * per_row:(rank + 1) * rows * per_row]))
    return out


@pytest.mark.parametrize('nav_shape', NAV_SHAPES)
def test_shard_block(nav_shape):
    for shard, block in shards_of(nav_shape):
        local_nav, p0, p1 = shard_block(nav_shape, shard)
        assert list(range(p0, p1)) == block
        world = 1 if shard is None else shard[1]
        assert local_nav == (nav_shape[0] // world,) + tuple(nav_shape[1:])
    for world in (2, 3, 4, 5):
        if nav_shape[0] % world:
            with pytest.raises(DataSetException, match=f'first nav axis {nav_shape[0]} does not split over '
                                                       f'{world} ranks'):
                shard_block(nav_shape, (0, world))


@pytest.mark.parametrize('nav_shape', NAV_SHAPES)
def test_valid_range_and_source_range(nav_shape):
    n_nav = n_positions(nav_shape)
    nothing_lands = 0
    for n_frames, so in itertools.product(range(0, 8), range(-6, 7)):
        # frame g of the files sits at scan position g - so
        held = [p for p in range(n_nav) if 0 <= p + so < n_frames]
        valid = valid_range(n_nav, n_frames, so)
        if valid is None:
            assert held == list(range(n_nav))
        else:
            lo, hi = valid
            assert 0 <= lo <= hi <= n_nav and held == list(range(lo, hi)) and held != list(range(n_nav))
        for shard, block in shards_of(nav_shape):
            _, p0, p1 = shard_block(nav_shape, shard)
            g0, g1 = source_range(p0, p1, so, n_frames)
            landing = [g for g in range(n_frames) if g - so in block]
            assert g0 <= g1 and list(range(g0, g1)) == landing, (n_frames, so, shard)
            if so <= -n_nav or so >= n_frames - p0:
                assert landing == []
                nothing_lands += 1
    assert nothing_lands > 0


def test_stream_window_and_partitions():
    cases = itertools.product((1, 3, 8), (100, 128), (0, 399, 4000, 1 << 40), (64, 1000, 1 << 32),
                              (None, 50, 384, 10 ** 6), (None, 1, 2, 5, 100))
    for n_local, frame_bytes, free_bytes, window_bytes, max_resident, num_partitions in cases:
        need = n_local * frame_bytes
        window, n_parts = stream_window(need, frame_bytes, n_local, free_bytes, window_bytes, max_resident,
                                        num_partitions)
        assert window >= frame_bytes
        limits = [window_bytes, free_bytes // 4] + ([] if max_resident is None else [max_resident])
        for limit in limits:
            # (a limit below one frame cannot apply: a partition holds whole frames)
            assert window <= max(limit, frame_bytes)
        assert window in limits + [frame_bytes]
        want = max(num_partitions or 1, -(-need // window))
        assert n_parts == min(want, n_local)
    assert stream_window(0, 128, 0, 1 << 40, 1 << 32, None, None)[1] == 1      # (an empty block: one partition)


def test_stream_window_values_the_gpu_tests_assert():
    free = 280 << 30
    # tests/test_k2is_gpu.py::test_streamed_like_resident: four frames, one may stay
    frame = 1860 * 2048 * 2
    assert stream_window(4 * frame, frame, 4, free, 4 << 30, frame, None) == (frame, 4)
    # tests/test_frms6_gpu.py::test_streamed_like_resident: eight frames of 8 x 8 uint16, three may stay
    assert stream_window(8 * 128, 128, 8, free, 4 << 30, 3 * 128, None) == (3 * 128, 3)
