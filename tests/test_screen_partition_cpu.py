"""
The partition the compaction of a screened best-UCB call runs on (csrc/screen.hpp: screen_partition, the function the kernels
call, exported as gpso_screen_partition_host): workgroup w of G owns a contiguous range of the batch's leaves, and the rank of a
survivor in the compact list is the number of survivors in the ranges in front of its own plus its rank inside -- so the ranges
must cover [0, m) exactly once, in ascending order.  A range is a whole number of 64-leaf steps (one coalesced load per lane),
but for the last non-empty one.  No GPU.
"""
import pytest

from pygpso_amd import HipGPEngine

MS = [1, 63, 64, 65, 16385, 24000, 65536, 2 ** 20]
GS = [1, 7, 64, 256]


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("m", MS)
def test_the_ranges_cover_the_batch_once_in_ascending_order(m, g):
    ranges = HipGPEngine.screen_partition_host(m, g)
    assert len(ranges) == g
    at = 0
    for lo, hi in ranges:
        assert lo == at and lo <= hi <= m  # (contiguous: nothing skipped, nothing twice)
        at = hi
    assert at == m
    full = [(lo, hi) for lo, hi in ranges if hi > lo]
    assert full and all((hi - lo) % 64 == 0 for lo, hi in full[:-1])
    assert len({hi - lo for lo, hi in full[:-1]}) <= 1  # (equal shares)
    assert all(hi == lo == m for lo, hi in ranges[len(full):])  # (the empty ranges stand behind the last leaf)


@pytest.mark.parametrize("m", MS)
def test_the_part_count_of_a_batch(m):
    g = HipGPEngine.screen_parts_host(m)
    assert 1 <= g <= 256 and g == min(256, (m + 255) // 256)
    ranges = HipGPEngine.screen_partition_host(m, g)
    assert ranges[0][0] == 0 and ranges[-1][1] == m
    # at most 256 leaves per wave until the batch outgrows 256 waves
    assert max(hi - lo for lo, hi in ranges) == min(m, max(256, (m + 16383) // 16384 * 64))
