"""Lists, host side (no GPU): the lane schedule `wrnn_list_plan` states in include/wavernn_amd.h —
longest-processing-time-first over the lanes (XCDs) of `WaveRNN.generate_list`.  The GPU side is
tests/test_gpu_generate_list.py."""
import numpy as np
import pytest

from wavernn_amd import _native as nat
from wavernn_amd.loop import list_plan


def _rule(frames, lanes):
    """The rule as the header states it: by decreasing length (ties: lower index first), each to
    the lane with the smallest load so far (ties: lowest lane), run in the order assigned."""
    load, count = [0] * lanes, [0] * lanes
    lane_of, pos = [None] * len(frames), [None] * len(frames)
    for i in sorted(range(len(frames)), key=lambda i: (-frames[i], i)):
        k = min(range(lanes), key=lambda k: (load[k], k))
        lane_of[i], pos[i] = k, count[k]
        load[k] += frames[i]
        count[k] += 1
    return lane_of, pos, load


@pytest.mark.parametrize("lanes", range(1, 9))
def test_plan_equals_the_stated_rule(lanes):
    rng = np.random.default_rng(lanes)
    for U in range(1, 41):
        # few distinct lengths: ties among utterances and among lane loads are the normal case
        frames = [int(f) for f in rng.integers(21, 21 + (4 if U % 2 else 400), U)]
        got = list_plan(frames, lanes)
        assert got == _rule(frames, lanes), (U, lanes, frames)
        lane_of, pos, load = got
        # every utterance exactly once: the (lane, position) pairs are the lanes' queues, no gaps
        assert sorted(zip(lane_of, pos)) == [(k, p) for k in range(lanes) for p in range(lane_of.count(k))]
        assert sum(load) == sum(frames)
        assert all(load[k] == sum(f for f, l in zip(frames, lane_of) if l == k) for k in range(lanes))
        # the list-scheduling bound (Graham): no lane ends later than the mean plus (1 − 1/m) of the longest job
        assert max(load) <= sum(frames) / lanes + (1 - 1 / lanes) * max(frames) + 1e-9
        # within a lane the utterances run longest first (the order they were assigned)
        for k in range(lanes):
            q = sorted((p, -frames[i], i) for i, (l, p) in enumerate(zip(lane_of, pos)) if l == k)
            assert q == sorted(q, key=lambda e: (e[1], e[2]))


def test_plan_is_stable_under_ties():
    # all equal: utterance i goes round the lanes in index order
    lane_of, pos, load = list_plan([30] * 11, 4)
    assert lane_of == [i % 4 for i in range(11)] and pos == [i // 4 for i in range(11)]
    assert load == [90, 90, 90, 60]
    # equal lengths keep their index order, equal loads take the lowest lane
    assert list_plan([21, 40, 21, 40], 2) == ([0, 0, 1, 1], [1, 0, 1, 0], [61, 61])
    assert list_plan([25, 25, 50], 3)[0] == [1, 2, 0]
    # the default lane count: min(8, U)
    assert len(list_plan([21] * 3)[2]) == 3 and len(list_plan([21] * 20)[2]) == 8
    # the same call twice gives the same schedule
    fr = [33, 21, 33, 47, 21, 47, 33]
    assert list_plan(fr, 3) == list_plan(fr, 3)


@pytest.mark.parametrize("frames,lanes", [([], 1), ([30, 30], 0), ([30, 30], 9), ([30, 20, 30], 2), ([21, 0], 2),
                                          ([-5], 1)])
def test_plan_refusals(frames, lanes):
    with pytest.raises(nat.WrnnError) as e:
        list_plan(frames, lanes)
    assert e.value.code == -1   # WRNN_EINVAL
