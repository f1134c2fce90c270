"""Wide lists, host side (no GPU): the schedule `wrnn_list_wide_plan` states in include/wavernn_amd.h —
wrnn_list_plan's assignment over up to 128 many-row slots, the common timeline cut at every utterance
end on any slot and again at the WRNN_TERMS_MB budget (wrnn_wide_steps_per_launch), the rows of a
launch the slots that still have a step to run.  The GPU side is tests/test_gpu_list_wide.py."""
import os
import re

import numpy as np
import pytest

from tests import geometries as geo
from wavernn_amd import _native as nat
from wavernn_amd.loop import list_plan, list_wide_plan, wide_steps_per_launch

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wavernn_amd.h")
N_MOL, N_RAW = 32 * 144, 32 * 144 + 512


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("WRNN_TERMS_MB", raising=False)


def _rule(frames, slots):
    """The assignment as the header states it (tests/test_list_plan.py restates the same rule)."""
    load, count = [0] * slots, [0] * slots
    slot_of, pos = [None] * len(frames), [None] * len(frames)
    for i in sorted(range(len(frames)), key=lambda i: (-frames[i], i)):
        k = min(range(slots), key=lambda k: (load[k], k))
        slot_of[i], pos[i] = k, count[k]
        load[k] += frames[i]
        count[k] += 1
    return slot_of, pos, load


def _frames(rng, U, spread):
    return [int(f) for f in rng.integers(21, 21 + spread, U)]


def _check_plan(frames, slots, hop, raw):
    """Every property of the schedule for one call; → the launches."""
    slot_of, pos, slot_frames, launches = list_wide_plan(frames, slots, hop=hop, raw=raw)
    U = len(frames)
    assert (slot_of, pos, slot_frames) == _rule(frames, slots)
    # every slot's utterances tile its timeline: in queue order, end to end, from 0 to slot_frames · hop
    ends = set()
    for k in range(slots):
        t = 0
        for i in sorted((i for i in range(U) if slot_of[i] == k), key=lambda i: pos[i]):
            t += frames[i] * hop
            ends.add(t)
        assert t == slot_frames[k] * hop
    longest = max(slot_frames) * hop
    # the launches tile [0, longest timeline)
    t = 0
    for first, steps, rows in launches:
        assert first == t and steps >= 1
        t += steps
    assert t == longest
    # every utterance end on any slot is a launch boundary
    bounds = {first for first, _, _ in launches} | {longest}
    assert ends <= bounds, sorted(ends - bounds)[:5]
    prev_rows = None
    for first, steps, rows in launches:
        # the rows: the slots with a step left at the launch's first step — and until its last one
        live = sum(slot_frames[k] * hop > first for k in range(slots))
        assert rows == live == sum(slot_frames[k] * hop >= first + steps for k in range(slots))
        assert 1 <= rows <= min(slots, U)
        assert prev_rows is None or rows <= prev_rows
        prev_rows = rows
        # no launch exceeds the budget for its row count; one that ends off an utterance end fills it
        cap = wide_steps_per_launch(rows, longest, raw=raw)
        assert steps <= cap
        if first + steps not in ends:
            assert steps == cap
    return launches


@pytest.mark.parametrize("slots", [1, 2, 3, 5, 8])
def test_assignment_equals_list_plan_up_to_eight_slots(slots):
    rng = np.random.default_rng(slots)
    for U in range(1, 30):
        frames = _frames(rng, U, 4 if U % 2 else 400)
        slot_of, pos, slot_frames, _ = list_wide_plan(frames, slots, hop=12)
        assert (slot_of, pos, slot_frames) == list_plan(frames, slots), (U, slots, frames)


def test_lpt_order_and_tie_breaks_at_128_slots():
    # 300 utterances of few distinct lengths: ties among utterances and among slot loads
    rng = np.random.default_rng(128)
    frames = _frames(rng, 300, 6)
    slot_of, pos, load, _ = list_wide_plan(frames, 128, hop=4)
    assert (slot_of, pos, load) == _rule(frames, 128)
    # all equal: utterance i goes round the slots in index order
    slot_of, pos, load, launches = list_wide_plan([30] * 140, 128, hop=4)
    assert slot_of == [i % 128 for i in range(140)] and pos == [i // 128 for i in range(140)]
    assert load == [60] * 12 + [30] * 116
    assert launches == [(0, 120, 128), (120, 120, 12)]
    # the default slot count: min(128, U)
    assert len(list_wide_plan([21] * 3, hop=4)[2]) == 3 and len(list_wide_plan([21] * 200, hop=4)[2]) == 128
    # within a slot the utterances run longest first
    frames = _frames(rng, 400, 300)
    slot_of, pos, _, _ = list_wide_plan(frames, 128, hop=4)
    for k in range(128):
        q = [frames[i] for i in sorted((i for i in range(400) if slot_of[i] == k), key=lambda i: pos[i])]
        assert q == sorted(q, reverse=True)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("slots, U, hop", [(1, 5, 12), (3, 11, 12), (7, 40, 4), (128, 140, 4), (128, 512, 275), (16, 16, 4)])
def test_launches_default_budget(slots, U, hop, raw):
    rng = np.random.default_rng(U)
    frames = [24] * U if slots == U else _frames(rng, U, 25 if hop < 275 else 300)
    launches = _check_plan(frames, slots, hop, raw)
    if hop == 275:      # 128 rows take 3 639 (MoL) / 3 275 (RAW) steps of the default 8192 MiB: the budget cuts too
        assert max(s for _, s, _ in launches) == wide_steps_per_launch(128, 10 ** 9, raw=raw)
        return
    # the default budget cuts nothing at these lengths: one launch per distinct utterance end
    slot_of, pos, _, _ = list_wide_plan(frames, slots, hop=hop)
    ends = set()
    for k in range(slots):
        t = 0
        for i in sorted((i for i in range(U) if slot_of[i] == k), key=lambda i: pos[i]):
            t += frames[i] * hop
            ends.add(t)
    assert len(launches) == len(ends)
    if slots == U:      # equal lengths: every slot ends at once, one launch, rows from U to none
        assert launches == [(0, 24 * hop, U)]


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("steps", [1, 77])
def test_launches_under_a_small_budget(monkeypatch, steps, raw):
    """WRNN_TERMS_MB that gives 9 rows exactly `steps` steps per launch (1: every launch one step), and
    fewer rows proportionally more: the budget is per launch, by its own row count."""
    frames = [30, 21, 26, 30, 23, 28, 21, 25, 22]
    rec = N_RAW if raw else N_MOL
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 9, rec))
    assert wide_steps_per_launch(9, 10 ** 6, raw=raw) == steps
    launches = _check_plan(frames, 9, 12, raw)
    assert launches[0] == (0, steps, 9)
    if steps == 1:
        assert sum(s == 1 for _, s, _ in launches) >= 21 * 12
    assert len({r for _, _, r in launches}) >= 5          # rows fall as slots end
    launches3 = _check_plan(frames, 3, 12, raw)            # 3 slots: a third of the rows, three times the floats each
    assert launches3[0] == (0, int((steps + 1.5) * 3 - 1), 3)
    monkeypatch.setenv("WRNN_TERMS_MB", "0.0001")
    one = _check_plan(frames, 4, 12, raw)
    assert all(s == 1 for _, s, _ in one)


def test_the_budget_depends_on_the_head(monkeypatch):
    frames = [40] * 9
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(77, 9, N_RAW))
    assert list_wide_plan(frames, 9, hop=12, raw=True)[3][0] == (0, 77, 9)
    assert list_wide_plan(frames, 9, hop=12, raw=False)[3][0] == (0, 86, 9)     # the terms alone


def test_same_call_same_plan():
    fr = [33, 21, 33, 47, 21, 47, 33]
    assert list_wide_plan(fr, 3, hop=12) == list_wide_plan(fr, 3, hop=12)


@pytest.mark.parametrize("frames, slots, hop", [([], 1, 12), ([30, 30], 0, 12), ([30, 30], 129, 12), ([30, 20, 30], 2, 12),
                                                ([30], 1, 0), ([-5], 1, 12), ([30], -1, 12)])
def test_refusals(frames, slots, hop):
    with pytest.raises(nat.WrnnError) as e:
        list_wide_plan(frames, slots, hop=hop)
    assert e.value.code == -1   # WRNN_EINVAL
    assert str(e.value).split(": ", 1)[1]     # the text is in wrnn_cond_last_error


def test_narrow_plan_keeps_its_limit():
    with pytest.raises(nat.WrnnError, match=r"lanes is 1\.\.8"):
        list_plan([30] * 20, 9)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(HDR).read()
    lib = nat.lib()
    for name, nargs in (("wrnn_list_wide_plan", 12), ("wrnn_generate_list_wide", 12), ("wrnn_postprocess_list", 8)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes)
    assert "#define WRNN_ABI_VERSION 7" in hdr      # additive: the version stays (7: wrnn_info grew)
