"""Host side of wide streaming sessions (wrnn_stream_open_wide): the entry points are exported,
declared and bound, the Python layers refuse malformed input before they reach the library, and the
round plan of a wide push (wrnn_wide_plan, host only) is pinned on ragged inputs.  No GPU: the
sessions here are bare objects with the attributes the checks read, never opened."""
import os
import re

import pytest
import torch

from wavernn_amd import _native as nat
from wavernn_amd import build as hbuild
from wavernn_amd import loop as wloop
from wavernn_amd.fatchord_version import WaveRNN, WaveRNNStream
from wavernn_amd.loop import FatchordLoop, FatchordStream

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wavernn_amd.h")


@pytest.fixture(scope="module")
def lib():
    hbuild.build(verbose=False)
    return nat.lib()


def _decl(name):
    text = open(HEADER).read()
    decl = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M | re.S)
    assert decl, f"include/wavernn_amd.h does not declare {name}"
    return [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]


def test_library_exports_and_native_binds_the_entries(lib):
    for name in ("wrnn_stream_open_wide", "wrnn_wide_plan"):
        assert name in nat.EXPORTS
    fn = lib.wrnn_stream_open_wide
    assert fn.restype is nat.ctypes.c_int32 or fn.restype is nat.ctypes.c_int
    assert list(fn.argtypes) == list(lib.wrnn_stream_open.argtypes) and len(fn.argtypes) == 11
    assert len(lib.wrnn_wide_plan.argtypes) == 8


def test_header_declares_the_entries_with_the_arguments_of_open():
    args = _decl("wrnn_stream_open_wide")
    assert args == _decl("wrnn_stream_open")
    assert args == ["wrnn_t *h", "const wrnn_upsample_cfg *ucfg", "const wrnn_melresnet_cfg *mcfg",
                    "const float *melresnet_packed", "int U", "int total_frames", "const float *noise", "int noise_steps",
                    "uint64_t seed", "int64_t row_offset", "wrnn_stream_t **out"]
    assert _decl("wrnn_wide_plan") == ["const int *steps", "const int *rows", "int count", "int steps_per_launch",
                                       "int *launch_first", "int *launch_steps", "int *launch_rows", "int cap"]


class _Lib:
    """Stands in for the library: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


def _bare_loop(feat=80):
    loop = object.__new__(FatchordLoop)
    loop.feat_dims, loop.device, loop._h = feat, 0, None
    return loop


def _bare_session(loop, n_streams=1, wide=False):
    s = object.__new__(FatchordStream)
    s.loop, s.n_streams, s.frames, s.finished, s.total_frames, s.wide = loop, n_streams, 0, False, None, wide
    s._s = nat.ctypes.c_void_p(1)
    s.close = lambda: None   # never opened: nothing for __del__ to hand to the library
    return s


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(nat, "lib", lambda: _Lib())


@pytest.mark.parametrize("n_streams", [0, 129, -1])
def test_wide_sessions_refuse_row_counts_outside_1_to_128(no_library, n_streams):
    loop = _bare_loop()
    packed = torch.zeros(4)
    try:
        with pytest.raises(ValueError, match=r"a wide session has 1\.\.128 utterances"):
            FatchordStream(loop, None, None, packed, n_streams, wide=True)
        model = object.__new__(WaveRNN)
        with pytest.raises(ValueError, match=r"a wide session has 1\.\.128 utterances"):
            WaveRNNStream(model, n_streams, None, None, 0, 0, wide=True)
    finally:
        loop._h = None   # nothing to destroy


def test_push_streams_refuses_mixed_families_and_129_rows(no_library):
    loop = _bare_loop()
    w1, w2, n1 = _bare_session(loop, 1, wide=True), _bare_session(loop, 128, wide=True), _bare_session(loop, 1)
    try:
        for pushes, text in (([(w1, None, False), (n1, None, False)], "wide sessions or narrow ones, not both"),
                             ([(n1, None, False), (w1, None, False)], "wide sessions or narrow ones, not both"),
                             ([(w1, None, False), (w2, None, False)], r"at most 128 rows \(16 per XCD\): these members have 129")):
            with pytest.raises(ValueError, match=text):
                loop.push_streams(pushes)
    finally:
        loop._h = None


def test_model_push_streams_refuses_mixed_families(no_library):
    model = object.__new__(WaveRNN)
    loop = _bare_loop()
    model.loop_handle = lambda: loop

    def wrapped(wide):
        w = object.__new__(WaveRNNStream)
        w._model, w.device, w._session = model, torch.device("cpu"), _bare_session(loop, wide=wide)
        return w

    try:
        with pytest.raises(ValueError, match="wide sessions or narrow ones, not both"):
            WaveRNN.push_streams(model, [(wrapped(True), None, False), (wrapped(False), None, False)])
    finally:
        loop._h = None


# ---- the round plan: distinct step counts → rounds, rows → (XCD, slot) ---------------------------------
def test_round_plan_cuts_at_the_distinct_step_counts(lib):
    """Members of 36, 12, 0, 36 and 84 steps with 1, 3, 2, 1 and 2 rows: rounds [0, 12), [12, 36),
    [36, 84); the 0-step member takes no slot, the 12-step member leaves after round 1, the rest are
    compacted."""
    plan = wloop.wide_plan([36, 12, 0, 36, 84], [1, 3, 2, 1, 2], 1000)
    assert [(f, n, len(rows)) for f, n, rows in plan] == [(0, 12, 7), (12, 24, 4), (36, 48, 2)]
    assert [(i, u) for i, u, _, _ in plan[0][2]] == [(0, 0), (1, 0), (1, 1), (1, 2), (3, 0), (4, 0), (4, 1)]
    assert [(i, u, x, s) for i, u, x, s in plan[1][2]] == [(0, 0, 0, 0), (3, 0, 1, 0), (4, 0, 2, 0), (4, 1, 3, 0)]
    assert plan[2][2] == [(4, 0, 0, 0), (4, 1, 1, 0)]


def test_round_plan_chunks_every_round_and_places_rows_on_xcd_r_mod_8(lib):
    """Ten one-row members, nine of 30 steps and one of 77, at 25 steps per launch: round [0, 30) is
    launches of 25 + 5, round [30, 77) of 25 + 22; row 8 and 9 of the first round sit in slot 1 of
    XCDs 0 and 1, and the long member (listed sixth) moves from (XCD 5, slot 0) to (XCD 0, slot 0)."""
    steps = [30] * 5 + [77] + [30] * 4
    plan = wloop.wide_plan(steps, [1] * 10, 25)
    assert [(f, n, len(rows)) for f, n, rows in plan] == [(0, 25, 10), (25, 5, 10), (30, 25, 1), (55, 22, 1)]
    assert plan[0][2][8] == (8, 0, 0, 1) and plan[0][2][9] == (9, 0, 1, 1) and plan[0][2][5] == (5, 0, 5, 0)
    assert plan[2][2] == [(5, 0, 0, 0)]
    # the full width: 128 rows of one step count are one round, slot r // 8 up to 15
    (first, n, rows), = wloop.wide_plan([12] * 16, [8] * 16, 12)
    assert (first, n) == (0, 12) and rows[-1] == (15, 7, 7, 15) and rows[64] == (8, 0, 0, 8)


def test_round_plan_refuses_bad_counts(lib):
    assert wloop.wide_plan([0, 0], [1, 1], 5) == []
    for steps, rows, per in (([5], [0], 1), ([-1], [1], 1), ([5], [1], 0), ([5, 5], [64, 65], 1)):
        with pytest.raises(nat.WrnnError):
            wloop.wide_plan(steps, rows, per)
