"""Host side of rows sessions (wrnn_stream_open_rows) and of the windowed conditioning records
(wrnn_upsample_pack_window): the entry points are exported, declared and bound; the emission rule is
the one every session kind shares; the Python layers refuse `rows=True, wide=True` and a rows member
of push_streams before they reach the library; and the window-coverage rule — which frames the
records of a step window read — is pinned for every geometry of tests/geometries.py against the
cascade's dependency cone worked out here, stage by stage.  No GPU: the sessions are bare objects
with the attributes the checks read, never opened (as tests/test_stream_wide_host.py)."""
import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests.test_stream_plan import _rule
from tests.test_stream_wide_host import _bare_loop, _bare_session, _decl, _Lib
from wavernn_amd import _native as nat
from wavernn_amd import build as hbuild
from wavernn_amd import condition
from wavernn_amd.fatchord_version import WaveRNN, WaveRNNStream
from wavernn_amd.loop import FatchordStream, stream_lookahead, stream_plan


@pytest.fixture(scope="module")
def lib():
    hbuild.build(verbose=False)
    return nat.lib()


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(nat, "lib", lambda: _Lib())


def _spec(geom):
    feat, scales, pad = geo.GEOMS[geom][:3]
    taps = [np.full(2 * s + 1, 1.0 / (2 * s + 1), np.float32) for s in scales]
    return condition.UpsampleSpec(feat, 16, pad, scales, taps), scales, pad


def test_library_exports_and_header_declares_the_entries(lib):
    for name in ("wrnn_stream_open_rows", "wrnn_upsample_pack_window", "wrnn_upsample_window_frames"):
        assert name in nat.EXPORTS and hasattr(lib, name)
    assert list(lib.wrnn_stream_open_rows.argtypes) == list(lib.wrnn_stream_open.argtypes)
    assert _decl("wrnn_stream_open_rows") == _decl("wrnn_stream_open")
    assert _decl("wrnn_upsample_pack_window") == [
        "const wrnn_upsample_cfg *cfg", "const float *mel", "int m0", "int nm", "const float *aux", "int a0", "int na",
        "int T", "int U", "int t0", "int n", "float *cond", "void *stream"]
    assert len(lib.wrnn_upsample_pack_window.argtypes) == 13


@pytest.mark.parametrize("geom", list(geo.GEOMS))
def test_plan_counts_are_those_of_the_other_kinds(lib, geom):
    """A rows session reports through wrnn_stream_plan, the function of every kind: the rule of the header."""
    spec, scales, pad = _spec(geom)
    hop = int(np.prod(scales))
    assert stream_lookahead(spec) == pad + 1
    for T in (None, 24):
        for R in range(0, 25):
            assert stream_plan(spec, R, False, T) == _rule(hop, pad, R, False, T), (geom, T, R)
        assert stream_plan(spec, 24, True, T) == _rule(hop, pad, 24, True, T)


def test_rows_with_wide_is_refused_before_the_library(no_library):
    loop = _bare_loop()
    try:
        with pytest.raises(ValueError, match="rows=True and wide=True"):
            FatchordStream(loop, None, None, torch.zeros(4), 1, wide=True, rows=True)
        model = object.__new__(WaveRNN)
        with pytest.raises(ValueError, match="rows=True and wide=True"):
            WaveRNNStream(model, 1, None, None, 0, 0, wide=True, rows=True)
    finally:
        loop._h = None


def test_push_streams_refuses_a_rows_member_before_the_library(no_library):
    loop = _bare_loop()
    narrow, rows = _bare_session(loop, 1), _bare_session(loop, 2)
    rows.rows = True
    try:
        for pushes in ([(rows, None, False)], [(narrow, None, False), (rows, None, False)]):
            with pytest.raises(ValueError, match="a rows session advances alone"):
                loop.push_streams(pushes)
        assert narrow.frames == 0 and not narrow.finished and rows.frames == 0
    finally:
        loop._h = None


# ---- the window-coverage rule ----------------------------------------------------------------------
def _cone(scales, pad, t0, n, T):
    """Level-0 rows the cascade's output steps [t0, t0 + n) depend on, stage by stage: output row q of
    a stage (Stretch2d(s), then Conv2d(1, 2s + 1) with s zero columns either side) reads stretched
    columns q − s .. q + s, i.e. input rows ⌊(q − s)/s⌋ .. ⌊(q + s)/s⌋ = q//s − 1 .. q//s + 1, those
    inside the input.  → the mel frames (level-0 row − pad) inside [0, T) (T None: no upper end)."""
    hop = int(np.prod(scales))
    rows = set(range(t0 + pad * hop, t0 + n + pad * hop))      # uncropped output coordinates
    for s in reversed(scales):
        rows = {m + d for q in rows for m in (q // s,) for d in (-1, 0, 1) if m + d >= 0}
    return sorted(f for f in (r - pad for r in rows) if f >= 0 and (T is None or f < T))


@pytest.mark.parametrize("geom", list(geo.GEOMS))
def test_window_frames_cover_the_cascades_cone_and_stay_inside_the_look_ahead(lib, geom):
    """For every push schedule position: the frames wrnn_upsample_window_frames lists for a step window
    hold the window's dependency cone (never fewer: a record would read a missing frame), exceed it by
    at most two frames a side (the kernel stages a row of slack per level end), and for the steps a
    session runs after R frames — below (R − pad − 1)·hop — end at or before frame R."""
    spec, scales, pad = _spec(geom)
    hop = int(np.prod(scales))
    T = 24
    for total in (None, T):
        for t0, n in [(0, 1), (0, hop), (hop - 1, 2), (3 * hop, 5 * hop), (7 * hop + 1, 1), (0, T * hop if total else 9 * hop)]:
            mlo, mhi, alo, ahi = condition.upsample_window_frames(spec, t0, n, total)
            need = _cone(scales, pad, t0, n, total)
            assert need and mlo <= need[0] and need[-1] < mhi, (geom, total, t0, n, (mlo, mhi), need)
            assert need[0] - mlo <= 2 and mhi - 1 - need[-1] <= 2, (geom, total, t0, n, (mlo, mhi), need)
            assert (alo, ahi) == (t0 // hop, (t0 + n - 1) // hop + 1)
            if total is not None:
                assert mhi <= total
    for R in range(pad + 2, 40):
        s_old, s_new = (R - pad - 2) * hop, (R - pad - 1) * hop
        mlo, mhi, alo, ahi = condition.upsample_window_frames(spec, s_old, s_new - s_old, None)
        assert mhi <= R and ahi <= R - pad, (geom, R, mhi, ahi)
        assert mlo >= max(0, R - pad - 2 - 3), (geom, R, mlo)   # the mel tail a session keeps is short


def test_window_frames_refuse_bad_windows(lib):
    spec, scales, pad = _spec("hop12")
    for t0, n, T in ((-1, 1, None), (0, 0, None), (0, 25 * 12, 24), (0, 1, -2)):
        with pytest.raises(nat.WrnnError):
            condition.upsample_window_frames(spec, t0, n, T)
