"""Host side of group pushes (wrnn_stream_push_group): the entry point is exported, declared and
bound, and the Python layers refuse malformed `pushes` before they reach the library.  No GPU: the
sessions here are bare objects with the attributes the checks read, never opened."""
import os
import re

import numpy as np
import pytest
import torch

from wavernn_amd import _native as nat
from wavernn_amd import build as hbuild
from wavernn_amd.fatchord_version import WaveRNN, WaveRNNStream
from wavernn_amd.loop import FatchordLoop, FatchordStream

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wavernn_amd.h")


@pytest.fixture(scope="module")
def lib():
    hbuild.build(verbose=False)
    return nat.lib()


def test_library_exports_and_native_binds_the_entry(lib):
    assert "wrnn_stream_push_group" in nat.EXPORTS
    fn = lib.wrnn_stream_push_group
    assert fn.restype is nat.ctypes.c_int32 or fn.restype is nat.ctypes.c_int
    assert len(fn.argtypes) == 9   # sessions, count, mel, n, final, wave, cap, n_out, stream


def test_header_declares_the_entry():
    text = open(HEADER).read()
    decl = re.search(r"^int wrnn_stream_push_group\(([^;]*)\);", text, re.M | re.S)
    assert decl, "include/wavernn_amd.h does not declare wrnn_stream_push_group"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert args == ["wrnn_stream_t *const *sessions", "int count", "const float *const *mel", "const int *n",
                    "const int *final", "double *const *wave", "const int *cap", "int *n_out", "void *stream"]


class _Lib:
    """Stands in for the library: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


def _bare_loop(feat=80):
    loop = object.__new__(FatchordLoop)
    loop.feat_dims, loop.device, loop._h = feat, 0, None
    return loop


def _bare_session(loop, n_streams=1, closed=False):
    s = object.__new__(FatchordStream)
    s.loop, s.n_streams, s.frames, s.finished, s.total_frames = loop, n_streams, 0, False, None
    s._s = None if closed else nat.ctypes.c_void_p(1)
    s.close = lambda: None   # never opened: nothing for __del__ to hand to the library
    return s


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(nat, "lib", lambda: _Lib())


def test_loop_push_streams_refuses_malformed_pushes(no_library):
    loop = _bare_loop()
    s = _bare_session(loop)
    try:
        for pushes, text in (([(s, None)], "tuples"), ([s], "tuples"), ([("session", None, False)], "tuples"),
                             ([], "at least one member"),
                             ([(_bare_session(loop, closed=True), None, False)], "closed"),
                             ([(_bare_session(_bare_loop()), None, False)], "another loop"),
                             ([(s, torch.zeros(1, 79, 4), False)], r"\[1\]\[80\]\[n\]"),
                             ([(s, np.zeros((1, 80, 4), np.float32), False)], r"\[1\]\[80\]\[n\]")):
            with pytest.raises(ValueError, match=text):
                loop.push_streams(pushes)
        s.finished = True
        with pytest.raises(ValueError, match="ended"):
            loop.push_streams([(s, None, True)])
    finally:
        loop._h = None   # nothing to destroy


def test_model_push_streams_refuses_malformed_pushes(no_library):
    model = object.__new__(WaveRNN)
    loop = _bare_loop()
    model.loop_handle = lambda: loop

    def wrapped(closed=False, owner=model):
        w = object.__new__(WaveRNNStream)
        w._model, w.device, w._session = owner, torch.device("cpu"), _bare_session(loop, closed=closed)
        return w

    keep = [wrapped(), wrapped(closed=True), wrapped(owner=None)]
    try:
        for pushes, text in (([(keep[0], None)], "tuples"), ([(keep[0]._session, None, False)], "tuples"), ([], "at least one"),
                             ([(keep[1], None, False)], "closed"), ([(keep[2], None, False)], "another model"),
                             ([(keep[0], np.zeros((79, 4), np.float32), False)], r"\[1\]\[80\]\[n\]")):
            with pytest.raises(ValueError, match=text):
                WaveRNN.push_streams(model, pushes)
    finally:
        loop._h = None
