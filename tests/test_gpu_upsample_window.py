"""Windowed conditioning records (C-ABI wrnn_upsample_pack_window, csrc/condition.hip) against the
whole-utterance records of wrnn_upsample_pack, bit for bit.

A rows session writes the records of the steps that became runnable, [S_old, S_new), from the frames
it holds while the utterance is still arriving.  For every geometry of tests/geometries.py (hop4: pad·hop
exactly the cascade's reach; hop12: 30 mels, the scalar column form; hop2: unit scales; hop16: four
stages; hop275: the reference's own), U = 2 and 24 frames: after each arrival of a frame schedule the
records of the new steps are formed with T = −1 from the frames received so far — once from the whole
received prefix, once from the smallest windows wrnn_upsample_window_frames allows, so frame offsets
m0, a0 > 0 are exercised — and on the last arrival with the true T.  Every record must equal the
whole-utterance one (np.array_equal): the window form is the same kernel body, and which tile a step
falls into decides what is staged, never a value.  A window that lacks a frame its steps read is
WRNN_EINVAL and writes nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import geometries as geo
from wavernn_amd import _native as nat
from wavernn_amd import condition
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import stream_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, T = 2, 24
SCHEDULES = {"uneven": [1, 5, 2, 7, 9], "ones": [1] * 24, "whole": [24]}
_CACHE = {}


def _case(geom):
    """(spec, dims, mel, aux, whole-utterance records [T·hop][U][CD]) of a geometry, computed once."""
    if geom not in _CACHE:
        d = geo.geom_dims(geom)
        state = geo.perturb_taps(syn.make_fatchord_state(d, geo.TAP_SEED), d, geo.TAP_SEED)
        taps = [state[f"upsample.up_layers.{2 * i + 1}.weight"] for i in range(len(d.upsample_factors))]
        spec = condition.UpsampleSpec(d.feat_dims, d.res_out_dims, d.pad, d.upsample_factors, taps)
        rng = np.random.default_rng(11)
        mel = torch.from_numpy(rng.random((U, d.feat_dims, T), dtype=np.float32)).to(DEV)
        # the kernel copies the aux frames: any values do, a MelResNet is not needed to pin it
        aux = torch.from_numpy(rng.standard_normal((U, d.res_out_dims, T)).astype(np.float32)).to(DEV)
        whole = condition.upsample_pack(spec, mel, aux).cpu().numpy()
        assert whole.shape == (T * d.hop_length, U, d.feat_dims + d.res_out_dims)
        _CACHE[geom] = (spec, d, mel, aux, whole)
    return _CACHE[geom]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("geom", list(geo.GEOMS))
def test_window_records_equal_the_whole_utterance_records(geom, schedule):
    spec, d, mel, aux, whole = _case(geom)
    pad = d.pad
    R, S_old, seen = 0, 0, 0
    counts = SCHEDULES[schedule]
    for i, n in enumerate(counts):
        R += n
        final = i == len(counts) - 1
        S_new = stream_plan(spec, R, final, None)[0]
        assert S_new == (T * d.hop_length if final else max(0, R - pad - 1) * d.hop_length)
        if S_new == S_old:
            continue
        total = T if final else None
        A = R if final else R - pad                      # aux frames a session has formed by now
        mlo, mhi, alo, ahi = condition.upsample_window_frames(spec, S_old, S_new - S_old, total)
        assert 0 <= mlo and mhi <= R and 0 <= alo and ahi <= A, (geom, R, (mlo, mhi, alo, ahi))
        want = whole[S_old:S_new]
        for (m0, m1), (a0, a1) in (((0, R), (0, A)), ((mlo, mhi), (alo, ahi))):
            got = condition.upsample_pack_window(spec, mel[:, :, m0:m1], m0, aux[:, :, a0:a1], a0, S_old, S_new - S_old,
                                                 total).cpu().numpy()
            assert got.shape == want.shape
            if not np.array_equal(got, want):
                at = tuple(np.argwhere(got != want)[0])
                raise AssertionError(f"{geom} {schedule} R={R} window mel [{m0}, {m1}) aux [{a0}, {a1}): record (step, row, "
                                     f"column) {at} is {got[at]!r}, whole utterance {want[at]!r}")
        seen += S_new - S_old
        S_old = S_new
    assert seen == T * d.hop_length


@pytest.mark.parametrize("geom", list(geo.GEOMS))
def test_a_window_that_lacks_a_frame_is_refused_before_any_launch(geom):
    spec, d, mel, aux, _ = _case(geom)
    hop, CD = d.hop_length, d.feat_dims + d.res_out_dims
    t0, n = 6 * hop, 3 * hop
    mlo, mhi, alo, ahi = condition.upsample_window_frames(spec, t0, n, None)
    cond = torch.full((n, U, CD), 7.0, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m0, m1, a0, a1, steps=n, T_=-1):
        mw, aw = mel[:, :, m0:m1].contiguous(), aux[:, :, a0:a1].contiguous()
        return nat.lib().wrnn_upsample_pack_window(ctypes.byref(spec.cfg), mw.data_ptr(), m0, m1 - m0, aw.data_ptr(), a0,
                                                   a1 - a0, T_, U, t0, steps, cond.data_ptr(), st)

    for m0, m1, a0, a1 in ((mlo + 1, mhi, alo, ahi), (mlo, mhi - 1, alo, ahi), (mlo, mhi, alo + 1, ahi),
                           (mlo, mhi, alo, ahi - 1)):
        assert call(m0, m1, a0, a1) == -1, (geom, m0, m1, a0, a1)            # WRNN_EINVAL
        assert "window holds" in nat.lib().wrnn_cond_last_error().decode()
    assert call(mlo, mhi, alo, ahi, steps=n, T_=8) == -1                      # steps past hop·T
    torch.cuda.synchronize()
    assert bool((cond == 7.0).all()), "a refused call wrote records"
    assert call(mlo, mhi, alo, ahi) == 0                                      # the same call with its frames
    torch.cuda.synchronize()
    assert not bool((cond == 7.0).any())
