"""Streaming sessions, host side (no GPU): the emission rule `wrnn_stream_plan` states in
include/wavernn_amd.h, and the dependency argument behind its look-ahead constant — conditioning
formed from a window of the running mel that carries `pad` real neighbour frames on each side
equals the whole-utterance conditioning (reference: pad_tensor → MelResNet / Stretch2d-Conv2d
cascade, fatchord_version.py:13-89, :183-186), in float64.  The GPU side is
tests/test_gpu_streaming.py."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import melresnet_ref as mr
from wavernn_amd import _native as nat
from wavernn_amd import condition
from wavernn_amd.loop import stream_lookahead, stream_plan

GEOMETRIES = [((5, 5, 11), 2), ((3, 4), 3)]
FADE_FRAMES = 20   # generate()'s fade-out: 20·hop_length samples (fatchord_version.py:255-258)


def _spec(scales, pad, feat=8, res_out=16, rng=None):
    if rng is None:
        taps = [np.full(2 * s + 1, 1.0 / (2 * s + 1), np.float32) for s in scales]
    else:
        taps = [(rng.standard_normal(2 * s + 1) * 0.3 + 1.0 / (2 * s + 1)).astype(np.float32) for s in scales]
    return condition.UpsampleSpec(feat, res_out, pad, scales, taps), taps


def _rule(hop, pad, R, final, T):
    """The rule as the header states it: (steps_done, audio_done)."""
    look = pad + 1
    if final:
        return R * hop, (R - 1) * hop
    steps = max(0, R - look) * hop
    if T is not None:
        return steps, min(steps, (T - 1) * hop)
    return steps, min(steps, max(0, (R - (FADE_FRAMES + 1)) * hop))


@pytest.mark.parametrize("scales,pad", GEOMETRIES)
def test_plan_follows_the_rule_for_every_frame_count(scales, pad):
    spec, _ = _spec(scales, pad)
    hop = int(np.prod(scales))
    assert stream_lookahead(spec) == pad + 1
    for T in (None, 21, 22, 41, 60):
        prev = (0, 0)
        for R in range(0, 61):
            if T is not None and R > T:
                with pytest.raises(nat.WrnnError):
                    stream_plan(spec, R, False, T)
                continue
            got = stream_plan(spec, R, False, T)
            assert got == _rule(hop, pad, R, False, T), (T, R, got)
            assert got[0] >= prev[0] and got[1] >= prev[1] and got[1] <= got[0], (T, R, got, prev)   # monotone in R
            prev = got
            # the end: only at the announced total, only with at least 21 frames
            if R < FADE_FRAMES + 1 or (T is not None and R != T):
                with pytest.raises(nat.WrnnError):
                    stream_plan(spec, R, True, T)
            else:
                fin = stream_plan(spec, R, True, T)
                assert fin == _rule(hop, pad, R, True, T) == (R * hop, (R - 1) * hop)
                assert fin[0] >= got[0] and fin[1] >= got[1]


@pytest.mark.parametrize("scales,pad", GEOMETRIES)
@pytest.mark.parametrize("known", [False, True])
def test_plan_totals_do_not_depend_on_the_chunking(scales, pad, known):
    spec, _ = _spec(scales, pad)
    hop = int(np.prod(scales))
    for T in (21, 22, 41, 60):
        total = T if known else None
        totals = set()
        for chunks in ([1] * T, [T], [1, 2, 1, 5] + [T - 9], [7, 1, 13, T - 21], [T - 1, 1]):
            assert sum(chunks) == T
            R, emitted, deltas = 0, 0, []
            for c in chunks:
                R += c
                a = stream_plan(spec, R, False, total)[1]
                deltas.append(a - emitted)
                emitted = a
            steps, a = stream_plan(spec, R, True, total)
            deltas.append(a - emitted)
            assert all(d >= 0 for d in deltas)
            assert sum(deltas) == (T - 1) * hop and steps == T * hop
            totals.add((steps, sum(deltas)))
        assert len(totals) == 1
    # a short first push emits nothing: the loop itself waits for the look-ahead
    assert stream_plan(spec, pad + 1, False, None) == (0, 0)
    assert stream_plan(spec, pad + 2, False, 60) == (hop, hop)


def test_plan_refuses_a_total_below_the_fade():
    spec, _ = _spec((5, 5, 11), 2)
    for T in (0, 1, 20):
        with pytest.raises(nat.WrnnError):
            stream_plan(spec, 0, False, T)


# ---- the dependency argument, in float64 ----------------------------------------------------------
def _mel_up(mel_of, jlo, coef, hop, p):
    """Σ_k coef[φ][k]·mel[f + k + jlo] at the steps p; mel_of(frame) → [feat] float64 (zeros outside)."""
    out = np.zeros((len(p), len(mel_of(0))))
    for i, pp in enumerate(p):
        f, ph = pp // hop, pp % hop
        for k in range(coef.shape[1]):
            out[i] += np.float64(coef[ph, k]) * mel_of(f + k + jlo)
    return out


def _whole(mel, res, spec, jlo, coef, hop, pad):
    """[T·hop][feat + R]: the whole-utterance conditioning (pad_tensor'd mel through the MelResNet,
    resnet_stretch; the cascade in its frame form, tests/test_frame_terms.py)."""
    feat, T = mel.shape
    padded = oracle.pad_tensor(mel.T[None].astype(np.float64), pad)[0].T[None]   # [1][feat][T + 2pad]
    _, _, aux = mr.reference(res, torch.from_numpy(padded))

    def mel_of(g):
        return mel[:, g].astype(np.float64) if 0 <= g < T else np.zeros(feat)
    p = np.arange(T * hop)
    return np.concatenate([_mel_up(mel_of, jlo, coef, hop, p), np.repeat(aux[0].T, hop, axis=0)], 1)


def _windowed(mel, received, T_known, res, jlo, coef, hop, pad, f0, f1, p):
    """The conditioning at the steps p (all inside frames [f0, f1)) from the window [f0 − pad, f1 + pad)
    of the running mel alone: frames >= `received` have not arrived (zeros stand in, which is right
    only past a known end), frames < 0 are pad_tensor's zeros."""
    feat = mel.shape[0]

    def mel_of(g):
        ok = 0 <= g < received and (T_known is None or g < T_known)
        return mel[:, g].astype(np.float64) if ok else np.zeros(feat)
    win = np.stack([mel_of(g) for g in range(f0 - pad, f1 + pad)], 1)[None]      # [1][feat][(f1 − f0) + 2pad]
    _, _, aux = mr.reference(res, torch.from_numpy(win))                          # frames f0 .. f1 − 1
    a = np.stack([aux[0][:, pp // hop - f0] for pp in p], 0)
    return np.concatenate([_mel_up(mel_of, jlo, coef, hop, p), a], 1)


@pytest.mark.parametrize("scales,pad", [((2, 3), 2), ((3, 4), 3), ((5, 5, 11), 2)])
def test_window_conditioning_equals_the_whole_utterance(scales, pad):
    rng = np.random.default_rng(3)
    feat, R_out, T = 8, 16, 12
    spec, _ = _spec(scales, pad, feat, R_out, rng)
    res = mr.build(2, feat, 16, R_out, pad, seed=1)
    jlo, nJ, coef = condition.frame_weights(spec)
    hop = int(np.prod(scales))
    assert jlo + nJ - 1 <= pad          # the cascade reaches no further ahead than the MelResNet window
    look = stream_lookahead(spec)
    mel = rng.uniform(0, 1, (feat, T)).astype(np.float32)
    want = _whole(mel, res, spec, jlo, coef, hop, pad)
    sub = lambda lo, hi: np.unique(np.concatenate([np.arange(lo, min(hi, lo + 3)), np.arange(max(lo, hi - 3), hi),
                                                   np.arange(lo, hi, max(1, hop // 2 + 1))]))
    # a non-final chunk: with `recv` frames in, the loop runs the frames [f0, recv − look) and reads the
    # conditioning of one step more, the first of frame recv − look
    for f0, recv in ((0, look + 1), (0, 7), (3, 9), (2, T)):
        f1 = recv - look
        p = np.append(sub(f0 * hop, f1 * hop), f1 * hop)
        got = _windowed(mel, recv, None, res, jlo, coef, hop, pad, f0, f1 + 1, p)
        np.testing.assert_allclose(got, want[p], rtol=0, atol=1e-12)
        # one frame less is not enough: that step's aux frame reads mel frame f1 + pad = recv − 1
        short = _windowed(mel, recv - 1, None, res, jlo, coef, hop, pad, f0, f1 + 1, np.array([f1 * hop]))
        assert np.abs(short - want[[f1 * hop]]).max() > 1e-6
    # the final chunk: zeros after frame T − 1, every remaining step, f1 = T
    for f0 in (0, T - look, T - 1):
        p = sub(f0 * hop, T * hop)
        got = _windowed(mel, T, T, res, jlo, coef, hop, pad, f0, T, p)
        np.testing.assert_allclose(got, want[p], rtol=0, atol=1e-12)
