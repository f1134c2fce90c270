"""WaveRNN.generate_list / wrnn_generate_list on the MI355X: utterances of unequal length queued on
the eight XCD lanes (include/wavernn_amd.h, "Lists"; the host side is tests/test_list_plan.py).

The contract under test: `generate_list(mels, seed=s, row_offset=r)[i]` is `generate(mels[i], None,
False, …, seed=s, row_offset=r + i)` BIT FOR BIT, for every lane count and every WRNN_TERMS_MB —
i.e. however the lanes' timelines are cut into rounds and pieces.  What each case would catch:
  1, 2, 5  a stale tag taken over from the lane's previous utterance (hand-off granules, the LDS
           step flags, the fc3 hand-off pairs), a wrong resume from the utterance's state record
           across a round boundary, a piece reading another piece's terms rows, a mis-ordered
           interpolation sum (the last bit of the terms);
  7        a list call touching a session's state, granules or stores (or the reverse);
  3        the whole path against the float64-post oracle, with injected draws per utterance.
  4        the same for the block-sparse rnn-896 kernel's list form.
Reference: gen_wavernn.py:11-35 (one generate() per utterance),
models/fatchord_version.py:169-264."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import regimes as rg
from wavernn_amd import _native as nat
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import list_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDES = ("WRNN_PATH", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES", "WRNN_TERMS_MB")
STD = rg.STREAM_STD_SEED
FRAMES_275 = (30, 41, 25, 22, 33, 21, 27, 36, 24, 29, 22)     # case 1: more utterances than lanes
# case 2 (hop 12): two 30-frame utterances head lanes 0 and 1 of a two-lane schedule, so lane-time
# 30 · 12 = 360 is an utterance boundary there
FRAMES_12 = (30, 21, 26, 30, 23, 28, 21, 25, 22, 27)
SEED = 123
_MODELS = {}


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


def _build(d, state):
    from wavernn_amd.fatchord_version import WaveRNN
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    return m.eval()


def _model(name):
    """One model per process: "mol275" (syn.DEFAULT_MOL, the reference geometry), "hop12" / "hop4"
    (the standard rnn-512 state at that geometry, perturbed taps)."""
    if name not in _MODELS:
        if name == "mol275":
            d = syn.DEFAULT_MOL
            _MODELS[name] = (d, _build(d, syn.make_fatchord_state(d, 3)))
        elif name == "sparse896":   # the 95 %-pruned rnn-896 model at hop 12
            inp = rg.stream_inputs("stdsparse896", "hop12", 2, 24, STD)
            _MODELS[name] = (inp.dims, _build(inp.dims, inp.state))
        else:
            inp = rg.stream_inputs("std512", name, 3, 24, STD)
            _MODELS[name] = (inp.dims, _build(inp.dims, inp.state))
    return _MODELS[name]


def _mels(d, frames, seed0):
    return [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed0 + i))[None] for i, T in enumerate(frames)]


@functools.lru_cache(maxsize=None)
def _singles(name, frames, seed0, seed, row_offset=0):
    """generate(mels[i], None, False, …, seed, row_offset + i) of every utterance, one call each:
    computed once per process, read-only."""
    d, m = _model(name)
    out = []
    for i, mel in enumerate(_mels(d, frames, seed0)):
        w = m.generate(mel, None, False, 11000, 550, False, seed=seed, row_offset=row_offset + i, verbose=False)
        assert m.loop_handle().info["last_path"] == (6 if name == "sparse896" else 5)
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.float64 and a.shape == b.shape, (what, i, a.shape, b.shape)
        assert np.array_equal(a, b), f"{what}, utterance {i}: differs from its single call, max |Δ| {np.abs(a - b).max():.3g}"


def _schedule(frames, lanes, hop, C):
    """The header's schedule restated: per lane the pieces (utterance, t0, Lc) of every round, from
    wrnn_list_plan's lanes and positions."""
    lane_of, pos, _ = list_plan(frames, lanes)
    rounds = {}
    for k in range(lanes):
        u0 = 0
        for i in sorted((i for i in range(len(frames)) if lane_of[i] == k), key=lambda i: pos[i]):
            L = frames[i] * hop
            j = u0 // C
            while j * C < u0 + L:
                a0, a1 = max(j * C, u0), min((j + 1) * C, u0 + L)
                rounds.setdefault((j, k), []).append((i, a0 - u0, a1 - a0))
                j += 1
            u0 += L
    return rounds


# ---- 1. more utterances than lanes, the reference geometry -------------------------------------------
def test_more_utterances_than_lanes_hop275():
    d, m = _model("mol275")
    want = _singles("mol275", FRAMES_275, 50, SEED)
    got = m.generate_list(_mels(d, FRAMES_275, 50), seed=SEED)
    assert m.loop_handle().info["last_path"] == 5
    _same(got, want, "11 utterances on 8 lanes")


# ---- 2. schedule independence ---------------------------------------------------------------------------
# (lanes, steps per round C or None for the default budget, the property of the cut this run is there for)
CUTS = [(1, 700, "pieces"), (2, 360, "boundary"), (3, 100, "rounds"), (8, None, None), (8, 100, "rounds"),
        (3, 1, None)]


@pytest.mark.parametrize("geom", ["hop12", "hop4"])
def test_every_schedule_gives_the_single_calls_bits(geom, monkeypatch):
    d, m = _model(geom)
    hop = d.hop_length
    frames = FRAMES_12
    want = _singles(geom, frames, 300, SEED, 5)
    mels = _mels(d, frames, 300)
    for lanes, C, prop in CUTS:
        if C is not None:
            C = max(1, C * hop // 12)           # the same cuts in frames at either hop
            if C == 1 and geom == "hop12":
                continue                        # one step per round: 3 000 launches at hop 12; hop 4 runs it
            monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(C, lanes, geo.N_TERMS))
            sch = _schedule(frames, lanes, hop, C)
            if prop == "pieces":      # a round holds at least three pieces on one lane
                assert max(len(v) for v in sch.values()) >= 3
            elif prop == "rounds":    # an utterance spans at least three rounds
                spans = {}
                for (j, k), v in sch.items():
                    for i, _, _ in v:
                        spans[i] = spans.get(i, 0) + 1
                assert max(spans.values()) >= 3
            elif prop == "boundary":  # a round boundary falls exactly on an utterance boundary inside a lane
                lane_of, pos, lane_frames = list_plan(frames, lanes)
                head = [i for i in range(len(frames)) if lane_of[i] == 0 and pos[i] == 0][0]
                assert frames[head] * hop % C == 0 and lane_frames[0] > frames[head]
                assert all(t0 == 0 for (j, k), v in sch.items() if k == 0 and j == frames[head] * hop // C for _, t0, _ in v[:1])
        else:
            monkeypatch.delenv("WRNN_TERMS_MB", raising=False)
        got = m.generate_list(mels, seed=SEED, row_offset=5, lanes=lanes)
        assert m.loop_handle().info["last_path"] == 5
        _same(got, want, f"{geom}, {lanes} lane(s), {C} step(s) per round")


# ---- 3. against the oracle ----------------------------------------------------------------------------------
def test_against_the_oracle_with_injected_draws():
    from oracle import oracle
    inp = rg.stream_inputs("std512", "hop12", 3, 24, STD)
    d, m = _model("hop12")
    hop = d.hop_length
    Ts = (24, 21, 22)
    mels = [np.array(inp.mels[u][None, :, :T], order="C") for u, T in enumerate(Ts)]      # copies: the inputs are read-only
    noise = [np.array(inp.noise[:T * hop, u], order="C") for u, T in enumerate(Ts)]
    got = m.generate_list(mels, noise=noise, lanes=2)
    worst = 0.0
    for u, T in enumerate(Ts):
        ref = inp.ref[u] if T == 24 else oracle.generate(inp.state, d, mels[u][0], False, 0, 0, False,
                                                               np.ascontiguousarray(noise[u][:, None]))
        assert got[u].shape == ref.shape == ((T - 1) * hop,)
        worst = max(worst, float(np.abs(got[u] - ref).max()))
    print(f"generate_list vs oracle.generate, injected draws: max |Δ| {worst:.3g}")
    assert worst <= 2e-5


# ---- 4. sparse rnn 896 --------------------------------------------------------------------------------------
def test_sparse896_nine_utterances(monkeypatch):
    d, m = _model("sparse896")
    frames = (26, 21, 24, 22, 25, 21, 23, 26, 22)
    want = _singles("sparse896", frames, 600, 31)
    mels = _mels(d, frames, 600)
    got = m.generate_list(mels, seed=31)
    h = m.loop_handle()
    assert h.info["last_path"] == 6 and h.info["sparse_blocks"] > 0, h.info
    _same(got, want, "sparse rnn 896, 9 utterances on 8 lanes")
    # two lanes, rounds of 100 steps: pieces resumed across rounds and several pieces per round
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(100, 2, 32 * _sparse_terms()))
    got = m.generate_list(mels, seed=31, lanes=2)
    assert m.loop_handle().info["last_path"] == 6
    _same(got, want, "sparse rnn 896, 2 lanes, 100 steps per round")


def _sparse_terms():
    """kSTerms of csrc/fatchord_xcds.h (terms per workgroup and step of the sparse kernel), read from
    the header so the budget below gives the rounds it says."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavernn_amd", "csrc", "fatchord_xcds.h")
    return int(re.search(r"kSTerms\s*=\s*(\d+)", open(path).read()).group(1))


# ---- 5. edges ---------------------------------------------------------------------------------------------------
def test_edges_one_three_and_eight_equal():
    d, m = _model("hop12")
    one = _singles("hop12", (23,), 400, 7)
    _same(m.generate_list(_mels(d, (23,), 400), seed=7), one, "U = 1")
    three = _singles("hop12", (22, 29, 21), 410, 7)
    _same(m.generate_list(_mels(d, (22, 29, 21), 410), seed=7), three, "U = 3, five XCDs idle")
    eight = _singles("hop12", (24,) * 8, 420, 7)
    _same(m.generate_list(_mels(d, (24,) * 8, 420), seed=7), eight, "eight equal lengths")


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    d, m = _model("hop12")
    want = _singles("hop12", (22, 29, 21), 410, 7)
    mels = _mels(d, (22, 29, 21), 410)
    with pytest.raises(ValueError):
        m.generate_list(mels + _mels(d, (20,), 9), seed=7)
    with pytest.raises(ValueError):
        m.generate_list(mels, seed=7, lanes=9)
    with pytest.raises(ValueError):
        m.generate_list([], seed=7)
    # the library's own checks, behind the Python ones: a 20-frame member and lanes = 9 through the loop
    loop, spec = m.loop_handle(), m._upsample_spec()
    fr = [m.frames(x.to(DEV)) for x in mels + _mels(d, (20,), 9)]
    for sel, lanes in ((slice(None), 4), (slice(0, 3), 9), (slice(0, 3), 0)):
        with pytest.raises(ValueError):
            loop.generate_list(spec, [f[0] for f in fr][sel], [f[1] for f in fr][sel], lanes=lanes, seed=7)
    again = [m.generate(x, None, False, 11000, 550, False, seed=7, row_offset=i, verbose=False) for i, x in enumerate(mels)]
    _same(again, want, "generate() after the refusals")
    _same(m.generate_list(mels, seed=7), want, "generate_list after the refusals")


def test_raw_model_is_refused():
    d = syn.DEFAULT_RAW
    m = _build(d, syn.make_fatchord_state(d, 6))
    mels = _mels(d, (21, 22), 30)
    before = m.generate(mels[0], None, False, 11000, 550, True, seed=4, verbose=False)
    with pytest.raises(NotImplementedError):
        m.generate_list(mels, seed=4)
    after = m.generate(mels[0], None, False, 11000, 550, True, seed=4, verbose=False)
    assert np.array_equal(before, after)


# ---- 7. neighbours on one handle -----------------------------------------------------------------------
def test_a_session_around_a_list_call():
    d, m = _model("hop12")
    mel = _mels(d, (26,), 500)[0]
    whole = np.concatenate(list(m.generate_stream(mel, (9, 9, 8), seed=11, row_offset=40)))
    want = _singles("hop12", (22, 29, 21), 410, 7)
    parts = []
    with m.stream(1, 26, seed=11, row_offset=40) as s:
        parts.append(s.push(mel[:, :, :9]))
        parts.append(s.push(mel[:, :, 9:18]))
        _same(m.generate_list(_mels(d, (22, 29, 21), 410), seed=7), want, "the list between two pushes")
        parts.append(s.push(mel[:, :, 18:]))
        parts.append(s.finish())
    got = np.concatenate([p[0] for p in parts if p.shape[1]])
    assert got.shape == whole.shape and np.array_equal(got, whole), "the session changed by the list call between its pushes"
    after = m.generate(_mels(d, (22,), 410)[0], None, False, 11000, 550, False, seed=7, verbose=False)
    assert np.array_equal(after, want[0])


# ---- 8. the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_three_utterances():
    d, m = _model("mol275")
    frames = FRAMES_275[:3]
    want = _singles("mol275", FRAMES_275, 50, SEED)[:3]
    from wavernn_amd import condition
    loop, spec = m.loop_handle(), m._upsample_spec()
    fr = [m.frames(x.to(DEV)) for x in _mels(d, frames, 50)]
    outs = [torch.empty(T * d.hop_length, dtype=torch.float32, device=DEV) for T in frames]
    vps = ctypes.c_void_p * 3
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc = nat.lib().wrnn_generate_list(loop._h, ctypes.byref(spec.cfg), vps(*[f[0].data_ptr() for f in fr]),
                                      vps(*[f[1].data_ptr() for f in fr]), (ctypes.c_int * 3)(*frames), 3, 3, None,
                                      ctypes.c_uint64(SEED), 0, vps(*[o.data_ptr() for o in outs]), stream)
    nat.check(loop._h, rc)
    loop.check(stream)
    assert loop.info["last_path"] == 5 and loop.elapsed_ms() > 0
    got = [condition.postprocess(o[None], False, 0, False, m.n_classes, f[2], 20 * d.hop_length).cpu().numpy()
           for o, f in zip(outs, fr)]
    _same(got, want, "wrnn_generate_list through ctypes")
