"""RAW wide streaming sessions (wrnn_stream_open_wide on a RAW handle, WaveRNN.stream(wide=True,
mu_law=)): sessions of a 9-bit rnn / fc 512 model on the grouped instantiation of the many-row XCD
kernel's softmax head (csrc/fatchord_xcdm.hip: kRaw && kGrp) — Exp(1) draws [steps][U][512] by
absolute step or Philox, audio only, mu-law expansion in the float64 post.

Inputs, expectations, the bound and the driver are tests/raw_streams.py's: every expectation is
oracle.generate on ONE utterance alone; with mu_law off the audio equals it bit for bit before the
fade-out and within rtol 1e-12 inside it (label-exactness, as tests/test_gpu_xcdm_raw.py demands of
the same kernel family), with mu_law on within rtol 1e-12 throughout.  Every push must return
exactly the count stream_plan announces, every case asserts last_path == 7.  "Bit-identical" is
np.array_equal.  The seeds are fixed: a mismatch is a failure to diagnose.

Measured on MI355X: with mu_law off 0 of the 8 307 body samples the cases print differ from the
oracle and 0 in the fades; with mu_law on the largest relative difference is 3.5e-15 (bound 1e-12).

A RAW path that indexed its f2 vector, its logits hop, its draws or its sampler by (XCD, slot) in a
way a session must own per row fails cases 2–4: the members differ in length, in frames per tick and
in the tick they join, so the surviving rows are re-compacted into other slots from round to round.
"""
import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import raw_streams as rs
from tests.raw_streams import Member, sched
from wavernn_amd.loop import wide_steps_per_launch

pytestmark = pytest.mark.gpu
OVERRIDES = ("WRNN_PATH", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES", "WRNN_TERMS_MB")
SEED = 3                                   # geometries.TAP_SEED
H12 = ("hop12", 9, 40, SEED)               # nine utterances of up to 40 frames at hop 12 (480 steps)
H4 = ("hop4", 4, 24, SEED)                 # four utterances of 24 frames at hop 4 (96 steps)
H275 = ("hop275", 3, 24, SEED, False, False)   # the reference geometry, Philox (no injected draws)
HOT = ("hop12", 2, 40, 7, True)            # regimes.STATE_SEED: labels reach classes 0 and 511 (checked below)


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


def _case(key):
    inp = rs.inputs(*key)
    return inp, rs.model(inp, key)


def _check(m, members, what, alone=False, **kw):
    outs, path = rs.run(m, members, **kw)
    assert path == 7, (what, path)
    for i, (mb, out) in enumerate(zip(members, outs)):
        rs.check(out, mb.ref(), mb.hop, mb.mu_law, f"{what} member {i}")
    if alone:
        solo, path = rs.run(m, members, grouped=False)
        assert path == 7, (what, path)
        for i, (a, b) in enumerate(zip(outs, solo)):
            assert np.array_equal(a, b), f"{what} member {i}: grouped differs from the session pushed alone"
    return outs


# ---- 1. one session alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows, mu_law, total, final_with_frames",
                         [([0], False, None, False), ([0], True, 40, True),
                          ([0, 1, 2], False, 40, True), ([0, 1, 2], True, None, False)])
def test_one_session_alone(rows, mu_law, total, final_with_frames):
    """One wide RAW session of U = 1 or 3, 40 frames: uneven pushes (1 frame, an empty push, 17 frames),
    the total announced or not, the final flag with frames or on an empty push, mu_law both ways."""
    inp, m = _case(H12)
    mb = Member(H12, rows, 40, sched([1, 0, 7, 13, 2, 17], final_with_frames=final_with_frames), total=total, mu_law=mu_law)
    _check(m, [mb], f"alone U={len(rows)}", grouped=False)
    if not mu_law:
        lab = rs.labels_of(mb.ref(), mb.hop)
        assert lab.min() >= 0 and lab.max() < rs.NC and len(np.unique(lab)) > 20


# ---- 2. groups: rounds and re-compaction -------------------------------------------------------------
def _nine_members():
    """Nine rows: U = 3, U = 2 (four ticks late) and four U = 1 of 25 / 28 / 33 / 40 frames, 1 to 20
    frames per tick; at tick 4 all nine rows run (XCD 0 holds two) in six rounds, the last of them member
    4 alone for 132 steps (its 20 frames, 228 steps, against 96 of the next longest).
    Member 3 is a mu_law session among mu_law-off ones."""
    return [Member(H12, [0, 1, 2], 40, sched([6] * 6 + [4])),
            Member(H12, [3, 4], 30, sched([6] + [3] * 8, start=4)),
            Member(H12, 5, 25, sched([1] * 25), total=25),
            Member(H12, 6, 28, sched([5, 5, 5, 5, 8], start=1), mu_law=True),
            Member(H12, 7, 33, sched([3, 0, 20, 10], start=2, final_with_frames=True)),
            Member(H12, 8, 40, sched([8] * 5, start=2))]


def _twenty_members():
    """The nine, the same (utterance, length) pairs again on other schedules (so the oracle runs no
    further utterance) and a U = 2 session: twenty rows, up to three slots on an XCD."""
    return _nine_members() + [Member(H12, [2, 0, 1], 40, sched([13, 13, 14], start=1)),
                              Member(H12, [4, 3], 30, sched([10, 10, 10])),
                              Member(H12, 5, 25, sched([5] * 5)),
                              Member(H12, 6, 28, sched([4] * 7, start=3), mu_law=True),
                              Member(H12, 7, 33, sched([3] * 11)),
                              Member(H12, 8, 40, sched([20, 20], final_with_frames=True)),
                              Member(H12, [1, 0], 40, sched([10] * 4, start=2))]


_NINE = {}


def _nine(m):
    """Case 2's nine-row group under the default budget, once per process (cases 2, 4 and 7 share it)."""
    if "outs" not in _NINE:
        _NINE["members"] = _nine_members()
        _NINE["outs"] = _check(m, _NINE["members"], "nine rows", alone=True)
    return _NINE["members"], _NINE["outs"]


@pytest.mark.parametrize("rows", [9, 20])
def test_group_rounds_and_recompaction(rows):
    """Members of U = 1, 2, 3 and 25–40 frames that join in different ticks with different frames per
    tick: a push has several rounds, the surviving rows change slot and XCD.  Each member against its
    oracle, bit-identical to itself pushed alone and to itself when the group lists its members in
    reverse order."""
    inp, m = _case(H12)
    if rows == 9:
        members, outs = _nine(m)
    else:
        members = _twenty_members()
        outs = _check(m, members, "twenty rows", alone=True)
    assert sum(mb.U for mb in members) == rows and {1, 2, 3} <= {mb.U for mb in members}
    assert min(mb.T for mb in members) == 25 and max(mb.T for mb in members) == 40
    assert len({mb.sched.count(None) for mb in members}) >= 3
    back, path = rs.run(m, members[::-1])
    assert path == 7
    for i, (a, b) in enumerate(zip(outs, back[::-1])):
        assert np.array_equal(a, b), f"{rows} rows, member {i}: differs when the group lists its members in reverse order"


# ---- 3. the full width -------------------------------------------------------------------------------
def test_128_rows():
    """Sixteen U = 8 sessions at hop 4, 24 frames, every slot of every XCD: session i holds utterances
    (i + j) % 4, j = 0..7, even sessions pushed 1 frame per tick, odd ones 3, the last four two ticks
    late (two rounds per tick, rows re-compacted).  Each utterance against its oracle once; all its
    32 rows, across sessions, slots and XCDs, bit-identical."""
    inp, m = _case(H4)
    members = [Member(H4, [(i + j) % 4 for j in range(8)], 24, sched([1] * 24 if i % 2 == 0 else [3] * 8, start=2 if i >= 12 else 0))
               for i in range(16)]
    assert sum(mb.U for mb in members) == 128
    outs, path = rs.run(m, members)
    assert path == 7
    first = {}
    for mb, out in zip(members, outs):
        for j, u in enumerate(mb.rows):
            if u not in first:
                first[u] = out[j]
                rs.check(out[j], rs.alone(H4, u, 24, False), mb.hop, False, f"128 rows, utterance {u}")
            assert np.array_equal(out[j], first[u]), f"128 rows: two rows of utterance {u} differ"
    assert len(first) == 4


# ---- 4. launch cutting -------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, geo.GEOMS["hop12"][7]])
def test_launch_cutting(monkeypatch, steps):
    """Case 2's nine rows at 1 step and at 77 steps per launch.  The budget is
    terms_budget_mb(steps, 9, 32·144 + 512): a RAW row-step costs its 4 608 terms and its 512 draws,
    so nine rows take exactly `steps` steps per launch (the MoL rule, terms alone, would take 86 at
    the 77-step budget) and fewer rows proportionally more; the launch counts follow through
    wide_plan.  Bit-identical to the default budget."""
    inp, m = _case(H12)
    members, whole = _nine(m)
    default = rs.launch_plan(m, members)
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 9, rs.N_RAW))
    assert wide_steps_per_launch(9, 10 ** 6, raw=True) == steps
    if steps == 77:
        assert wide_steps_per_launch(9, 10 ** 6, raw=False) == 86
    cut = rs.launch_plan(m, members)
    full = 0
    for (live, per, count), (_, per0, count0) in zip(cut, default):
        if live == 0:
            continue
        longest = per0                    # the default budget never cuts: one launch per round
        assert per == min(longest, int((steps + 1.5) * 9 / live - 1)), (live, per, longest)
        assert count >= count0
        full += live == 9 and longest > steps
    assert full >= 1, "no tick runs all nine rows for more steps than one launch takes"
    assert sum(c for _, _, c in cut) > sum(c for _, _, c in default)
    got, path = rs.run(m, members)
    assert path == 7
    for i, (a, b) in enumerate(zip(got, whole)):
        assert np.array_equal(a, b), f"{steps} step(s) per launch, member {i}: differs from the default budget"


# ---- 5. Philox ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu_law", [False, True])
def test_philox_rows_are_generates(mu_law):
    """The reference geometry (hop 275), 24 frames, one U = 3 session with a seed and row_offset 5:
    row i equals one-shot generate(seed=, row_offset=5 + i) of its own mel, at the bound."""
    inp, m = _case(H275)
    seed = 20240611
    mb = Member(H275, [0, 1, 2], 24, sched([8, 1, 0, 15]), philox=(seed, 5), mu_law=mu_law)
    (out,), path = rs.run(m, [mb], grouped=False)
    assert path == 7
    for i in range(3):
        want = m.generate(torch.from_numpy(mb.mel[i:i + 1]), None, False, 0, 0, mu_law, seed=seed, row_offset=5 + i, verbose=False)
        assert m.loop_handle().info["last_path"] == 7
        rs.check(out[i], np.asarray(want, np.float64), mb.hop, mu_law, f"Philox row_offset {5 + i}")


# ---- 6. full amplitude -------------------------------------------------------------------------------
def test_full_amplitude():
    """The saturated RAW state (rg.hot_fatchord_state at the raw512 regime's gain and end biases) at
    hop 12: the oracle's labels reach class 0 and class 511 (x = ∓1 fed back through the per-row state
    records between launches), 1-frame and 3-frame pushes."""
    inp, m = _case(HOT)
    members = [Member(HOT, 0, 40, sched([1] * 40)), Member(HOT, 1, 40, sched([3] * 13 + [1]))]
    lab = np.concatenate([rs.labels_of(mb.ref(), mb.hop).ravel() for mb in members])
    assert (lab == 0).any() and (lab == rs.NC - 1).any(), "the chosen seed does not reach both end classes"
    _check(m, members, "hot raw512", alone=True)


# ---- 7. interleaving ---------------------------------------------------------------------------------
def test_one_shot_generate_between_pushes():
    """A RAW one-shot generate() (its own many-row launches over the handle's hop area, terms and draws)
    between the pushes of case 2's nine-row group: the group's audio is bit-identical to the
    uninterrupted run, and the one-shot result to itself without the group."""
    inp, m = _case(H12)
    members, plain = _nine(m)
    mel = torch.from_numpy(inp.mels[8:9].copy())
    want = m.generate(mel, None, False, 0, 0, False, seed=1, verbose=False)
    got = []

    def between(tick):
        if tick in (2, 4, 7):
            got.append(m.generate(mel, None, False, 0, 0, False, seed=1, verbose=False))

    mixed, path = rs.run(m, members, between=between)
    assert len(got) == 3 and all(np.array_equal(g, want) for g in got)
    for i, (a, b) in enumerate(zip(mixed, plain)):
        assert np.array_equal(a, b), f"member {i} changed by a one-shot generate() between the group pushes"


# ---- 8. refusals -------------------------------------------------------------------------------------
def _bare_model(mode="RAW", **dims_kw):
    """A model at hop 12 that no oracle run goes with (the refusals need none)."""
    from wavernn_amd import synthetic as syn
    from wavernn_amd.fatchord_version import WaveRNN
    d = geo.geom_dims("hop12", mode=mode, **dims_kw)
    m = WaveRNN(**d.ctor_kwargs()).to(rs.DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, SEED).items()}, strict=True)
    return m.eval()


def test_refusals():
    """No refused call launches the loop: 10-bit and rnn-896 RAW models opened wide (the library's
    message names the condition), draws of the MoL width, draws shorter than the steps reached,
    wrnn_stream_mu_law on a MoL session and after a push.  A refused session is unchanged: it goes on,
    and the one refused wrnn_stream_mu_law after its first push ends with its oracle's audio."""
    with pytest.raises(NotImplementedError, match=r"512 classes \(bits = 9\): this handle has 1024 classes"):
        _bare_model(rnn_dims=512, bits=10).stream(1, None, seed=1, wide=True)
    with pytest.raises(NotImplementedError, match=r"rnn / fc 512\): this handle has rnn 896, fc 512"):
        _bare_model(rnn_dims=896).stream(1, None, seed=1, wide=True)
    inp, m = _case(H12)
    hop, look = inp.dims.hop_length, inp.dims.pad + 1
    with pytest.raises(NotImplementedError):                   # narrow RAW stays refused
        m.stream(1, None, seed=1)
    with pytest.raises(ValueError, match=r"\[steps\]\[1\]\[512\]"):
        m.stream(1, None, noise=np.zeros((40 * hop, 1, 11), np.float32), wide=True)
    mel = inp.mels[0:1]
    with m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:10 * hop - 1, 0:1]), wide=True, mu_law=False) as s:
        with pytest.raises(ValueError, match=f"the injected draws cover {10 * hop - 1} steps, the loop reaches {10 * hop}"):
            s.push(mel[:, :, :10 + look])
        assert s.push(mel[:, :, :look]).shape == (1, 0)        # refused before anything was queued: still usable
        with pytest.raises(ValueError, match="before the session's first push"):
            s.set_mu_law(True)
        a = s.push(mel[:, :, look:9 + look])                   # 9 frames of steps: inside the draws
        assert a.shape == (1, 0) and s._session.frames == 9 + look
    with m.stream(1, 40, noise=np.ascontiguousarray(inp.noise[:, 0:1]), wide=True, mu_law=False) as s:
        s.set_mu_law(True)                                     # before the first push: accepted
        out = [s.push(mel[:, :, :13])]
        with pytest.raises(ValueError, match="before the session's first push"):
            s.set_mu_law(False)
        out += [s.push(mel[:, :, 13:]), s.finish()]            # the refusal left it as it was: mu_law on
        assert m.loop_handle().info["last_path"] == 7
    rs.check(np.concatenate(out, 1), rs.alone(H12, 0, 40, True)[None], hop, True, "after a refused wrnn_stream_mu_law")
    with _bare_model("MOL", rnn_dims=512).stream(1, None, seed=1, wide=True, mu_law=True) as s:   # the keyword is ignored for MoL models
        with pytest.raises(ValueError, match="this session is MoL"):
            s.set_mu_law(True)
        assert s.push(mel[:, :, :look]).shape == (1, 0)
