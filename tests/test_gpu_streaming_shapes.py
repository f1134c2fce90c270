"""Streaming sessions away from the one shape tests/test_gpu_streaming.py pins: the upsample
geometries of tests/geometries.py (pad 1 and 3, 3 / 5 / 7 frame weights, hop 2 … 16, four stages),
several utterances per session, time-chunked launches inside a push (WRNN_TERMS_MB, down to one
step per launch), store swaps while samples are held back for the fade, full-amplitude states
(tests/regimes.py), and the C-ABI shapes the Python wrapper never produces.

Every expectation is `oracle.generate` (unbatched, float64 MelResNet and cascade, the C loop, the
float64 post), one call per utterance with that utterance's column of the injected draws
(regimes.stream_inputs); the bound is 2·MOL_TOL, the project's bound for whole-generate()
comparisons with the oracle (test_gpu_regimes.test_dropin_generate_hot_regime,
test_torch_cpu_baseline.py).  Each push must return exactly the count `stream_plan` announces
(`_run_session` of tests/test_gpu_streaming.py) and every session must have run the windowed
instantiation of its kernel (last_path 5 dense, 6 sparse).  The Philox cases compare with one-shot
generate() at MOL_TOL, on top of the oracle cases.

Measured on MI355X (max |Δ| against the oracle, bound 2e-5):
  every geometry, dense (U = 1 and 3, three schedules, total unknown / announced: one figure per
    geometry, the schedules agree to the last bit)   hop12 4.1e-8, hop4 2.8e-8, hop2 3.2e-8, hop16 3.3e-8
  70 frames in 1-frame pushes, U = 2                 hop12 4.3e-8, hop2 3.4e-8
  chunks of 77 steps / one step per launch           hop12 4.1e-8, hop2 3.2e-8 (chunked = unchunked bit for bit)
  sparse rnn 896 at hop12, U = 1 and 8               3.5e-8
  hot dense hop 275 / hop12 (also one step per launch) / hot sparse hop12   7.8e-7 / 6.0e-7 / 4.8e-7
  final push with frames; cap = m + 7 and refusals; empty pushes; side stream   4.1e-8 (hot hop 275: 7.8e-7)
  Philox streamed vs generate() at hop12, dense and sparse   0 (bit-identical on that build, not asserted)
No case needed a change to the library.  Value-only mutations, each built once and run once under
this file (28 tests): the mel tail read one frame late, the coefficient phase off by one and the
fade index off by one each fail all 28; the d_y swap copying held − 1 samples fails 17 (every
total-unknown session, the 70-frame, chunked, sparse and hot 1-frame sessions, empty pushes, the
side stream); the windowed dense kernel's upper clamp at 0.999 fails the 5 hot dense cases (max
|Δ| 1.0e-3) and nothing else."""
import ctypes

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import regimes as rg
from tests.golden import fixtures as gf
from tests.test_gpu_streaming import _run_session
from wavernn_amd import _native as nat
from wavernn_amd.loop import stream_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2 * gf.MOL_TOL
OVERRIDES = ("WRNN_PATH", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES", "WRNN_TERMS_MB")
STD = rg.STREAM_STD_SEED
_MODELS = {}


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


def _case(model, geom, n_utt, frames, seed):
    """(inputs, WaveRNN on the GPU); one model per (model, geometry, seed), shared by the tests."""
    from wavernn_amd.fatchord_version import WaveRNN
    inp = rg.stream_inputs(model, geom, n_utt, frames, seed)
    key = (model, geom, seed)
    if key not in _MODELS:
        m = WaveRNN(**inp.dims.ctor_kwargs()).to(DEV)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in inp.state.items()}, strict=True)
        _MODELS[key] = m.eval()
    return inp, _MODELS[key]


def _rows(inp, U):
    """The first U utterances of an input: (mels, their columns of the draws, their expectations)."""
    return inp.mels[:U].copy(), inp.noise[:, :U].copy(), inp.ref[:U]


def _vs_oracle(chunks, ref, what):
    out = np.concatenate(chunks, 1)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    diff = np.abs(out - ref)
    print(f"STREAM {what}: max |Δ| {diff.max():.3g} over {diff.size} samples")
    assert diff.max() <= TOL, f"{what}: max |Δ| {diff.max():.3g}, first over at (row, sample) {tuple(np.argwhere(diff > TOL)[0])}"
    return out


def _session(m, inp, U, pushes, total, what, want_path=5, **kw):
    mel, noise, ref = _rows(inp, U)
    assert sum(n or 0 for n in pushes) == mel.shape[2]
    chunks, path = _run_session(m, mel, pushes, total, noise=noise, **kw)
    assert path == want_path, (what, path)
    return _vs_oracle(chunks, ref, what)


# ---- 1. every geometry, dense ---------------------------------------------------------------------
@pytest.mark.parametrize("total", [None, 24], ids=["unknown", "announced"])
@pytest.mark.parametrize("geom", geo.ODD)
def test_every_geometry_dense(geom, total):
    """24 frames in 1-frame pushes, in [look − 1, 1, 1, rest] (the first loop step runs in the
    third push) and in one push; one utterance, and three with different mels, each row against
    its own oracle output (a row that read another row's frame terms, mel tail or samples fails)."""
    inp, m = _case("std512", geom, 3, 24, STD)
    look = inp.dims.pad + 1
    for U in (1, 3):
        for name, pushes in (("ones", [1] * 24), ("straddle", [look - 1, 1, 1, 24 - look - 1]), ("whole", [24])):
            _session(m, inp, U, pushes, total, f"{geom} U={U} total={total} {name}")


# ---- 2. store swaps under held-back audio ---------------------------------------------------------
def _store_swaps(hop, pad, jlo, nJ, frames, U):
    """The session's bookkeeping for `frames` 1-frame pushes and finish(), total unknown, restated
    from capi_stream.cpp (win_reserve; stream_push's d_y branch): ([FT swaps], [AT swaps] as (frames
    received, rows copied), [d_y swaps] as (frames received, samples held, samples emitted))."""
    look, jhi = pad + 1, jlo + nJ - 1

    class Win:
        cap, cur, base, end = None, 0, 0, 0

    def reserve(w, keep, add, R):
        keep = min(max(keep, w.base), w.end)
        if w.end + add - w.base <= w.cap[w.cur]:
            return
        o, need = 1 - w.cur, w.end - keep + add
        if need > w.cap[o]:
            w.cap[o] = 2 * need
        w.swaps.append((R, w.end - keep))
        w.cur, w.base = o, keep

    FT, AT = Win(), Win()
    for w in (FT, AT):
        w.cap, w.swaps = [0, 0], []
    reserve(FT, 0, -jlo, 0)
    FT.end = -jlo
    R = A = steps = audio = 0
    y_cap, y_ld, y_cur, y_t0, y_swaps = [0, 0], [0, 0], 0, 0, []
    for final in [False] * frames + [True]:
        n = 0 if final else 1
        Rn = R + n
        S = Rn * hop if final else max(0, Rn - look) * hop
        Au = (Rn - 1) * hop if final else min(S, max(0, (Rn - 21) * hop))
        keep = steps // hop
        A_new = Rn if final else max(A, Rn - pad)
        add = n + (max(0, jhi) if final else 0)
        if add:
            reserve(FT, keep, add, Rn)
            FT.end += add
        if A_new > A:
            reserve(AT, keep, A_new - A, Rn)
            AT.end += A_new - A
        if S > steps and S - y_t0 > y_ld[y_cur]:
            o, need = 1 - y_cur, S - audio
            if need * U > y_cap[o]:
                y_cap[o] = 2 * need * U
            y_ld[o] = y_cap[o] // U
            y_swaps.append((Rn, steps - audio, audio))
            y_cur, y_t0 = o, audio
        R, A, steps, audio = Rn, A_new, S, Au
    return FT.swaps, AT.swaps, y_swaps


@pytest.mark.parametrize("geom,want", [("hop12", (13, 35, 7)), ("hop2", (10, 35, 7))])
def test_store_swaps_while_samples_are_held_back(geom, want):
    """70 frames in 1-frame pushes, total unknown, two utterances.  Until the end is known the
    session holds back 21 frames of samples (the fade could still reach them), so from frame 22 on
    every d_y swap copies held samples, and the frame-term stores swap all along.

    d_y (hop12, look 4): push R runs the steps up to S = (R − 4)·12 and emits up to (R − 21)·12.
    A swap allocates twice the samples it must hold (need = S − emitted), per utterance:
      R = 5: need 12 → ld 24;  R = 7: S = 36 > 24, 24 held → ld 72;  R = 11: 84 > 72 → ld 168;
      R = 19: 180 > 168 → ld 360 (nothing emitted so far, origin 0);
      R = 35: S = 372 > 360, emitted 156, held 360 − 156 = 204, need 216 → ld 432, origin 156;
      R = 54: S − 156 = 444 > 432, emitted 384, held 204 → back to the ld-360 buffer, origin 384;
      R = 67: S − 384 = 372 > 360, emitted 540, held 204 → the ld-432 buffer, origin 540;
      finish(): 840 − 540 = 300 fits.
    Seven swaps, three of them with 204 samples held after audio has begun; hop2 is the same
    schedule in units of 2 (34 held at R = 35, 54, 67).  FT (rows of U·N floats, keep = frame of the
    next step = R − 5): 2 zero rows, then capacity 2 → 10 → 16 rows with 6 live rows copied every
    4 + 8 pushes, 13 swaps (hop2, 3 zero rows and 7 live: 10 swaps); AT holds one live row in a
    2- and a 4-row buffer and swaps on two pushes of every four, and twice in finish(): 35.
    `_store_swaps` restates that bookkeeping; the counts are asserted so a change of the schedule
    that stops exercising the swaps is noticed."""
    inp, m = _case("std512", geom, 2, 70, STD)
    jlo, nJ = geo.GEOMS[geom][3:5]
    ft, at, y = _store_swaps(inp.dims.hop_length, inp.dims.pad, jlo, nJ, 70, 2)
    held_after_audio = [s for s in y if s[1] > 0 and s[2] > 0]
    print(f"STREAM {geom} 70 frames: FT swaps {len(ft)}, AT swaps {len(at)}, d_y swaps {y}")
    assert (len(ft), len(at), len(y)) == want
    assert len(held_after_audio) == 3 and [s[0] for s in held_after_audio] == [35, 54, 67]
    assert sum(1 for s in ft if s[1] > 0) >= 2 and sum(1 for s in at if s[1] > 0) >= 2
    _session(m, inp, 2, [1] * 70, None, f"{geom} U=2 70 frames ones")


# ---- 3. chunked launches inside a push ------------------------------------------------------------
def _chunked(m, inp, U, pushes, mb, what, monkeypatch, **kw):
    """The session unchunked, then under WRNN_TERMS_MB = mb: both against the oracle, and against
    each other (2·MOL_TOL, as test_gpu_frame_geometry.test_time_chunked_launches)."""
    whole = _session(m, inp, U, pushes, None, what + " one launch per push", **kw)
    monkeypatch.setenv("WRNN_TERMS_MB", mb)
    got = _session(m, inp, U, pushes, None, what + " chunked", **kw)
    err = float(np.abs(got - whole).max())
    print(f"STREAM {what}: chunked vs one launch per push max |Δ| {err:.3g}")
    assert err <= TOL, (what, err)


def test_chunks_of_77_steps_start_in_mid_frame(monkeypatch):
    """hop12, 3 utterances, 24 frames as 8 + 8 + (8, final): the pushes run 48, 96 and 144 steps, so
    under a budget of 77 steps per launch (stream_launches: ⌊budget / (U·N) − 1⌋, N = 5120) the
    second is 77 + 19 and the final one 77 + 67 — chunks begin at steps 125 and 221, in mid-frame,
    and the last chunk takes the `last` row rule (no terms row past step 287) and L = t_end."""
    inp, m = _case("std512", "hop12", 3, 24, STD)
    hop, X = inp.dims.hop_length, geo.GEOMS["hop12"][7]
    spec = m._upsample_spec()
    assert X % hop and (48 + X) % hop and stream_plan(spec, 24, True)[0] - stream_plan(spec, 16)[0] > X
    _chunked(m, inp, 3, [8, 8, 8], geo.terms_budget_mb(X, 3, geo.N_TERMS), "hop12 U=3 X=77", monkeypatch, final_last=True)


@pytest.mark.parametrize("geom", ["hop12", "hop2"])
def test_one_step_per_launch(geom, monkeypatch):
    """regimes.ONE_STEP_BUDGET_MB: every windowed launch is one step (two terms rows, one in the
    very last), the final push included; at hop 2 a frame is two launches."""
    inp, m = _case("std512", geom, 3, 24, STD)
    _chunked(m, inp, 3, [8, 8, 8], rg.ONE_STEP_BUDGET_MB, f"{geom} U=3 one step per launch", monkeypatch, final_last=True)


# ---- 4. sparse sessions at another geometry -------------------------------------------------------
@pytest.mark.parametrize("U", [1, 8])
def test_sparse_sessions_at_hop12(U):
    """The 95 %-pruned rnn-896 state behind the hop12 upsampler (pad 3, feat 30): the windowed
    block-sparse kernel, one and eight utterances."""
    inp, m = _case("stdsparse896", "hop12", 8, 24, STD)
    for name, pushes in (("uneven", [7, 1, 13, 3]), ("ones", [1] * 24)):
        _session(m, inp, U, pushes, None, f"sparse896 hop12 U={U} {name}", want_path=6)


# ---- 5. full amplitude ----------------------------------------------------------------------------
@pytest.mark.parametrize("pushes,total", [([1] * 24, None), ([5, 19], 24)], ids=["ones", "5+19"])
def test_hot_dense_at_hop_275(pushes, total):
    """regimes.generate_inputs(False): the hot rnn-512 state at the reference's geometry (the
    input of test_gpu_regimes.test_dropin_generate_hot_regime, streamed)."""
    inp, m = _case(*rg.STREAM_HOT_275)
    pos, neg = rg.stream_clamps(inp.ref, inp.dims.hop_length)
    assert pos.any() and neg.any()
    _session(m, inp, 1, pushes, total, f"hot mol512 hop275 {len(pushes)} pushes")


@pytest.mark.parametrize("budget", [None, rg.ONE_STEP_BUDGET_MB], ids=["push", "1step"])
def test_hot_dense_at_hop12_clamps_cross_relaunches(budget, monkeypatch):
    """1-frame pushes: x = ±1 is carried through d_state and the hop tags into the next launch at
    every frame boundary, and with the one-step budget at every step.  Both signs must occur at
    steps that are followed by another (read off the oracle's audio, regimes.stream_clamps), in
    both utterances' share of the session."""
    inp, m = _case(*rg.STREAM_HOT_DENSE)
    hop = inp.dims.hop_length
    pos, neg = rg.stream_clamps(inp.ref, hop)
    assert pos.any() and neg.any()
    # … and at the last step of a frame, the one a push boundary follows
    assert pos[:, hop - 1::hop].any() and neg[:, hop - 1::hop].any()
    if budget:
        monkeypatch.setenv("WRNN_TERMS_MB", budget)
    _session(m, inp, 2, [1] * 24, None, f"hot mol512 hop12 U=2 ones{' one step per launch' if budget else ''}")


def test_hot_sparse_at_hop12():
    inp, m = _case(*rg.STREAM_HOT_SPARSE)
    pos, neg = rg.stream_clamps(inp.ref, inp.dims.hop_length)
    assert pos.any() and neg.any()
    _session(m, inp, 2, [1] * 30, None, "hot sparse896 hop12 U=2 ones", want_path=6)


# ---- 6. C-ABI shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("key,U", [(("std512", "hop12", 3, 24, STD), 2), (rg.STREAM_HOT_275, 1)], ids=["hop12", "hop275"])
def test_final_push_carries_frames(key, U):
    """push(mel, final=True) with the last 1, pad and pad + 3 frames in the final call: the aux
    window of that push is n + pad frames with zeros after the end beside the new frames, the FT
    store gets its new rows and its max(0, jhi) zero rows in one pass."""
    inp, m = _case(*key)
    T, pad = inp.mels.shape[2], inp.dims.pad
    for k in (1, pad, pad + 3):
        _session(m, inp, U, [T - k, k], None, f"{key[1]} U={U} final push of {k} frames", final_last=True)


SENTINEL = -7.25


class _Raw:
    """A session driven through wrnn_stream_push itself (opened by the wrapper, which keeps the
    tensors the session reads alive)."""

    def __init__(self, m, U, total, noise):
        self.ws = m.stream(U, total, noise=noise)
        self.sess = self.ws._session
        self.U, self.total, self.frames = U, total, 0

    def plan(self, n, final):
        spec = self.sess.spec
        return stream_plan(spec, self.frames + n, final, self.total)[1] - stream_plan(spec, self.frames, False, self.total)[1]

    def call(self, mel, final, wave_ptr, cap):
        """(status, n_out, the library's message)."""
        n = 0 if mel is None else mel.shape[2]
        t = torch.from_numpy(np.ascontiguousarray(mel)).to(self.sess.device) if n else None
        got = ctypes.c_int(-1)
        st = torch.cuda.current_stream(self.sess.device).cuda_stream
        rc = nat.lib().wrnn_stream_push(self.sess._s, t.data_ptr() if n else None, n, int(final), wave_ptr, cap,
                                        ctypes.byref(got), st)
        msg = (nat.lib().wrnn_last_error(self.sess.loop._h) or b"").decode(errors="replace")
        if rc == 0:
            self.sess.loop.check(st)
            self.frames += n
        return rc, got.value, msg

    def push(self, mel, final=False, extra=7):
        """A correct call with cap = m + extra into a sentinel-filled buffer: [U][m], after checking
        that nothing outside columns [0, m) of the U rows at stride cap was written."""
        m_, U = self.plan(0 if mel is None else mel.shape[2], final), self.U
        cap = m_ + extra
        buf = torch.full((U * cap + 16,), SENTINEL, dtype=torch.float64, device=self.sess.device)
        rc, got, msg = self.call(mel, final, buf.data_ptr(), cap)
        assert rc == 0 and got == m_, (rc, got, m_, msg)
        host = buf.cpu().numpy()
        rows = host[:U * cap].reshape(U, cap)
        assert (rows[:, m_:] == SENTINEL).all() and (host[U * cap:] == SENTINEL).all()
        assert not (rows[:, :m_] == SENTINEL).any()
        return rows[:, :m_].copy()

    def close(self):
        self.ws.close()


def test_wave_rows_at_stride_cap_and_refusals_leave_the_session_usable():
    """hop12, 3 utterances, total announced (audio flows from the fifth frame on).  Every correct
    call passes cap = m + 7: row u of the audio starts at wave[u·cap], columns [m, cap) and
    everything past the last row keep the sentinel.  In between, calls the library must refuse
    before any state advances — cap = m − 1, wave = NULL with m > 0 — return WRNN_EINVAL with its
    message and n_out = 0; the session then goes on, and its whole audio is the oracle's."""
    inp, m = _case("std512", "hop12", 3, 24, STD)
    mel, noise, ref = _rows(inp, 3)
    s = _Raw(m, 3, 24, noise)
    try:
        chunks = [s.push(mel[:, :, 0:5]), s.push(mel[:, :, 5:6])]
        assert chunks[0].shape[1] == 12 and chunks[1].shape[1] == 12
        nxt = mel[:, :, 6:13]
        m_ = s.plan(7, False)
        assert m_ == 84
        small = torch.full((3 * m_,), SENTINEL, dtype=torch.float64, device=DEV)
        rc, got, msg = s.call(nxt, False, small.data_ptr(), m_ - 1)
        assert (rc, got) == (-1, 0) and msg == f"this push emits {m_} samples per utterance: wave holds {m_ - 1}", (rc, got, msg)
        rc, got, msg = s.call(nxt, False, None, m_)
        assert (rc, got) == (-1, 0) and msg == f"this push emits {m_} samples per utterance: wave holds 0", (rc, got, msg)
        torch.cuda.synchronize()
        assert (small.cpu().numpy() == SENTINEL).all()
        chunks += [s.push(nxt), s.push(mel[:, :, 13:24]), s.push(None, final=True)]
        assert m.loop_handle().info["last_path"] == 5
        rc, got, msg = s.call(None, True, None, 0)
        assert rc == -1 and "finished" in msg
    finally:
        s.close()
    _vs_oracle(chunks, ref, "hop12 U=3 cap = m + 7, refusals in between")


def test_draws_one_step_short_are_refused_before_the_push():
    """Injected draws for 10·hop − 1 steps: a push that brings the loop to step 10·hop is refused
    (WRNN_EINVAL, the library's message), one that stops a frame earlier is served, and the audio
    of the session up to there is the oracle's."""
    inp, m = _case("std512", "hop12", 3, 24, STD)
    mel, noise, ref = _rows(inp, 2)
    hop, look = inp.dims.hop_length, inp.dims.pad + 1
    short = np.ascontiguousarray(noise[:10 * hop - 1])
    s = _Raw(m, 2, 24, short)
    try:
        chunks = [s.push(mel[:, :, 0:8])]
        m_ = s.plan(10 + look - 8, False)
        buf = torch.full((2 * m_,), SENTINEL, dtype=torch.float64, device=DEV)
        rc, got, msg = s.call(mel[:, :, 8:10 + look], False, buf.data_ptr(), m_)
        assert (rc, got) == (-1, 0), (rc, got, msg)
        assert msg == f"the injected draws cover {10 * hop - 1} steps, the loop reaches {10 * hop}", msg
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        chunks.append(s.push(mel[:, :, 8:9 + look]))
        assert m.loop_handle().info["last_path"] == 5
    finally:
        s.close()
    _vs_oracle(chunks, ref[:, :9 * hop], "hop12 U=2 after a refused push, first 9 frames")


def test_empty_pushes_change_nothing():
    """A non-final push(None) and a zero-width mel, before the first frame, inside the look-ahead
    and in mid-session: [U][0] each time, and the audio is the oracle's."""
    inp, m = _case("std512", "hop12", 3, 24, STD)
    for total in (None, 24):
        _session(m, inp, 3, [None, 0, 2, None, 0, 7, None, 0, 15, None], total, f"hop12 U=3 total={total} with empty pushes")


def test_session_on_a_side_stream():
    """One whole session inside torch.cuda.stream(side): every call of the session (uploads,
    kernels, rocBLAS, the store swaps' copies, wrnn_check) is on that stream."""
    inp, m = _case("std512", "hop12", 3, 24, STD)
    m.loop_handle()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side != torch.cuda.default_stream(DEV)
        _session(m, inp, 3, [1, 2, 1, 5, 15], None, "hop12 U=3 on a side stream")
    side.synchronize()


# ---- 7. Philox at another geometry ----------------------------------------------------------------
@pytest.mark.parametrize("model,want_path", [("std512", 5), ("stdsparse896", 6)])
def test_philox_streamed_equals_one_shot_at_hop12(model, want_path):
    inp, m = _case(model, "hop12", 8 if model == "stdsparse896" else 3, 24, STD)
    mel = inp.mels[:1].copy()
    seed = 20240611
    want = m.generate(torch.from_numpy(mel), None, False, 11000, 550, False, seed=seed, row_offset=5, verbose=False)
    assert m.loop_handle().info["last_path"] == want_path
    got = np.concatenate(list(m.generate_stream(mel, 8, seed=seed, row_offset=5)))
    assert m.loop_handle().info["last_path"] == want_path
    assert got.shape == want.shape == (23 * inp.dims.hop_length,)
    err = float(np.abs(got - want).max())
    print(f"STREAM {model} hop12 Philox streamed vs generate(): max |Δ| {err:.3g}")
    assert err <= gf.MOL_TOL
    other = np.concatenate(list(m.generate_stream(mel, 8, seed=seed, row_offset=6)))
    assert np.abs(other - want).max() > 1e-3
