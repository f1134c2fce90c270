"""Group pushes (wrnn_stream_push_group, WaveRNN.push_streams): independent streaming sessions of
one handle advanced in one call, each by its own frames with its own end, their rows sharing one
persistent launch per time chunk — row (session, utterance) on its own XCD over its own step
window (the kernels' grouped instantiation, csrc/fatchord_xcd.h: XcdRow).

Measured on MI355X (max |Δ| against the oracle, bound 2e-5): ragged dense 3.0e-8; eight rows sparse
hop12 / dense hop2 ≤ 3.5e-8 / 2.8e-8; chunked (1 and 77 steps per launch) 3.0e-8 and bit for bit
the unchunked group; hot dense / sparse 6.0e-7 / 4.8e-7; Philox against generate() 0 (bound
MOL_TOL); after refusals 3.0e-8.  Every grouped member was bit-identical to its session alone.

Every expectation is `oracle.generate` on ONE utterance alone: its own mel, truncated to its own
length, and its own column of the injected draws (`_alone`, computed once per process and shared;
whole-length utterances take regimes.stream_inputs' own).  The bound is 2·MOL_TOL, the project's
bound for whole-generate() comparisons with the oracle (tests/test_gpu_streaming_shapes.py); the
Philox case compares with one-shot generate() at MOL_TOL.  Every push must return exactly the count
`stream_plan` announces for that member (`_run`).  Where a case says "bit-identical" it is
np.array_equal against the same session pushed alone through push() on the same schedule: the
grouped kernel runs the same arithmetic per row, and no hand-off crosses XCDs.

A row that read another row's window (t0 / Lc / L), terms stride, state, granules, draws or output
origin fails cases 1–3: the members there differ in length, in frames received, in the tick they
end, in U (the terms stride of a U = 2 member is 2·N) and in the origin of their held-back sample
window (one total announced, the others unknown).

Mutations of the grouped instantiation (csrc/fatchord_xcd.hip, csrc/fatchord_xcds.hip):
  the terms step stride taken as N instead of U_s·N — built once into a scratch library and run once
      under this file (9 tests): fails exactly the two eight-row
      cases, at the U = 2 member (the only one whose stride is not N), from its second sample on:
      max |Δ| 4.8e-2 sparse, 1.5e-2 dense; the seven other tests pass.
  row k taking row 0's out_t0 — reasoned from the code, not run: the mutant stores sample t of row
      k at column t − out_t0(row 0) of row k's window, and where row 0's origin lies past t (case 1:
      row 0 has its total announced and has emitted audio, so its window has moved on, when the
      late member starts at t = 0) that column is negative: a store in front of the member's
      buffer, which must not be run on a shared GPU.  Where the origins differ the member's post
      reads columns nobody wrote, so cases 1, 2, 6 and 7 (one total announced beside unknown ones)
      would fail at the first emitted sample; cases 3 and 4 (equal origins throughout) would not.
  an empty row not returning early — reasoned from the code only, never run: a row with Lc = 0 that
      stayed would load its weights, run the prologue (at t0 = 0: publish and gather the step-0
      terms), skip the loop and reach the state write-back, which stores x from xs[(t_end − 1) & 1]
      — the slot of step t0 − 1's parity only by luck of the LDS image, uninitialised for t0 = 0 —
      over the member's carried state; the ring prefetch would also read the terms rows of steps
      t0 .. t0 + 2 from a d_T the host never filled for it.  The host never lists such a row
      (group_launches skips members without a runnable step), and the membership step of the
      kernel refuses it again (`Lc > 0`), before any weight load or hop wait.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import regimes as rg
from tests.golden import fixtures as gf
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


def _model(inp, key, fresh=False):
    """One WaveRNN on the GPU per (model, geometry, seed), shared by the tests (fresh: another one)."""
    from wavernn_amd.fatchord_version import WaveRNN
    if fresh or key not in _MODELS:
        m = WaveRNN(**inp.dims.ctor_kwargs()).to(DEV)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in inp.state.items()}, strict=True)
        if fresh:
            return m.eval()
        _MODELS[key] = m.eval()
    return _MODELS[key]


def _case(model, geom, n_utt, frames, seed):
    inp = rg.stream_inputs(model, geom, n_utt, frames, seed)
    return inp, _model(inp, (model, geom, seed))


@functools.lru_cache(maxsize=None)
def _alone(key, u, T):
    """oracle.generate of utterance u of stream_inputs(*key) alone, on its first T frames and its
    own column of the draws: float64 [(T − 1)·hop] (read-only, shared)."""
    from oracle import oracle
    inp = rg.stream_inputs(*key)
    if T == inp.mels.shape[2]:
        return inp.ref[u]
    hop = inp.dims.hop_length
    ref = oracle.generate(inp.state, inp.dims, np.ascontiguousarray(inp.mels[u][:, :T]), False, 0, 0, False,
                          np.ascontiguousarray(inp.noise[:T * hop, u:u + 1]))
    assert ref.shape == ((T - 1) * hop,) and ref.dtype == np.float64
    ref.setflags(write=False)
    return ref


class Member:
    """One session of a group: utterances [u0, u0 + U) of an input truncated to T frames, its
    schedule (one entry per tick: None = not listed, else (frames, final)), and its expectation."""

    def __init__(self, key, u0, U, T, sched, total=None, philox=None, noise_steps=None):
        inp = rg.stream_inputs(*key)
        hop = inp.dims.hop_length
        self.key, self.u0, self.U, self.T, self.sched, self.total = key, u0, U, T, sched, total
        self.mel = np.ascontiguousarray(inp.mels[u0:u0 + U, :, :T])
        self.kw = {}
        if philox is None:
            self.kw["noise"] = np.ascontiguousarray(inp.noise[:(noise_steps or T * hop), u0:u0 + U])
        else:
            self.kw.update(seed=philox[0], row_offset=philox[1])
        assert sum(e[0] for e in sched if e) == T and [e[1] for e in sched if e].count(True) == 1 and sched[-1][1]

    def ref(self):
        return np.stack([_alone(self.key, self.u0 + j, self.T) for j in range(self.U)])


def sched(counts, start=0, final_with_frames=False):
    """A schedule: not listed for `start` ticks, then one push per count (0: an empty push), the
    final flag on the last count's push or on an empty push after it."""
    s = [None] * start + [(n, False) for n in counts]
    if final_with_frames:
        s[-1] = (counts[-1], True)
    else:
        s.append((0, True))
    return s


def _run(m, members, grouped=True, between=None):
    """Drive the members through their schedules: per tick one push_streams over the members listed
    (grouped), or every member's whole session alone through push(), one after the other.  Each
    push must return the count stream_plan announces.  → ([U][(T − 1)·hop] per member, last_path)."""
    spec = m._upsample_spec()

    def want(mb, f, n, final):
        return stream_plan(spec, f + n, final, mb.total)[1] - stream_plan(spec, f, False, mb.total)[1]

    def chunk(mb, f, n):
        return mb.mel[:, :, f:f + n] if n else None

    chunks = [[] for _ in members]
    if not grouped:
        for i, mb in enumerate(members):
            with m.stream(mb.U, mb.total, **mb.kw) as s:
                f = 0
                for e in mb.sched:
                    if e is None:
                        continue
                    n, final = e
                    t = torch.from_numpy(chunk(mb, f, n).copy()).to(DEV) if n else None
                    out = s._session.push(t, final=final).cpu().numpy()
                    assert out.shape == (mb.U, want(mb, f, n, final)), (i, f, out.shape)
                    chunks[i].append(out)
                    f += n
        return [np.concatenate(c, 1) for c in chunks], m.loop_handle().info["last_path"]
    sess, f = [None] * len(members), [0] * len(members)
    try:
        for tick in range(max(len(mb.sched) for mb in members)):
            listed = [i for i, mb in enumerate(members) if tick < len(mb.sched) and mb.sched[tick] is not None]
            for i in listed:
                if sess[i] is None:
                    sess[i] = m.stream(members[i].U, members[i].total, **members[i].kw)
            pushes = [(sess[i], chunk(members[i], f[i], members[i].sched[tick][0]), members[i].sched[tick][1]) for i in listed]
            outs = m.push_streams(pushes) if pushes else []
            assert len(outs) == len(listed)
            for i, out in zip(listed, outs):
                n, final = members[i].sched[tick]
                assert out.dtype == np.float64 and out.shape == (members[i].U, want(members[i], f[i], n, final)), (tick, i, out.shape)
                chunks[i].append(out)
                f[i] += n
                assert sess[i]._session.frames == f[i] and sess[i]._session.finished == final
            if between:
                between(tick)
        path = m.loop_handle().info["last_path"]
    finally:
        for s in sess:
            if s is not None:
                s.close()
    return [np.concatenate(c, 1) for c in chunks], path


def _vs_oracle(out, ref, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    diff = np.abs(out - ref)
    print(f"GROUP {what}: max |Δ| {diff.max():.3g} over {diff.size} samples")
    assert diff.max() <= TOL, f"{what}: max |Δ| {diff.max():.3g}, first over at (row, sample) {tuple(np.argwhere(diff > TOL)[0])}"


def _check(m, members, what, want_path=5, alone=True, **kw):
    outs, path = _run(m, members, **kw)
    assert path == want_path, (what, path)
    for i, (mb, out) in enumerate(zip(members, outs)):
        _vs_oracle(out, mb.ref(), f"{what} member {i}")
    if alone:
        solo, _ = _run(m, members, grouped=False)
        for i, (a, b) in enumerate(zip(outs, solo)):
            assert np.array_equal(a, b), f"{what} member {i}: grouped differs from the session pushed alone, max |Δ| {np.abs(a - b).max():.3g}"
    return outs


RAGGED = ("std512", "hop12", 3, 30, STD)


def _ragged(philox=None):
    """Three U = 1 sessions of 21, 24 and 30 frames: 1-frame pushes with the total announced;
    5-frame pushes; a session that joins four ticks late, 3 frames per tick.  They end in ticks 21,
    5 and 14."""
    px = (lambda r: (philox, r)) if philox is not None else (lambda r: None)
    return [Member(RAGGED, 0, 1, 21, sched([1] * 21), total=21, philox=px(5)),
            Member(RAGGED, 1, 1, 24, sched([5, 5, 5, 5, 4]), philox=px(9)),
            Member(RAGGED, 2, 1, 30, sched([3] * 10, start=4), philox=px(2))]


# ---- 1. ragged lengths and schedules, dense ---------------------------------------------------------
def test_ragged_lengths_and_schedules_dense():
    inp, m = _case(*RAGGED)
    members = _ragged()
    assert sorted(len(mb.sched) for mb in members) == [6, 15, 22]   # they end in different ticks
    _check(m, members, "std512 hop12 ragged 21/24/30")


# ---- 2. eight rows, mixed U ------------------------------------------------------------------------
@pytest.mark.parametrize("model,geom,want_path", [("stdsparse896", "hop12", 6), ("std512", "hop2", 5)])
def test_eight_rows_mixed_u(model, geom, want_path):
    """One U = 2 session (terms stride 2·N, rows on XCDs 0 and 1) and six U = 1 sessions of 24, 22
    and 21 frames.  Look-ahead 4: tick 0 gives everyone 2 frames (no member has a runnable step: no
    persistent launch, every count 0), tick 1 brings only the U = 2 member past its look-ahead (the
    others get n = 0), later ticks leave some members empty-handed while the others run."""
    key = (model, geom, 8, 24, STD)
    inp, m = _case(*key)
    assert inp.dims.pad + 1 == 4
    members = [Member(key, 0, 2, 24, sched([2, 3, 4, 0, 7, 8])),
               Member(key, 2, 1, 24, sched([2, 0, 4, 6, 0, 12])),
               Member(key, 3, 1, 22, sched([2, 0, 0, 9, 5, 6], final_with_frames=True)),
               Member(key, 4, 1, 21, sched([2, 0, 1, 1, 10, 7]), total=21),
               Member(key, 5, 1, 24, sched([2, 0, 8, 8, 6])),
               Member(key, 6, 1, 22, sched([2, 0, 2, 0, 9, 9]), total=22),
               Member(key, 7, 1, 21, sched([2, 0, 5, 5, 5, 4], final_with_frames=True))]
    assert sum(mb.U for mb in members) == 8 and len({mb.T for mb in members}) == 3
    _check(m, members, f"{model} {geom} eight rows", want_path=want_path)


# ---- 3. uneven step counts under chunking -----------------------------------------------------------
def test_uneven_step_counts_under_chunking(monkeypatch):
    """hop12, look-ahead 4: tick 0 makes 12 steps runnable in one session (5 frames) and 84 in the
    other (11), tick 1 and later 12 and 36 (1 and 3 frames).  The budget is shared by the rows with
    steps: at 77 steps per launch tick 0 is 77 + 7 with the short member gone from round 2; at one
    step per launch the short member drops out after 12 of 36 (84) rounds."""
    inp, m = _case(*RAGGED)
    members = [Member(RAGGED, 0, 1, 21, sched([5] + [1] * 16)), Member(RAGGED, 1, 1, 24, sched([11, 3, 3, 3, 3, 1]))]
    whole = _check(m, members, "chunking: one launch per tick")
    for steps in (1, geo.GEOMS["hop12"][7]):
        monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 2, geo.N_TERMS))
        got = _check(m, members, f"chunking: {steps} step(s) per launch", alone=False)
        for i, (a, b) in enumerate(zip(got, whole)):
            assert np.array_equal(a, b), f"{steps} step(s) per launch, member {i}: differs from the unchunked group"


# ---- 4. hot states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key,want_path", [(rg.STREAM_HOT_DENSE, 5), (rg.STREAM_HOT_SPARSE, 6)], ids=["dense", "sparse"])
def test_hot_states(key, want_path):
    """The full-amplitude sessions of tests/regimes.py (x = ±1 carried through the state between
    launches; CPU preconditions in tests/test_regimes.py) as two U = 1 sessions: 1-frame pushes and
    3-frame pushes, each against its own oracle output."""
    inp, m = _case(*key)
    T = key[3]
    pos, neg = rg.stream_clamps(inp.ref, inp.dims.hop_length)
    assert pos.any() and neg.any()
    members = [Member(key, 0, 1, T, sched([1] * T)), Member(key, 1, 1, T, sched([3] * (T // 3)))]
    _check(m, members, f"hot {key[0]}", want_path=want_path)


# ---- 5. Philox -------------------------------------------------------------------------------------
def test_philox_rows_keep_their_keys():
    """Seed s and row_offset 5, 9, 2: each member equals one-shot generate() of its own mel with its
    own key, whatever XCD the group gave it."""
    inp, m = _case(*RAGGED)
    seed = 20240611
    members = _ragged(philox=seed)
    outs, path = _run(m, members)
    assert path == 5
    for mb, out in zip(members, outs):
        want = m.generate(torch.from_numpy(mb.mel), None, False, 11000, 550, False, seed=seed, row_offset=mb.kw["row_offset"],
                          verbose=False)
        err = float(np.abs(out[0] - want).max())
        print(f"GROUP Philox row_offset {mb.kw['row_offset']}: streamed vs generate() max |Δ| {err:.3g}")
        assert out[0].shape == want.shape and err <= gf.MOL_TOL


# ---- 6. interleaving -------------------------------------------------------------------------------
def test_other_work_between_group_pushes():
    """A one-shot generate() and a single push() of a non-member session between group pushes (they
    take the handle's control words, membership counters and XCDs in between): every member's audio
    is bit-identical to the run without them."""
    inp, m = _case(*RAGGED)
    members = _ragged()
    plain, _ = _run(m, members)
    other = m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:, 2:3]))
    fed = [0]

    def between(tick):
        if tick in (2, 7):
            m.generate(torch.from_numpy(inp.mels[:1, :, :21].copy()), None, False, 11000, 550, False, seed=1, verbose=False)
        if tick in (3, 7, 8) and fed[0] < 30:
            other.push(inp.mels[2:3, :, fed[0]:fed[0] + 6])
            fed[0] += 6

    try:
        mixed, _ = _run(m, members, between=between)
    finally:
        other.close()
    assert fed[0] == 18
    for i, (a, b) in enumerate(zip(mixed, plain)):
        assert np.array_equal(a, b), f"member {i} changed by work between the group pushes"
        _vs_oracle(a, members[i].ref(), f"interleaved member {i}")


# ---- 7. refusals are atomic ------------------------------------------------------------------------
SENTINEL = -7.25


def _raw_group(loop, items):
    """wrnn_stream_push_group itself: items = (FatchordStream, mel [U][feat][n] or None, final, cap)
    → (status, n_out list, message, wave buffers)."""
    count = len(items)
    vps, ints = ctypes.c_void_p * count, ctypes.c_int * count
    mels = [torch.from_numpy(np.ascontiguousarray(mel)).to(DEV) if mel is not None and mel.shape[2] else None for _, mel, _, _ in items]
    waves = [torch.full((max(1, s.n_streams * cap),), SENTINEL, dtype=torch.float64, device=DEV) for s, _, _, cap in items]
    got = ints(*([-1] * count))
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc = nat.lib().wrnn_stream_push_group(vps(*[s._s.value for s, _, _, _ in items]), count,
                                          vps(*[t.data_ptr() if t is not None else None for t in mels]),
                                          ints(*[t.shape[2] if t is not None else 0 for t in mels]),
                                          ints(*[int(f) for _, _, f, _ in items]), vps(*[w.data_ptr() for w in waves]),
                                          ints(*[cap for _, _, _, cap in items]), got, st)
    msg = (nat.lib().wrnn_last_error(loop._h) or b"").decode(errors="replace")
    torch.cuda.synchronize()
    return rc, list(got), msg, waves


def test_refusals_are_atomic():
    """Three members (21 frames with the total announced, 24, 30) advance by group pushes; a fourth
    session is finished, a fifth has injected draws one step short of 10 frames, a U = 8 session and
    a session of another handle stand by.  Each refused call — nine rows, a session listed twice,
    sessions of two handles, a finished member, one member's cap one short, one member's draws one
    step short — returns WRNN_EINVAL with the library's message, n_out = 0 for everyone and
    untouched wave buffers; afterwards every member goes on and its whole audio is its oracle's."""
    inp, m = _case(*RAGGED)
    hop, look = inp.dims.hop_length, inp.dims.pad + 1
    spec = m._upsample_spec()
    loop = m.loop_handle()
    m2 = _model(inp, None, fresh=True)
    mel = inp.mels
    A = m.stream(1, 21, noise=np.ascontiguousarray(inp.noise[:21 * hop, 0:1]))
    B = m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:24 * hop, 1:2]))
    C = m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:, 2:3]))
    done = m.stream(1, 21, noise=np.ascontiguousarray(inp.noise[:21 * hop, 0:1]))
    short = m.stream(1, 24, noise=np.ascontiguousarray(inp.noise[:10 * hop - 1, 1:2]))
    wide = m.stream(8, None, seed=3)
    alien = m2.stream(1, None, seed=3)
    sessions = [A, B, C, done, short, wide, alien]
    try:
        done.push(mel[0:1, :, :21])
        done.finish()
        a, b, c = (m.push_streams([(A, mel[0:1, :, :8], False), (B, mel[1:2, :, :8], False), (C, mel[2:3, :, :8], False)]))
        short_out = [short.push(mel[1:2, :, :8])]
        outs = {0: [a], 1: [b], 2: [c]}
        nxt = [(A._session, mel[0:1, :, 8:9], False, hop), (B._session, mel[1:2, :, 8:11], False, 0), (C._session, None, False, 0)]
        assert stream_plan(spec, 9, False, 21)[1] - stream_plan(spec, 8, False, 21)[1] == hop

        def refused(items, text):
            rc, got, msg, waves = _raw_group(loop, items)
            assert rc == -1 and got == [0] * len(items), (rc, got, msg)
            assert text in msg, msg
            for w in waves:
                assert (w.cpu().numpy() == SENTINEL).all()

        refused(nxt[:1] + [(wide._session, None, False, 0)], "at most 8 rows (one per XCD): these members have 9")
        refused(nxt + [nxt[0]], "members 0 and 3 are the same session")
        refused(nxt + [(alien._session, None, False, 0)], "member 3 belongs to another handle")
        refused(nxt + [(done._session, None, False, 0)], "member 3: push after the final one: the session is finished")
        refused([(A._session, mel[0:1, :, 8:9], False, hop - 1)] + nxt[1:],
                f"member 0: this push emits {hop} samples per utterance: wave holds {hop - 1}")
        refused(nxt + [(short._session, mel[1:2, :, 8:10 + look], False, 10 * hop)],
                f"member 3: the injected draws cover {10 * hop - 1} steps, the loop reaches {10 * hop}")
        # every member goes on: the refused frames again, then the rest
        a, b, c, s_ = m.push_streams([(A, mel[0:1, :, 8:9], False), (B, mel[1:2, :, 8:11], False), (C, None, False),
                                      (short, mel[1:2, :, 8:9 + look], False)])
        outs[0].append(a), outs[1].append(b), outs[2].append(c), short_out.append(s_)
        a, b, c = m.push_streams([(A, mel[0:1, :, 9:21], True), (B, mel[1:2, :, 11:24], False), (C, mel[2:3, :, 8:30], False)])
        outs[0].append(a), outs[1].append(b), outs[2].append(c)
        b, c = m.push_streams([(B, None, True), (C, None, True)])
        outs[1].append(b), outs[2].append(c)
        with pytest.raises(ValueError, match="ended"):
            m.push_streams([(A, None, True)])
        assert loop.info["last_path"] == 5
    finally:
        for s in sessions:
            s.close()
        del m2
    for i, T in enumerate((21, 24, 30)):
        _vs_oracle(np.concatenate(outs[i], 1), _alone(RAGGED, i, T)[None], f"after refusals member {i}")
    _vs_oracle(np.concatenate(short_out, 1), _alone(RAGGED, 1, 24)[None, :9 * hop], "after a refused push, draws one step short")
