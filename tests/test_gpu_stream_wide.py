"""Wide streaming groups (wrnn_stream_open_wide, WaveRNN.stream(wide=True)): sessions on the many-row
XCD kernel's grouped instantiation (csrc/fatchord_xcdm.h: XcdmRow) — up to 128 session rows per push,
16 per XCD, each row at its own step of its own utterance with its own draws, output window and
state record, the row set changing from push to push.

Measured on MI355X (max |Δ| against the oracle, bound 2e-5): nine rows 3.7e-8; twenty rows 4.2e-8; 40
and 128 rows ≤ 3.7e-8; hot dense 6.6e-7; Philox against generate() 3.0e-8 (bound MOL_TOL); a lock-step
U = 24 session 4.1e-8; interleaved and after refusals ≤ 3.7e-8.  Every grouped member was
bit-identical to its session alone, to itself in the reversed grouping, under 1 and 77 steps per
launch and with other work between the pushes.

Every expectation is `oracle.generate` on ONE utterance alone: its own mel, truncated to its own
length, and its own column of the injected draws (`_alone`, computed once per process and shared;
whole-length utterances take regimes.stream_inputs' own).  The bound is 2·MOL_TOL, the project's
bound for whole-generate() comparisons with the oracle; the Philox case compares with one-shot
generate() at MOL_TOL.  Every push must return exactly the count `stream_plan` announces for that
member (`_run`).  "Bit-identical" is np.array_equal: every wide launch is the four-quad form of the
kernel, in which batch rows are independent MFMA columns, so a row's bits depend neither on its
company nor on the XCD and slot it sits in.  Every case asserts last_path == 7.

A row that read another row's table entry (draws, output base, state record, resume flag, frame-term
stores or first step), or a state record addressed by (XCD, slot) instead of by row, fails cases 1–3:
the members there differ in length, in frames received, in the tick they join and end, in U and in
the origin of their held-back sample window, and the surviving rows are re-compacted into other
slots whenever a member drops out of a round.

Rows of one utterance (case 3) sit in sessions of one shape (the same U, the same schedule), so the
conditioning GEMMs that feed them have the same dimensions: the comparison is about the loop.
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
N_WIDE = 32 * 144            # kXcdWgs · kMRing floats per row and step (csrc/fatchord_xcdm.h)
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
    """One session of a group: the utterances `rows` of an input (an index may repeat: the same mel
    and the same draws in several rows) truncated to T frames, its schedule (one entry per tick:
    None = not listed, else (frames, final)), and its expectation."""

    def __init__(self, key, rows, T, sched, total=None, philox=None, noise_steps=None, wide=True):
        inp = rg.stream_inputs(*key)
        hop = inp.dims.hop_length
        rows = [rows] if isinstance(rows, int) else list(rows)
        self.key, self.rows, self.U, self.T, self.sched, self.total = key, rows, len(rows), T, sched, total
        self.mel = np.ascontiguousarray(inp.mels[rows][:, :, :T])
        self.kw = {"wide": wide}
        if philox is None:
            self.kw["noise"] = np.ascontiguousarray(inp.noise[:(noise_steps or T * hop)][:, rows])
        else:
            self.kw.update(seed=philox[0], row_offset=philox[1])
        assert sum(e[0] for e in sched if e) == T and [e[1] for e in sched if e].count(True) == 1 and sched[-1][1]

    def ref(self, j=None):
        if j is not None:
            return _alone(self.key, self.rows[j], self.T)
        return np.stack([_alone(self.key, u, self.T) for u in self.rows])


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
    print(f"WIDE {what}: max |Δ| {diff.max():.3g} over {diff.size} samples")
    assert diff.max() <= TOL, f"{what}: max |Δ| {diff.max():.3g}, first over at (row, sample) {tuple(np.argwhere(diff > TOL)[0])}"


def _check(m, members, what, alone=True, **kw):
    outs, path = _run(m, members, **kw)
    assert path == 7, (what, path)
    for i, (mb, out) in enumerate(zip(members, outs)):
        _vs_oracle(out, mb.ref(), f"{what} member {i}")
    if alone:
        solo, path = _run(m, members, grouped=False)
        assert path == 7, (what, path)
        for i, (a, b) in enumerate(zip(outs, solo)):
            assert np.array_equal(a, b), f"{what} member {i}: grouped differs from the session pushed alone, max |Δ| {np.abs(a - b).max():.3g}"
    return outs


# Twenty utterances of 30 frames at hop 12 (360 steps each); the first nine are also run truncated
WIDE = ("std512", "hop12", 20, 30, STD)
T_OF = {0: 21, 1: 24, 2: 30, 3: 21, 4: 24, 5: 30, 6: 21, 7: 24, 8: 30}


def _singles():
    """Utterances 0..8 and 14..19 as U = 1 wide sessions of 21 / 24 / 30 frames: 1-frame pushes with
    the total announced, several-frame pushes, empty pushes in between, members that join one, two
    and four ticks late, a final flag with and without frames.  The first nine are case 1's."""
    S = {0: dict(sched=sched([1] * 21), total=21), 1: dict(sched=sched([5, 5, 5, 5, 4])),
         2: dict(sched=sched([3] * 10, start=4)), 3: dict(sched=sched([7, 7, 7], final_with_frames=True)),
         4: dict(sched=sched([3] * 8)), 5: dict(sched=sched([10, 10, 10])),
         6: dict(sched=sched([4, 0, 4, 0, 4, 0, 4, 5])), 7: dict(sched=sched([8, 8, 8], start=1)),
         8: dict(sched=sched([2] * 15)), 14: dict(sched=sched([1, 3] * 7 + [2])), 15: dict(sched=sched([15, 15])),
         16: dict(sched=sched([5] * 6, start=2)), 17: dict(sched=sched([30], final_with_frames=True)),
         18: dict(sched=sched([4, 4, 4, 4, 4, 4, 6])), 19: dict(sched=sched([9, 0, 0, 9, 12]))}
    return [Member(WIDE, u, T_OF.get(u, 30), **S[u]) for u in sorted(S)]


_NINE = {}


def _nine(m):
    """Case 1's group run unchunked, once per process (cases 1 and 4 share it)."""
    if "outs" not in _NINE:
        members = _singles()[:9]
        _NINE["members"], _NINE["outs"] = members, _check(m, members, "nine rows")
    return _NINE["members"], _NINE["outs"]


# ---- 1. nine rows ----------------------------------------------------------------------------------
def test_nine_rows():
    """Nine U = 1 wide sessions of 21 / 24 / 30 frames: XCD 0 holds two rows (launch rows 0 and 8)
    while all nine run, the others one; each against its oracle and bit-identical to the session
    pushed alone through push() on the same schedule (a wide group of one)."""
    inp, m = _case(*WIDE)
    members, _ = _nine(m)
    assert len(members) == 9 and sorted({mb.T for mb in members}) == [21, 24, 30]
    assert len({len(mb.sched) for mb in members}) >= 4 and sum(mb.sched[0] is None for mb in members) == 2
    assert sum(mb.total is not None for mb in members) == 1


# ---- 2. slots move ---------------------------------------------------------------------------------
def test_slots_move():
    """Twenty rows: one U = 3 session, one U = 2 (four ticks late), fifteen U = 1.  Members end in many
    different ticks and join late, so the surviving rows change XCD and slot from round to round; a
    second grouping lists the members in reverse order, which puts every row elsewhere again."""
    inp, m = _case(*WIDE)
    members = [Member(WIDE, [9, 10, 11], 30, sched([6] * 5)), Member(WIDE, [12, 13], 30, sched([3] * 10, start=4))] + _singles()
    assert sum(mb.U for mb in members) == 20 and sorted(mb.U for mb in members)[-2:] == [2, 3]
    assert len({len(mb.sched) for mb in members}) >= 4 and sum(mb.sched[0] is None for mb in members) >= 2
    outs = _check(m, members, "twenty rows", alone=False)
    back, path = _run(m, members[::-1])
    assert path == 7
    for i, (a, b) in enumerate(zip(outs, back[::-1])):
        assert np.array_equal(a, b), f"member {i}: differs when the group lists its members in reverse order"


# ---- 3. two quads on an XCD and the full width -------------------------------------------------------
@pytest.mark.parametrize("rows", [40, 128])
def test_quads_and_full_width(rows):
    """Sixteen distinct utterances (0..8 truncated as above, 9..15 whole): even ones pushed 1 frame
    per tick, odd ones 3, the last four two ticks late — so every tick has members that differ in
    step count (12 and 36 steps: two rounds, the short members drop out and the rest are compacted).
    40 rows: utterances 0..7 as two U = 2 sessions, 8..15 as one U = 1 session (slots 0..4 of every
    XCD in use: two quads).  128 rows: every utterance as two U = 4 sessions (every slot)."""
    inp, m = _case(*WIDE)
    members, owner = [], []
    for u in range(16):
        T = T_OF.get(u, 30)
        sc = sched([1] * T if u % 2 == 0 else [3] * (T // 3), start=2 if u >= 12 else 0)
        shapes = [4, 4] if rows == 128 else [2, 2] if u < 8 else [1]
        for U in shapes:
            members.append(Member(WIDE, [u] * U, T, sc))
            owner.append(u)
    assert sum(mb.U for mb in members) == rows
    outs, path = _run(m, members)
    assert path == 7
    first = {}
    for mb, u, out in zip(members, owner, outs):
        if u not in first:
            first[u] = out[0]
            _vs_oracle(out[:1], mb.ref(0)[None], f"{rows} rows, utterance {u}")
        for j in range(mb.U):
            assert np.array_equal(out[j], first[u]), f"{rows} rows: two rows of utterance {u} on one schedule differ"
    assert len(first) == 16


# ---- 4. chunking -------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, geo.GEOMS["hop12"][7]])
def test_chunked_launches(monkeypatch, steps):
    """Case 1's members at 1 step and at 77 steps per launch (the budget is shared by the rows with
    steps to run: nine while all run): bit-identical to the unchunked run."""
    inp, m = _case(*WIDE)
    members, whole = _nine(m)
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 9, N_WIDE))
    got, path = _run(m, members)
    assert path == 7
    for i, (a, b) in enumerate(zip(got, whole)):
        assert np.array_equal(a, b), f"{steps} step(s) per launch, member {i}: differs from the unchunked group"


# ---- 5. hot states -----------------------------------------------------------------------------------
def test_hot_states():
    """The full-amplitude dense sessions of tests/regimes.py as two wide U = 1 sessions, 1-frame and
    3-frame pushes: x = ±1 is carried through the per-row state records between launches."""
    key = rg.STREAM_HOT_DENSE
    inp, m = _case(*key)
    T = key[3]
    pos, neg = rg.stream_clamps(inp.ref, inp.dims.hop_length)
    assert pos.any() and neg.any()
    members = [Member(key, 0, T, sched([1] * T)), Member(key, 1, T, sched([3] * (T // 3)))]
    _check(m, members, "hot mol512")


# ---- 6. Philox ---------------------------------------------------------------------------------------
def test_philox_rows_keep_their_keys():
    """One seed and row_offset 5, 9, 2: each member equals one-shot generate() of its own mel with its
    own key, whatever slot the group gave it."""
    inp, m = _case(*WIDE)
    seed = 20240611
    members = [Member(WIDE, 0, 21, sched([1] * 21), total=21, philox=(seed, 5)),
               Member(WIDE, 1, 24, sched([5, 5, 5, 5, 4]), philox=(seed, 9)),
               Member(WIDE, 2, 30, sched([3] * 10, start=4), philox=(seed, 2))]
    outs, path = _run(m, members)
    assert path == 7
    for mb, out in zip(members, outs):
        want = m.generate(torch.from_numpy(mb.mel), None, False, 11000, 550, False, seed=seed, row_offset=mb.kw["row_offset"],
                          verbose=False)
        err = float(np.abs(out[0] - want).max())
        print(f"WIDE Philox row_offset {mb.kw['row_offset']}: streamed vs generate() max |Δ| {err:.3g}")
        assert out[0].shape == want.shape and err <= gf.MOL_TOL


# ---- 7. a lock-step wide session ---------------------------------------------------------------------
def test_lock_step_wide_session():
    """stream(24, wide=True): 24 utterances in lock step (the twenty and four of them again) in one
    session, three quads' worth of rows; and generate_stream(..., wide=True) of one utterance."""
    inp, m = _case(*WIDE)
    rows = list(range(20)) + [3, 0, 19, 7]
    mb = Member(WIDE, rows, 30, sched([4, 1, 7, 0, 6, 12]))
    (out,), path = _run(m, [mb], grouped=False)
    assert path == 7
    _vs_oracle(out, mb.ref(), "lock step, 24 rows")
    for j, u in enumerate(rows[20:]):
        assert np.array_equal(out[20 + j], out[u]), f"rows {20 + j} and {u} hold the same utterance and differ"
    chunks = list(m.generate_stream(inp.mels[5:6], 7, noise=np.ascontiguousarray(inp.noise[:, 5:6]), wide=True))
    assert m.loop_handle().info["last_path"] == 7 and all(c.ndim == 1 for c in chunks)
    _vs_oracle(np.concatenate(chunks)[None], inp.ref[5:6], "generate_stream(wide=True)")


# ---- 8. interleaving ---------------------------------------------------------------------------------
def test_other_work_between_wide_pushes():
    """Between wide group pushes: a fold-batched generate() (15 folds: its own many-row launches over
    the handle's hop area, state and terms), a narrow session's push() and a narrow push_streams.
    Every wide member is bit-identical to the run without them, and the narrow results to theirs."""
    inp, m = _case(*WIDE)
    members = _singles()[:9]
    plain, _ = _run(m, members)
    mel_b = torch.from_numpy(inp.mels[9:10].copy())

    def others(hook):
        """The other work, in the order the ticks call for it → its results."""
        got = {"gen": [], "solo": [], "pair": []}
        hop = inp.dims.hop_length
        solo = m.stream(1, 24, noise=np.ascontiguousarray(inp.noise[:24 * hop, 10:11]))
        pair = [m.stream(1, 21, noise=np.ascontiguousarray(inp.noise[:21 * hop, 11 + j:12 + j])) for j in range(2)]
        fed = [0, 0]

        def between(tick):
            if tick in (2, 7):
                got["gen"].append(m.generate(mel_b, None, True, 20, 4, False, seed=1, verbose=False))
            if tick in (3, 7, 8):
                got["solo"].append(solo.push(inp.mels[10:11, :, fed[0]:fed[0] + 8]))
                fed[0] += 8
            if tick in (1, 5, 9):
                got["pair"].append(m.push_streams([(s, inp.mels[11 + j:12 + j, :, fed[1]:fed[1] + 7], False) for j, s in enumerate(pair)]))
                fed[1] += 7

        try:
            res = hook(between)
            got["solo"].append(solo.finish())
            got["pair"].append(m.push_streams([(s, None, True) for s in pair]))
        finally:
            for s in [solo] + pair:
                s.close()
        assert len(got["gen"]) == 2 and fed == [24, 21] and sum(x.shape[1] for x in got["solo"]) == 23 * hop
        return res, got

    def bare(between):
        for tick in range(10):
            between(tick)

    _, want = others(bare)
    (mixed, path), got = others(lambda between: _run(m, members, between=between))
    assert path == 7
    for i, (a, b) in enumerate(zip(mixed, plain)):
        assert np.array_equal(a, b), f"wide member {i} changed by work between the group pushes"
        _vs_oracle(a, members[i].ref(), f"interleaved member {i}")
    for a, b in zip(got["gen"] + got["solo"], want["gen"] + want["solo"]):
        assert np.array_equal(a, b), "a one-shot generate() or a narrow push changed between wide pushes"
    for a, b in zip(got["pair"], want["pair"]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "a narrow group push changed between wide pushes"


# ---- 9. refusals are atomic --------------------------------------------------------------------------
SENTINEL = -7.25
RAGGED = ("std512", "hop12", 3, 30, STD)


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
    """Three wide members (21 frames with the total announced, 24, 30) advance by group pushes; a
    fourth wide session is finished, a fifth has injected draws one step short of 10 frames, a wide
    U = 126 session and a narrow session stand by.  Each refused call — 129 rows, a wide and a narrow
    member, a session listed twice, a finished member, one member's cap one short, one member's draws
    one step short — returns WRNN_EINVAL with the library's message, n_out = 0 for everyone and
    untouched wave buffers; afterwards every member goes on and its whole audio is its oracle's."""
    inp, m = _case(*RAGGED)
    hop, look = inp.dims.hop_length, inp.dims.pad + 1
    spec = m._upsample_spec()
    loop = m.loop_handle()
    mel = inp.mels
    A = m.stream(1, 21, noise=np.ascontiguousarray(inp.noise[:21 * hop, 0:1]), wide=True)
    B = m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:24 * hop, 1:2]), wide=True)
    C = m.stream(1, None, noise=np.ascontiguousarray(inp.noise[:, 2:3]), wide=True)
    done = m.stream(1, 21, noise=np.ascontiguousarray(inp.noise[:21 * hop, 0:1]), wide=True)
    short = m.stream(1, 24, noise=np.ascontiguousarray(inp.noise[:10 * hop - 1, 1:2]), wide=True)
    big = m.stream(126, None, seed=3, wide=True)
    narrow = m.stream(1, None, seed=3)
    sessions = [A, B, C, done, short, big, narrow]
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

        refused(nxt + [(big._session, None, False, 0)], "a wide group has at most 128 rows (16 per XCD): these members have 129")
        refused(nxt + [(narrow._session, None, False, 0)], "member 3 runs another loop kernel than member 0")
        refused(nxt + [nxt[0]], "members 0 and 3 are the same session")
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
        assert loop.info["last_path"] == 7
    finally:
        for s in sessions:
            s.close()
    for i, T in enumerate((21, 24, 30)):
        _vs_oracle(np.concatenate(outs[i], 1), _alone(RAGGED, i, T)[None], f"after refusals member {i}")
    _vs_oracle(np.concatenate(short_out, 1), _alone(RAGGED, 1, 24)[None, :9 * hop], "after a refused push, draws one step short")


# ---- 10. narrow groups unchanged -----------------------------------------------------------------------
def test_narrow_groups_keep_their_limit():
    """Nine narrow rows are refused as before, word for word; a wide session opened on the same handle
    (so that the wide path exists) does not change that."""
    inp, m = _case(*RAGGED)
    loop = m.loop_handle()
    eight, one, w = m.stream(8, None, seed=3), m.stream(1, None, seed=4), m.stream(1, None, seed=5, wide=True)
    try:
        rc, got, msg, waves = _raw_group(loop, [(one._session, None, False, 0), (eight._session, None, False, 0)])
        assert rc == -1 and got == [0, 0]
        assert "a group has at most 8 rows (one per XCD): these members have 9" in msg, msg
        with pytest.raises(ValueError, match=r"at most 8 rows \(one per XCD\): these members have 9"):
            m.push_streams([(one, None, False), (eight, None, False)])
        out = w.push(inp.mels[0:1, :, :8])
        assert out.shape == (1, 0) or out.shape[0] == 1
        assert loop.info["last_path"] == 7
    finally:
        for s in (eight, one, w):
            s.close()
