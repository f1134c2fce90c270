"""Wide lists on the MI355X: WaveRNN.generate_list(wide=True) / wrnn_generate_list_wide — a list of
utterances of unequal length on up to 128 slots of the many-row XCD kernel's grouped launches, MoL and
RAW (include/wavernn_amd.h, "Wide lists"; the host side is tests/test_list_wide_plan.py), and the
one-launch post wrnn_postprocess_list.

Every expectation is oracle.generate on ONE utterance alone (its own mel truncated to its own length,
its own column of the draws), built from tests/regimes.py, tests/geometries.py and
tests/raw_streams.py.  MoL: |Δ| <= 2e-5 (the wide bound, 2·MOL_TOL); under Philox <= MOL_TOL of
generate(seed=, row_offset=r + i).  RAW: raw_streams.check — with mu_law off every sample before the
fade equals the oracle's bit for bit (the labels are exact), the fade within rtol 1e-12; with mu_law
on rtol 1e-12 throughout.  "Bit-identical" is np.array_equal.  What each case would catch:
  1     a slot reused after an end with its predecessor's state, an utterance resumed from the wrong
        record after its row moved to another launch row (compaction);
  2, 3  any dependence of a member on its company, its slot, the list order or `slots`;
  4     a launch boundary inside a frame, a look-ahead read past a launch's terms;
  5     every slot ending at once; the list of one;
  8     a wide list touching a session's records, the one-shot state or the narrow list's stores;
  9     a refusal that queued something or left the handle changed;
  10    the table-driven post against the per-utterance one.

Measured on MI355X: MoL against the oracle 3.7e-8 on the standard state and 6.6e-7 at full amplitude
(bound 2e-5), under Philox 2.2e-8 against generate() (bound 1e-5); RAW 0 differing samples with
mu_law off, 7.8e-16 relative with it on (bound 1e-12); every bit-for-bit comparison holds; the file
runs in 8 s."""
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import raw_streams as rs
from tests import regimes as rg
from tests.golden import fixtures as gf
from wavernn_amd import condition
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import list_wide_plan, wide_steps_per_launch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDES = ("WRNN_PATH", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES", "WRNN_TERMS_MB")
STD = rg.STREAM_STD_SEED
WIDE_TOL = 2 * gf.MOL_TOL                      # the many-row kernel against the oracle
N_MOL = 32 * 144                               # terms of one MoL row-step (kXcdWgs · kMRing)
# case 1: 11 utterances of 21 … 36 frames on 3 slots (hop 12)
FRAMES_1 = (30, 36, 25, 22, 33, 21, 27, 35, 24, 29, 23)
# case 2: 140 utterances of 21 … 45 frames on all 128 slots (hop 4): member i is pool utterance i % 12
FRAMES_2 = tuple(21 + (7 * i) % 25 for i in range(140))
SAMPLE_2 = (0, 3, 17, 31, 64, 100, 127, 128, 129, 133, 138, 139)   # slots with one and with two utterances
ALONE_2 = (3, 17, 64, 128, 133, 139)
SEED, ROW0 = 20240611, 5
_MODELS = {}


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


# ---- inputs ------------------------------------------------------------------------------------------
class Pool:
    """`n` utterances of up to `frames` frames at a geometry, with injected draws by the utterance's
    own step, and oracle.generate of any (utterance, length) alone (cached, read-only)."""

    def __init__(self, mode, geom, n, frames, hot=False):
        self.mode, self.geom = mode, geom
        if mode == "RAW":
            self.key = (geom, n, frames, rg.STATE_SEED if hot else STD, hot)
            inp = rs.inputs(*self.key)
            self.dims, self.state, self.mels, self.noise = inp.dims, inp.state, inp.mels, inp.noise
        elif hot:       # the full-amplitude MoL regime of tests/regimes.py (its oracle runs are at 24 frames)
            inp = rg.stream_inputs(*rg.STREAM_HOT_DENSE)
            assert (geom, n, frames) == rg.STREAM_HOT_DENSE[1:4]
            self.dims, self.state, self.mels, self.noise = inp.dims, inp.state, inp.mels, inp.noise
        else:           # the standard rnn-512 state of regimes.stream_inputs("std512", geom, …), without its oracle runs
            d = geo.geom_dims(geom, rnn_dims=512)
            state = geo.perturb_taps(syn.make_fatchord_state(d, STD), d, STD)
            mels = np.stack([syn.make_mel(d.feat_dims, frames, 1000 * STD + 40 + i) for i in range(n)])
            noise = syn.make_noise(d.mode, n, frames * d.hop_length, d.n_classes, 1000 * STD + 21)
            for a in (mels, noise):
                a.setflags(write=False)
            self.dims, self.state, self.mels, self.noise = d, state, mels, noise
        self.hop, self.n = self.dims.hop_length, n
        self._ref = {}

    def mel(self, u, T):
        return np.array(self.mels[u % self.n][None, :, :T], order="C")

    def draws(self, u, T):
        return np.array(self.noise[:T * self.hop, u % self.n], order="C")

    def ref(self, u, T, mu_law=False):
        from oracle import oracle
        k = (u % self.n, T, mu_law)
        if k not in self._ref:
            if self.mode == "RAW":
                self._ref[k] = rs.alone(self.key, u % self.n, T, mu_law)
            else:
                r = oracle.generate(self.state, self.dims, self.mel(u, T)[0], False, 0, 0, False,
                                    np.ascontiguousarray(self.draws(u, T)[:, None]))
                r.setflags(write=False)
                self._ref[k] = r
        return self._ref[k]

    def model(self):
        from wavernn_amd.fatchord_version import WaveRNN
        k = (self.mode, self.geom, id(self.state))
        if k not in _MODELS:
            m = WaveRNN(**self.dims.ctor_kwargs()).to(DEV)
            m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in self.state.items()}, strict=True)
            _MODELS[k] = m.eval()
        return _MODELS[k]


@functools.lru_cache(maxsize=None)
def pool(mode, geom, hot=False):
    if hot:
        return Pool(mode, geom, 2, 24, True)
    return Pool(mode, geom, 12, 45) if geom == "hop4" else Pool(mode, geom, 11, 36)


def _check(p, got, u, T, what, mu_law=False):
    ref = p.ref(u, T, mu_law)
    assert got.dtype == np.float64 and got.shape == ref.shape == ((T - 1) * p.hop,), (what, got.shape, ref.shape)
    if p.mode == "RAW":
        rs.check(got, ref, p.hop, mu_law, what)
        return 0.0
    err = float(np.abs(got - ref).max())
    print(f"WIDE LIST {what}: max |Δ| {err:.3g} vs the oracle (bound {WIDE_TOL:g})")
    assert err <= WIDE_TOL, f"{what}: max |Δ| {err:.3g} > {WIDE_TOL:g}"
    return err


def _run(p, members, mu_law=False, injected=True, **kw):
    """generate_list(wide=True) of the members (pool utterance, frames) → the waveforms; last_path 7."""
    m = p.model()
    mels = [p.mel(u, T) for u, T in members]
    if injected:
        kw["noise"] = [p.draws(u, T) for u, T in members]
    got = m.generate_list(mels, wide=True, mu_law=mu_law, **kw)
    assert m.loop_handle().info["last_path"] == 7
    assert len(got) == len(members)
    return got


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.float64 and a.shape == b.shape, (what, i, a.shape, b.shape)
        assert np.array_equal(a, b), f"{what}, utterance {i}: differs, max |Δ| {np.abs(a - b).max():.3g}"


@functools.lru_cache(maxsize=None)
def _case1(mode):
    """Case 1's run, once per process (cases 3 and 4 compare with it): read-only."""
    p = pool(mode, "hop12")
    members = tuple((i, T) for i, T in enumerate(FRAMES_1))
    got = _run(p, members, slots=3)
    for g in got:
        g.setflags(write=False)
    return members, tuple(got)


@functools.lru_cache(maxsize=None)
def _case2(mode):
    """Case 2's run: MoL under Philox (seed, row_offset), RAW with injected draws."""
    p = pool(mode, "hop4")
    members = tuple((i, T) for i, T in enumerate(FRAMES_2))
    if mode == "MOL":
        got = _run(p, members, injected=False, seed=SEED, row_offset=ROW0)
    else:
        got = _run(p, members)
    for g in got:
        g.setflags(write=False)
    return members, tuple(got)


# ---- 1. more utterances than slots ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_more_utterances_than_slots(mode):
    p = pool(mode, "hop12")
    slot_of, pos, _, launches = list_wide_plan(FRAMES_1, 3, hop=12, raw=mode == "RAW")
    assert max(pos) >= 3                                       # slots are reused after an end
    assert len({r for _, _, r in launches}) == 3               # rows fall 3 → 2 → 1: survivors are re-compacted
    # an utterance is resumed across several launches
    spans = [sum(1 for f, s, _ in launches if f < e and f + s > e - T * 12) for T, e in [(FRAMES_1[1], FRAMES_1[1] * 12)]]
    assert spans[0] >= 2
    members, got = _case1(mode)
    for i, (u, T) in enumerate(members):
        _check(p, got[i], u, T, f"{mode} 11 on 3 slots, utterance {i}")
    if mode == "RAW":
        lab = rs.labels_of(got[1], 12)
        assert lab.min() >= 0 and lab.max() < rs.NC and len(np.unique(lab)) > 20


# ---- 2. all 128 slots and one refill -------------------------------------------------------------------
def test_128_slots_philox_mol():
    p = pool("MOL", "hop4")
    m = p.model()
    slot_of, pos, _, _ = list_wide_plan(FRAMES_2, hop=4)
    assert sorted(set(slot_of)) == list(range(128)) and max(pos) == 1
    members, got = _case2("MOL")
    worst = 0.0
    for i in SAMPLE_2:
        u, T = members[i]
        want = m.generate(p.mel(u, T), None, False, 0, 0, False, seed=SEED, row_offset=ROW0 + i, verbose=False)
        assert got[i].shape == want.shape == ((T - 1) * 4,)
        worst = max(worst, float(np.abs(got[i] - want).max()))
    print(f"WIDE LIST 140 on 128 slots, Philox: max |Δ| {worst:.3g} vs generate(seed, row_offset + i) (bound {gf.MOL_TOL:g})")
    assert worst <= gf.MOL_TOL


def test_128_slots_injected_raw():
    p = pool("RAW", "hop4")
    members, got = _case2("RAW")
    for i in SAMPLE_2:
        u, T = members[i]
        _check(p, got[i], u, T, f"RAW 140 on 128 slots, utterance {i}")


# ---- 3. company independence, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_alone_reversed_serial_and_other_slot_counts(mode):
    p = pool(mode, "hop4")
    members, got = _case2(mode)
    kw = dict(injected=False, seed=SEED) if mode == "MOL" else {}
    for i in ALONE_2:                                          # a wide list of one, with row_offset + i
        alone = _run(p, [members[i]], row_offset=ROW0 + i, **kw) if mode == "MOL" else _run(p, [members[i]])
        _same(alone, [got[i]], f"{mode} utterance {i} of the 140 alone")
    seven = _run(p, members, slots=7, row_offset=ROW0, **kw) if mode == "MOL" else _run(p, members, slots=7)
    _same(seven, got, f"{mode} slots=128 against slots=7")
    # the reversed list and the serial queue, with injected draws (under Philox the row is the place in the list)
    if mode == "RAW":
        _same(_run(p, members[::-1])[::-1], got, "RAW the list of 140 reversed")
    m1, got1 = _case1(mode)
    p1 = pool(mode, "hop12")
    back = _run(p1, m1[::-1], slots=3)
    _same(back[::-1], got1, f"{mode} the list of 11 reversed")
    serial = _run(p1, m1[:5], slots=1)
    assert list_wide_plan(FRAMES_1[:5], 1, hop=12)[1] == [2, 0, 3, 4, 1]
    _same(serial, got1[:5], f"{mode} slots=1 on the first five")


# ---- 4. budget cuts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
@pytest.mark.parametrize("steps", [1, geo.GEOMS["hop12"][7]])
def test_budget_cuts(monkeypatch, mode, steps):
    p = pool(mode, "hop12")
    m1, got1 = _case1(mode)
    raw = mode == "RAW"
    uncut = len(list_wide_plan(FRAMES_1[:9], 9, hop=12, raw=raw)[3])
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 9, rs.N_RAW if raw else N_MOL))
    assert wide_steps_per_launch(9, 10 ** 6, raw=raw) == steps
    launches = list_wide_plan(FRAMES_1[:9], 9, hop=12, raw=raw)[3]
    assert launches[0] == (0, steps, 9) and len(launches) > uncut
    assert any(f % 12 for f, _, _ in launches)                 # launch boundaries inside frames
    got = _run(p, m1[:9], slots=9)
    _same(got, got1[:9], f"{mode} {steps} step(s) per launch against the uncut run")


# ---- 5. equal lengths, and the list of one -------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_equal_lengths_and_one(mode):
    p = pool(mode, "hop4")
    members = [(i, 24) for i in range(16)]
    assert list_wide_plan([24] * 16, hop=4, raw=mode == "RAW")[3] == [(0, 96, 16)]
    got = _run(p, members)
    for i in (0, 7, 8, 15):
        _check(p, got[i], i, 24, f"{mode} 16 × 24 frames, utterance {i}")
    _same([got[i] for i in range(12, 16)], [got[i - 12] for i in range(12, 16)], f"{mode} the same utterance in two slots")
    one = _run(p, [(7, 24)])
    _same(one, [got[7]], f"{mode} U = 1")


# ---- 6. mu-law on, RAW ---------------------------------------------------------------------------------
def test_raw_mu_law():
    p = pool("RAW", "hop12")
    members = [(0, 30), (3, 22), (5, 21), (2, 25)]
    got = _run(p, members, mu_law=True, slots=2)
    for i, (u, T) in enumerate(members):
        _check(p, got[i], u, T, f"RAW mu_law on, utterance {i}", mu_law=True)
    off = _run(p, members, mu_law=False, slots=2)
    assert not np.array_equal(off[0], got[0])


# ---- 7. saturated state --------------------------------------------------------------------------------
def test_full_amplitude_mol():
    p = pool("MOL", "hop12", True)
    inp = rg.stream_inputs(*rg.STREAM_HOT_DENSE)
    members = [(0, 24), (1, 24), (0, 21), (1, 22)]
    for u in (0, 1):
        p._ref[(u, 24, False)] = inp.ref[u]
    hi, lo = rg.stream_clamps(inp.ref, p.hop)
    assert hi.any() and lo.any(), "the regime does not reach both clamps"
    got = _run(p, members, slots=2)
    for i, (u, T) in enumerate(members):
        _check(p, got[i], u, T, f"hot mol512, utterance {i}")


# ---- 8. coexistence ------------------------------------------------------------------------------------
def test_neighbours_on_one_handle():
    p = pool("MOL", "hop12")
    m = p.model()
    wide_members, wide_want = _case1("MOL")
    wide_members, wide_want = wide_members[:5], wide_want[:5]
    narrow_mels = [p.mel(u, T) for u, T in ((6, 22), (7, 29), (8, 21))]
    one_mel = p.mel(9, 26)
    sess_mel = p.mel(10, 30)

    def session(between):
        parts = []
        with m.stream(1, 30, seed=11, row_offset=40, wide=True) as s:
            parts.append(s.push(sess_mel[:, :, :10]))
            between(0)
            # a push left outstanding on the stream while the wide list is queued behind it
            t = torch.from_numpy(sess_mel[:, :, 10:20].copy()).to(DEV)
            pending = s._session.push(t, check=False)
            between(1)
            parts.append(pending.cpu().numpy())
            parts.append(s.push(sess_mel[:, :, 20:]))
            between(2)
            parts.append(s.finish())
        return np.concatenate([q for q in parts if q.shape[1]], 1)

    def narrow():
        return m.generate_list(narrow_mels, seed=7)

    def one():
        return m.generate(one_mel, None, False, 0, 0, False, seed=3, row_offset=2, verbose=False)

    def wide():
        return _run(p, wide_members, slots=2)

    want = dict(session=session(lambda k: None), narrow=narrow(), one=one())
    _same(wide(), wide_want, "the wide list with two slots")
    got = dict(narrow=[], one=[], wide=[])

    def between(k):
        got["narrow"].append(narrow())
        got["one"].append(one())
        got["wide"].append(wide())
        got["one"].append(one())
        got["narrow"].append(narrow())

    mixed = session(between)
    assert np.array_equal(mixed, want["session"]), "the wide session changed by its neighbours"
    assert len(got["wide"]) == 3
    for g in got["wide"]:
        _same(g, wide_want, "a wide list among a session's pushes, a narrow list and generate()")
    for g in got["narrow"]:
        _same(g, want["narrow"], "the narrow list around a wide list")
    for g in got["one"]:
        assert np.array_equal(g, want["one"]), "generate() around a wide list"


# ---- 9. refusals ---------------------------------------------------------------------------------------
def _bare_model(mode="RAW", **dims_kw):
    """A model at hop 12 that no oracle run goes with (the refusals need none)."""
    from wavernn_amd.fatchord_version import WaveRNN
    d = geo.geom_dims("hop12", mode=mode, **dims_kw)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, STD).items()}, strict=True)
    return m.eval()


def test_refusals_leave_the_handle_usable():
    p = pool("RAW", "hop12")
    m = p.model()
    members = [(0, 30), (3, 22), (5, 21)]
    before = _run(p, members, slots=2)
    mels = [p.mel(u, T) for u, T in members]
    noise = [p.draws(u, T) for u, T in members]
    with pytest.raises(ValueError, match="slots is 1..128"):
        m.generate_list(mels, noise=noise, wide=True, slots=129)
    with pytest.raises(ValueError, match="slots is 1..128"):
        m.generate_list(mels, noise=noise, wide=True, slots=0)
    with pytest.raises(ValueError, match="lanes"):
        m.generate_list(mels, noise=noise, wide=True, lanes=2)
    with pytest.raises(ValueError, match="21 frames"):
        m.generate_list(mels + [p.mel(1, 20)], wide=True, seed=1)
    with pytest.raises(ValueError, match="one .* per utterance"):
        m.generate_list(mels, noise=noise[:2], wide=True)
    with pytest.raises(ValueError):                            # the MoL width
        m.generate_list(mels, noise=[z[:, :11] for z in noise], wide=True)
    with pytest.raises(NotImplementedError):                   # the narrow list stays MoL only
        m.generate_list(mels, seed=1)
    # the library's own checks, behind the Python ones
    loop, spec = m.loop_handle(), m._upsample_spec()
    fr = [m.frames(torch.from_numpy(x).to(DEV)) for x in mels + [p.mel(1, 20)]]
    with pytest.raises(ValueError, match="utterance 3 has 20 frames"):
        loop.generate_list_wide(spec, [f[0] for f in fr], [f[1] for f in fr], seed=1)
    with pytest.raises(ValueError, match="slots is 1..128"):
        loop.generate_list_wide(spec, [f[0] for f in fr[:3]], [f[1] for f in fr[:3]], slots=129, seed=1)
    x = [p.mel(0, 21)]
    with pytest.raises(NotImplementedError, match=r"512 classes \(bits = 9\): this handle has 1024 classes"):
        _bare_model(rnn_dims=512, bits=10).generate_list(x, wide=True, seed=1)
    with pytest.raises(NotImplementedError, match=r"rnn / fc 512\): this handle has rnn 896, fc 512"):
        _bare_model(rnn_dims=896).generate_list(x, wide=True, seed=1)
    with pytest.raises(NotImplementedError, match="four co-resident quads per XCD"):
        _bare_model("MOL", rnn_dims=896).generate_list(x, wide=True, seed=1)
    _same(_run(p, members, slots=2), before, "the wide list after the refusals")


# ---- 10. the post in one launch ------------------------------------------------------------------------
@pytest.mark.parametrize("mu_law", [False, True])
def test_postprocess_list(mu_law):
    hop, nc = 12, 512
    rng = np.random.default_rng(10)
    frames = (21, 40, 22, 33, 64)
    ys = []
    for T in frames:
        y = rng.uniform(-1, 1, T * hop).astype(np.float32)
        y[::7] = np.float32(2 * rng.integers(0, nc, y[::7].shape) / (nc - 1.0) - 1.0)   # class values, ±1 among them
        y[3], y[5], y[-2] = 1.0, -1.0, 0.0
        ys.append(torch.from_numpy(y).to(DEV))
    lens = [(T - 1) * hop for T in frames]
    wave, off = condition.postprocess_list(ys, lens, mu_law, nc, 20 * hop)
    assert wave.dtype == torch.float64 and wave.shape == (sum(lens),) and off == list(np.cumsum([0] + lens[:-1]))
    host = wave.cpu().numpy()
    for i, (y, n) in enumerate(zip(ys, lens)):
        want = condition.postprocess(y[None], False, 0, mu_law, nc, n, 20 * hop).cpu().numpy()
        got = host[off[i]:off[i] + n]
        if mu_law:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"utterance {i}")
        else:
            assert np.array_equal(got, want), f"utterance {i}: max |Δ| {np.abs(got - want).max():.3g}"
    with pytest.raises(ValueError):
        condition.postprocess_list(ys[:1], [10 * hop], mu_law, nc, 20 * hop)
