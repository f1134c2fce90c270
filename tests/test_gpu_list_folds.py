"""Folded lists on the MI355X: WaveRNN.generate_list(wide=True, batched=True) /
wrnn_generate_list_folds — the folds of a list of unequal utterances as the rows of the many-row XCD
kernel's grouped launches, MoL and RAW (include/wavernn_amd.h, "Folded lists"; the host side is
tests/test_list_folds_plan.py), and the one-launch cross-fade post wrnn_postprocess_list_folds.

Every expectation is oracle.generate(batched=True) on ONE utterance alone (its own mel truncated to its
own length, its own draws [target + 2·overlap][folds][K]), built on tests/geometries.py,
tests/raw_streams.py and the Pool of tests/test_gpu_list_wide.py.

Bounds.  MoL: |Δ| <= √2 · 2·MOL_TOL = 2.83e-5 against the oracle on the same draws — a sample is the
sum of at most two fold samples, each within the wide bound 2·MOL_TOL = 2e-5 of the oracle's, with
cross-fade weights sqrt(½(1 ± t)) whose sum is at most √2; the final fade is at most 1.  Under Philox
|Δ| <= √2 · MOL_TOL against generate(batched=True, seed, row_offset + first_row[i]).  RAW: the loop
outputs equal generate_frames(target, overlap) of the utterance alone bit for bit; the waveform holds
assert_allclose(rtol=1e-12, atol=0) against the oracle (the project's bound for the float64 post), and
with mu_law off every sample outside the overlaps and the fade-out is equal.  "Bit-identical" is
np.array_equal.  What each case would catch:
  1     a wrong phase when a fold starts inside a frame, a tail read past the frame-term stores, a fold
        resumed from a neighbour's state record;
  2     any dependence of an utterance on its company, the list order or `slots`; a round boundary
        inside an utterance;
  3     a launch boundary inside a fold (resume, the fold-local Philox step, the draws' offset);
  4     the Philox keys of a fold row;
  5     the table-driven cross-fade post against the per-utterance one;
  6     a folded list touching a session's records or the one-shot state;
  7     a refusal that queued something or left the handle changed.

Measured on MI355X (each case prints its figures, `FOLD LIST …`): MoL against the oracle at most
4.7e-8 (hop 12, (150, 20), 60 frames; 3.1e-8 on the 231 folds of case 2, 2.6e-8 at hop 2, 2.1e-8 on the
single fold that is mostly tail; bound 2.83e-5), under Philox 2.6e-8 against generate(batched=True)
(bound 1.41e-5); RAW 0 of 2 280 loop samples differ from generate_frames (injected and Philox), 0
samples outside overlaps and fade differ from the oracle, rtol 1e-12 holds with mu_law on and off;
every bit-for-bit comparison holds; the file runs in 7 s."""
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import raw_streams as rs
from tests.golden import fixtures as gf
from tests.test_gpu_list_wide import DEV, OVERRIDES, Pool, _bare_model, _same
from wavernn_amd import condition
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import list_folds_plan, wide_steps_per_launch

pytestmark = pytest.mark.gpu
FOLD_TOL = float(np.sqrt(2.0)) * 2 * gf.MOL_TOL      # against the oracle on the same draws
PHILOX_TOL = float(np.sqrt(2.0)) * gf.MOL_TOL        # against generate(batched=True) under Philox
N_MOL = 32 * 144
FOLD = {"hop12": (150, 20), "hop4": (20, 4), "hop2": (10, 2)}
FRAMES_1 = (21, 30, 36, 60)                          # 30 frames: 360 = 2·170 + 20, no zero tail
FRAMES_2 = tuple(21 + (7 * i) % 25 for i in range(40))
FRAMES_3 = (21, 24, 29)
SEED, ROW0 = 20240917, 9


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


# ---- inputs ------------------------------------------------------------------------------------------
class FoldPool(Pool):
    """The Pool of the wide-list tests with fold-batched draws and references: utterance (u, T) at
    (target, overlap) has draws [Lf][folds][K] of its own and oracle.generate(batched=True) alone."""

    def __init__(self, mode, geom, n, frames):
        super().__init__(mode, geom, n, frames)
        self._fref, self._fnoise = {}, {}

    def folds(self, T, target, overlap):
        return list_folds_plan([T], self.hop, target, overlap)[0][0]

    def fdraws(self, u, T, target, overlap):
        k = (u % self.n, T, target, overlap)
        if k not in self._fnoise:
            z = syn.make_noise(self.dims.mode, self.folds(T, target, overlap), target + 2 * overlap, self.dims.n_classes,
                               7000 + 97 * k[0] + T)
            z.setflags(write=False)
            self._fnoise[k] = z
        return self._fnoise[k]

    def fref(self, u, T, target, overlap, mu_law=False):
        from oracle import oracle
        k = (u % self.n, T, target, overlap, mu_law)
        if k not in self._fref:
            r = oracle.generate(self.state, self.dims, self.mel(u, T)[0], True, target, overlap, mu_law,
                                self.fdraws(u, T, target, overlap))
            assert r.shape == ((T - 1) * self.hop,) and r.dtype == np.float64
            r.setflags(write=False)
            self._fref[k] = r
        return self._fref[k]


@functools.lru_cache(maxsize=None)
def pool(mode, geom):
    n, frames = {"hop12": (4, 60), "hop4": (12, 45), "hop2": (3, 29)}[geom]
    return FoldPool(mode, geom, n, frames)


def _check(p, got, u, T, target, overlap, what, mu_law=False):
    ref = p.fref(u, T, target, overlap, mu_law)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.shape, ref.shape)
    if p.mode == "RAW":
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=what)
        if not mu_law:   # outside the overlaps and the fade a sample is one label's value: exact
            t = np.arange(got.shape[0])
            stride, rows = target + overlap, p.folds(T, target, overlap)
            body = (t % stride >= overlap) & (t < rows * stride) & (t < got.shape[0] - rs.FADE_FRAMES * p.hop)
            neq = int((got[body] != ref[body]).sum())
            print(f"FOLD LIST {what}: {neq} of {int(body.sum())} samples outside overlaps and fade differ")
            assert neq == 0, what
        return 0.0
    err = float(np.abs(got - ref).max())
    print(f"FOLD LIST {what}: max |Δ| {err:.3g} vs the oracle (bound {FOLD_TOL:.3g})")
    assert err <= FOLD_TOL, f"{what}: max |Δ| {err:.3g} > {FOLD_TOL:.3g}"
    return err


def _run(p, members, fold=None, mu_law=False, injected=True, **kw):
    """generate_list(wide=True, batched=True) of the members (pool utterance, frames) → the waveforms; last_path 7."""
    target, overlap = fold or FOLD[p.geom]
    m = p.model()
    mels = [p.mel(u, T) for u, T in members]
    if injected:
        kw["noise"] = [np.array(p.fdraws(u, T, target, overlap)) for u, T in members]
    got = m.generate_list(mels, wide=True, batched=True, target=target, overlap=overlap, mu_law=mu_law, **kw)
    assert m.loop_handle().info["last_path"] == 7
    assert len(got) == len(members)
    for g, (u, T) in zip(got, members):
        assert g.dtype == np.float64 and g.shape == ((T - 1) * p.hop,)
    return got


@functools.lru_cache(maxsize=None)
def _case1(mode):
    p = pool(mode, "hop12")
    members = tuple((i, T) for i, T in enumerate(FRAMES_1))
    got = _run(p, members, slots=3)
    for g in got:
        g.setflags(write=False)
    return members, tuple(got)


@functools.lru_cache(maxsize=None)
def _case2(mode):
    p = pool(mode, "hop4")
    members = tuple((i, T) for i, T in enumerate(FRAMES_2))
    got = _run(p, members)
    for g in got:
        g.setflags(write=False)
    return members, tuple(got)


def _sample2():
    """Six members of case 2: the first, the last, the one whose folds straddle the round boundary
    (fold 127 | 128), its neighbours' side of each round and one more."""
    folds, first, _ = list_folds_plan(FRAMES_2, 4, *FOLD["hop4"])
    cross = [i for i in range(len(folds)) if first[i] <= 127 < first[i] + folds[i] - 1]
    assert len(cross) == 1, "no utterance straddles the round boundary"
    c = cross[0]
    return (0, 3, c - 1, c, c + 1, len(folds) - 1)


# ---- 1. folds that start inside a frame, with and without a zero tail ----------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_folds_start_inside_frames(mode):
    p = pool(mode, "hop12")
    target, overlap = FOLD["hop12"]
    assert (target + overlap) % 12                              # fold 1 starts at phase 170 % 12 = 2
    folds, first, launches = list_folds_plan(FRAMES_1, 12, target, overlap, 3, raw=mode == "RAW")
    assert folds == [2, 2, 3, 5] and launches == [(q * 190, 190, 3) for q in range(4)]
    assert [(f - 1) * 170 + 190 - 12 * T for f, T in zip(folds, FRAMES_1)] == [108, 0, 98, 150]   # zero tails
    members, got = _case1(mode)
    for i, (u, T) in enumerate(members):
        _check(p, got[i], u, T, target, overlap, f"{mode} hop12 (150, 20), {T} frames")
    assert len(np.unique(got[3][20:170])) > 20                  # fold 0's body past its fade-in: not a constant
    # one fold that is mostly tail: 21 frames in (300, 20)
    assert list_folds_plan([21], 12, 300, 20)[0] == [1]
    one = _run(p, [(1, 21)], fold=(300, 20))
    _check(p, one[0], 1, 21, 300, 20, f"{mode} hop12 (300, 20), 21 frames: a single fold")


# ---- 2. two rounds, company independence ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_two_rounds_and_independence(mode):
    p = pool(mode, "hop4")
    target, overlap = FOLD["hop4"]
    folds, first, launches = list_folds_plan(FRAMES_2, 4, target, overlap, raw=mode == "RAW")
    F = sum(folds)
    assert F > 128 and launches == [(0, 28, 128), (28, 28, F - 128)]
    members, got = _case2(mode)
    sample = _sample2()
    for i in sample:
        u, T = members[i]
        _check(p, got[i], u, T, target, overlap, f"{mode} 40 utterances, {F} folds, utterance {i}")
    for i in sample:
        _same(_run(p, [members[i]]), [got[i]], f"{mode} utterance {i} of the 40 alone")
    _same(_run(p, members[::-1])[::-1], got, f"{mode} the list of 40 reversed")
    _same(_run(p, members, slots=5), got, f"{mode} slots=5 against 128")


# ---- 3. budget cuts inside a fold ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["MOL", "RAW"])
def test_budget_cuts_inside_folds(monkeypatch, mode):
    p = pool(mode, "hop2")
    target, overlap = FOLD["hop2"]
    raw = mode == "RAW"
    members = [(i, T) for i, T in enumerate(FRAMES_3)]
    folds = list_folds_plan(FRAMES_3, 2, target, overlap)[0]
    F = sum(folds)
    assert folds == [4, 4, 5]
    uncut = _run(p, members)
    for i, (u, T) in enumerate(members):
        _check(p, uncut[i], u, T, target, overlap, f"{mode} hop2 (10, 2), {T} frames")
    for steps in (geo.GEOMS["hop2"][7], 1):
        monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, F, rs.N_RAW if raw else N_MOL))
        assert wide_steps_per_launch(F, 14, raw=raw) == steps
        launches = list_folds_plan(FRAMES_3, 2, target, overlap, raw=raw)[2]
        assert launches == [(off, min(steps, 14 - off), F) for off in range(0, 14, steps)] and len(launches) > 1
        _same(_run(p, members), uncut, f"{mode} {steps} step(s) per launch against the uncut run")


# ---- 4. Philox -----------------------------------------------------------------------------------------
def test_philox_mol_against_generate():
    p = pool("MOL", "hop12")
    m = p.model()
    target, overlap = FOLD["hop12"]
    members = [(i, T) for i, T in enumerate(FRAMES_1)]
    folds, first, _ = list_folds_plan(FRAMES_1, 12, target, overlap)
    got = _run(p, members, injected=False, seed=SEED, row_offset=ROW0, slots=4)
    worst = 0.0
    for i, (u, T) in enumerate(members):
        want = m.generate(p.mel(u, T), None, True, target, overlap, False, seed=SEED, row_offset=ROW0 + first[i], verbose=False)
        assert got[i].shape == want.shape
        worst = max(worst, float(np.abs(got[i] - want).max()))
        alone = _run(p, [(u, T)], injected=False, seed=SEED, row_offset=ROW0 + first[i])
        _same(alone, [got[i]], f"MOL Philox, utterance {i} alone with row_offset + first_row")
    print(f"FOLD LIST Philox MoL: max |Δ| {worst:.3g} vs generate(batched=True, seed, row_offset + first_row) (bound {PHILOX_TOL:.3g})")
    assert worst <= PHILOX_TOL
    assert not np.array_equal(_run(p, members[:1], injected=False, seed=SEED + 1, row_offset=ROW0)[0], got[0])


@pytest.mark.parametrize("philox", [True, False])
def test_raw_loop_outputs_equal_generate_frames(philox):
    p = pool("RAW", "hop12")
    m = p.model()
    target, overlap = FOLD["hop12"]
    members = [(i, T) for i, T in enumerate(FRAMES_1)]
    folds, first, _ = list_folds_plan(FRAMES_1, 12, target, overlap, raw=True)
    loop, spec = m.loop_handle(), m._upsample_spec()
    fr = [m.frames(torch.from_numpy(p.mel(u, T)).to(DEV)) for u, T in members]
    nz = None if philox else [torch.from_numpy(np.array(p.fdraws(u, T, target, overlap))).to(DEV) for u, T in members]
    outs = loop.generate_list_folds(spec, [f[0] for f in fr], [f[1] for f in fr], target, overlap, slots=3, noise=nz,
                                    seed=SEED, row_offset=ROW0)
    assert loop.info["last_path"] == 7
    for i, f in enumerate(fr):
        want, _ = loop.generate_frames(spec, f[0], f[1], target, overlap, noise=None if philox else nz[i], seed=SEED,
                                       row_offset=ROW0 + first[i])
        assert tuple(outs[i].shape) == tuple(want.shape) == (folds[i], 190)
        a, b = outs[i].cpu().numpy(), want.cpu().numpy()
        print(f"FOLD LIST RAW loop output, utterance {i} ({'Philox' if philox else 'injected'}): {int((a != b).sum())} of {a.size} differ")
        assert np.array_equal(a, b), f"utterance {i}"
        assert len(np.unique(a)) > 20


def test_raw_mu_law():
    p = pool("RAW", "hop12")
    members = [(1, 30), (3, 60)]
    got = _run(p, members, mu_law=True, slots=4)
    for i, (u, T) in enumerate(members):
        _check(p, got[i], u, T, *FOLD["hop12"], f"RAW mu_law on, {T} frames", mu_law=True)
    assert not np.array_equal(got[0], _case1("RAW")[1][1])


# ---- 5. the cross-fade post in one launch --------------------------------------------------------------
@pytest.mark.parametrize("mu_law", [False, True])
@pytest.mark.parametrize("target, overlap", [(150, 20), (37, 0), (40, 7), (5, 1)])
def test_postprocess_list_folds(mu_law, target, overlap):
    hop, nc = 1, 512
    steps, stride = target + 2 * overlap, target + overlap
    rng = np.random.default_rng(10 + target)
    rows = (4, 6, 9, 5)
    ys, lens = [], []
    for i, n in enumerate(rows):
        y = rng.uniform(-1, 1, (n, steps)).astype(np.float32)
        y[:, ::7] = np.float32(2 * rng.integers(0, nc, y[:, ::7].shape) / (nc - 1.0) - 1.0)   # class values, ±1 among them
        y[0, 0], y[-1, -1], y[0, steps // 2] = 1.0, -1.0, 0.0
        ys.append(torch.from_numpy(y).to(DEV))
        total = n * stride + overlap
        lens.append(total - (0, 3, 1, stride // 2)[i])                                        # trims of several kinds
        assert 20 * hop <= lens[-1] <= total
    wave, off = condition.postprocess_list_folds(ys, overlap, lens, mu_law, nc, 20 * hop)
    assert wave.dtype == torch.float64 and wave.shape == (sum(lens),) and off == list(np.cumsum([0] + lens[:-1]))
    host = wave.cpu().numpy()
    for i, (y, n) in enumerate(zip(ys, lens)):
        want = condition.postprocess(y, True, overlap, mu_law, nc, n, 20 * hop).cpu().numpy()
        got = host[off[i]:off[i] + n]
        if mu_law:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"utterance {i}")
        else:
            assert np.array_equal(got, want), f"utterance {i}: max |Δ| {np.abs(got - want).max():.3g}"
    with pytest.raises(ValueError):
        condition.postprocess_list_folds(ys[:1], overlap, [10 * hop], mu_law, nc, 20 * hop)          # shorter than the fade
    with pytest.raises(ValueError):
        condition.postprocess_list_folds(ys[:1], overlap, [rows[0] * stride + overlap + 1], mu_law, nc, 20 * hop)
    with pytest.raises(ValueError):
        condition.postprocess_list_folds(ys[:1], steps, lens[:1], mu_law, nc, 20 * hop)             # no target left


# ---- 6. coexistence ------------------------------------------------------------------------------------
def test_neighbours_on_one_handle():
    p = pool("MOL", "hop12")
    m = p.model()
    members, want = _case1("MOL")
    members, want = members[:3], want[:3]
    one_mel = p.mel(2, 26)
    sess_mel = p.mel(3, 30)

    def session(between):
        parts = []
        with m.stream(1, 30, seed=11, row_offset=40, wide=True) as s:
            parts.append(s.push(sess_mel[:, :, :10]))
            between()
            parts.append(s.push(sess_mel[:, :, 10:20]))
            between()
            parts.append(s.push(sess_mel[:, :, 20:]))
            parts.append(s.finish())
        return np.concatenate([q for q in parts if q.shape[1]], 1)

    def one():
        return m.generate(one_mel, None, True, 150, 20, False, seed=3, row_offset=2, verbose=False)

    alone = dict(session=session(lambda: None), one=one())
    got = dict(folds=[], one=[])

    def between():
        got["folds"].append(_run(p, members, slots=2))
        got["one"].append(one())                               # generate() right after a folded list

    mixed = session(between)
    assert np.array_equal(mixed, alone["session"]), "the wide session changed by the folded lists between its pushes"
    assert len(got["folds"]) == 2
    for g in got["folds"]:
        _same(g, want, "a folded list between the pushes of a wide session")
    for g in got["one"]:
        assert np.array_equal(g, alone["one"]), "generate() after a folded list"


# ---- 7. refusals ---------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    p = pool("RAW", "hop12")
    m = p.model()
    target, overlap = FOLD["hop12"]
    members = [(1, 30), (0, 21)]
    before = _run(p, members, slots=2)
    mels = [p.mel(u, T) for u, T in members]
    noise = [np.array(p.fdraws(u, T, target, overlap)) for u, T in members]
    kw = dict(wide=True, batched=True, target=target, overlap=overlap)

    def still_fine(what):
        _same(_run(p, members, slots=2), before, f"the folded list after: {what}")

    for bad, match in ((dict(wide=False), "needs wide=True"), (dict(lanes=2), "lanes"), (dict(slots=129), r"slots is 1\.\.128"),
                       (dict(slots=0), r"slots is 1\.\.128"), (dict(target=0), "target"), (dict(overlap=-1), "overlap"),
                       (dict(overlap=253), "overlap"), (dict(noise=noise[:1]), "one .* per utterance"),
                       (dict(noise=[z[:, :, :11] for z in noise]), r"noise\[0\] must be"),
                       (dict(noise=[z[:-1] for z in noise]), r"noise\[0\] must be")):
        args = dict(kw, noise=noise)
        args.update(bad)
        with pytest.raises(ValueError, match=match):
            m.generate_list(mels, **args)
        still_fine(str(bad))
    with pytest.raises(ValueError, match="21 frames"):
        m.generate_list(mels + [p.mel(2, 20)], seed=1, **kw)
    still_fine("an utterance of 20 frames")
    # the library's own checks, behind the Python ones
    loop, spec = m.loop_handle(), m._upsample_spec()
    fr = [m.frames(torch.from_numpy(x).to(DEV)) for x in mels + [p.mel(2, 20)]]
    with pytest.raises(ValueError, match="utterance 2 has 20 frames"):
        loop.generate_list_folds(spec, [f[0] for f in fr], [f[1] for f in fr], target, overlap, seed=1)
    with pytest.raises(ValueError, match="target is at least 1"):
        loop.generate_list_folds(spec, [f[0] for f in fr[:2]], [f[1] for f in fr[:2]], 0, overlap, seed=1)
    with pytest.raises(ValueError, match="less than the overlap"):
        loop.generate_list_folds(spec, [f[0] for f in fr[:2]], [f[1] for f in fr[:2]], target, 253, seed=1)
    lib_rc = condition.nat.lib().wrnn_generate_list_folds(loop._h, None, None, None, None, 2, target, overlap, 0, None, 0, 0,
                                                          None, None)
    assert lib_rc == -1
    still_fine("the library's refusals")
    # the handles the wide list refuses, with its texts; generate() on them is as before
    x = [p.mel(0, 21)]
    for bare, exc_match in ((_bare_model(rnn_dims=512, bits=10), r"512 classes \(bits = 9\): this handle has 1024 classes"),
                            (_bare_model(rnn_dims=896), r"rnn / fc 512\): this handle has rnn 896, fc 512"),
                            (_bare_model("MOL", rnn_dims=896), "four co-resident quads per XCD")):
        g0 = bare.generate(x[0], None, False, 0, 0, False, seed=1, verbose=False)
        with pytest.raises(NotImplementedError, match=exc_match):
            bare.generate_list(x, seed=1, **kw)
        g1 = bare.generate(x[0], None, False, 0, 0, False, seed=1, verbose=False)
        assert np.array_equal(g0, g1), "generate() after a refused folded list"
    # batched=False is the wide list, unchanged by the new keywords
    w0 = m.generate_list(mels, wide=True, seed=5, mu_law=False)
    w1 = m.generate_list(mels, wide=True, seed=5, mu_law=False, batched=False, target=7, overlap=3)
    _same(w1, w0, "the unbatched wide list ignores target / overlap")
