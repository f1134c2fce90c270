"""The Tacotron decoder loop on the GPU (csrc/tacotron_decoder.hip) against the reference's records.

hparams sizes throughout (the kernel's partition is tied to them); at most 48 decoder steps a case.
Bounds: a forced single step max(1e-6, 8·d1), a free run max(1e-5, 8·d), with d1 / d the reference's
own float32-against-float64 deviation recorded with each fixture.  The saturated regime is forced
steps only: free-running float32 and float64 diverge completely there.
"""
import functools

import numpy as np
import pytest
import torch

from tests.taco_fixtures import DIMS, FIELDS, REGIMES, load_runs, load_steps, make_model, step_bound, step_cases
from wavernn_amd import synthetic as syn
from wavernn_amd.tacotron import DecoderSession, Tacotron

pytestmark = pytest.mark.gpu
NEVER = -1e30


@functools.lru_cache(maxsize=None)
def model(regime):
    return make_model(regime, device="cuda")


def _cases(regime):
    fx = load_steps(regime)
    return [str(c) for c in fx["cases"]]


# ------------------------------------------------------------------ 1. forced single steps
@pytest.mark.parametrize("regime", list(REGIMES))
def test_forced_single_steps(regime):
    fx, m = load_steps(regime), model(regime)
    worst = {}
    for case, T, r, k, enc, proj in step_cases(fx):
        sess = DecoderSession(m, [torch.from_numpy(enc).cuda()], [torch.from_numpy(proj).cuda()], steps=(k + 1) * r, r=r,
                              stop_threshold=NEVER)
        for f in FIELDS:
            sess.field(f)[0, :fx[f"{case}.{k}.state.{f}"].shape[0]] = torch.from_numpy(fx[f"{case}.{k}.state.{f}"]).cuda()
        sess.field("step")[0] = k
        sess.run(1)
        assert sess.steps_done() == [k + 1]
        mel, attn, _ = sess.outputs()[0]
        got = {"frames": mel[k * r:].t(), "scores": attn[k]}
        got.update({f: sess.field(f)[0] for f in FIELDS if f != "frame"})
        want = {"frames": fx[f"{case}.{k}.frames"], "scores": fx[f"{case}.{k}.scores"]}
        want.update({f: fx[f"{case}.{k}.next.{f}"] for f in FIELDS if f != "frame"})
        assert torch.equal(sess.field("frame")[0], mel[k * r + r - 1])
        bound = step_bound(fx, case, k)
        for name, w in want.items():
            err = float(np.abs(got[name].cpu().numpy()[..., :w.shape[-1]] - w).max())
            worst[name] = max(worst.get(name, 0.0), err / bound)
            print(regime, case, k, name, "err %.3g" % err, "bound %.3g" % bound)
            assert err <= bound, (case, k, name, err, bound)
    print(regime, "worst err / bound", {k: round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------ 2. free-running parity
@pytest.mark.parametrize("regime", ["tame", "lively"])
def test_free_run_against_the_reference(regime):
    fx, m = load_runs(), model(regime)
    m.r = 2
    m.stop_threshold.fill_(NEVER)
    mel, lin, att = m.generate(fx[f"free.{regime}.x"], steps=96, backend="hip")
    bound = max(1e-5, 8 * float(fx[f"free.{regime}.d"]))
    for name, got in (("mel", mel), ("linear", lin), ("attention", att)):
        want = fx[f"free.{regime}.{name}"]
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        print(regime, name, "err %.3g" % err, "bound %.3g" % bound)
        assert err <= bound, (name, err, bound)


# ------------------------------------------------------------------ 3. stop rule
@pytest.mark.parametrize("name", ["first_r1", "first_r7", "first_r20", "ragged_r7", "count_r2", "mid"])
def test_stop_steps_equal_the_reference(name):
    fx, m = load_runs(), model("lively")
    m.r = int(fx[f"stop.{name}.r"])
    m.stop_threshold.fill_(float(fx[f"stop.{name}.thr"]))
    mel, lin, att = m.generate(fx[f"stop.{name}.x"], steps=int(fx[f"stop.{name}.steps"]), backend="hip")
    want = fx[f"stop.{name}.mel"]
    assert att.shape[0] == int(fx[f"stop.{name}.n_steps"])
    assert mel.shape == want.shape and lin.shape == want.shape       # the stopping step's frames are kept
    if name == "ragged_r7":     # steps = 25 is no multiple of r = 7: ceil(25 / 7) = 4 steps, every one all 7 frames
        assert (att.shape[0], mel.shape[1]) == (4, 28) and float(fx["stop.ragged_r7.thr"]) < -1e29
    if name == "count_r2":      # no step is eligible (t <= 8): the count ends the loop, not the rule
        assert (att.shape[0], mel.shape[1]) == (5, 10) and float(mel.max()) < float(fx["stop.count_r2.thr"])
    assert float(np.abs(mel - want).max()) <= max(1e-5, 8 * float(fx[f"stop.{name}.d"]))


# ------------------------------------------------------------------ 4. lists
@functools.lru_cache(maxsize=None)
def _list_singles():
    fx, m = load_runs(), model("lively")
    m.r = int(fx["list.r"])
    m.stop_threshold.fill_(float(fx["list.thr"]))
    xs = [fx[f"list.{i}.x"] for i in range(5)]
    return xs, [m.generate(x, steps=int(fx["list.steps"]), backend="hip") for x in xs]


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (3, 3, 0)])
def test_list_rows_equal_their_own_generate(order):
    fx, m = load_runs(), model("lively")
    xs, singles = _list_singles()
    m.r = int(fx["list.r"])
    m.stop_threshold.fill_(float(fx["list.thr"]))
    outs = m.generate_list([xs[i] for i in order], steps=int(fx["list.steps"]))
    for i, o in zip(order, outs):
        assert o[2].shape[0] == int(fx[f"list.{i}.n_steps"])          # the reference's step count
        assert o[0].shape == fx[f"list.{i}.mel"].shape
        assert _same(o, singles[i]), i


def test_list_rows_in_any_slot_of_a_session():
    """The decoder's own outputs, bit for bit, whatever the slot and the company (no torch module between)."""
    fx, m = load_runs(), model("lively").eval()
    xs, _ = _list_singles()
    m.r = int(fx["list.r"])
    m.stop_threshold.fill_(float(fx["list.thr"]))
    with torch.no_grad():
        coded = [m.encode(x) for x in xs]
    steps = int(fx["list.steps"])

    def run(idx):
        s = DecoderSession(m, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], steps)
        s.run(s.step_cap)
        return [(a.clone(), b.clone(), n) for a, b, n in s.outputs()]
    alone = [run([i])[0] for i in range(5)]
    for idx in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2, 4, 0]):
        for i, (mel, att, n) in zip(idx, run(idx)):
            assert n == alone[i][2] == int(fx[f"list.{i}.n_steps"])
            assert torch.equal(mel, alone[i][0]) and torch.equal(att, alone[i][1]), (idx, i)
    assert len({a[2] for a in alone}) >= 4 and max(a[2] for a in alone) == -(-steps // m.r)


def test_list_of_130_rows_crosses_the_launch_cap():
    m = model("lively")
    m.r = 2
    m.stop_threshold.fill_(NEVER)
    xs = [syn.make_text_ids(1 + i % 7, DIMS.num_chars, seed=40 + i % 9) for i in range(130)]
    outs = m.generate_list(xs, steps=8)
    singles = {}
    for x, o in zip(xs, outs):
        key = x.tobytes()
        if key not in singles:
            singles[key] = m.generate(x, steps=8, backend="hip")
        assert o[0].shape == (80, 8) and _same(o, singles[key])


# ------------------------------------------------------------------ 5. chunking
@pytest.mark.parametrize("cap_steps", [80, 58])      # the fixture's cap (rows stop at 9, 10, 36; one runs out) / a cap that cuts two rows off
def test_chunked_launches_equal_one_launch(cap_steps):
    fx, m = load_runs(), model("lively").eval()
    xs, _ = _list_singles()
    m.r = int(fx["list.r"])
    m.stop_threshold.fill_(float(fx["list.thr"]))
    with torch.no_grad():
        coded = [m.encode(x) for x in xs]

    def session():
        return DecoderSession(m, [c[0][0] for c in coded], [c[1][0] for c in coded], cap_steps)
    one = session()
    one.run(one.step_cap)
    cut = session()
    for n in (1, 3, 7, cut.step_cap):    # rows stop inside the third launch; the last asks for more steps than are left
        cut.run(n)
    assert cut.steps_done() == one.steps_done()
    assert torch.equal(cut.state, one.state)
    for a, b in zip(one.outputs(), cut.outputs()):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    stopped = one.field("stopped").cpu().tolist()
    assert 0 in stopped and 1 in stopped
    # a finished session writes nothing further
    before = (one.mel.clone(), one.attn.clone(), one.state.clone())
    one.run(4)
    assert torch.equal(one.mel, before[0]) and torch.equal(one.attn, before[1]) and torch.equal(one.state, before[2])


# ------------------------------------------------------------------ 6. weights
def test_data_update_and_reload_reach_the_kernel():
    m = make_model("lively", device="cuda")
    m.stop_threshold.fill_(NEVER)
    x = syn.make_text_ids(9, DIMS.num_chars, seed=3)
    base = m.generate(x, steps=12, backend="hip")
    assert _same(base, m.generate(x, steps=12, backend="hip"))
    with torch.no_grad():
        m.decoder.res_rnn2.weight_hh.data[5, 7] += 0.5
    touched = m.generate(x, steps=12, backend="hip")
    assert not np.array_equal(touched[0], base[0])
    m.decoder.mel_proj.weight.data = m.decoder.mel_proj.weight.data.clone() * 0.5      # a new tensor behind .data
    halved = m.generate(x, steps=12, backend="hip")
    assert np.array_equal(halved[0][:, :2], 0.5 * touched[0][:, :2])      # the first step sees the same inputs
    assert not np.array_equal(halved[0], touched[0])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in
                       syn.make_tacotron_state(DIMS, seed=11, scale=REGIMES["lively"]).items()})
    m.stop_threshold.fill_(NEVER)
    assert _same(base, m.generate(x, steps=12, backend="hip"))
    t = m.generate(x, steps=12, backend="torch")
    assert float(np.abs(t[0] - base[0]).max()) < 1e-3


def test_wrong_size_model_raises_under_hip_and_falls_back_under_none():
    kw = dict(DIMS.ctor_kwargs(), lstm_dims=256)
    torch.manual_seed(0)
    m = Tacotron(**kw).cuda()
    m.r = 2
    x = syn.make_text_ids(5, DIMS.num_chars, seed=1)
    with pytest.raises(RuntimeError, match="lstm"):
        m.generate(x, steps=6, backend="hip")
    with pytest.raises(RuntimeError, match="lstm"):
        m.generate_list([x], steps=6, backend="hip")
    a = m.generate(x, steps=6)
    b = m.generate(x, steps=6, backend="torch")
    assert a[0].shape == (80, 6) and _same(a, b)


# ------------------------------------------------------------------ 7. end to end
def test_synthesize_list_equals_the_calls_by_hand():
    from tests import geometries as geo
    from wavernn_amd import gen_tacotron as gt
    from wavernn_amd.fatchord_version import WaveRNN
    m = model("lively")
    m.r = 2
    m.stop_threshold.fill_(NEVER)
    # the list tests' smallest geometry (hop 4, pad 1, MoL rnn 512) at Tacotron's 80 mels
    d = geo.dims(DIMS.n_mels, (4,), 1, rnn_dims=512)
    voc = WaveRNN(**d.ctor_kwargs()).cuda()
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, geo.TAP_SEED).items()})
    voc.eval()
    xs = [syn.make_text_ids(n, DIMS.num_chars, seed=60 + n) for n in (3, 7, 5)]
    wavs = gt.synthesize_list(m, voc, xs, seed=9, steps=24)
    by_hand = voc.generate_list([gt.tacotron_mel_to_vocoder(m.generate(x, steps=24)[1]) for x in xs], seed=9, wide=True)
    assert len(wavs) == 3
    for a, b in zip(wavs, by_hand):
        assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a, b)
