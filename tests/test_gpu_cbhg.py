"""The ragged CBHGs on the GPU (csrc/cbhg.hip) against the reference's records, and their independence.

hparams sizes throughout (the kernels take nothing else).  Bound of every comparison with a record:
max(1e-6, 8·d), d the reference's own float32-against-float64 deviation recorded with the case or
stage; the end-to-end free runs keep their own max(1e-5, 8·d).  Everything about independence is
`np.array_equal`.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import cbhg_ref as ref
from tests.taco_fixtures import load_runs, make_model
from wavernn_amd import _native as nat
from wavernn_amd import synthetic as syn
from wavernn_amd import tacotron as taco
from wavernn_amd.tacotron import Tacotron

pytestmark = pytest.mark.gpu
NEVER = -1e30
WHICH = {"enc": "encoder", "post": "postnet"}
ENC_LIST = (1, 17, 2, 33, 16, 40, 15)
POST_LIST = (1, 31, 2, 64, 9, 16)


def build(state):
    m = Tacotron(**ref.DIMS.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    m.r = 2
    return m.cuda()


@functools.lru_cache(maxsize=None)
def model(regime):
    return build(ref.state(regime))


def rows_of(which, inputs):
    if which == "enc":
        return [torch.from_numpy(np.asarray(x)).to("cuda", torch.int32) for x in inputs]
    return [torch.from_numpy(np.asarray(x)).cuda().t() for x in inputs]


def run(m, which, inputs, budget=None, keep=None):
    """Per sentence (rnn, proj) as numpy, through the ragged pass."""
    outs = m._cbhg_run_list(WHICH[which], rows_of(which, inputs), budget, keep)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in outs]


def stages(cfg, scratch, P):
    offs = (ctypes.c_int64 * len(nat.CBHG_STAGES))()
    nat.check_cond(nat.lib().wrnn_cbhg_scratch_layout(ctypes.byref(cfg), P, offs))
    widths = {"front": cfg.in_channels, "bank": cfg.K * cfg.channels, "pooled": cfg.K * cfg.channels, "proj1": cfg.proj1,
              "residual": cfg.proj2, "highway_in": cfg.channels, "highway_out": cfg.channels, "gi": 6 * cfg.channels,
              "rnn": 2 * cfg.channels}
    return {n: scratch[o:o + P * widths[n]].view(P, widths[n]).cpu().numpy() for n, o in zip(nat.CBHG_STAGES, offs) if o >= 0}


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def inputs_of(which, lengths):
    return [ref.enc_input(T) if which == "enc" else ref.post_input(T) for T in lengths]


# ------------------------------------------------------------------ 1. against the reference
def check_records(which, regime, lengths):
    fx, m = ref.load(which, regime), model(regime)
    worst = {}
    for T in lengths:
        keep = []
        (rnn, proj), = run(m, which, [ref.fixture_input(fx, which, T)], keep=keep)
        got = {"rnn": rnn, "proj": proj}
        items = [(n, fx[f"T{T}.{n}"], fx[f"T{T}.d"]) for n in ("rnn", "proj")]
        if T in fx["stage_lengths"]:
            cfg, scratch, P = keep[0]
            st = stages(cfg, scratch, P)
            assert P == T and np.array_equal(st["rnn"], rnn)
            for s in ref.STAGES:
                if f"T{T}.stage.{s}" in fx:
                    got["stage." + s] = st[s]
                    items.append(("stage." + s, fx[f"T{T}.stage.{s}"], fx[f"T{T}.stage.{s}.d"]))
        for name, want, d in items:
            assert got[name].shape == want.shape, (T, name)
            err, b = float(np.abs(got[name] - want).max()), ref.bound(d)
            worst[name] = max(worst.get(name, 0.0), err / b)
            print(which, regime, T, name, "err %.3g" % err, "bound %.3g" % b)
            assert err <= b, (which, regime, T, name, err, b)
    print(which, regime, "worst err / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("regime", list(ref.REGIMES))
@pytest.mark.parametrize("which", ["enc", "post"])
def test_outputs_and_stages_against_the_reference(which, regime):
    check_records(which, regime, [int(t) for t in ref.load(which, regime)["lengths"]])


@pytest.mark.parametrize("which", ["enc", "post"])
def test_one_and_two_positions(which):
    """T = 1, 2: max-pool's absent left neighbour, K = 16 with all taps but one or two outside, one-step scans."""
    for regime in ref.REGIMES:
        check_records(which, regime, [1, 2])
    m = model("hot")
    (rnn, _), = run(m, which, inputs_of(which, [1]))
    assert rnn.shape == (1, 256) and np.isfinite(rnn).all() and np.abs(rnn).max() > 0


@pytest.mark.parametrize("regime", list(ref.REGIMES))
def test_postnet_of_400_frames_against_the_restatement(regime):
    """Many tiles and a long scan; d is the restatement's own float32-against-float64 deviation."""
    x = syn.make_taco_mel(400, 80, seed=77)
    st = ref.state(regime)
    r64, = ref.cbhg_list(st, "post", [x], np.float64)
    r32, = ref.cbhg_list(st, "post", [x], np.float32)
    (rnn, proj), = run(model(regime), "post", [x])
    for name, got in (("rnn", rnn), ("proj", proj)):
        d = float(np.abs(r32[name].astype(np.float64) - r64[name]).max())
        err = float(np.abs(got - r64[name]).max())
        print(regime, name, "d %.3g" % d, "err %.3g" % err, "bound %.3g" % ref.bound(d))
        assert err <= ref.bound(d), (name, err, d)


# ------------------------------------------------------------------ 2. independence
@functools.lru_cache(maxsize=None)
def alone(which):
    m = model("hot")
    xs = inputs_of(which, ENC_LIST if which == "enc" else POST_LIST)
    return xs, [run(m, which, [x])[0] for x in xs]


@pytest.mark.parametrize("which", ["enc", "post"])
def test_members_equal_themselves_alone_in_any_order_and_slot(which):
    m = model("hot")
    xs, singles = alone(which)
    n = len(xs)
    for out, single in zip(run(m, which, xs), singles):
        assert same(out, single)
    for out, single in zip(run(m, which, xs[::-1]), singles[::-1]):
        assert same(out, single)
    for x, single in zip(xs, singles):
        outs = run(m, which, [x] * n)
        assert all(same(o, single) for o in outs)
    # a member between copies of every other member (its neighbours change, it does not)
    for i, (x, single) in enumerate(zip(xs, singles)):
        j = (i + 1) % n
        outs = run(m, which, [xs[j], x, xs[j], x])
        assert same(outs[1], single) and same(outs[3], single) and same(outs[0], singles[j])


@pytest.mark.parametrize("which", ["enc", "post"])
def test_a_tiny_chunk_budget_changes_no_bit(which):
    m = model("hot")
    xs, singles = alone(which)
    keep = []
    outs = run(m, which, xs, budget=1, keep=keep)
    assert len(keep) == len(xs)                      # every sentence its own run
    assert all(same(o, s) for o, s in zip(outs, singles))
    cfg = m.cbhg_cfg(WHICH[which])
    lens = [len(x) if which == "enc" else x.shape[1] for x in xs]
    mid = int(nat.lib().wrnn_cbhg_scratch_bytes(ctypes.byref(cfg), lens[0] + lens[1] + lens[2]))
    keep = []
    outs = run(m, which, xs, budget=mid, keep=keep)
    assert 1 < len(keep) < len(xs) and sum(k[2] for k in keep) == sum(lens)
    assert all(same(o, s) for o, s in zip(outs, singles))
    keep = []
    run(m, which, xs, keep=keep)
    assert len(keep) == 1 and taco.CBHG_SCRATCH_BUDGET == 1 << 30


@pytest.mark.parametrize("which", ["enc", "post"])
def test_the_only_short_member_among_127_others(which):
    """128 sentences: 256 scan workgroups, more than one round of them on the device."""
    m = model("hot")
    xs, singles = alone(which)
    others = inputs_of(which, [40, 39, 40])
    for i, (x, single) in enumerate(zip(xs, singles)):
        lst = [others[k % 3] for k in range(127)]
        lst.insert((i * 19) % 128, x)
        outs = run(m, which, lst)
        assert same(outs[(i * 19) % 128], single), i
        if i == 0:
            o40 = run(m, which, [others[0]])[0]
            assert all(same(outs[k], o40) for k in range(128) if lst[k] is others[0])


# ------------------------------------------------------------------ 3. isolation
def test_nan_and_huge_members_stay_in_their_own_sentence():
    m = model("hot")
    a, b, c = inputs_of("post", [9, 31, 2])
    nan = np.full((80, 16), np.nan, np.float32)
    huge = np.where(syn.make_taco_mel(16, 80, seed=1) > 0, 1e30, -1e30).astype(np.float32)
    singles = [run(m, "post", [x])[0] for x in (a, b, c)]
    outs = run(m, "post", [a, nan, b, huge, c, nan])
    assert same(outs[0], singles[0]) and same(outs[2], singles[1]) and same(outs[4], singles[2])
    assert all(np.isfinite(o).all() for i in (0, 2, 4) for o in outs[i])


# ------------------------------------------------------------------ 4. weights
def test_weight_updates_and_reloads_reach_the_next_call():
    m = build(ref.state("tame"))
    xe, xp = inputs_of("enc", [17]), inputs_of("post", [31])

    def both(mod):
        return run(mod, "enc", xe)[0] + run(mod, "post", xp)[0]

    def fresh():
        return both(build({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}))
    last = both(m)
    assert same(last, both(model("tame")))
    with torch.no_grad():
        edits = [lambda c: c.conv1d_bank[4].conv.weight.data.mul_(1.25),
                 lambda c: c.conv1d_bank[2].bnorm.running_var.mul_(1.5),
                 lambda c: c.highways[1].W2.bias.data.add_(0.25),
                 lambda c: setattr(c.rnn.weight_hh_l0_reverse, "data", c.rnn.weight_hh_l0_reverse.data.clone() * 1.25)]
        for edit in edits:
            for c in (m.encoder.cbhg, m.postnet):
                edit(c)
            now = both(m)
            assert not np.array_equal(now[0], last[0]) and not np.array_equal(now[2], last[2])
            assert same(now, fresh())
            last = now
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.state("hot").items()})
    assert same(both(m), both(model("hot")))


def test_an_id_outside_the_embedding_and_an_empty_sentence_are_refused():
    m = model("tame")
    with pytest.raises(nat.WrnnError, match="outside the embedding"):
        m.encode_list([np.array([3, ref.DIMS.num_chars])], cbhg="hip")
    with pytest.raises(nat.WrnnError, match="outside the embedding"):
        m.encode_list([np.array([3]), np.array([-1, 4])], cbhg="hip")
    with pytest.raises(ValueError, match="at least one position"):
        m.encode_list([np.array([3]), np.array([], np.int64)], cbhg="hip")


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("regime", ["tame", "lively"])
def test_free_run_with_hip_cbhgs_against_the_reference(regime, monkeypatch):
    fx, m = load_runs(), make_model(regime, device="cuda")
    m.stop_threshold.fill_(NEVER)

    def refuse(*a, **k):
        raise AssertionError("a torch module or the deterministic switches were used")
    monkeypatch.setattr(taco, "repeatable_modules", refuse)
    hooks = [mod.register_forward_pre_hook(refuse) for mod in (m.encoder, m.encoder_proj, m.postnet, m.post_proj)]
    try:
        mel, lin, att = m.generate(fx[f"free.{regime}.x"], steps=96, backend="hip", cbhg="hip")
    finally:
        for h in hooks:
            h.remove()
    bound = max(1e-5, 8 * float(fx[f"free.{regime}.d"]))
    for name, got in (("mel", mel), ("linear", lin), ("attention", att)):
        want = fx[f"free.{regime}.{name}"]
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        print(regime, name, "err %.3g" % err, "bound %.3g" % bound)
        assert err <= bound, (name, err, bound)
    monkeypatch.undo()
    # the torch decoder loop behind the HIP encoder is the same model
    t = m.generate(fx[f"free.{regime}.x"], steps=12, backend="torch", cbhg="hip")
    assert t[0].shape == (80, 12) and float(np.abs(t[0] - mel[:, :12]).max()) < 1e-3


def test_list_rows_stop_at_the_recorded_step_and_equal_their_own_generate():
    fx, m = load_runs(), make_model("lively", device="cuda")
    m.r = int(fx["list.r"])
    m.stop_threshold.fill_(float(fx["list.thr"]))
    xs = [fx[f"list.{i}.x"] for i in range(5)]
    steps = int(fx["list.steps"])
    outs = m.generate_list(xs, steps=steps, cbhg="hip")
    for i, (x, o) in enumerate(zip(xs, outs)):
        assert o[2].shape[0] == int(fx[f"list.{i}.n_steps"]) and o[0].shape == fx[f"list.{i}.mel"].shape
        assert same(o, m.generate(x, steps=steps, cbhg="hip")), i
    assert same(outs[3], m.generate_list(xs[::-1], steps=steps, cbhg="hip", cbhg_budget=1)[1])


def test_default_is_the_torch_path_bit_for_bit():
    m = make_model("lively", device="cuda")
    m.stop_threshold.fill_(NEVER)
    xs = [syn.make_text_ids(n, ref.DIMS.num_chars, seed=60 + n) for n in (3, 7, 5)]
    a, b = m.generate_list(xs, steps=8), m.generate_list(xs, steps=8, cbhg="torch")
    assert all(same(u, v) for u, v in zip(a, b))
    assert same(m.generate(xs[1], steps=8), m.generate(xs[1], steps=8, cbhg="torch"))
    h = m.generate_list(xs, steps=8, cbhg="hip")
    assert all(u[0].shape == v[0].shape and float(np.abs(u[1] - v[1]).max()) < 1e-3 for u, v in zip(a, h))


def test_wrong_size_model_raises_under_cbhg_hip():
    torch.manual_seed(0)
    m = Tacotron(**dict(ref.DIMS.ctor_kwargs(), postnet_K=4)).cuda()
    m.r = 2
    x = syn.make_text_ids(5, ref.DIMS.num_chars, seed=1)
    assert "postnet" in m.cbhg_unsupported_reason()
    with pytest.raises(RuntimeError, match="got K 4"):
        m.generate(x, steps=6, cbhg="hip")
    with pytest.raises(RuntimeError, match="got K 4"):
        m.encode_list([x], cbhg="hip")
    assert m.generate(x, steps=6)[0].shape == (80, 6)


def test_synthesize_list_with_hip_cbhgs():
    from tests import geometries as geo
    from wavernn_amd import gen_tacotron as gt
    from wavernn_amd.fatchord_version import WaveRNN
    m = make_model("lively", device="cuda")
    m.stop_threshold.fill_(NEVER)
    d = geo.dims(ref.DIMS.n_mels, (4,), 1, rnn_dims=512)
    voc = WaveRNN(**d.ctor_kwargs()).cuda()
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, geo.TAP_SEED).items()})
    voc.eval()
    xs = [syn.make_text_ids(n, ref.DIMS.num_chars, seed=60 + n) for n in (3, 7, 5)]
    wavs = gt.synthesize_list(m, voc, xs, seed=9, steps=24, cbhg="hip")
    by_hand = voc.generate_list([gt.tacotron_mel_to_vocoder(m.generate(x, steps=24, cbhg="hip")[1]) for x in xs], seed=9,
                                wide=True)
    torch_path = gt.synthesize_list(m, voc, xs, seed=9, steps=24)
    assert len(wavs) == 3
    for a, b, c in zip(wavs, by_hand, torch_path):
        assert a.shape == b.shape == c.shape and a.shape[0] > 0 and np.array_equal(a, b)
