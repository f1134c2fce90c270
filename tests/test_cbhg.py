"""The ragged CBHG without a GPU: the float64 restatement (tests/cbhg_ref.py) against the reference's
records, and the parts of the wrnn_cbhg_* C-ABI that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cbhg_ref as ref
from wavernn_amd import _native as nat
from wavernn_amd import synthetic as syn
from wavernn_amd.tacotron import Tacotron

ENC = (16, 128, 128, 128, 128, 0, 4, 1, 256, 148, 256, 256)
POST = (8, 80, 128, 256, 80, 1, 4, 0, 0, 0, 0, 80)
FIELDS = [f for f, _ in nat.CbhgCfg._fields_]


def cfg(base, **kw):
    v = dict(zip(FIELDS, base))
    v.update(kw)
    return nat.CbhgCfg(*[v[f] for f in FIELDS])


# ------------------------------------------------------------------ the restatement against the records
@pytest.mark.parametrize("regime", list(ref.REGIMES))
@pytest.mark.parametrize("which", ["enc", "post"])
def test_restatement_meets_every_recorded_stage_and_output(which, regime):
    """All recorded lengths packed into ONE ragged list: every sentence must come out as the reference
    computed it alone."""
    fx = ref.load(which, regime)
    lengths = [int(t) for t in fx["lengths"]]
    outs = ref.cbhg_list(ref.state(regime), which, [ref.fixture_input(fx, which, T) for T in lengths])
    worst = {}
    for T, o in zip(lengths, outs):
        for name in ("rnn", "proj"):
            err = float(np.abs(o[name] - fx[f"T{T}.{name}"]).max())
            worst[name] = max(worst.get(name, 0.0), err / ref.bound(fx[f"T{T}.d"]))
            assert err <= ref.bound(fx[f"T{T}.d"]), (T, name, err)
        if T in fx["stage_lengths"]:
            for s in ref.STAGES:
                if f"T{T}.stage.{s}" not in fx:
                    assert s == "front" and which == "post"
                    continue
                err = float(np.abs(o[s] - fx[f"T{T}.stage.{s}"]).max())
                worst[s] = max(worst.get(s, 0.0), err / ref.bound(fx[f"T{T}.stage.{s}.d"]))
                assert err <= ref.bound(fx[f"T{T}.stage.{s}.d"]), (T, s, err)
    print(which, regime, "worst err / bound", {k: round(v, 3) for k, v in worst.items()})


def test_default_state_is_unchanged_by_the_hot_parameter():
    a = syn.make_tacotron_state(ref.DIMS, seed=ref.SEED)
    assert syn.state_digest(a) == syn.state_digest(ref.state("tame"))
    hot = ref.state("hot")
    scaled = [k for k in a if not np.array_equal(a[k], hot[k])]
    assert scaled and all(syn.is_cbhg_gate_matrix(k) for k in scaled)
    assert len(scaled) == 2 * (4 + 4)       # per CBHG: four GRU matrices, four W2
    k = "postnet.rnn.weight_hh_l0_reverse"
    np.testing.assert_allclose(hot[k], 5.0 * a[k], rtol=2e-7, atol=0)     # scaled in float64, rounded once


# ------------------------------------------------------------------ the C-ABI without a device
def test_supported_takes_the_two_size_sets_only():
    L = nat.lib()
    assert L.wrnn_cbhg_supported(ctypes.byref(cfg(ENC))) == 0
    assert L.wrnn_cbhg_supported(ctypes.byref(cfg(POST))) == 0
    assert L.wrnn_cbhg_supported(ctypes.byref(cfg(ENC, num_chars=40))) == 0
    for bad in (cfg(ENC, K=17), cfg(ENC, channels=256), cfg(ENC, highways=3), cfg(POST, K=16), cfg(POST, highways=3),
                cfg(POST, proj1=128), cfg(POST, pre_highway=0), cfg(ENC, front=0)):
        assert L.wrnn_cbhg_supported(ctypes.byref(bad)) == -6
        msg = L.wrnn_cond_last_error().decode()
        assert "K 16" in msg and "K 8" in msg and f"got K {bad.K}" in msg
    assert L.wrnn_cbhg_scratch_bytes(ctypes.byref(cfg(ENC, K=17)), 10) == -6
    assert L.wrnn_cbhg_supported(None) == -1


@pytest.mark.parametrize("base", [ENC, POST])
def test_scratch_layout(base):
    L, c = nat.lib(), cfg(base)
    widths = {"front": c.in_channels, "bank": c.K * c.channels, "pooled": c.K * c.channels, "proj1": c.proj1,
              "residual": c.proj2, "highway_in": c.channels, "highway_out": c.channels, "gi": 6 * c.channels,
              "rnn": 2 * c.channels}
    for P in (1, 33, 1000):
        total = L.wrnn_cbhg_scratch_bytes(ctypes.byref(c), P)
        offs = (ctypes.c_int64 * len(nat.CBHG_STAGES))()
        assert L.wrnn_cbhg_scratch_layout(ctypes.byref(c), P, offs) == 0
        o = dict(zip(nat.CBHG_STAGES, list(offs)))
        assert (o["front"] == -1) == (c.front == 0)
        assert (o["highway_in"] == o["residual"]) == (c.pre_highway == 0)
        spans = sorted({(v, v + P * widths[k]) for k, v in o.items() if v >= 0})
        assert all(a % 64 == 0 for a, _ in spans)                       # 256-byte sections
        assert all(b <= a2 for (_, b), (a2, _) in zip(spans, spans[1:]))    # disjoint
        assert spans[-1][1] * 4 <= total
    assert L.wrnn_cbhg_scratch_bytes(ctypes.byref(c), 1000) > L.wrnn_cbhg_scratch_bytes(ctypes.byref(c), 33)
    assert L.wrnn_cbhg_scratch_bytes(ctypes.byref(c), 0) == -1
    assert L.wrnn_cbhg_scratch_layout(ctypes.byref(c), 5, None) == -1
    # the pooled bank is 8 KB a position in the encoder (K·channels floats)
    assert widths["pooled"] * 4 == (8192 if base is ENC else 4096)


def test_run_refuses_bad_arguments_before_it_touches_the_device():
    """Pointers here are made-up addresses: every refusal must come before anything reads them."""
    L, c = nat.lib(), cfg(POST)
    fake = 0x10000
    w = nat.CbhgWeights()
    for name, typ in nat.CbhgWeights._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, fake)
        else:
            arr = getattr(w, name)
            for i in range(len(arr)):
                arr[i] = fake
    need = L.wrnn_cbhg_scratch_bytes(ctypes.byref(c), 12)

    def run(offsets, n, weights=w, scratch_bytes=need, inp=fake, out=fake):
        offs = (ctypes.c_int * len(offsets))(*offsets)
        rc = L.wrnn_cbhg_run(ctypes.byref(c), ctypes.byref(weights), inp, offs, n, None, out, fake, scratch_bytes, None)
        return rc, L.wrnn_cond_last_error().decode()
    assert run([0, 5, 12], 0)[0] == -1
    rc, msg = run([1, 5, 12], 2)
    assert rc == -1 and "offsets[0]" in msg
    rc, msg = run([0, 5, 5], 2)
    assert rc == -1 and "offsets[2]" in msg
    rc, msg = run([0, 7, 5], 2)
    assert rc == -1 and "offsets[2]" in msg
    rc, msg = run([0, 5, 12], 2, scratch_bytes=need - 1)
    assert rc == -1 and "scratch" in msg and str(need) in msg
    assert run([0, 5, 12], 2, inp=None)[0] == -1
    assert run([0, 5, 12], 2, out=None)[0] == -1
    assert run([0, 5, 12], 2, inp=fake + 4)[0] == -1                    # misaligned
    w2 = nat.CbhgWeights.from_buffer_copy(w)
    w2.rnn_w_hh_r = None
    rc, msg = run([0, 5, 12], 2, weights=w2)
    assert rc == -1 and "weight pointer" in msg
    w3 = nat.CbhgWeights.from_buffer_copy(w)
    w3.bank_w[9] = None             # beyond the postnet's K = 8: ignored, the next refusal is the scratch
    rc, msg = run([0, 5, 12], 2, weights=w3, scratch_bytes=need - 1)
    assert rc == -1 and "scratch" in msg
    assert L.wrnn_cbhg_run(ctypes.byref(cfg(POST, K=9)), ctypes.byref(w), fake, (ctypes.c_int * 2)(0, 3), 1, None, fake, fake,
                           need, None) == -6


# ------------------------------------------------------------------ Python surface without a GPU
def test_cbhg_hip_on_a_cpu_model_raises_with_the_reason():
    torch.manual_seed(0)
    m = Tacotron(**ref.DIMS.ctor_kwargs())
    m.r = 2
    x = ref.enc_input(5)
    assert m.cbhg_unsupported_reason() == "the model is not on a GPU"
    for call in (lambda: m.generate(x, steps=4, cbhg="hip"), lambda: m.generate_list([x], steps=4, cbhg="hip"),
                 lambda: m.encode_list([x], cbhg="hip"),
                 lambda: m.postprocess_list([torch.zeros(1, 80, 4)], cbhg="hip")):
        with pytest.raises(RuntimeError, match="not on a GPU"):
            call()
    with pytest.raises(ValueError, match="cbhg must be"):
        m.generate(x, steps=4, cbhg="fast")
    a = m.generate(x, steps=4, backend="torch")
    b = m.generate(x, steps=4, backend="torch", cbhg="torch")
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    c = m.kernel_cfg and m.cbhg_cfg("encoder")
    assert (c.K, c.in_channels, c.front, c.num_chars, c.tail_out) == (16, 128, 1, ref.DIMS.num_chars, 256)
    c = m.cbhg_cfg("postnet")
    assert (c.K, c.in_channels, c.proj1, c.proj2, c.pre_highway, c.front, c.tail_out) == (8, 80, 256, 80, 1, 0, 80)
