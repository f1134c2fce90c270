"""The frame-rate conditioning terms (csrc/frame_terms.hip: frame_cond_kernel, terms_interp_kernel)
at upsample geometries other than the reference's (5, 5, 11) / pad 2: hop below the 32 steps a
workgroup interpolates, 3 and 7 frame weights, pad·hop exactly the cascade's reach, four stages, an
odd feature count — unbatched, fold-batched with a tail fold past the utterance, and in time
chunks that start in mid-frame (WRNN_TERMS_MB).  Model dims rnn / fc 512, res_out 128, so the
XCD-resident kernel runs (last_path 5, WRNN_PATH=xcd also for more than 8 rows).

Checked against (a) the per-sample route on the same handle and seed (upsample_pack → generate,
2·MOL_TOL as tests/test_gpu_frame_terms.py) and (b) the oracle loop on the oracle's own upsampled
mel (oracle.upsample, pinned to the reference at hop 12 by tests/golden/gen_mol_hop12.npz) with
injected draws, MOL_TOL.  The oracle's aux input is the device's MelResNet output stretched: the
tiny MelResNet is not under test here, the terms are.  Geometries the frame form refuses must take
the per-sample records bit for bit.  Reference: fatchord_version.py:64-89, :169-241, :293-340."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.geometries import GEOMS, N_TERMS, ODD, TAP_SEED, dims as _dims, perturb_taps, terms_budget_mb
from tests.golden import fixtures as gf

from wavernn_amd import _native as nat
from wavernn_amd import condition
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _build(d, seed):
    """(state with the box taps perturbed by factors in [0.5, 1.5] so tap order matters, model)."""
    from wavernn_amd.fatchord_version import WaveRNN
    state = perturb_taps(syn.make_fatchord_state(d, seed), d, seed)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return state, m.eval()


@functools.lru_cache(maxsize=None)
def _geom(name):
    feat, factors, pad, jlo, nJ = GEOMS[name][:5]
    d = _dims(feat, factors, pad)
    state, m = _build(d, TAP_SEED)
    assert condition.frame_weights(m._upsample_spec())[:2] == (jlo, nJ)
    return d, state, m


@functools.lru_cache(maxsize=None)
def _launch(name, n_utt, frames, target, overlap):
    """One launch's inputs, computed once and left unchanged: frames on the device, injected draws
    and the oracle's samples for them."""
    d, state, m = _geom(name)
    mel = np.stack([syn.make_mel(d.feat_dims, frames, 40 + i) for i in range(n_utt)])
    mel_f, aux, _ = m.frames(torch.from_numpy(mel).to(DEV))
    hop = d.hop_length
    ms, as_ = [], []
    for u in range(n_utt):
        mp = orc.pad_tensor(mel[u].T[None], d.pad)[0].T
        um, _ = orc.upsample(mp, state, d.upsample_factors, d.res_blocks, d.pad)
        ua = np.repeat(aux[u].cpu().numpy(), hop, axis=1).T            # resnet_stretch of the device's aux
        um, ua = um[None], np.ascontiguousarray(ua)[None]
        if target > 0:
            um, ua = orc.fold_with_overlap(um, target, overlap), orc.fold_with_overlap(ua, target, overlap)
        ms.append(um)
        as_.append(ua)
    ms, as_ = np.concatenate(ms, 0), np.concatenate(as_, 0)
    rows, steps = ms.shape[:2]
    noise = syn.make_noise("MOL", rows, steps, d.n_classes, 21)
    ref, _ = orc.fatchord_loop(state, "MOL", ms, as_, noise)
    return mel_f, aux, torch.from_numpy(noise).to(DEV), ref


def _env(monkeypatch, terms_mb=None):
    monkeypatch.setenv("WRNN_PATH", "xcd")
    for k in ("WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES"):
        monkeypatch.delenv(k, raising=False)
    if terms_mb is None:
        monkeypatch.delenv("WRNN_TERMS_MB", raising=False)
    else:
        monkeypatch.setenv("WRNN_TERMS_MB", terms_mb)


def _vs_records(m, mel_f, aux, target, overlap, seed, what, exact=False):
    """(a): the frames entry against upsample_pack → generate, same handle and seed."""
    spec, loop = m._upsample_spec(), m.loop_handle()
    got, _ = loop.generate_frames(spec, mel_f, aux, target, overlap, seed=seed)
    assert loop.info["last_path"] == 5
    ref, _ = loop.generate(condition.upsample_pack(spec, mel_f, aux, target, overlap), seed=seed)
    assert loop.info["last_path"] == 5 and got.shape == ref.shape
    err = float((got - ref).abs().max())
    print(f"{what}: frames vs per-sample records max |Δ| {err:.3g}")
    if exact:
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    else:
        assert err <= 2 * gf.MOL_TOL, (what, err)
    return got


def _vs_oracle(m, mel_f, aux, target, overlap, noise, ref, what):
    """(b): the frames entry with injected draws against the oracle loop."""
    loop = m.loop_handle()
    got, _ = loop.generate_frames(m._upsample_spec(), mel_f, aux, target, overlap, noise=noise)
    assert loop.info["last_path"] == 5 and tuple(got.shape) == ref.shape
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"{what}: vs oracle max |Δ| {err:.3g}")
    assert err <= gf.MOL_TOL, (what, err)


@pytest.mark.parametrize("name", ODD)
def test_unbatched_one_and_eight_utterances(name, monkeypatch):
    _env(monkeypatch)
    d, _, m = _geom(name)
    frames = GEOMS[name][5]
    for n_utt in (1, 8):
        mel = torch.cat([torch.from_numpy(syn.make_mel(d.feat_dims, frames, 90 + i))[None] for i in range(n_utt)], 0)
        mel_f, aux, _ = m.frames(mel.to(DEV))
        _vs_records(m, mel_f, aux, 0, 0, 11, f"{name}, {n_utt} utterances")


@pytest.mark.parametrize("name", ODD)
def test_unbatched_vs_oracle(name, monkeypatch):
    _env(monkeypatch)
    _, _, m = _geom(name)
    mel_f, aux, noise, ref = _launch(name, 2, GEOMS[name][5], 0, 0)
    _vs_oracle(m, mel_f, aux, 0, 0, noise, ref, f"{name}, 2 utterances")


@pytest.mark.parametrize("name", ODD)
def test_fold_batched_two_utterances_with_a_tail_fold(name, monkeypatch):
    """≥ 4 folds per utterance, the last one running past the utterance (its steps take
    W·[0 | 0 | 1]); two utterances in one launch, so row r is fold r % nf of utterance r / nf.
    hop12: 720 samples, stride 170 → 5 folds, the last from 680 to 870; 10 rows: two launches of
    the one-row-per-XCD kernel (8 + 2)."""
    _env(monkeypatch)
    d, _, m = _geom(name)
    frames, target, overlap = GEOMS[name][6]
    L = frames * d.hop_length
    nf = m.fold_count(L, target, overlap)[0]
    assert nf >= 4 and (nf - 1) * (target + overlap) + target + 2 * overlap > L
    mel_f, aux, noise, ref = _launch(name, 2, frames, target, overlap)
    assert ref.shape == (2 * nf, target + 2 * overlap)
    _vs_records(m, mel_f, aux, target, overlap, 12, f"{name}, 2 × {nf} folds")
    _vs_oracle(m, mel_f, aux, target, overlap, noise, ref, f"{name}, 2 × {nf} folds")


@pytest.mark.parametrize("name", list(GEOMS))
def test_time_chunked_launches(name, monkeypatch):
    """WRNN_TERMS_MB sized for X steps per launch, X neither a multiple of hop nor of 32: chunks
    start in mid-frame and in mid-workgroup, each with one extra terms row.  The launch loop takes
    Lc_max = ⌊budget / (nb·(N + KXc)) − 1⌋ steps (budget in floats, N = 5120 terms, KXc = feat +
    128 + 4), so a budget of (X + 1.5)·nb·(N + KXc) floats gives exactly X."""
    d, _, m = _geom(name)
    n_utt = 1 if name == "hop275" else 2
    frames, X = GEOMS[name][5], GEOMS[name][7]
    L = frames * d.hop_length
    assert X % d.hop_length and X % 32 and -(-L // X) >= 3
    mel_f, aux, noise, ref = _launch(name, n_utt, frames, 0, 0)
    _env(monkeypatch)
    spec, loop = m._upsample_spec(), m.loop_handle()
    whole, _ = loop.generate_frames(spec, mel_f, aux, 0, 0, seed=13)
    _env(monkeypatch, terms_budget_mb(X, n_utt, N_TERMS + d.feat_dims + 128 + 4))
    _vs_oracle(m, mel_f, aux, 0, 0, noise, ref, f"{name}, chunks of {X} steps")
    chunked, _ = loop.generate_frames(spec, mel_f, aux, 0, 0, seed=13)
    assert loop.info["last_path"] == 5
    err = float((chunked - whole).abs().max())
    print(f"{name}: chunked vs one launch max |Δ| {err:.3g}")
    assert err <= 2 * gf.MOL_TOL, err


@pytest.mark.parametrize("feat,factors,pad,frames", [(80, (5, 5, 11), 1, 21), (80, (1, 1, 1, 2), 4, 24)])
def test_refused_geometries_take_the_per_sample_records(feat, factors, pad, frames, monkeypatch):
    """wrnn_frame_weights refuses pad·hop below the reach ((5, 5, 11) with pad 1: 275 < 341) and
    more than 8 frame weights ((1, 1, 1, 2) with pad 4: 9): on the XCD path the frames entry then
    builds the per-sample records itself — bit-identical to the two calls."""
    _env(monkeypatch)
    d = _dims(feat, factors, pad)
    _, m = _build(d, 5)
    with pytest.raises(nat.WrnnError):
        condition.frame_weights(m._upsample_spec())
    mel = torch.cat([torch.from_numpy(syn.make_mel(feat, frames, 70 + i))[None] for i in range(2)], 0)
    mel_f, aux, _ = m.frames(mel.to(DEV))
    _vs_records(m, mel_f, aux, 0, 0, 14, f"{factors} pad {pad}", exact=True)
