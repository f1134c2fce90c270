"""Deterministic synthetic inputs for the WaveRNN generation path.

There are no pretrained weights (the reference's `pretrained/*.zip` are absent,
SURVEY.md §8(c)), so every configuration runs on random weights.  This module is
the single documented generator used by the golden-fixture script, the tests and
`bench.py`; the fixtures store a SHA-256 of what it produced so any drift in it is
caught instead of silently invalidating the goldens.

Key naming and shapes follow the reference state_dict of
`models/fatchord_version.py:92-129` (measured key list: SURVEY.md §8(a15)) and
`models/deepmind_version.py:9-34`.
"""
from __future__ import annotations

import hashlib
import zlib
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np


@dataclass(frozen=True)
class FatchordDims:
    """Constructor arguments of the reference `WaveRNN` (fatchord_version.py:93-95)."""
    rnn_dims: int = 512
    fc_dims: int = 512
    bits: int = 9
    pad: int = 2
    upsample_factors: Tuple[int, ...] = (5, 5, 11)
    feat_dims: int = 80
    compute_dims: int = 128
    res_out_dims: int = 128
    res_blocks: int = 10
    hop_length: int = 275
    sample_rate: int = 22050
    mode: str = "MOL"

    @property
    def aux_dims(self) -> int:          # fatchord_version.py:110
        return self.res_out_dims // 4

    @property
    def n_classes(self) -> int:         # fatchord_version.py:99-102
        return 2 ** self.bits if self.mode == "RAW" else 30

    def ctor_kwargs(self) -> dict:
        return dict(rnn_dims=self.rnn_dims, fc_dims=self.fc_dims, bits=self.bits, pad=self.pad,
                    upsample_factors=self.upsample_factors, feat_dims=self.feat_dims,
                    compute_dims=self.compute_dims, res_out_dims=self.res_out_dims,
                    res_blocks=self.res_blocks, hop_length=self.hop_length,
                    sample_rate=self.sample_rate, mode=self.mode)


# The hparams.py vocoder section (hparams.py:20-44) in the 800k MoL configuration.
DEFAULT_MOL = FatchordDims()
DEFAULT_RAW = FatchordDims(mode="RAW")
# Small dims used to exercise the generic-dimension code paths (fc != rnn, bits != 9).
TINY_RAW = FatchordDims(rnn_dims=64, fc_dims=96, bits=8, compute_dims=16, res_out_dims=16,
                        res_blocks=1, mode="RAW")
TINY_MOL = FatchordDims(rnn_dims=64, fc_dims=96, compute_dims=16, res_out_dims=16,
                        res_blocks=1, mode="MOL")
# BASELINE config 4: rnn_dims 896 with 4x4 block-sparse GRU weights (pruning.prune_state, 95 %)
SPARSE896_MOL = FatchordDims(rnn_dims=896, mode="MOL")


def fatchord_state_shapes(d: FatchordDims) -> Dict[str, Tuple[tuple, str]]:
    """Every state_dict key of the reference model → (shape, kind)."""
    s: Dict[str, Tuple[tuple, str]] = {"step": ((1,), "step")}
    c, k = d.compute_dims, 2 * d.pad + 1
    s["upsample.resnet.conv_in.weight"] = ((c, d.feat_dims, k), "w")

    def bn(prefix: str):
        s[prefix + ".weight"] = ((c,), "bn_w")
        s[prefix + ".bias"] = ((c,), "bn_b")
        s[prefix + ".running_mean"] = ((c,), "bn_rm")
        s[prefix + ".running_var"] = ((c,), "bn_rv")
        s[prefix + ".num_batches_tracked"] = ((), "nbt")

    bn("upsample.resnet.batch_norm")
    for i in range(d.res_blocks):
        p = f"upsample.resnet.layers.{i}"
        s[p + ".conv1.weight"] = ((c, c, 1), "w")
        s[p + ".conv2.weight"] = ((c, c, 1), "w")
        bn(p + ".batch_norm1")
        bn(p + ".batch_norm2")
    s["upsample.resnet.conv_out.weight"] = ((d.res_out_dims, c, 1), "w")
    s["upsample.resnet.conv_out.bias"] = ((d.res_out_dims,), "b:upsample.resnet.conv_out.weight")
    for i, sc in enumerate(d.upsample_factors):
        s[f"upsample.up_layers.{2 * i + 1}.weight"] = ((1, 1, 1, 2 * sc + 1), "box")
    r, f, a = d.rnn_dims, d.fc_dims, d.aux_dims
    s["I.weight"] = ((r, d.feat_dims + a + 1), "w")
    s["I.bias"] = ((r,), "b:I.weight")
    for name, n_in in (("rnn1", r), ("rnn2", r + a)):
        s[f"{name}.weight_ih_l0"] = ((3 * r, n_in), "w")
        s[f"{name}.weight_hh_l0"] = ((3 * r, r), "w")
        s[f"{name}.bias_ih_l0"] = ((3 * r,), f"b:{name}.weight_ih_l0")
        s[f"{name}.bias_hh_l0"] = ((3 * r,), f"b:{name}.weight_hh_l0")
    s["fc1.weight"] = ((f, r + a), "w")
    s["fc1.bias"] = ((f,), "b:fc1.weight")
    s["fc2.weight"] = ((f, f + a), "w")
    s["fc2.bias"] = ((f,), "b:fc2.weight")
    s["fc3.weight"] = ((d.n_classes, f), "w")
    s["fc3.bias"] = ((d.n_classes,), "b:fc3.weight")
    return s


def _rng(seed: int, key: str) -> np.random.Generator:
    return np.random.default_rng(np.random.SeedSequence([seed, zlib.crc32(key.encode())]))


def make_fatchord_state(d: FatchordDims, seed: int = 0, step: int = 800_000) -> Dict[str, np.ndarray]:
    """Random weights in the reference layout: weights/biases U(±1/sqrt(fan_in)) as torch's
    default init, BatchNorm statistics in a plausible range, up-layer box filters 1/k (the
    reference's init, fatchord_version.py:78) with ±10% jitter.  One independent stream per key."""
    shapes = fatchord_state_shapes(d)
    out: Dict[str, np.ndarray] = {}
    for key in sorted(shapes):
        shape, kind = shapes[key]
        g = _rng(seed, key)
        if kind == "step":
            out[key] = np.array([step], dtype=np.int64)
        elif kind == "nbt":
            out[key] = np.array(0, dtype=np.int64)
        elif kind == "w":
            bound = 1.0 / np.sqrt(float(np.prod(shape[1:])))
            out[key] = g.uniform(-bound, bound, size=shape).astype(np.float32)
        elif kind.startswith("b:"):
            wshape = shapes[kind[2:]][0]
            bound = 1.0 / np.sqrt(float(np.prod(wshape[1:])))
            out[key] = g.uniform(-bound, bound, size=shape).astype(np.float32)
        elif kind == "bn_w":
            out[key] = g.uniform(0.8, 1.2, size=shape).astype(np.float32)
        elif kind == "bn_b":
            out[key] = g.uniform(-0.1, 0.1, size=shape).astype(np.float32)
        elif kind == "bn_rm":
            out[key] = g.uniform(-0.2, 0.2, size=shape).astype(np.float32)
        elif kind == "bn_rv":
            out[key] = g.uniform(0.5, 1.5, size=shape).astype(np.float32)
        elif kind == "box":
            kk = shape[-1]
            out[key] = (np.full(shape, 1.0 / kk) * (1.0 + g.uniform(-0.1, 0.1, size=shape))).astype(np.float32)
        else:  # pragma: no cover
            raise ValueError(kind)
    # Shape the output head like a trained vocoder's so parity tests are sensitive to the
    # network arithmetic: with plain init the RAW softmax is ~uniform (labels then follow
    # the Exp(1) noise alone) and MoL log-scales ~0 clamp half the samples to ±1.
    if d.mode == "RAW":
        out["fc3.weight"] = (out["fc3.weight"] * np.float32(16.0)).astype(np.float32)
    else:
        nr = d.n_classes // 3
        out["fc3.bias"][2 * nr:] -= np.float32(5.0)
    return out


def make_mel(n_mels: int, n_frames: int, seed: int = 1) -> np.ndarray:
    """Normalised mel (n_mels, T) in [0, 1) — the range gen_wavernn.py:52-55 accepts."""
    return np.random.default_rng(seed).random((n_mels, n_frames), dtype=np.float32)


def frames_for_seconds(seconds: float, sample_rate: int = 22050, hop: int = 275) -> int:
    """T such that wave_len = hop*(T-1) covers `seconds`."""
    return int(seconds * sample_rate / hop) + 1


def make_conditioning(B: int, L: int, feat: int, res_out: int, seed: int = 2):
    """Upsampled conditioning as generate() sees it after fold: mels [B][L][feat] in [0,1),
    aux [B][L][res_out] ~ 0.5·N(0,1) (MelResNet output scale)."""
    g = np.random.default_rng(seed)
    mels = g.random((B, L, feat), dtype=np.float32)
    aux = (0.5 * g.standard_normal((B, L, res_out))).astype(np.float32)
    return mels, aux


MOL_NOISE_K = 11   # u1[10] (mixture Gumbel draw) then u2 (logistic draw): distribution.py:106,118


def make_noise(mode: str, B: int, L: int, n_classes: int, seed: int = 3) -> np.ndarray:
    """Injected noise in the reference draw order, layout [L][B][K].

    MOL: u1[0:10] then u2, both U(1e-5, 1-1e-5) (utils/distribution.py:106,118).
    RAW: q[0:n_classes] ~ Exp(1); Categorical.sample() ≡ argmax(probs / q).
    """
    g = np.random.default_rng(seed)
    if mode == "MOL":
        u = g.random((L, B, MOL_NOISE_K))
        u = 1e-5 + (1.0 - 2e-5) * u
        return np.clip(u.astype(np.float32), np.float32(1e-5), np.float32(1.0 - 1e-5))
    if mode == "RAW":
        q = g.standard_exponential((L, B, n_classes), dtype=np.float32)
        return np.maximum(q, np.float32(1e-30))
    raise ValueError(mode)


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def state_digest(state: Dict[str, np.ndarray]) -> str:
    return digest(*[state[k] for k in sorted(state)])


# ---------------------------------------------------------------------- deepmind_version
@dataclass(frozen=True)
class DeepmindDims:
    """Constructor arguments of models/deepmind_version.py:WaveRNN (:9-34)."""
    hidden_size: int = 896
    quantisation: int = 256

    @property
    def split_size(self) -> int:
        return self.hidden_size // 2

    def ctor_kwargs(self) -> dict:
        return dict(hidden_size=self.hidden_size, quantisation=self.quantisation)


DEFAULT_DM = DeepmindDims()
TINY_DM = DeepmindDims(hidden_size=64, quantisation=256)


def deepmind_state_shapes(d: DeepmindDims) -> Dict[str, tuple]:
    H, S, Q = d.hidden_size, d.split_size, d.quantisation
    return {"R.weight": (3 * H, H), "O1.weight": (S, S), "O1.bias": (S,), "O2.weight": (Q, S), "O2.bias": (Q,),
            "O3.weight": (S, S), "O3.bias": (S,), "O4.weight": (Q, S), "O4.bias": (Q,),
            "I_coarse.weight": (3 * S, 2), "I_fine.weight": (3 * S, 3),
            "bias_u": (H,), "bias_r": (H,), "bias_e": (H,)}


def make_deepmind_state(d: DeepmindDims, seed: int = 0) -> Dict[str, np.ndarray]:
    """Random weights U(±1/sqrt(fan_in)) (torch Linear init); the gate biases (zeros in the
    reference init, :29-31) get U(±0.1) and the two output heads are scaled ×16, so the sampled
    labels depend on the network arithmetic and not only on the noise."""
    out: Dict[str, np.ndarray] = {}
    for key, shape in sorted(deepmind_state_shapes(d).items()):
        g = _rng(seed, "dm:" + key)
        if key.startswith("bias_"):
            out[key] = g.uniform(-0.1, 0.1, size=shape).astype(np.float32)
            continue
        fan_in = shape[1] if len(shape) == 2 else deepmind_state_shapes(d)[key.replace("bias", "weight")][1]
        bound = 1.0 / np.sqrt(float(fan_in))
        out[key] = g.uniform(-bound, bound, size=shape).astype(np.float32)
    for k in ("O2.weight", "O4.weight"):
        out[k] = (out[k] * np.float32(16.0)).astype(np.float32)
    return out


def make_dm_noise(B: int, L: int, Q: int = 256, seed: int = 3) -> np.ndarray:
    """Exp(1) draws [L][B][2·Q]: the coarse Categorical's q, then the fine one's, per step."""
    g = np.random.default_rng(seed)
    return g.exponential(1.0, size=(L, B, 2 * Q)).astype(np.float32)


# ---------------------------------------------------------------------- tacotron
@dataclass(frozen=True)
class TacotronDims:
    """Constructor arguments of models/tacotron.py:Tacotron (:290); the defaults are hparams.py:67-77
    with the symbol table's size left to the caller."""
    embed_dims: int = 256
    num_chars: int = 148
    encoder_dims: int = 128
    decoder_dims: int = 256
    n_mels: int = 80
    fft_bins: int = 80
    postnet_dims: int = 128
    encoder_K: int = 16
    lstm_dims: int = 512
    postnet_K: int = 8
    num_highways: int = 4
    dropout: float = 0.5
    stop_threshold: float = -3.4

    def ctor_kwargs(self) -> dict:
        return {k: getattr(self, k) for k in self.__dataclass_fields__}


DEFAULT_TACOTRON = TacotronDims()


def tacotron_state_shapes(d: TacotronDims) -> Dict[str, Tuple[tuple, str]]:
    """Every state_dict key of the reference Tacotron → (shape, kind). Kinds: 'x' xavier matrix,
    'xd' xavier matrix of the decoder (scaled), 'b' bias, bn_*, 'emb', and the scalar buffers."""
    s: Dict[str, Tuple[tuple, str]] = {"step": ((1,), "step"), "stop_threshold": ((), "thr"), "decoder.r": ((), "r")}

    def lin(p, o, i, bias=True, kind="x"):
        s[p + ".weight"] = ((o, i), kind)
        if bias:
            s[p + ".bias"] = ((o,), "b")

    def bnconv(p, i, o, k):
        s[p + ".conv.weight"] = ((o, i, k), "x")
        s[p + ".bnorm.weight"] = ((o,), "bn_w")
        s[p + ".bnorm.bias"] = ((o,), "bn_b")
        s[p + ".bnorm.running_mean"] = ((o,), "bn_rm")
        s[p + ".bnorm.running_var"] = ((o,), "bn_rv")
        s[p + ".bnorm.num_batches_tracked"] = ((), "nbt")

    def cbhg(p, K, cin, ch, proj):
        for k in range(1, K + 1):
            bnconv(f"{p}.conv1d_bank.{k - 1}", cin, ch, k)
        bnconv(p + ".conv_project1", K * ch, proj[0], 3)
        bnconv(p + ".conv_project2", proj[0], proj[1], 3)
        if proj[1] != ch:
            lin(p + ".pre_highway", ch, proj[1], bias=False)
        for i in range(d.num_highways):
            lin(f"{p}.highways.{i}.W1", ch, ch)
            lin(f"{p}.highways.{i}.W2", ch, ch)
        for sfx in ("", "_reverse"):
            s[f"{p}.rnn.weight_ih_l0{sfx}"] = ((3 * ch, ch), "x")
            s[f"{p}.rnn.weight_hh_l0{sfx}"] = ((3 * ch, ch), "x")
            s[f"{p}.rnn.bias_ih_l0{sfx}"] = ((3 * ch,), "b")
            s[f"{p}.rnn.bias_hh_l0{sfx}"] = ((3 * ch,), "b")

    D, H, M = d.decoder_dims, d.lstm_dims, d.n_mels
    s["encoder.embedding.weight"] = ((d.num_chars, d.embed_dims), "emb")
    lin("encoder.pre_net.fc1", 256, d.embed_dims)
    lin("encoder.pre_net.fc2", 128, 256)
    cbhg("encoder.cbhg", d.encoder_K, d.encoder_dims, d.encoder_dims, (d.encoder_dims, d.encoder_dims))
    lin("encoder_proj", D, D, bias=False)
    lin("decoder.prenet.fc1", 256, M, kind="xd")
    lin("decoder.prenet.fc2", 128, 256, kind="xd")
    s["decoder.attn_net.conv.weight"] = ((32, 2, 31), "xd")
    lin("decoder.attn_net.L", D, 32, kind="xd")
    lin("decoder.attn_net.W", D, D, kind="xd")
    lin("decoder.attn_net.v", 1, D, bias=False, kind="xd")
    s["decoder.attn_rnn.weight_ih"] = ((3 * D, D + D // 2), "xd")
    s["decoder.attn_rnn.weight_hh"] = ((3 * D, D), "xd")
    s["decoder.attn_rnn.bias_ih"] = ((3 * D,), "b")
    s["decoder.attn_rnn.bias_hh"] = ((3 * D,), "b")
    lin("decoder.rnn_input", H, 2 * D, kind="xd")
    for n in ("res_rnn1", "res_rnn2"):
        s[f"decoder.{n}.weight_ih"] = ((4 * H, H), "xd")
        s[f"decoder.{n}.weight_hh"] = ((4 * H, H), "xd")
        s[f"decoder.{n}.bias_ih"] = ((4 * H,), "b")
        s[f"decoder.{n}.bias_hh"] = ((4 * H,), "b")
    lin("decoder.mel_proj", M * 20, H, bias=False, kind="xd")
    cbhg("postnet", d.postnet_K, M, d.postnet_dims, (256, 80))
    lin("post_proj", d.fft_bins, 2 * d.postnet_dims, bias=False)
    return s


def is_cbhg_gate_matrix(key: str) -> bool:
    """The matrices that drive the gates of the two CBHGs: the bidirectional GRU's and the highways' W2."""
    if not (key.startswith("encoder.cbhg.") or key.startswith("postnet.")):
        return False
    return ".rnn.weight_" in key or (".highways." in key and key.endswith(".W2.weight"))


def make_tacotron_state(d: TacotronDims = DEFAULT_TACOTRON, seed: int = 0, scale: float = 1.0, r: int = 2,
                        step: int = 180_000, cbhg_gate_scale: float = 1.0) -> Dict[str, np.ndarray]:
    """Random Tacotron weights in the reference layout: matrices xavier-uniform (the reference's init),
    biases U(±0.1), BatchNorm statistics in a plausible range, the embedding N(0, 1); the decoder's
    matrices are multiplied by `scale` (1 tame, 2 lively, 3-4 saturated attention and gates), the CBHGs'
    gate matrices (is_cbhg_gate_matrix) by `cbhg_gate_scale` (1 tame, 5 hot: saturated GRU and highway
    gates). One independent stream per key."""
    shapes = tacotron_state_shapes(d)
    out: Dict[str, np.ndarray] = {}
    for key in sorted(shapes):
        shape, kind = shapes[key]
        g = _rng(seed, "taco:" + key)
        if kind == "step":
            out[key] = np.array([step], dtype=np.int64)
        elif kind == "thr":
            out[key] = np.array(d.stop_threshold, dtype=np.float32)
        elif kind == "r":
            out[key] = np.array(r, dtype=np.int32)
        elif kind == "nbt":
            out[key] = np.array(0, dtype=np.int64)
        elif kind in ("x", "xd"):
            rf = float(np.prod(shape[2:])) if len(shape) > 2 else 1.0
            bound = np.sqrt(6.0 / ((shape[0] + shape[1]) * rf))
            w = g.uniform(-bound, bound, size=shape)
            mult = scale if kind == "xd" else (cbhg_gate_scale if is_cbhg_gate_matrix(key) else 1.0)
            out[key] = (w * mult).astype(np.float32)
        elif kind == "emb":
            out[key] = g.standard_normal(shape).astype(np.float32)
        elif kind == "b":
            out[key] = g.uniform(-0.1, 0.1, size=shape).astype(np.float32)
        elif kind == "bn_w":
            out[key] = g.uniform(0.8, 1.2, size=shape).astype(np.float32)
        elif kind == "bn_b":
            out[key] = g.uniform(-0.1, 0.1, size=shape).astype(np.float32)
        elif kind == "bn_rm":
            out[key] = g.uniform(-0.2, 0.2, size=shape).astype(np.float32)
        elif kind == "bn_rv":
            out[key] = g.uniform(0.5, 1.5, size=shape).astype(np.float32)
        else:  # pragma: no cover
            raise ValueError(kind)
    return out


def make_text_ids(n: int, num_chars: int = 148, seed: int = 5) -> np.ndarray:
    """n symbol ids in [1, num_chars) — a text_to_sequence output of length n."""
    return np.random.default_rng([seed, n]).integers(1, num_chars, size=n).astype(np.int64)


def make_taco_mel(frames: int, n_mels: int = 80, seed: int = 9) -> np.ndarray:
    """(n_mels, frames) float32 ~ 2·N(0, 1): a decoder output in the lively regime's range."""
    return (2.0 * np.random.default_rng([seed, frames, n_mels]).standard_normal((n_mels, frames))).astype(np.float32)


def make_encoder_seq(t_enc: int, dims: int = 256, seed: int = 7):
    """(encoder_seq, encoder_seq_proj), each (t_enc, dims) float32: a biGRU-like output in (−1, 1) and an
    independent projection-like array ~ 0.5·N(0, 1) — decoder inputs that need no encoder run."""
    g = np.random.default_rng([seed, t_enc, dims])
    enc = np.tanh(g.standard_normal((t_enc, dims))).astype(np.float32)
    proj = (0.5 * g.standard_normal((t_enc, dims))).astype(np.float32)
    return enc, proj
