"""Device-side producer and consumer around the sample loop (C-ABI `wrnn_upsample_pack`,
`wrnn_postprocess`, csrc/condition.hip).

* `upsample_pack` turns the generate() mel input and the MelResNet output into the loop's
  time-major conditioning records in one HIP kernel: pad_tensor, the UpsampleNetwork's
  Stretch2d/Conv2d chain and crop, resnet_stretch, fold_with_overlap and the cat/transpose
  (models/fatchord_version.py:82-89, :183-205, :293-340).
* `melresnet` runs the UpsampleNetwork's MelResNet (:13-48) as one HIP kernel on weights packed by
  `melresnet_pack` (every BatchNorm folded into its conv; csrc/melresnet.hip).
* `postprocess` is generate()'s float64 tail on the device: decode_mu_law (utils/dsp.py:98-103),
  xfade_and_unfold (:342-405), trim and the 20·hop linear fade-out (:243-258).

No CPU fallback: the tensors must live on a GPU and the HIP library must be built."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat


class UpsampleSpec:
    """The mel-path shape of an UpsampleNetwork: scales, taps (host fp32) and pad."""

    def __init__(self, feat_dims: int, res_out_dims: int, pad: int, scales: Sequence[int],
                 taps: Sequence[np.ndarray]):
        if len(scales) != len(taps) or not 1 <= len(scales) <= 4:
            raise ValueError("1..4 upsample scales, one tap vector each")
        self.scales = tuple(int(s) for s in scales)
        self._taps = [np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1)) for t in taps]
        for s, t in zip(self.scales, self._taps):
            if t.size != 2 * s + 1:
                raise ValueError(f"scale {s} needs {2 * s + 1} taps, got {t.size}")
        self.cfg = nat.UpsampleCfg()
        self.cfg.feat_dims, self.cfg.res_out_dims, self.cfg.pad = feat_dims, res_out_dims, pad
        self.cfg.n_scales = len(self.scales)
        fp = ctypes.POINTER(ctypes.c_float)
        for i, (s, t) in enumerate(zip(self.scales, self._taps)):
            self.cfg.scales[i] = s
            self.cfg.taps[i] = t.ctypes.data_as(fp)
        self.hop = int(np.prod(self.scales))

    @classmethod
    def from_module(cls, upsample, feat_dims: int, pad: int) -> "UpsampleSpec":
        """From an UpsampleNetwork (reference layout: up_layers = [Stretch2d, Conv2d] × n)."""
        convs = [m for m in upsample.up_layers if isinstance(m, torch.nn.Conv2d)]
        scales = [(c.kernel_size[1] - 1) // 2 for c in convs]
        taps = [c.weight.detach().float().cpu().numpy() for c in convs]
        res_out = upsample.resnet.conv_out.out_channels
        return cls(feat_dims, res_out, pad, scales, taps)

    def with_res_out(self, res_out_dims: int) -> "UpsampleSpec":
        """The same cascade for an aux input of res_out_dims channels (zero-padded dims)."""
        return UpsampleSpec(self.cfg.feat_dims, res_out_dims, self.cfg.pad, self.scales, self._taps)

    def shape(self, B: int, T: int, target: int, overlap: int) -> Tuple[int, int]:
        steps, rows = ctypes.c_int(), ctypes.c_int()
        nat.check_cond(nat.lib().wrnn_cond_shape(ctypes.byref(self.cfg), B, T, target, overlap,
                                                 ctypes.byref(steps), ctypes.byref(rows)))
        return steps.value, rows.value


def frame_weights(spec: UpsampleSpec) -> Tuple[int, int, np.ndarray]:
    """(jlo, nJ, coef [hop][nJ]) with mel_up(f·hop + φ) = Σ_k coef[φ][k]·mel[f + k + jlo] — the
    cascade's frame weights wrnn_generate_frames forms the conditioning terms with (host call)."""
    hop, nJ, jlo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = nat.lib().wrnn_frame_weights(ctypes.byref(spec.cfg), ctypes.byref(hop), ctypes.byref(nJ), ctypes.byref(jlo),
                                      None, 0)
    if rc != 0:
        raise nat.WrnnError(rc, "the upsample cascade has no exact frame-rate form (pad frames < its reach)")
    coef = np.zeros((hop.value, nJ.value), np.float32)
    nat.check_cond(nat.lib().wrnn_frame_weights(ctypes.byref(spec.cfg), None, None, None,
                                                coef.ctypes.data_as(ctypes.c_void_p), coef.size))
    return jlo.value, nJ.value, coef


def melresnet_cfg(resnet) -> "nat.MelResNetCfg":
    """The wrnn_melresnet_cfg of a MelResNet module (reference layout, fatchord_version.py:30-48)."""
    cfg = nat.MelResNetCfg()
    cfg.in_dims = resnet.conv_in.in_channels
    cfg.compute_dims = resnet.conv_in.out_channels
    cfg.res_out_dims = resnet.conv_out.out_channels
    cfg.res_blocks = len(resnet.layers)
    cfg.pad = (resnet.conv_in.kernel_size[0] - 1) // 2
    return cfg


@torch.no_grad()
def melresnet_pack(resnet) -> torch.Tensor:
    """wrnn_melresnet's packed weights from a MelResNet module: each BatchNorm (running statistics,
    eval form) folded into the conv before it — W' = W·γ/√(var + ε), b' = β − μ·γ/√(var + ε), in
    float64 — matrices k-major.  Lives on the module's device."""
    def fold(w, bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return w.double() * s.view(-1, *([1] * (w.dim() - 1))), bn.bias.double() - bn.running_mean.double() * s

    parts = []
    w0, b0 = fold(resnet.conv_in.weight, resnet.batch_norm)            # [C][in][K]
    parts += [w0.permute(1, 2, 0).reshape(-1), b0]                     # [(c·K + tap)][C]
    for blk in resnet.layers:
        w1, b1 = fold(blk.conv1.weight[:, :, 0], blk.batch_norm1)
        w2, b2 = fold(blk.conv2.weight[:, :, 0], blk.batch_norm2)
        parts += [w1.t().reshape(-1), b1, w2.t().reshape(-1), b2]
    parts += [resnet.conv_out.weight[:, :, 0].double().t().reshape(-1), resnet.conv_out.bias.double()]
    return torch.cat([p.reshape(-1) for p in parts]).float().contiguous()


def melresnet(cfg, packed: torch.Tensor, mel_padded: torch.Tensor) -> torch.Tensor:
    """MelResNet(pad_tensor(mel)) in one HIP kernel: mel_padded [U][in][T + 2·pad] → aux [U][R][T].
    Raises WrnnError(WRNN_EUNSUPPORTED) for channel counts the kernel does not cover."""
    _need_gpu(mel_padded, packed)
    x = mel_padded.contiguous().float()
    U, cin, Tp = x.shape
    T = Tp - 2 * cfg.pad
    if cin != cfg.in_dims or T < 1 or packed.numel() != nat.lib().wrnn_melresnet_floats(ctypes.byref(cfg)):
        raise ValueError("mel / packed weights do not match the MelResNet config")
    aux = torch.empty(U, cfg.res_out_dims, T, device=x.device, dtype=torch.float32)
    rc = nat.lib().wrnn_melresnet(ctypes.byref(cfg), packed.data_ptr(), x.data_ptr(), U, T, aux.data_ptr(),
                                  _stream(x.device))
    if rc != 0:
        raise nat.WrnnError(rc, "wrnn_melresnet")
    return aux


def _stream(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t.device.type != "cuda":
            raise RuntimeError("the conditioning/post-processing kernels run on the MI355X: tensors must be on a "
                               "GPU (no CPU fallback)")


def upsample_pack(spec: UpsampleSpec, mel: torch.Tensor, aux: torch.Tensor, target: int = 0,
                  overlap: int = 0) -> torch.Tensor:
    """mel [B][feat][T], aux [B][res_out][T] (MelResNet of the padded mel) → cond
    [steps][rows][feat + res_out] fp32; target <= 0 means unbatched."""
    _need_gpu(mel, aux)
    mel = mel.contiguous().float()
    aux = aux.contiguous().float()
    B, feat, T = mel.shape
    if feat != spec.cfg.feat_dims or aux.shape != (B, spec.cfg.res_out_dims, T):
        raise ValueError(f"mel {tuple(mel.shape)} / aux {tuple(aux.shape)} do not match the upsample spec")
    steps, rows = spec.shape(B, T, target, overlap)
    cond = torch.empty(steps, rows, feat + spec.cfg.res_out_dims, device=mel.device, dtype=torch.float32)
    nat.check_cond(nat.lib().wrnn_upsample_pack(ctypes.byref(spec.cfg), mel.data_ptr(), aux.data_ptr(), B, T,
                                                target, overlap, cond.data_ptr(), _stream(mel.device)))
    return cond


def upsample_window_frames(spec: UpsampleSpec, t0: int, n: int, total_frames: Optional[int] = None):
    """(mel_lo, mel_hi, aux_lo, aux_hi): the mel frames [mel_lo, mel_hi) and aux frames [aux_lo, aux_hi)
    upsample_pack_window reads for steps [t0, t0 + n) (C-ABI wrnn_upsample_window_frames, host only);
    clipped to the utterance when total_frames is given."""
    v = [ctypes.c_int() for _ in range(4)]
    nat.check_cond(nat.lib().wrnn_upsample_window_frames(ctypes.byref(spec.cfg), -1 if total_frames is None else int(total_frames),
                                                         int(t0), int(n), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def upsample_pack_window(spec: UpsampleSpec, mel: torch.Tensor, m0: int, aux: torch.Tensor, a0: int, t0: int, n: int,
                         total_frames: Optional[int] = None) -> torch.Tensor:
    """upsample_pack's unbatched records for steps [t0, t0 + n) of an utterance still arriving (C-ABI
    wrnn_upsample_pack_window): mel [U][feat][nm] holds frames [m0, m0 + nm), aux [U][res_out][na]
    frames [a0, a0 + na); total_frames None while the end is unknown → cond [n][U][feat + res_out],
    bit for bit the records upsample_pack writes for those steps of the whole utterance.  A window
    that lacks a frame the steps read raises WrnnError(WRNN_EINVAL) before any launch."""
    _need_gpu(mel, aux)
    mel = mel.contiguous().float()
    aux = aux.contiguous().float()
    U, feat, nm = mel.shape
    if feat != spec.cfg.feat_dims or aux.dim() != 3 or tuple(aux.shape[:2]) != (U, spec.cfg.res_out_dims):
        raise ValueError(f"mel {tuple(mel.shape)} / aux {tuple(aux.shape)} do not match the upsample spec")
    cond = torch.empty(max(int(n), 0), U, feat + spec.cfg.res_out_dims, device=mel.device, dtype=torch.float32)
    nat.check_cond(nat.lib().wrnn_upsample_pack_window(
        ctypes.byref(spec.cfg), mel.data_ptr(), int(m0), nm, aux.data_ptr(), int(a0), aux.shape[2],
        -1 if total_frames is None else int(total_frames), U, int(t0), int(n), cond.data_ptr(), _stream(mel.device)))
    return cond


def postprocess(y: torch.Tensor, batched: bool, overlap: int, mu_law: bool, n_classes: int, wave_len: int,
                fade_len: int) -> torch.Tensor:
    """Loop output y [rows][steps] fp32 → float64 waveform [wave_len] (device tensor)."""
    _need_gpu(y)
    y = y.contiguous().float()
    rows, steps = y.shape
    if fade_len > wave_len:
        # the reference fails here in numpy (output[-fade:] *= fade_out, :255-258)
        raise ValueError(f"operands could not be broadcast together with shapes ({wave_len},) ({fade_len},) ")
    wave = torch.empty(wave_len, device=y.device, dtype=torch.float64)
    nat.check_cond(nat.lib().wrnn_postprocess(y.data_ptr(), rows, steps, int(batched), overlap, int(mu_law),
                                              n_classes, wave_len, fade_len, wave.data_ptr(), _stream(y.device)))
    return wave


POST_ENTRY = np.dtype([("y", np.uint64), ("dst", np.int64), ("steps", np.int32), ("wave_len", np.int32)])


def postprocess_list(ys, wave_lens, mu_law: bool, n_classes: int, fade_len: int) -> Tuple[torch.Tensor, list]:
    """The unbatched postprocess of every utterance of a list in one launch (C-ABI
    wrnn_postprocess_list): ys[i] [steps_i] fp32 loop output on the GPU, wave_lens[i] its waveform
    length → (one float64 device buffer, the utterances' offsets in it): utterance i's waveform is
    buffer[off_i : off_i + wave_lens[i]], what postprocess(ys[i][None], False, 0, mu_law, n_classes,
    wave_lens[i], fade_len) gives (bit for bit; with mu-law on to pow's accuracy)."""
    ys = [y.contiguous().float() for y in ys]
    _need_gpu(*ys)
    wave_lens = [int(w) for w in wave_lens]
    if not ys or len(ys) != len(wave_lens):
        raise ValueError("ys and wave_lens hold one entry per utterance, at least one")
    tab = np.zeros(len(ys), POST_ENTRY)
    off, total = [], 0
    for i, (y, w) in enumerate(zip(ys, wave_lens)):
        if y.dim() != 1 or w > y.shape[0]:
            raise ValueError(f"ys[{i}] must be a [steps] tensor of at least wave_len = {w} steps")
        if fade_len > w:
            raise ValueError(f"operands could not be broadcast together with shapes ({w},) ({fade_len},) ")
        tab[i] = (y.data_ptr(), total, y.shape[0], w)
        off.append(total)
        total += w
    dev = ys[0].device
    d_tab = torch.from_numpy(tab.view(np.uint8)).to(dev)
    wave = torch.empty(total, device=dev, dtype=torch.float64)
    nat.check_cond(nat.lib().wrnn_postprocess_list(d_tab.data_ptr(), len(ys), max(wave_lens), int(mu_law), n_classes,
                                                   fade_len, wave.data_ptr(), _stream(dev)))
    return wave, off


POST_FOLD_ENTRY = np.dtype([("y", np.uint64), ("dst", np.int64), ("rows", np.int32), ("wave_len", np.int32)])


def postprocess_list_folds(ys, overlap: int, wave_lens, mu_law: bool, n_classes: int,
                           fade_len: int) -> Tuple[torch.Tensor, list]:
    """The batched postprocess of every utterance of a folded list in one launch (C-ABI
    wrnn_postprocess_list_folds): ys[i] [folds_i][steps] fp32 fold outputs on the GPU (one `steps` =
    target + 2·overlap for all), wave_lens[i] its waveform length → (one float64 device buffer, the
    utterances' offsets in it): utterance i's waveform is buffer[off_i : off_i + wave_lens[i]], what
    postprocess(ys[i], True, overlap, mu_law, n_classes, wave_lens[i], fade_len) gives (bit for bit;
    with mu-law on to pow's accuracy)."""
    ys = [y.contiguous().float() for y in ys]
    _need_gpu(*ys)
    wave_lens = [int(w) for w in wave_lens]
    if not ys or len(ys) != len(wave_lens):
        raise ValueError("ys and wave_lens hold one entry per utterance, at least one")
    if any(y.dim() != 2 or y.shape[0] < 1 for y in ys) or len({y.shape[1] for y in ys}) != 1:
        raise ValueError("every ys[i] must be a [folds][steps] tensor, one steps for all")
    steps, overlap = int(ys[0].shape[1]), int(overlap)
    if overlap < 0 or steps - 2 * overlap < 1:
        raise ValueError(f"bad overlap {overlap} for the fold length {steps}")
    tab = np.zeros(len(ys), POST_FOLD_ENTRY)
    off, total = [], 0
    for i, (y, w) in enumerate(zip(ys, wave_lens)):
        if w > y.shape[0] * (steps - overlap) + overlap:
            raise ValueError(f"wave_lens[{i}] = {w} exceeds the unfolded length of ys[{i}]")
        if fade_len > w:
            raise ValueError(f"operands could not be broadcast together with shapes ({w},) ({fade_len},) ")
        tab[i] = (y.data_ptr(), total, y.shape[0], w)
        off.append(total)
        total += w
    dev = ys[0].device
    d_tab = torch.from_numpy(tab.view(np.uint8)).to(dev)
    wave = torch.empty(total, device=dev, dtype=torch.float64)
    nat.check_cond(nat.lib().wrnn_postprocess_list_folds(d_tab.data_ptr(), len(ys), steps, overlap, max(wave_lens),
                                                         int(mu_law), n_classes, fade_len, wave.data_ptr(), _stream(dev)))
    return wave, off
