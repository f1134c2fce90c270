"""Drop-in `WaveRNN` for models/fatchord_version.py whose generate() runs on MI355X.

Same constructor, submodule names, state_dict keys (so `load()` takes the reference's
`*.pyt` checkpoints), `get_step`, `load`, `save` and `generate(mels, save_path, batched,
target, overlap, mu_law)` contract as the reference (fatchord_version.py:92-435).  What
changes is where the sample loop runs: instead of the host-driven per-step loop
(:201-241), generate() packs the upsampled conditioning time-major and calls ONE persistent
HIP kernel through the C-ABI (`FatchordLoop`).  There is no CPU fallback: the model must
live on a GPU and the HIP library must be built, otherwise generate() raises.

Pre-processing: MelResNet as ONE fused HIP kernel (`wrnn_melresnet`, every BatchNorm folded on the
host; the torch module only for channel counts the kernel does not cover), then the loop entry
`wrnn_generate_frames`: pad + the stretch/box-conv chain + crop + aux stretch + fold are applied to
the conditioning TERMS at frame rate on the XCD-resident paths (csrc/frame_terms.hip), or through
the per-sample records of `condition.upsample_pack` on the others.
Post-processing (mu-law, cross-fade/unfold, trim, fade-out) is one float64 HIP kernel
(`condition.postprocess`) with the reference's operation order; only the finished waveform
crosses to the host.
"""
from __future__ import annotations

import os
import time
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from . import condition, dsp
from .loop import LOOP_KEYS, FatchordLoop, FatchordStream, content_key, noise_width


# --------------------------------------------------------------------- upsample network
class ResBlock(nn.Module):
    """1×1 conv → BN → ReLU → 1×1 conv → BN, plus identity (fatchord_version.py:13-28)."""

    def __init__(self, dims):
        super().__init__()
        self.conv1 = nn.Conv1d(dims, dims, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(dims, dims, kernel_size=1, bias=False)
        self.batch_norm1 = nn.BatchNorm1d(dims)
        self.batch_norm2 = nn.BatchNorm1d(dims)

    def forward(self, x):
        y = F.relu(self.batch_norm1(self.conv1(x)))
        return self.batch_norm2(self.conv2(y)) + x


class MelResNet(nn.Module):
    """Valid conv (k = 2·pad+1) → BN → ReLU → res blocks → 1×1 conv (fatchord_version.py:31-48)."""

    def __init__(self, res_blocks, in_dims, compute_dims, res_out_dims, pad):
        super().__init__()
        self.conv_in = nn.Conv1d(in_dims, compute_dims, kernel_size=2 * pad + 1, bias=False)
        self.batch_norm = nn.BatchNorm1d(compute_dims)
        self.layers = nn.ModuleList([ResBlock(compute_dims) for _ in range(res_blocks)])
        self.conv_out = nn.Conv1d(compute_dims, res_out_dims, kernel_size=1)

    def forward(self, x):
        x = F.relu(self.batch_norm(self.conv_in(x)))
        for layer in self.layers:
            x = layer(x)
        return self.conv_out(x)


class Stretch2d(nn.Module):
    """Nearest-neighbour repeat along (freq, time) (fatchord_version.py:51-61)."""

    def __init__(self, x_scale, y_scale):
        super().__init__()
        self.x_scale, self.y_scale = x_scale, y_scale

    def forward(self, x):
        return x.repeat_interleave(self.y_scale, dim=2).repeat_interleave(self.x_scale, dim=3)


class UpsampleNetwork(nn.Module):
    """MelResNet aux features stretched ×hop, and the mel upsampled by per-factor
    stretch + (1, 2s+1) box convs, cropped by pad·hop each side (fatchord_version.py:64-89).
    Returns (mels [B][L][feat], aux [B][L][res_out]) as contiguous time-major tensors."""

    def __init__(self, feat_dims, upsample_scales, compute_dims, res_blocks, res_out_dims, pad):
        super().__init__()
        total_scale = int(np.prod(upsample_scales))
        self.indent = pad * total_scale
        self.resnet = MelResNet(res_blocks, feat_dims, compute_dims, res_out_dims, pad)
        self.resnet_stretch = Stretch2d(total_scale, 1)
        self.up_layers = nn.ModuleList()
        for scale in upsample_scales:
            k = 2 * scale + 1
            conv = nn.Conv2d(1, 1, kernel_size=(1, k), padding=(0, scale), bias=False)
            conv.weight.data.fill_(1.0 / k)
            self.up_layers.append(Stretch2d(scale, 1))
            self.up_layers.append(conv)

    def forward(self, m):
        aux = self.resnet_stretch(self.resnet(m).unsqueeze(1)).squeeze(1)
        m = m.unsqueeze(1)
        for f in self.up_layers:
            m = f(m)
        m = m.squeeze(1)[:, :, self.indent:-self.indent]
        return m.transpose(1, 2), aux.transpose(1, 2)


# ------------------------------------------------------------------------------ model
class WaveRNN(nn.Module):
    def __init__(self, rnn_dims, fc_dims, bits, pad, upsample_factors, feat_dims, compute_dims,
                 res_out_dims, res_blocks, hop_length, sample_rate, mode='RAW'):
        super().__init__()
        self.mode = mode
        self.pad = pad
        if mode == 'RAW':
            self.n_classes = 2 ** bits
        elif mode == 'MOL':
            self.n_classes = 30
        else:
            raise RuntimeError("Unknown model mode value - ", mode)
        self.rnn_dims = rnn_dims
        self.fc_dims = fc_dims
        self.feat_dims = feat_dims
        self.aux_dims = res_out_dims // 4
        self.hop_length = hop_length
        self.sample_rate = sample_rate
        self.upsample = UpsampleNetwork(feat_dims, upsample_factors, compute_dims, res_blocks, res_out_dims, pad)
        self.I = nn.Linear(feat_dims + self.aux_dims + 1, rnn_dims)
        self.rnn1 = nn.GRU(rnn_dims, rnn_dims, batch_first=True)
        self.rnn2 = nn.GRU(rnn_dims + self.aux_dims, rnn_dims, batch_first=True)
        self.fc1 = nn.Linear(rnn_dims + self.aux_dims, fc_dims)
        self.fc2 = nn.Linear(fc_dims + self.aux_dims, fc_dims)
        self.fc3 = nn.Linear(fc_dims, self.n_classes)
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.num_params()
        self._loop: Optional[FatchordLoop] = None
        self._loop_key = None
        self.last_gen_seconds = 0.0

    # -------------------------------------------------------------- training forward
    def forward(self, x, mels):
        """Teacher-forced forward (fatchord_version.py:131-167); training is out of scope for
        the MI355X path, this keeps the module usable with the reference's train loop."""
        self.step += 1
        b = x.size(0)
        h1 = torch.zeros(1, b, self.rnn_dims, device=x.device)
        h2 = torch.zeros(1, b, self.rnn_dims, device=x.device)
        mels, aux = self.upsample(mels)
        a1, a2, a3, a4 = aux.split(self.aux_dims, dim=2)
        x = self.I(torch.cat([x.unsqueeze(-1), mels, a1], dim=2))
        res = x
        x, _ = self.rnn1(x, h1)
        x = x + res
        res = x
        x, _ = self.rnn2(torch.cat([x, a2], dim=2), h2)
        x = x + res
        x = F.relu(self.fc1(torch.cat([x, a3], dim=2)))
        x = F.relu(self.fc2(torch.cat([x, a4], dim=2)))
        return self.fc3(x)

    # -------------------------------------------------------------------- loop handle
    def _loop_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in LOOP_KEYS}

    def loop_handle(self, grid: int = 0) -> FatchordLoop:
        """The device handle, (re)packed whenever the loop weights changed: a load, a training step,
        or an in-place update through `.data` (the reference pruner's `W *= M`), which only the
        content fingerprint of loop.content_key sees."""
        device = next(self.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError("WaveRNN.generate runs on the MI355X HIP path: move the model to a GPU "
                               "(model.to('cuda')); there is no CPU fallback")
        params = self._loop_params()
        key = (device.index or 0, grid) + content_key(params.values(), self.__dict__.setdefault("_fp_loop", {}))
        if self._loop is None or self._loop_key is None or self._loop_key[:2] != key[:2]:
            if self._loop is not None:
                self._loop.close()
            self._loop = FatchordLoop(self.mode, self.rnn_dims, self.fc_dims, self.aux_dims, self.feat_dims,
                                      self.n_classes, device=device.index or 0, grid=grid)
            self._loop_key = None
        if self._loop_key != key:
            self._loop.set_weights(params)
            self._loop_key = key
        return self._loop

    # ---------------------------------------------------------------------- generate
    def _upsample_spec(self) -> condition.UpsampleSpec:
        """Host copy of the box-conv taps, refreshed when those parameters change."""
        convs = [m.weight for m in self.upsample.up_layers if isinstance(m, nn.Conv2d)]
        key = content_key(convs, self.__dict__.setdefault("_fp_up", {}))
        if getattr(self, "_up_key", None) != key:
            self._up_spec = condition.UpsampleSpec.from_module(self.upsample, self.feat_dims, self.pad)
            self._up_key = key
        return self._up_spec

    @torch.no_grad()
    def frames(self, mels):
        """generate()'s inputs at frame rate: (mel [U][feat][T], MelResNet(pad_tensor(mel))
        [U][res_out][T], wave_len) — fatchord_version.py:183-186 up to the upsampling, which the
        loop entry (wrnn_generate_frames) or condition.upsample_pack performs on the device."""
        device = next(self.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError("WaveRNN.generate runs on the MI355X HIP path: move the model to a GPU "
                               "(model.to('cuda')); there is no CPU fallback")
        was_training = self.training
        self.eval()
        try:
            mels = torch.as_tensor(mels, device=device).to(torch.float32)
            wave_len = (mels.size(-1) - 1) * self.hop_length
            padded = self.pad_tensor(mels.transpose(1, 2), pad=self.pad, side='both').transpose(1, 2)
            aux = self._melresnet(padded)
        finally:
            self.train(was_training)
        return mels.contiguous(), aux.contiguous().float(), wave_len

    def _melresnet(self, padded):
        """MelResNet(padded) through the fused HIP kernel (wrnn_melresnet: every BatchNorm folded,
        one launch); the torch module (MIOpen) only for channel counts the kernel does not cover."""
        res = self.upsample.resnet
        if os.environ.get("WRNN_TORCH_MELRESNET"):   # A/B: the torch module (MIOpen)
            return res(padded)
        try:
            return condition.melresnet(*self._melresnet_packed(), padded)
        except nat.WrnnError as e:
            if e.code != -6:   # WRNN_EUNSUPPORTED
                raise
            return res(padded)

    @torch.no_grad()
    def _melresnet_packed(self):
        """(wrnn_melresnet_cfg, packed weights) of the MelResNet, repacked when its parameters or
        BatchNorm statistics changed."""
        res = self.upsample.resnet
        key = content_key(list(res.parameters()) + list(res.buffers()), self.__dict__.setdefault("_fp_mr", {}))
        if getattr(self, "_mr_key", None) != key:
            self._mr_cfg = condition.melresnet_cfg(res)
            self._mr_packed = condition.melresnet_pack(res)
            self._mr_key = key
        return self._mr_cfg, self._mr_packed

    @torch.no_grad()
    def conditioning(self, mels, batched, target, overlap):
        """pad → upsample → (fold) → time-major [L][B][feat + 4·aux] (fatchord_version.py:183-190).
        MelResNet in eval form (BatchNorm running statistics, folded) is the `wrnn_melresnet` HIP
        kernel; everything after it the `wrnn_upsample_pack` HIP kernel."""
        mels, aux, wave_len = self.frames(mels)
        cond = condition.upsample_pack(self._upsample_spec(), mels, aux, target if batched else 0, overlap)
        return cond, wave_len

    def generate(self, mels, save_path: Union[str, Path, None], batched, target, overlap, mu_law, *,
                 noise=None, seed: Optional[int] = None, row_offset: int = 0, verbose: bool = True):
        """fatchord_version.py:169-264 with the loop on the GPU.

        Keyword-only extensions: `noise` [L][B][K] injects the sampler draws in reference order
        (parity testing); otherwise draws come from in-kernel Philox keyed by `seed` (default:
        drawn from torch's global RNG, so torch.manual_seed governs reproducibility) and by the
        global row id `row_offset + b` of each loop row b (a fold when batched) — the key that
        makes `generate_many` and the sharded entry points reproduce single calls."""
        self.eval()
        mu_law = mu_law if self.mode == 'RAW' else False
        start = time.time()
        with torch.no_grad():
            # the loop takes the frames: pad → upsample → fold happen inside wrnn_generate_frames
            # (the conditioning terms formed at frame rate, csrc/frame_terms.hip)
            mel_f, aux, wave_len = self.frames(mels)
            loop = self.loop_handle()
            nz = None
            if noise is not None:
                nz = torch.as_tensor(noise, dtype=torch.float32).to(mel_f.device).contiguous()
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            out, _ = loop.generate_frames(self._upsample_spec(), mel_f, aux, target if batched else 0, overlap,
                                          noise=nz, seed=seed, row_offset=row_offset)
            b_size, seq_len = out.shape
            # mu-law, xfade_and_unfold / row 0, trim, fade-out (:243-258) in float64 on the device
            output = condition.postprocess(out, batched, overlap, mu_law, self.n_classes, wave_len,
                                           20 * self.hop_length).cpu().numpy()
        self.last_gen_seconds = time.time() - start
        if verbose:
            self.gen_display(seq_len - 1, seq_len, b_size, start)
        dsp.save_wav(output, save_path, self.sample_rate)
        self.train()
        return output

    def rows_of(self, n_frames: int, batched: bool, target: int, overlap: int) -> int:
        """Loop rows generate() runs for a mel of n_frames frames: 1, or its fold count."""
        if not batched:
            return 1
        return self.fold_count(n_frames * self.hop_length, target, overlap)[0]

    def _mel_list(self, mels: Sequence) -> List[torch.Tensor]:
        device = next(self.parameters()).device
        ms = [torch.as_tensor(m, device=device).to(torch.float32) for m in mels]
        ms = [m if m.dim() == 3 else m[None] for m in ms]
        if not ms or any(m.dim() != 3 or m.shape[0] != 1 or m.shape[1] != self.feat_dims for m in ms):
            raise ValueError(f"mels must be a non-empty sequence of (1, {self.feat_dims}, T) arrays")
        return ms

    @torch.no_grad()
    def conditioning_many(self, mels: Sequence, batched: bool, target: int, overlap: int):
        """Conditioning of several utterances as the rows of ONE loop launch.

        Returns (cond [L][rows][C], per-utterance (first row, rows, steps, wave_len)).  Unbatched:
        row i is utterance i, its records padded with zeros after its own L_i steps (a row's
        samples depend only on earlier steps, so trimming to L_i is exact).  Batched: the folds
        of utterance i are rows [r_i, r_i + nf_i), all folds sharing the window target + 2·overlap.
        Mels of one length go through MelResNet and the upsample kernel together."""
        ms = self._mel_list(mels)
        device = ms[0].device
        if len({m.shape[2] for m in ms}) == 1:
            cond, wave_len = self.conditioning(torch.cat(ms, 0), batched, target, overlap)
            per = cond.shape[1] // len(ms)
            return cond, [(i * per, per, cond.shape[0], wave_len) for i in range(len(ms))]
        parts = [self.conditioning(m, batched, target, overlap) for m in ms]
        L = max(c.shape[0] for c, _ in parts)
        rows = sum(c.shape[1] for c, _ in parts)
        cond = torch.zeros(L, rows, parts[0][0].shape[2], dtype=torch.float32, device=device)
        spans, r = [], 0
        for c, wave_len in parts:
            cond[:c.shape[0], r:r + c.shape[1]] = c
            spans.append((r, c.shape[1], c.shape[0], wave_len))
            r += c.shape[1]
        return cond, spans

    def generate_many(self, mels: Sequence, save_paths: Optional[Sequence] = None, batched: bool = False,
                      target: int = 11000, overlap: int = 550, mu_law: bool = True, *, noise=None,
                      seed: Optional[int] = None, row_offset: int = 0, verbose: bool = False) -> List[np.ndarray]:
        """generate() for several utterances in ONE persistent-kernel launch (the utterances —
        or, batched, all their folds — are the launch's rows).  The reference vocodes a list one
        generate() at a time (gen_wavernn.py:11-35, gen_tacotron.py:142-168); this returns the
        same list of float64 waveforms.  Utterance i's rows are keyed row_offset + (rows of the
        utterances before it) + j, so under Philox `generate_many(mels, seed=s)[i]` equals
        `generate(mels[i], seed=s, row_offset=<that first row>)` bit for bit.  `noise`, when given,
        is [L_max][rows][K] in that row order.

        Unequal lengths with batched=True: prefer generate_list(mels, wide=True, batched=True, target=,
        overlap=) — the same rows and Philox keys, but the conditioning terms stay at frame rate and the
        folds fill the 128 many-row slots, where this entry materialises sample-rate conditioning for
        every fold (conditioning_many)."""
        self.eval()
        mu_law = mu_law if self.mode == 'RAW' else False
        start = time.time()
        with torch.no_grad():
            ms = self._mel_list(mels)
            loop = self.loop_handle()
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            dev = next(self.parameters()).device
            nz = None if noise is None else torch.as_tensor(noise, dtype=torch.float32).to(dev).contiguous()
            if len({m.shape[2] for m in ms}) == 1:
                # one length: the frames of all utterances go to the loop entry together
                mel_f, aux, wave_len = self.frames(torch.cat(ms, 0))
                out, _ = loop.generate_frames(self._upsample_spec(), mel_f, aux, target if batched else 0, overlap,
                                              noise=nz, seed=seed, row_offset=row_offset)
                per = out.shape[0] // len(ms)
                spans = [(i * per, per, out.shape[1], wave_len) for i in range(len(ms))]
            else:
                cond, spans = self.conditioning_many(ms, batched, target, overlap)
                out, _ = loop.generate(cond, noise=nz, seed=seed, row_offset=row_offset)
            waves = [condition.postprocess(out[r0:r0 + n, :steps], batched, overlap, mu_law, self.n_classes,
                                           wave_len, 20 * self.hop_length)
                     for r0, n, steps, wave_len in spans]
            outputs = [w.cpu().numpy() for w in waves]
        self.last_gen_seconds = time.time() - start
        if verbose:
            self.gen_display(out.shape[1] - 1, out.shape[1], out.shape[0], start)
        for i, output in enumerate(outputs):
            if save_paths is not None and save_paths[i] is not None:
                dsp.save_wav(output, save_paths[i], self.sample_rate)
        self.train()
        return outputs

    def generate_list(self, mels: Sequence, save_paths: Optional[Sequence] = None, *, noise=None,
                      seed: Optional[int] = None, row_offset: int = 0, lanes: Optional[int] = None,
                      verbose: bool = False, wide: bool = False, slots: Optional[int] = None,
                      mu_law: bool = True, batched: bool = False, target: int = 11000,
                      overlap: int = 550) -> List[np.ndarray]:
        """generate(mels[i], None, False, …) for a list of utterances of ANY lengths (each (1, feat,
        T_i), T_i ≥ 21; unbatched: no folds) in one call: the eight XCDs are eight lanes, each runs
        a queue of utterances back to back inside the persistent launch (longest first, each to the
        least loaded lane), so nothing waits for the longest member and no row runs past its own
        end (C-ABI wrnn_generate_list).  → the list of float64 waveforms.

        `generate_list(mels, seed=s, row_offset=r)[i]` equals `generate(mels[i], None, False, …,
        seed=s, row_offset=r + i)` bit for bit, for every `lanes` (1..8, default min(8, len(mels));
        for tests and experiments) and every WRNN_TERMS_MB: utterance i is Philox row row_offset + i
        with its step counter at 0, and its conditioning (MelResNet, frame records, W·frames GEMM)
        runs per utterance with the shapes of its single call.  `noise`: a sequence of per-utterance
        [hop·T_i][11] draws, indexed by the utterance's own step.  Modes and dims without a list
        kernel (anything but MoL rnn / fc 512 dense or rnn 896 block-sparse: the one-row XCD kernels) raise
        NotImplementedError; bad arguments raise ValueError before anything is queued.

        Wide lists.  `wide=True` runs the list on the many-row kernel (C-ABI wrnn_generate_list_wide,
        loop path 7): up to 128 slots, 16 per XCD (`slots` 1..128, default min(128, len(mels));
        `lanes` must be None), each a queue of utterances that refills when one ends — the form for
        a batch of hundreds of sentences, and the only list form of a RAW model (9 bits, rnn / fc
        512; `noise[i]` is then [hop·T_i][512] Exp(1) draws, and `mu_law`, default True as
        generate_many, expands the samples; it is ignored for MoL).  The post of all utterances is
        one launch and one copy to the host (wrnn_postprocess_list).  What a wide list promises:
        utterance i's waveform does not depend on the other utterances, their order, `slots` or
        WRNN_TERMS_MB — it is bit-identical to the wide list of mels[i] alone with row_offset + i;
        MoL lies within 2e-5 of the oracle on the same draws and, with `seed`, within MoL tolerance
        of generate(mels[i], seed=s, row_offset=r + i), but is NOT bit-identical to the narrow list
        or to generate() (another kernel); RAW class labels are the oracle's and generate()'s on the
        same draws bit for bit, so with mu_law=False every sample before the fade is exact.

        Folded lists.  `batched=True` (with `wide=True`; the narrow lanes have no folded form) is the
        reference's default way to vocode, for a list: every utterance is cut into folds of
        `target + 2·overlap` steps and the folds of ALL utterances fill the slots (C-ABI
        wrnn_generate_list_folds: fold g of the utterance-major numbering runs in round g // slots as
        launch row g % slots), then one cross-fade launch (wrnn_postprocess_list_folds) and one copy
        to the host → what generate(mels[i], None, True, target, overlap, mu_law) returns, (T_i − 1)·hop
        float64 samples each.  `noise[i]` is [target + 2·overlap][folds_i][K], generate()'s layout for
        that utterance alone; under Philox fold j of utterance i is row row_offset + (folds of the
        utterances before it) + j, generate_many's key.  A long utterance spreads over many slots
        instead of holding one, so this is the form for lists with long or very unequal members; for
        hundreds of SHORT utterances (a fold or two each) the unbatched wide list does the same work
        without the overlaps' extra steps.  Promises: independence of company as above (bit-identical
        to the folded list of mels[i] alone with row_offset + its first row); RAW fold outputs equal
        generate()'s bit for bit on the same draws; MoL within √2·2e-5 of the oracle on the same draws
        (two cross-faded fold samples) and, with `seed`, within √2·1e-5 of generate(..., True, target,
        overlap, ..., seed=s, row_offset=r + first row)."""
        if batched:
            if not wide:
                raise ValueError("batched=True needs wide=True: folds run on the many-row slots, the narrow lanes have "
                                 "no folded form")
            return self._generate_list_folds(mels, save_paths, noise, seed, row_offset, lanes, slots, mu_law, target,
                                             overlap, verbose)
        if wide:
            return self._generate_list_wide(mels, save_paths, noise, seed, row_offset, lanes, slots, mu_law, verbose)
        self.eval()
        start = time.time()
        with torch.no_grad():
            ms = self._mel_list(mels)
            if noise is not None and len(noise) != len(ms):
                raise ValueError("noise holds one [hop·T][11] array per utterance")
            if lanes is not None and not 1 <= int(lanes) <= 8:
                raise ValueError("lanes is 1..8 (one per XCD)")
            if any(m.shape[2] < 21 for m in ms):   # before the MelResNet launches: nothing is queued
                raise ValueError("every utterance needs at least 21 frames (the fade-out)")
            if self.mode != 'MOL':
                raise NotImplementedError("generate_list runs the one-row XCD MoL kernels: this model is not MoL")
            loop = self.loop_handle()
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            dev = ms[0].device
            nz = None if noise is None else [torch.as_tensor(z, dtype=torch.float32).to(dev).contiguous() for z in noise]
            fr = [self.frames(m) for m in ms]   # one MelResNet launch per utterance, at its own shape
            outs = loop.generate_list(self._upsample_spec(), [f[0] for f in fr], [f[1] for f in fr], lanes=lanes,
                                      noise=nz, seed=seed, row_offset=row_offset)
            outputs = [condition.postprocess(o[None], False, 0, False, self.n_classes, f[2],
                                             20 * self.hop_length).cpu().numpy() for o, f in zip(outs, fr)]
        self.last_gen_seconds = time.time() - start
        if verbose:
            longest = max(o.shape[0] for o in outs)
            self.gen_display(longest - 1, longest, len(outs), start)
        for i, output in enumerate(outputs):
            if save_paths is not None and save_paths[i] is not None:
                dsp.save_wav(output, save_paths[i], self.sample_rate)
        self.train()
        return outputs

    def _generate_list_wide(self, mels, save_paths, noise, seed, row_offset, lanes, slots, mu_law, verbose):
        """generate_list(wide=True): every refusal that needs no device work comes before any launch."""
        if lanes is not None:
            raise ValueError("lanes belongs to the narrow list: a wide list takes slots (1..128)")
        if slots is not None and not 1 <= int(slots) <= 128:
            raise ValueError("slots is 1..128 (16 per XCD)")
        self.eval()
        mu_law = mu_law if self.mode == 'RAW' else False
        start = time.time()
        with torch.no_grad():
            ms = self._mel_list(mels)
            if noise is not None and len(noise) != len(ms):
                raise ValueError(f"noise holds one [hop·T][{self.noise_width()}] array per utterance")
            if any(m.shape[2] < 21 for m in ms):   # before the MelResNet launches: nothing is queued
                raise ValueError("every utterance needs at least 21 frames (the fade-out)")
            loop = self.loop_handle()
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            dev = ms[0].device
            nz = None if noise is None else [torch.as_tensor(z, dtype=torch.float32).to(dev).contiguous() for z in noise]
            if nz is not None:
                for i, (z, m) in enumerate(zip(nz, ms)):
                    if tuple(z.shape) != (m.shape[2] * self.hop_length, self.noise_width()):
                        raise ValueError(f"noise[{i}] must be [{m.shape[2] * self.hop_length}][{self.noise_width()}]")
            fr = [self.frames(m) for m in ms]   # one MelResNet launch per utterance, at its own shape
            outs = loop.generate_list_wide(self._upsample_spec(), [f[0] for f in fr], [f[1] for f in fr], slots=slots,
                                           noise=nz, seed=seed, row_offset=row_offset)
            wave, off = condition.postprocess_list(outs, [f[2] for f in fr], mu_law, self.n_classes, 20 * self.hop_length)
            host = wave.cpu().numpy()
            outputs = [host[o:o + f[2]].copy() for o, f in zip(off, fr)]
        self.last_gen_seconds = time.time() - start
        if verbose:
            longest = max(o.shape[0] for o in outs)
            self.gen_display(longest - 1, longest, len(outs), start)
        for i, output in enumerate(outputs):
            if save_paths is not None and save_paths[i] is not None:
                dsp.save_wav(output, save_paths[i], self.sample_rate)
        self.train()
        return outputs

    def _generate_list_folds(self, mels, save_paths, noise, seed, row_offset, lanes, slots, mu_law, target, overlap,
                             verbose):
        """generate_list(wide=True, batched=True): every refusal that needs no device work comes before any launch."""
        if lanes is not None:
            raise ValueError("lanes belongs to the narrow list: a folded list takes slots (1..128)")
        if slots is not None and not 1 <= int(slots) <= 128:
            raise ValueError("slots is 1..128 (16 per XCD)")
        target, overlap = int(target), int(overlap)
        if target < 1 or overlap < 0:
            raise ValueError(f"target is at least 1 and overlap at least 0, not ({target}, {overlap})")
        self.eval()
        mu_law = mu_law if self.mode == 'RAW' else False
        start = time.time()
        with torch.no_grad():
            ms = self._mel_list(mels)
            if noise is not None and len(noise) != len(ms):
                raise ValueError(f"noise holds one [target + 2·overlap][folds][{self.noise_width()}] array per utterance")
            if any(m.shape[2] < 21 for m in ms):   # before the MelResNet launches: nothing is queued
                raise ValueError("every utterance needs at least 21 frames (the fade-out)")
            if any(m.shape[2] * self.hop_length < overlap for m in ms):
                raise ValueError("every utterance needs at least `overlap` samples")
            Lf = target + 2 * overlap
            folds = [self.rows_of(m.shape[2], True, target, overlap) for m in ms]
            loop = self.loop_handle()
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            dev = ms[0].device
            nz = None if noise is None else [torch.as_tensor(z, dtype=torch.float32).to(dev).contiguous() for z in noise]
            if nz is not None:
                for i, z in enumerate(nz):
                    if tuple(z.shape) != (Lf, folds[i], self.noise_width()):
                        raise ValueError(f"noise[{i}] must be [{Lf}][{folds[i]}][{self.noise_width()}]")
            fr = [self.frames(m) for m in ms]   # one MelResNet launch per utterance, at its own shape
            outs = loop.generate_list_folds(self._upsample_spec(), [f[0] for f in fr], [f[1] for f in fr], target,
                                            overlap, slots=slots, noise=nz, seed=seed, row_offset=row_offset)
            wave, off = condition.postprocess_list_folds(outs, overlap, [f[2] for f in fr], mu_law, self.n_classes,
                                                         20 * self.hop_length)
            host = wave.cpu().numpy()
            outputs = [host[o:o + f[2]].copy() for o, f in zip(off, fr)]
        self.last_gen_seconds = time.time() - start
        if verbose:
            self.gen_display(Lf - 1, Lf, sum(folds), start)
        for i, output in enumerate(outputs):
            if save_paths is not None and save_paths[i] is not None:
                dsp.save_wav(output, save_paths[i], self.sample_rate)
        self.train()
        return outputs

    # --------------------------------------------------------------------- wav input
    def _front(self, hp=None):
        """The mel front end for this model (wavernn_amd.melspec.MelSpec): hop_length, sample_rate and
        num_mels are the model's; n_fft, win_length, fmin and min_level_db come from `hp` (an HParams
        or a mapping) or the reference's defaults."""
        from .melspec import MelSpec
        device = next(self.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError("WaveRNN.melspectrogram runs on the MI355X HIP path: move the model to a GPU "
                               "(model.to('cuda')); dsp.melspectrogram(device='cpu') is the host path")
        p = dsp.melspec_params(hp, hop_length=self.hop_length, sample_rate=self.sample_rate, num_mels=self.feat_dims)
        return MelSpec.get(p, device)

    @torch.no_grad()
    def melspectrogram(self, wavs, hp=None) -> List[torch.Tensor]:
        """utils/dsp.py:75-78 on the GPU (C-ABI wrnn_melspec, csrc/melspec.hip): `wavs` is a 1-D
        signal, a [U][n] tensor, or a list of 1-D tensors / arrays of unequal length (float, the
        model's sample rate) → a list of device mels (1, num_mels, 1 + n_u // hop) from ONE launch,
        ready for generate, generate_many and generate_list."""
        if isinstance(wavs, (torch.Tensor, np.ndarray)):
            wavs = [wavs] if wavs.ndim == 1 else list(wavs)
        return [m[None] for m in self._front(hp).run(list(wavs))]

    def generate_from_wav(self, wav, save_path: Union[str, Path, None], batched, target, overlap, mu_law, *,
                          hp=None, **kw):
        """Copy synthesis (gen_wavernn.py --file x.wav): melspectrogram(wav), then generate() as it is;
        keywords go to generate()."""
        return self.generate(self.melspectrogram(wav, hp)[0], save_path, batched, target, overlap, mu_law, **kw)

    def generate_list_from_wavs(self, wavs: Sequence, save_paths: Optional[Sequence] = None, *, hp=None, **kw):
        """melspectrogram(wavs) (one launch for the whole list), then generate_list() as it is."""
        return self.generate_list(self.melspectrogram(wavs, hp), save_paths, **kw)

    # --------------------------------------------------------------------- streaming
    def stream(self, n_streams: int = 1, total_frames: Optional[int] = None, *, noise=None,
               seed: Optional[int] = None, row_offset: int = 0, wide: bool = False,
               mu_law: bool = True, rows: bool = False, total_samples: Optional[int] = None,
               hp=None) -> "WaveRNNStream":
        """A streaming session: push mel frames as the acoustic model produces them, get the audio
        that has become final — unbatched MoL generate() in pieces, the recurrent state kept on the
        GPU between pushes (C-ABI wrnn_stream_*).  `n_streams` utterances (1..8) advance in lock
        step.  `total_frames`, when known, lets the session emit up to the fade-out instead of
        holding back 21 frames.  `noise` [steps][n_streams][11] injects the sampler draws by
        absolute step; otherwise Philox keyed by `seed` and row_offset + u, the draws generate()
        takes.  Modes and dims the session kernels do not cover raise NotImplementedError.

        A session binds the weights it was opened with.  Opening it looks at the model's weights
        (as generate() does); a push does not.  If the loop weights are loaded again while it is
        open (by a generate() or a new stream() after load_state_dict, a training step or a `.data`
        update) its next push raises and the session is dead: close it and open a new one.  A
        change that only pushes would see (a `.data` update with no generate() or stream() after
        it) is not detected: the session goes on with the weights it was opened with.

        `wide=True` runs the session on the many-row kernel (16 rows per XCD; loop path 7):
        `n_streams` may be 1..128, and push_streams takes up to 128 rows of wide sessions per call.
        The emission rule, look-ahead, push() / finish() / close(), weight binding and refusals are
        the same.  A wide member's audio does not depend on its company: every wide launch is the
        kernel's four-quad form, in which batch rows are independent MFMA columns, so a member is
        bit-identical alone, in any group, in any slot; it lies within the project's bound of the
        oracle, and with `seed` equals generate(seed=, row_offset=) within MOL tolerance.  It is
        NOT bit-identical to the same session opened narrow (another kernel, sums associated
        differently), and the members' conditioning is not batched across sessions: callers who can
        lock-step should open one U-wide session.

        A RAW model (9 bits, rnn / fc 512) streams through wide sessions only (`wide=True`; narrow
        RAW raises NotImplementedError, as do other bit depths and dims): the many-row kernel's
        softmax head, whose class labels are those of generate() on the same draws bit for bit.
        `noise` is then [steps][n_streams][512] Exp(1) draws by absolute step, the layout
        generate(noise=) takes; `mu_law` (default True, as generate_many) expands the emitted samples
        as generate(mu_law=) does and is ignored for MoL models.

        `rows=True` runs the session on the multi-row kernel (loop path 2; 9 when the weights are
        streamed from HBM), the kernel generate() falls to for every model the XCD-resident ones do
        not cover: MoL or RAW, any rnn / fc dims that are multiples of 4, any bit depth.  It is
        opt-in: without it stream() accepts and refuses what it always did.  `n_streams` goes up to
        one row block of the kernel for this model (ValueError beyond it, with the limit); `noise`
        is [steps][n_streams][11] for MoL and [steps][n_streams][n_classes] Exp(1) draws for RAW;
        `mu_law` as for wide RAW sessions.  With the same draws the session's samples are those of
        generate() on the multi-row kernel (WRNN_PATH=rows).  A rows session advances alone
        (push_streams refuses it), and `rows=True, wide=True` is a ValueError.

        Audio in: a session of any kind also takes PCM — push_audio(pcm) / finish_audio() run the mel
        front end (melspectrogram's kernel, `hp` its geometry) on the frames that became final and
        hand them to push().  `total_samples=` in place of `total_frames=` states the length in
        samples (1 + total_samples // hop frames)."""
        if total_samples is not None:
            if total_frames is not None:
                raise ValueError("give total_frames or total_samples, not both")
            total_frames = 1 + int(total_samples) // self.hop_length
        return WaveRNNStream(self, n_streams, total_frames, noise, seed, row_offset, wide, mu_law, rows,
                             total_samples=total_samples, hp=hp)

    def push_streams(self, pushes) -> list:
        """Advance several sessions of this model in one call: `pushes` is a sequence of
        (WaveRNNStream, mel_chunk or None, final) → one float64 numpy array [U_i][m_i] per member,
        what stream.push(mel_chunk) (or finish(), with final) returns for each, bit for bit.
        Inside a session the utterances advance in lock step: the same frames in the same push, one
        total_frames, one end.  A group lifts that between sessions — requests that arrived at
        different times, with different lengths, whose frames come in at different moments: each
        member gets its own frames and its own end, and all of them share one persistent launch per
        push, every row on its own XCD (C-ABI wrnn_stream_push_group), instead of one launch per
        session that leaves seven XCDs idle.  The members' rows together are at most 8; a finished
        session is no longer listed.  Refusals raise ValueError and leave every member unchanged.
        A group whose members were all opened with wide=True may hold up to 128 rows (16 per XCD,
        one persistent launch per round of equal step counts); wide and narrow members do not mix.
        A member may also be (WaveRNNStream, pcm): an audio push, what stream.push_audio(pcm) returns;
        the new mel frames of all such members come from one front-end launch (C-ABI
        wrnn_melspec_windows) before the group push.  A member ends its audio with finish_audio()."""
        members, audio = [], []
        for item in pushes:
            if not isinstance(item, (tuple, list)) or len(item) not in (2, 3) or not isinstance(item[0], WaveRNNStream) \
                    or (len(item) == 2 and item[1] is None):   # an audio push brings samples
                raise ValueError("pushes holds (WaveRNNStream, mel_chunk or None, final) or (WaveRNNStream, pcm) tuples")
            if item[0]._model is not self:
                raise ValueError("a member session belongs to another model")
            if len(item) == 2:
                audio.append((len(members), item[0], item[0]._audio_feed().stage(item[1])))
                members.append(None)
            else:
                s, mel, final = item
                members.append((s._session, s._mel_tensor(mel), bool(final)))
        if not members:
            raise ValueError("push_streams needs at least one member")
        if audio:
            # ONE front-end launch for the new frames of all audio members of one geometry (sessions
            # opened with another hp= have their own tables: a launch each), then the group push as it is
            fronts = {}
            for i, s, (_, js, _) in audio:
                fronts.setdefault(s._audio_feed().front, []).append((i, s, js))
            for front, group in fronts.items():
                jobs = [j for _, _, js in group for j in js]
                mels = front.windows(jobs) if jobs else []
                at = 0
                for i, s, js in group:
                    members[i] = (s._session, torch.stack(mels[at:at + len(js)]) if js else None, False)
                    at += len(js)
        # the members' own loop, as it is: a push does not look at the weights (WaveRNN.stream)
        waves = [w.cpu().numpy() for w in members[0][0].loop.push_streams(members)]
        for _, s, (state, _, _) in audio:   # a refusal raised above: no audio member has changed
            s._audio_feed().commit(state)
        return waves

    def generate_stream(self, mels, chunk_frames: int = 8, *, noise=None, seed: Optional[int] = None,
                        row_offset: int = 0, wide: bool = False, mu_law: bool = True, rows: bool = False):
        """generate(mels, None, False, ...) as a generator of float64 chunks, for a mel known up
        front: mels [1][feat][T] (or [U][feat][T], chunks [U][m]) pushed `chunk_frames` at a time
        (or by the frame counts of a sequence).  The chunks concatenate to generate()'s output.
        `wide` is passed to stream(): up to 128 utterances in lock step on the many-row kernel.
        `mu_law` likewise: a RAW model streams wide only, its samples mu-law expanded by default.
        `rows` is passed to stream() too: the multi-row kernel's sessions, for any model."""
        device = next(self.parameters()).device
        mels = torch.as_tensor(mels, device=device).to(torch.float32)
        if mels.dim() != 3:
            raise ValueError("mels must be [U][feat][T]")
        U, _, T = mels.shape
        counts = [chunk_frames] * (-(-T // chunk_frames)) if isinstance(chunk_frames, int) else list(chunk_frames)
        if any(c < 1 for c in counts):
            raise ValueError("chunk_frames must be positive")
        with self.stream(U, T, noise=noise, seed=seed, row_offset=row_offset, wide=wide, mu_law=mu_law, rows=rows) as s:
            f = 0
            for c in counts:
                if f >= T:
                    break
                out = s.push(mels[:, :, f:f + c])
                f = min(T, f + c)
                if out.shape[1]:
                    yield out[0] if U == 1 else out
            out = s.finish()
            if out.shape[1]:
                yield out[0] if U == 1 else out

    def gen_display(self, i, seq_len, b_size, start):
        gen_rate = (i + 1) / max(time.time() - start, 1e-9) * b_size / 1000
        print(f'| {i + 1}/{seq_len} steps × {b_size} rows | Gen Rate: {gen_rate:.1f}kHz |')

    def get_gru_cell(self, gru):
        """nn.GRUCell view of a single-layer GRU's weights (fatchord_version.py:273-279)."""
        cell = nn.GRUCell(gru.input_size, gru.hidden_size).to(gru.weight_hh_l0.device)
        cell.weight_hh.data = gru.weight_hh_l0.data
        cell.weight_ih.data = gru.weight_ih_l0.data
        cell.bias_hh.data = gru.bias_hh_l0.data
        cell.bias_ih.data = gru.bias_ih_l0.data
        return cell

    @staticmethod
    def pad_tensor(x, pad, side='both'):
        """Zero-pad the time axis of [b][t][c] (fatchord_version.py:281-291)."""
        b, t, c = x.size()
        total = t + 2 * pad if side == 'both' else t + pad
        padded = torch.zeros(b, total, c, device=x.device, dtype=x.dtype)
        if side in ('before', 'both'):
            padded[:, pad:pad + t, :] = x
        elif side == 'after':
            padded[:, :t, :] = x
        return padded

    @staticmethod
    def fold_count(total_len, target, overlap):
        n = (total_len - overlap) // (target + overlap)
        remaining = total_len - (n * (overlap + target) + overlap)
        return n + (1 if remaining != 0 else 0), remaining

    def fold_with_overlap(self, x, target, overlap):
        """[1][L][F] → [num_folds][target + 2·overlap][F]; consecutive folds share `overlap`
        steps, the tail is zero-padded (fatchord_version.py:293-340)."""
        _, total_len, features = x.size()
        num_folds, remaining = self.fold_count(total_len, target, overlap)
        if remaining != 0:
            x = self.pad_tensor(x, target + 2 * overlap - remaining, side='after')
        win = target + 2 * overlap
        folds = x[0].unfold(0, win, target + overlap)          # [n][F][win] views
        return folds[:num_folds].transpose(1, 2).contiguous()

    @staticmethod
    def xfade_and_unfold(y, target, overlap):
        """Equal-power cross-fade of folds and overlap-add back to 1-D float64
        (fatchord_version.py:342-405; `fade_out` keeps the reference's leading ones).  Host
        numpy for callers of the reference API; generate() runs the device kernel
        (`condition.postprocess`)."""
        num_folds, length = y.shape
        target = length - 2 * overlap
        total_len = num_folds * (target + overlap) + overlap
        silence_len = overlap // 2
        fade_len = overlap - silence_len
        t = np.linspace(-1, 1, fade_len, dtype=np.float64)
        fade_in = np.concatenate([np.zeros(silence_len, dtype=np.float64), np.sqrt(0.5 * (1 + t))])
        fade_out = np.concatenate([np.ones(silence_len, dtype=np.float64), np.sqrt(0.5 * (1 - t))])
        y = np.array(y, dtype=np.float64, copy=True)
        y[:, :overlap] *= fade_in
        y[:, -overlap:] *= fade_out
        unfolded = np.zeros(total_len, dtype=np.float64)
        for i in range(num_folds):
            s = i * (target + overlap)
            unfolded[s:s + length] += y[i]
        return unfolded

    # ------------------------------------------------------------------ bookkeeping
    def get_step(self):
        return self.step.data.item()

    def log(self, path, msg):
        with open(path, 'a') as f:
            print(msg, file=f)

    def load(self, path: Union[str, Path]):
        """Reference checkpoint (a state_dict saved with torch.save) → this model.  Loaded
        with weights_only=True: a checkpoint never executes code."""
        device = next(self.parameters()).device
        self.load_state_dict(torch.load(path, map_location=device, weights_only=True), strict=False)

    def save(self, path: Union[str, Path]):
        torch.save(self.state_dict(), path)

    def num_params(self, print_out=True):
        n = sum(p.numel() for p in self.parameters() if p.requires_grad) / 1_000_000
        if print_out:
            print('Trainable Parameters: %.3fM' % n)
        return n

    def noise_width(self) -> int:
        return noise_width(self.mode, self.n_classes)


class WaveRNNStream:
    """The session WaveRNN.stream() returns: push(mel_chunk) → float64 [U][m] (m may be 0),
    finish() → the tail; a context manager; `lookahead_frames` is how many frames behind the
    newest one the loop runs (voc_pad + 1).  Its `n_streams` utterances advance in lock step;
    WaveRNN.push_streams advances several sessions in one call, each at its own pace."""

    def __init__(self, model: WaveRNN, n_streams: int, total_frames: Optional[int], noise, seed: Optional[int],
                 row_offset: int, wide: bool = False, mu_law: bool = True, rows: bool = False, *,
                 total_samples: Optional[int] = None, hp=None):
        if rows and wide:
            raise ValueError("rows=True and wide=True name two kernels: a session runs on one")
        # audio in (push_audio / finish_audio): the signal's length when known, the front end's geometry
        self._total_samples, self._hp, self._feed = total_samples, hp, None
        if wide and not 1 <= int(n_streams) <= 128:
            raise ValueError(f"a wide session has 1..128 utterances, not {n_streams!r}")
        device = next(model.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError("WaveRNN.stream runs on the MI355X HIP path: move the model to a GPU "
                               "(model.to('cuda')); there is no CPU fallback")
        self.device = device
        self._model = model
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float32).to(device).contiguous()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        cfg, packed = model._melresnet_packed()
        self._session = FatchordStream(model.loop_handle(), model._upsample_spec(), cfg, packed, n_streams,
                                       total_frames, nz, seed, row_offset, wide=wide, mu_law=bool(mu_law),
                                       rows=bool(rows))
        self.wide = bool(wide)
        self.rows = bool(rows)
        self.n_streams = n_streams
        self.lookahead_frames = self._session.lookahead_frames

    def _mel_tensor(self, mel_chunk):
        if mel_chunk is None:
            return None
        mel = torch.as_tensor(mel_chunk, device=self.device).to(torch.float32)
        if mel.dim() == 2:
            mel = mel[None]
        return mel.contiguous()

    def set_mu_law(self, on: bool) -> None:
        """RAW sessions, before the first push: switch the mu-law expansion of the emitted samples."""
        self._session.set_mu_law(on)

    def push(self, mel_chunk) -> np.ndarray:
        return self._session.push(self._mel_tensor(mel_chunk)).cpu().numpy()

    def finish(self) -> np.ndarray:
        return self._session.push(None, final=True).cpu().numpy()

    # audio in: the mel front end in front of push()
    def _audio_feed(self):
        if self._feed is None:
            from .melspec import AudioFeed
            self._feed = AudioFeed(self._model._front(self._hp), self.n_streams, self._total_samples)
        return self._feed

    def push_audio(self, pcm) -> np.ndarray:
        """PCM in ([n], or [U][n] for U streams in lock step; float, the model's sample rate): the mel
        frames that became final with these samples (wrnn_melspec_plan) are computed on the GPU from
        the session's PCM tail (wrnn_melspec_windows) and pushed → what push() returns for them,
        float64 [U][m] (m = 0 while no frame is final).  The frames are bit-identical to
        melspectrogram() of the whole signal, however the samples were cut into pushes."""
        feed = self._audio_feed()
        state, jobs, nt = feed.stage(pcm)
        out = self.push(torch.stack(feed.front.windows(jobs))) if nt else np.zeros((self.n_streams, 0))
        feed.commit(state)
        return out

    def finish_audio(self) -> np.ndarray:
        """The signal has ended: its remaining frames (the right edge reflected now that the length is
        known) are pushed and the session finished → the rest of the audio."""
        feed = self._audio_feed()
        state, jobs, nt = feed.stage(None, final=True)
        out = [self.push(torch.stack(feed.front.windows(jobs)))] if nt else []
        feed.commit(state)
        return np.concatenate(out + [self.finish()], axis=1)

    def close(self) -> None:
        self._session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
