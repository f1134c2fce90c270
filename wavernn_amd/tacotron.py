"""Tacotron acoustic model: text ids → mel, the front half of the reference's gen_tacotron.py.

`Tacotron` has the reference's constructor, parameter and buffer names and shapes
(models/tacotron.py:290), so a reference `.pyt` loads unchanged, and the reference's generation
interface:

    mel, linear, attention = model.generate(x, steps=2000)          # one sentence
    results = model.generate_list([x0, x1, ...], steps=2000)        # N sentences, N lengths

Two backends compute the same thing:

* ``backend='torch'`` restates the definitions in ordinary torch ops (CPU or GPU, any size).
* ``backend='hip'`` (the default on a GPU at the sizes the kernel takes) runs the decoder loop —
  prenet, attention GRU, location-sensitive attention, two residual LSTM cells, mel projection and
  the stop test — as ONE persistent HIP launch for up to 128 sentences (csrc/tacotron_decoder.hip,
  DESIGN.md §4.9). The encoder, `encoder_proj`, the postnet CBHG and `post_proj` run once per
  sentence, parallel over time, as torch-ROCm modules.

``cbhg='hip'`` (opt-in, independent of `backend`; also `encode_list`, `postprocess_list`) runs those
two CBHGs as ragged HIP passes instead (csrc/cbhg.hip): all sentences of a list packed
end to end on the time axis, one `wrnn_cbhg_run` for the encoders and one for the postnets per chunk
of `cbhg_budget` bytes of scratch. With `backend='hip'` as well no torch module runs and torch's
deterministic switches (below) are not touched. ``cbhg=None`` / ``'torch'`` is the path described here.

`generate()` runs in eval mode: no prenet dropout, no zoneout; the loop is deterministic.
The text front end (`text_to_sequence`) stays with the caller: inputs are sequences of ids.
While a call runs, the encoder and postnet modules run under torch's process-wide deterministic-algorithm
switches (`repeatable_modules`): not thread-safe, other torch callers in the process see them meanwhile.
Tacotron frames are not streamed into a `WaveRNNStream`: the reference vocodes the postnet's
output, and the postnet's bidirectional GRU needs the whole utterance first.
"""
from __future__ import annotations

import contextlib
import ctypes
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

MAX_ROWS = 128          # sentences per launch: the vocoder's slot count
BACKENDS = (None, 'torch', 'hip')
CBHGS = (None, 'torch', 'hip')
CBHG_SCRATCH_BUDGET = 1 << 30   # bytes of device scratch one ragged CBHG pass may take before a list is cut into chunks


@contextlib.contextmanager
def repeatable_modules():
    """The torch-ROCm modules around the decoder loop (encoder, postnet) under deterministic
    algorithms: with the default ones two calls on the same input differ in the last bits on the GPU,
    and a list's sentence has to equal its own generate() bit for bit.

    These are torch's process-wide switches (use_deterministic_algorithms, cudnn.deterministic,
    cudnn.benchmark), restored on exit: while a generate() / generate_list() call runs, torch work
    issued by other threads of the process runs under them too, and two threads inside this context
    at once may restore each other's values. Call generation from one thread."""
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev[2], prev[3]


class Highway(nn.Module):
    """y = g·relu(W1 x) + (1 − g)·x with g = sigmoid(W2 x)."""

    def __init__(self, size: int):
        super().__init__()
        self.W1 = nn.Linear(size, size)
        self.W2 = nn.Linear(size, size)
        with torch.no_grad():
            self.W1.bias.zero_()

    def forward(self, x):
        gate = torch.sigmoid(self.W2(x))
        return gate * F.relu(self.W1(x)) + (1.0 - gate) * x


class PreNet(nn.Module):
    def __init__(self, in_dims: int, fc1_dims: int = 256, fc2_dims: int = 128, dropout: float = 0.5):
        super().__init__()
        self.fc1 = nn.Linear(in_dims, fc1_dims)
        self.fc2 = nn.Linear(fc1_dims, fc2_dims)
        self.p = dropout

    def forward(self, x):
        for fc in (self.fc1, self.fc2):
            x = F.dropout(F.relu(fc(x)), self.p, training=self.training)
        return x


class BatchNormConv(nn.Module):
    """Bias-free 'same' convolution, optional ReLU, then BatchNorm."""

    def __init__(self, in_channels: int, out_channels: int, kernel: int, relu: bool = True):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel, stride=1, padding=kernel // 2, bias=False)
        self.bnorm = nn.BatchNorm1d(out_channels)
        self.relu = relu

    def forward(self, x):
        y = self.conv(x)
        if self.relu:
            y = F.relu(y)
        return self.bnorm(y)


class CBHG(nn.Module):
    """Conv bank (kernels 1..K) → max-pool → two projections → residual → highways → biGRU."""

    def __init__(self, K: int, in_channels: int, channels: int, proj_channels: Sequence[int], num_highways: int):
        super().__init__()
        self.conv1d_bank = nn.ModuleList(BatchNormConv(in_channels, channels, k) for k in range(1, K + 1))
        self.maxpool = nn.MaxPool1d(kernel_size=2, stride=1, padding=1)
        self.conv_project1 = BatchNormConv(K * channels, proj_channels[0], 3)
        self.conv_project2 = BatchNormConv(proj_channels[0], proj_channels[1], 3, relu=False)
        self.highway_mismatch = proj_channels[-1] != channels
        if self.highway_mismatch:
            self.pre_highway = nn.Linear(proj_channels[-1], channels, bias=False)
        self.highways = nn.ModuleList(Highway(channels) for _ in range(num_highways))
        self.rnn = nn.GRU(channels, channels, batch_first=True, bidirectional=True)

    def forward(self, x):
        T = x.size(-1)
        # an even kernel's padding yields T + 1 outputs; the last one is dropped
        bank = torch.cat([conv(x)[:, :, :T] for conv in self.conv1d_bank], dim=1)
        y = self.maxpool(bank)[:, :, :T]
        y = self.conv_project2(self.conv_project1(y)) + x
        y = y.transpose(1, 2)
        if self.highway_mismatch:
            y = self.pre_highway(y)
        for hw in self.highways:
            y = hw(y)
        self.rnn.flatten_parameters()
        return self.rnn(y)[0]


class Encoder(nn.Module):
    def __init__(self, embed_dims, num_chars, cbhg_channels, K, num_highways, dropout):
        super().__init__()
        self.embedding = nn.Embedding(num_chars, embed_dims)
        self.pre_net = PreNet(embed_dims)
        self.cbhg = CBHG(K, cbhg_channels, cbhg_channels, [cbhg_channels, cbhg_channels], num_highways)

    def forward(self, x):
        return self.cbhg(self.pre_net(self.embedding(x)).transpose(1, 2))


class LSA(nn.Module):
    """Location-sensitive attention with the 'smooth' normalisation sigmoid(u) / Σ sigmoid(u)."""

    def __init__(self, attn_dim: int, kernel_size: int = 31, filters: int = 32):
        super().__init__()
        self.conv = nn.Conv1d(2, filters, padding=(kernel_size - 1) // 2, kernel_size=kernel_size, bias=False)
        self.L = nn.Linear(filters, attn_dim, bias=True)
        self.W = nn.Linear(attn_dim, attn_dim, bias=True)
        self.v = nn.Linear(attn_dim, 1, bias=False)


class Decoder(nn.Module):
    max_r = 20

    def __init__(self, n_mels: int, decoder_dims: int, lstm_dims: int):
        super().__init__()
        self.register_buffer('r', torch.tensor(1, dtype=torch.int))
        self.n_mels = n_mels
        self.prenet = PreNet(n_mels)
        self.attn_net = LSA(decoder_dims)
        self.attn_rnn = nn.GRUCell(decoder_dims + decoder_dims // 2, decoder_dims)
        self.rnn_input = nn.Linear(2 * decoder_dims, lstm_dims)
        self.res_rnn1 = nn.LSTMCell(lstm_dims, lstm_dims)
        self.res_rnn2 = nn.LSTMCell(lstm_dims, lstm_dims)
        self.mel_proj = nn.Linear(lstm_dims, n_mels * self.max_r, bias=False)


# recurrent state of one sentence, in the order the C-ABI lists the fields
STATE_FIELDS = ('attn_hidden', 'rnn1_hidden', 'rnn1_cell', 'rnn2_hidden', 'rnn2_cell', 'context', 'cumulative',
                'attention', 'frame')


def zero_state(model: 'Tacotron', t_enc: int, device=None, dtype=None) -> dict:
    p = model.encoder_proj.weight
    kw = dict(device=device if device is not None else p.device, dtype=dtype if dtype is not None else p.dtype)
    z = lambda n: torch.zeros(1, n, **kw)   # noqa: E731
    return {'attn_hidden': z(model.decoder_dims), 'rnn1_hidden': z(model.lstm_dims), 'rnn1_cell': z(model.lstm_dims),
            'rnn2_hidden': z(model.lstm_dims), 'rnn2_cell': z(model.lstm_dims), 'context': z(model.decoder_dims),
            'cumulative': z(t_enc), 'attention': z(t_enc), 'frame': z(model.n_mels)}


def decoder_step(dec: Decoder, enc: torch.Tensor, enc_proj: torch.Tensor, s: dict, r: int):
    """One eval-mode decoder step in torch ops: (frames (1, n_mels, r), scores (1, T), new state).
    enc, enc_proj are (1, T, decoder_dims); `s` is a state dict as zero_state() makes it."""
    a = dec.attn_net
    h = dec.attn_rnn(torch.cat([s['context'], dec.prenet(s['frame'])], dim=-1), s['attn_hidden'])
    loc = a.L(a.conv(torch.stack([s['cumulative'], s['attention']], dim=1)).transpose(1, 2))
    u = a.v(torch.tanh(a.W(h).unsqueeze(1) + enc_proj + loc)).squeeze(-1)
    sg = torch.sigmoid(u)
    scores = sg / sg.sum(dim=1, keepdim=True)
    ctx = torch.bmm(scores.unsqueeze(1), enc).squeeze(1)
    x = dec.rnn_input(torch.cat([ctx, h], dim=1))
    h1, c1 = dec.res_rnn1(x, (s['rnn1_hidden'], s['rnn1_cell']))
    x = x + h1
    h2, c2 = dec.res_rnn2(x, (s['rnn2_hidden'], s['rnn2_cell']))
    x = x + h2
    frames = dec.mel_proj(x).view(-1, dec.n_mels, dec.max_r)[:, :, :r]
    new = {'attn_hidden': h, 'rnn1_hidden': h1, 'rnn1_cell': c1, 'rnn2_hidden': h2, 'rnn2_cell': c2, 'context': ctx,
           'cumulative': s['cumulative'] + scores, 'attention': scores, 'frame': frames[:, :, -1]}
    return frames, scores, new


class DecoderSession:
    """Up to 128 sentences in the HIP decoder loop: owns the device buffers of one list of encoder
    outputs and runs `run(n)` further steps of every sentence still going. The recurrent state is
    the tensor `state` (rows, floats); `field(name)` views one field of it (float32, or int32 for
    'step' and 'stopped') and may be read and written between runs."""

    def __init__(self, model: 'Tacotron', encs: Sequence[torch.Tensor], projs: Sequence[torch.Tensor], steps: int,
                 r: Optional[int] = None, stop_threshold: Optional[float] = None, timeout_ms: int = 0):
        from . import _native as nat
        self.nat, self.model = nat, model
        self.cfg = model.kernel_cfg()
        nat.check_cond(nat.lib().wrnn_taco_supported(ctypes.byref(self.cfg)))
        rows = len(encs)
        if not 1 <= rows <= MAX_ROWS:
            raise ValueError(f'a decoder launch takes 1..{MAX_ROWS} sentences, got {rows}')
        dev = encs[0].device
        if dev.type != 'cuda':
            raise RuntimeError("backend='hip' needs the model on a GPU")
        self.rows, self.dev = rows, dev
        self.r = int(model.r if r is None else r)
        self.thr = float(model.stop_threshold if stop_threshold is None else stop_threshold)
        self.step_cap = max(1, -(-int(steps) // self.r))
        self.t_enc = [int(e.shape[0]) for e in encs]
        self.t_max = max(self.t_enc)
        D = model.decoder_dims
        self.enc = torch.zeros(rows, self.t_max, D, device=dev, dtype=torch.float32)
        self.proj = torch.zeros(rows, self.t_max, D, device=dev, dtype=torch.float32)
        for b, (e, p) in enumerate(zip(encs, projs)):
            self.enc[b, :e.shape[0]] = e
            self.proj[b, :e.shape[0]] = p
        self.t_enc_dev = torch.tensor(self.t_enc, device=dev, dtype=torch.int32)
        L = nat.lib()
        ld = L.wrnn_taco_state_floats(ctypes.byref(self.cfg), self.t_max)
        if ld < 0:
            nat.check_cond(ld)
        offs = (ctypes.c_int * len(nat.TACO_STATE_FIELDS))()
        nat.check_cond(L.wrnn_taco_state_layout(ctypes.byref(self.cfg), self.t_max, offs))
        self.offsets = dict(zip(nat.TACO_STATE_FIELDS, list(offs)))
        self.state = torch.zeros(rows, ld, device=dev, dtype=torch.float32)
        self.mel = torch.zeros(rows, self.step_cap * self.r, model.n_mels, device=dev, dtype=torch.float32)
        self.attn = torch.zeros(rows, self.step_cap, self.t_max, device=dev, dtype=torch.float32)
        n = L.wrnn_taco_scratch_floats(ctypes.byref(self.cfg), rows)
        if n < 0:
            nat.check_cond(int(n))
        self.scratch = torch.zeros(int(n), device=dev, dtype=torch.float32)
        self.timeout_ms = timeout_ms

    def field(self, name: str) -> torch.Tensor:
        o = self.offsets[name]
        sizes = {'attn_hidden': self.model.decoder_dims, 'context': self.model.decoder_dims, 'cumulative': self.t_max,
                 'attention': self.t_max, 'frame': self.model.n_mels, 'step': 1, 'stopped': 1}
        n = sizes.get(name, self.model.lstm_dims)
        if name in ('step', 'stopped'):
            return self.state.view(torch.int32)[:, o]
        return self.state[:, o:o + n]

    def run(self, n_steps: int):
        nat = self.nat
        w = self.model.kernel_weights()      # collected per call: .data updates and reloads reach the kernel
        ws = nat.TacoWeights(*[t.data_ptr() for t in w])
        rc = nat.lib().wrnn_taco_run(ctypes.byref(self.cfg), ctypes.byref(ws), self.enc.data_ptr(), self.proj.data_ptr(),
                                     self.t_enc_dev.data_ptr(), self.t_max, self.rows, self.r, self.thr, self.step_cap,
                                     int(n_steps), self.state.data_ptr(), self.mel.data_ptr(), self.attn.data_ptr(),
                                     self.scratch.data_ptr(), self.timeout_ms,
                                     torch.cuda.current_stream(self.dev).cuda_stream)
        del w
        nat.check_cond(rc)

    def steps_done(self) -> List[int]:
        return [int(v) for v in self.field('step').cpu()]

    def outputs(self) -> List[Tuple[torch.Tensor, torch.Tensor, int]]:
        """Per sentence: mel (frames, n_mels), attention (steps, T_enc), decoder steps (device tensors)."""
        out = []
        for b, n in enumerate(self.steps_done()):
            out.append((self.mel[b, :n * self.r], self.attn[b, :n, :self.t_enc[b]], n))
        return out


class Tacotron(nn.Module):
    def __init__(self, embed_dims, num_chars, encoder_dims, decoder_dims, n_mels, fft_bins, postnet_dims,
                 encoder_K, lstm_dims, postnet_K, num_highways, dropout, stop_threshold, mode='teacher_forcing'):
        super().__init__()
        self.n_mels = n_mels
        self.lstm_dims = lstm_dims
        self.decoder_dims = decoder_dims
        self.encoder = Encoder(embed_dims, num_chars, encoder_dims, encoder_K, num_highways, dropout)
        self.encoder_proj = nn.Linear(decoder_dims, decoder_dims, bias=False)
        self.decoder = Decoder(n_mels, decoder_dims, lstm_dims)
        self.postnet = CBHG(postnet_K, n_mels, postnet_dims, [256, 80], num_highways)
        self.post_proj = nn.Linear(postnet_dims * 2, fft_bins, bias=False)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.register_buffer('stop_threshold', torch.tensor(stop_threshold, dtype=torch.float32))
        self.mode = mode

    # ------------------------------------------------------------------ reference housekeeping
    @property
    def r(self) -> int:
        return self.decoder.r.item()

    @r.setter
    def r(self, value):
        self.decoder.r = self.decoder.r.new_tensor(int(value), requires_grad=False)

    def get_step(self) -> int:
        return self.step.data.item()

    def load(self, path: Union[str, Path]):
        device = next(self.parameters()).device
        state = torch.load(path, map_location=device, weights_only=True)
        if 'r' in state and 'decoder.r' not in state:    # checkpoints from before r was a buffer
            self.r = state['r']
        self.load_state_dict(state, strict=False)

    def save(self, path: Union[str, Path]):
        torch.save(self.state_dict(), path)

    # ------------------------------------------------------------------ the HIP decoder's view
    def kernel_cfg(self):
        from . import _native as nat
        d = self.decoder
        return nat.TacoCfg(self.n_mels, self.decoder_dims, self.lstm_dims, self.encoder_proj.in_features,
                           d.prenet.fc1.out_features, d.prenet.fc2.out_features, d.attn_net.conv.out_channels,
                           d.attn_net.conv.kernel_size[0], d.max_r)

    def kernel_weights(self) -> List[torch.Tensor]:
        """The decoder's tensors in _native.TACO_WEIGHTS order, read in place (fp32, contiguous)."""
        d = self.decoder
        ts = [d.prenet.fc1.weight, d.prenet.fc1.bias, d.prenet.fc2.weight, d.prenet.fc2.bias,
              d.attn_rnn.weight_ih, d.attn_rnn.weight_hh, d.attn_rnn.bias_ih, d.attn_rnn.bias_hh,
              d.attn_net.conv.weight, d.attn_net.L.weight, d.attn_net.L.bias, d.attn_net.W.weight, d.attn_net.W.bias,
              d.attn_net.v.weight, d.rnn_input.weight, d.rnn_input.bias,
              d.res_rnn1.weight_ih, d.res_rnn1.weight_hh, d.res_rnn1.bias_ih, d.res_rnn1.bias_hh,
              d.res_rnn2.weight_ih, d.res_rnn2.weight_hh, d.res_rnn2.bias_ih, d.res_rnn2.bias_hh, d.mel_proj.weight]
        return [t.detach().to(torch.float32).contiguous() for t in ts]

    def hip_unsupported_reason(self) -> Optional[str]:
        """None when backend='hip' can run this model where it is, else why not."""
        p = self.encoder_proj.weight
        if p.device.type != 'cuda':
            return 'the model is not on a GPU'
        if p.dtype != torch.float32:
            return f'the kernel takes float32 weights, the model is {p.dtype}'
        cus = torch.cuda.get_device_properties(p.device).multi_processor_count
        if cus < MAX_ROWS:
            return f'the kernel needs at least {MAX_ROWS} CUs (one workgroup per CU, one owner per sentence), the device has {cus}'
        from . import _native as nat
        cfg = self.kernel_cfg()
        if nat.lib().wrnn_taco_supported(ctypes.byref(cfg)) != 0:
            return (nat.lib().wrnn_cond_last_error() or b'').decode(errors='replace')
        return None

    def _backend(self, backend) -> str:
        if backend not in BACKENDS:
            raise ValueError(f'backend must be one of {BACKENDS}, got {backend!r}')
        if backend == 'torch':
            return 'torch'
        why = self.hip_unsupported_reason()
        if why is None:
            return 'hip'
        if backend == 'hip':
            raise RuntimeError(f"backend='hip' cannot run this model: {why}")
        return 'torch'

    # ------------------------------------------------------------------ the HIP CBHGs' view
    def cbhg_cfg(self, which: str):
        """The wrnn_cbhg_cfg of 'encoder' or 'postnet'."""
        from . import _native as nat
        enc = which == 'encoder'
        c = self.encoder.cbhg if enc else self.postnet
        e = self.encoder
        return nat.CbhgCfg(len(c.conv1d_bank), c.conv1d_bank[0].conv.in_channels, c.conv1d_bank[0].conv.out_channels,
                           c.conv_project1.conv.out_channels, c.conv_project2.conv.out_channels, int(c.highway_mismatch),
                           len(c.highways), int(enc), e.embedding.embedding_dim if enc else 0,
                           e.embedding.num_embeddings if enc else 0, e.pre_net.fc1.out_features if enc else 0,
                           (self.encoder_proj if enc else self.post_proj).out_features)

    def cbhg_weights(self, which: str):
        """(wrnn_cbhg_weights, the tensors it points to): the module's own tensors, collected per call,
        so .data updates, reloads and changed BatchNorm statistics reach the kernels."""
        from . import _native as nat
        enc = which == 'encoder'
        c = self.encoder.cbhg if enc else self.postnet
        keep: List[torch.Tensor] = []

        def ptr(t):
            t = t.detach().to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        w = nat.CbhgWeights()
        if enc:
            e = self.encoder
            w.embedding, w.prenet_fc1_w, w.prenet_fc1_b = ptr(e.embedding.weight), ptr(e.pre_net.fc1.weight), ptr(e.pre_net.fc1.bias)
            w.prenet_fc2_w, w.prenet_fc2_b = ptr(e.pre_net.fc2.weight), ptr(e.pre_net.fc2.bias)

        def bnconv(m):
            return (ptr(m.conv.weight), ptr(m.bnorm.weight), ptr(m.bnorm.bias), ptr(m.bnorm.running_mean),
                    ptr(m.bnorm.running_var))
        for k, m in enumerate(c.conv1d_bank):
            w.bank_w[k], w.bank_bn_w[k], w.bank_bn_b[k], w.bank_bn_mean[k], w.bank_bn_var[k] = bnconv(m)
        w.proj1_w, w.proj1_bn_w, w.proj1_bn_b, w.proj1_bn_mean, w.proj1_bn_var = bnconv(c.conv_project1)
        w.proj2_w, w.proj2_bn_w, w.proj2_bn_b, w.proj2_bn_mean, w.proj2_bn_var = bnconv(c.conv_project2)
        if c.highway_mismatch:
            w.pre_highway_w = ptr(c.pre_highway.weight)
        for i, h in enumerate(c.highways):
            w.hw_w1[i], w.hw_b1[i], w.hw_w2[i], w.hw_b2[i] = ptr(h.W1.weight), ptr(h.W1.bias), ptr(h.W2.weight), ptr(h.W2.bias)
        r = c.rnn
        w.rnn_w_ih, w.rnn_w_hh, w.rnn_b_ih, w.rnn_b_hh = ptr(r.weight_ih_l0), ptr(r.weight_hh_l0), ptr(r.bias_ih_l0), ptr(r.bias_hh_l0)
        w.rnn_w_ih_r, w.rnn_w_hh_r = ptr(r.weight_ih_l0_reverse), ptr(r.weight_hh_l0_reverse)
        w.rnn_b_ih_r, w.rnn_b_hh_r = ptr(r.bias_ih_l0_reverse), ptr(r.bias_hh_l0_reverse)
        w.tail_w = ptr((self.encoder_proj if enc else self.post_proj).weight)
        return w, keep

    def cbhg_unsupported_reason(self) -> Optional[str]:
        """None when cbhg='hip' can run this model where it is, else why not."""
        p = self.encoder_proj.weight
        if p.device.type != 'cuda':
            return 'the model is not on a GPU'
        if p.dtype != torch.float32:
            return f'the kernels take float32 weights, the model is {p.dtype}'
        from . import _native as nat
        for which in ('encoder', 'postnet'):
            c = self.encoder.cbhg if which == 'encoder' else self.postnet
            if len(c.conv1d_bank) > nat.CBHG_MAX_K or len(c.highways) > nat.CBHG_HIGHWAYS:
                return f'the {which} CBHG has {len(c.conv1d_bank)} bank kernels and {len(c.highways)} highways; at most ' \
                       f'{nat.CBHG_MAX_K} and {nat.CBHG_HIGHWAYS} are taken'
            cfg = self.cbhg_cfg(which)
            if nat.lib().wrnn_cbhg_supported(ctypes.byref(cfg)) != 0:
                return f'{which}: ' + (nat.lib().wrnn_cond_last_error() or b'').decode(errors='replace')
        return None

    def _cbhg(self, cbhg) -> str:
        if cbhg not in CBHGS:
            raise ValueError(f'cbhg must be one of {CBHGS}, got {cbhg!r}')
        if cbhg != 'hip':
            return 'torch'
        why = self.cbhg_unsupported_reason()
        if why is not None:
            raise RuntimeError(f"cbhg='hip' cannot run this model: {why}")
        return 'hip'

    def _cbhg_run_list(self, which: str, rows: Sequence[torch.Tensor], budget: Optional[int], keep_scratch: Optional[list] = None):
        """`rows`: per sentence int32 ids (T,) or float rows (T, in_channels) on the device. One wrnn_cbhg_run
        per chunk of whole sentences whose scratch stays within `budget` bytes (a sentence that alone
        exceeds it runs alone). Returns per sentence (GRU output (T, 2·channels), tail output (T, tail)).
        `keep_scratch`: a list that receives (cfg, scratch tensor, positions) of every run, for reading stages."""
        from . import _native as nat
        L = nat.lib()
        cfg = self.cbhg_cfg(which)
        budget = CBHG_SCRATCH_BUDGET if budget is None else int(budget)
        dev = self.encoder_proj.weight.device
        lens = [int(r.shape[0]) for r in rows]
        if min(lens, default=1) < 1:
            raise ValueError('every sentence needs at least one position')
        need = lambda p: int(L.wrnn_cbhg_scratch_bytes(ctypes.byref(cfg), p))   # noqa: E731
        out: list = [None] * len(rows)
        k = 0
        while k < len(rows):
            n, pos = 1, lens[k]
            while k + n < len(rows) and need(pos + lens[k + n]) <= budget:
                pos += lens[k + n]
                n += 1
            nbytes = need(pos)
            if nbytes < 0:
                nat.check_cond(nbytes)
            offs = (ctypes.c_int * (n + 1))(*np.concatenate([[0], np.cumsum(lens[k:k + n])]).tolist())
            packed = torch.cat(list(rows[k:k + n]), dim=0).contiguous()
            scratch = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
            rnn = torch.empty(pos, 2 * cfg.channels, device=dev, dtype=torch.float32)
            tail = torch.empty(pos, cfg.tail_out, device=dev, dtype=torch.float32)
            w, keep = self.cbhg_weights(which)
            rc = L.wrnn_cbhg_run(ctypes.byref(cfg), ctypes.byref(w), packed.data_ptr(), offs, n, rnn.data_ptr(), tail.data_ptr(),
                                 scratch.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
            del keep
            nat.check_cond(rc)
            if keep_scratch is not None:
                keep_scratch.append((cfg, scratch, pos))
            for i in range(n):
                out[k + i] = (rnn[offs[i]:offs[i + 1]], tail[offs[i]:offs[i + 1]])
            k += n
        return out

    def encode_list(self, xs: Sequence, cbhg: Optional[str] = None, cbhg_budget: Optional[int] = None) -> list:
        """Per sentence (encoder_seq, encoder_seq_proj), each (1, T, decoder_dims). cbhg='hip': every
        sentence's encoder in one ragged HIP pass per chunk (eval-mode arithmetic whatever the module's
        mode); None / 'torch': encode() per sentence, in the module's current mode."""
        if self._cbhg(cbhg) == 'torch':
            return [self.encode(x) for x in xs]
        dev = self.encoder_proj.weight.device
        ids = [torch.as_tensor(np.asarray(x).reshape(-1) if not torch.is_tensor(x) else x.reshape(-1)).to(dev, torch.int32)
               for x in xs]
        return [(e.unsqueeze(0), p.unsqueeze(0)) for e, p in self._cbhg_run_list('encoder', ids, cbhg_budget)]

    def postprocess_list(self, mels: Sequence[torch.Tensor], cbhg: Optional[str] = None,
                         cbhg_budget: Optional[int] = None) -> list:
        """Per mel (1, n_mels, frames) the linear (1, fft_bins, frames); cbhg as in encode_list."""
        if self._cbhg(cbhg) == 'torch':
            return [self.postprocess(m) for m in mels]
        dev = self.encoder_proj.weight.device
        rows = [torch.as_tensor(m).to(dev, torch.float32).reshape(self.n_mels, -1).t() for m in mels]
        return [lin.t().unsqueeze(0) for _, lin in self._cbhg_run_list('postnet', rows, cbhg_budget)]

    # ------------------------------------------------------------------ generation
    def encode(self, x) -> Tuple[torch.Tensor, torch.Tensor]:
        """One sentence's ids → (encoder_seq, encoder_seq_proj), each (1, T, decoder_dims)."""
        x = torch.as_tensor(x, dtype=torch.long, device=self.encoder_proj.weight.device).reshape(1, -1)
        enc = self.encoder(x)
        return enc, self.encoder_proj(enc)

    def decode_torch(self, enc, proj, steps: int):
        """The loop in torch ops: mel (1, n_mels, frames), attention (1, decoder_steps, T)."""
        r, thr = self.r, self.stop_threshold
        s = zero_state(self, enc.shape[1], enc.device, enc.dtype)
        mels, attn = [], []
        for t in range(0, steps, r):
            frames, scores, s = decoder_step(self.decoder, enc, proj, s, r)
            mels.append(frames)
            attn.append(scores.unsqueeze(1))
            if t > 10 and bool((frames < thr).all()):
                break
        return torch.cat(mels, dim=2), torch.cat(attn, dim=1)

    def postprocess(self, mel: torch.Tensor) -> torch.Tensor:
        """mel (1, n_mels, frames) → linear (1, fft_bins, frames)."""
        return self.post_proj(self.postnet(mel)).transpose(1, 2)

    @staticmethod
    def _numpy(mel, linear, attn):
        return mel[0].cpu().numpy(), linear[0].cpu().numpy(), attn[0].cpu().numpy()

    def generate(self, x, steps: int = 2000, backend: Optional[str] = None, cbhg: Optional[str] = None,
                 cbhg_budget: Optional[int] = None):
        """(mel (n_mels, frames), linear (fft_bins, frames), attention (decoder_steps, T_enc)) as numpy,
        in the reference's order and shapes. cbhg='hip' runs the encoder and the postnet as ragged HIP
        passes (csrc/cbhg.hip) instead of torch modules; it is independent of `backend`."""
        if self._cbhg(cbhg) == 'hip':
            return self.generate_list([x], steps, backend, cbhg='hip', cbhg_budget=cbhg_budget)[0]
        if self._backend(backend) == 'hip':
            return self.generate_list([x], steps)[0]
        self.eval()
        try:
            with torch.no_grad(), repeatable_modules():
                enc, proj = self.encode(x)
                mel, attn = self.decode_torch(enc, proj, steps)
                return self._numpy(mel, self.postprocess(mel), attn)
        finally:
            self.train()      # as the reference leaves the model, also when the call raised

    def generate_list(self, xs: Sequence, steps: int = 2000, backend: Optional[str] = None, cbhg: Optional[str] = None,
                      cbhg_budget: Optional[int] = None) -> list:
        """N sentences of N lengths; each stops on its own. Returns generate()'s triple per sentence,
        in the order given. cbhg='hip': the list's encoders are one ragged HIP pass and its postnets
        another (per chunk of `cbhg_budget` bytes of scratch, default CBHG_SCRATCH_BUDGET); with
        backend='hip' as well no torch module runs and torch's deterministic switches stay untouched."""
        if self._cbhg(cbhg) == 'hip':
            return self._generate_list_cbhg(xs, steps, self._backend(backend), cbhg_budget)
        if self._backend(backend) == 'torch':
            return [self.generate(x, steps, backend='torch') for x in xs]
        self.eval()
        out: list = [None] * len(xs)
        try:
            with torch.no_grad(), repeatable_modules():
                coded = [self.encode(x) for x in xs]
                # longest encoder sequence first, so a launch's rows are of similar length
                order = sorted(range(len(xs)), key=lambda i: -coded[i][0].shape[1])
                for k in range(0, len(order), MAX_ROWS):
                    idx = order[k:k + MAX_ROWS]
                    sess = DecoderSession(self, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], steps)
                    sess.run(sess.step_cap)
                    for i, (mel, attn, _) in zip(idx, sess.outputs()):
                        mel = mel.transpose(0, 1).unsqueeze(0).contiguous()
                        out[i] = self._numpy(mel, self.postprocess(mel), attn.unsqueeze(0))
        finally:
            self.train()      # as the reference leaves the model, also when a launch failed (WRNN_ETIMEOUT, …)
        return out

    def _generate_list_cbhg(self, xs: Sequence, steps: int, backend: str, budget: Optional[int]) -> list:
        """generate_list with the CBHGs in HIP: encode_list → decoder loop (hip launches of up to 128
        sentences, or the torch loop per sentence) → postprocess_list."""
        if len(xs) == 0:
            return []
        self.eval()
        mels: list = [None] * len(xs)
        attns: list = [None] * len(xs)
        try:
            with torch.no_grad():
                coded = self.encode_list(xs, cbhg='hip', cbhg_budget=budget)
                if backend == 'hip':
                    order = sorted(range(len(xs)), key=lambda i: -coded[i][0].shape[1])
                    for k in range(0, len(order), MAX_ROWS):
                        idx = order[k:k + MAX_ROWS]
                        sess = DecoderSession(self, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], steps)
                        sess.run(sess.step_cap)
                        for i, (mel, attn, _) in zip(idx, sess.outputs()):
                            mels[i], attns[i] = mel.transpose(0, 1).unsqueeze(0).contiguous(), attn.unsqueeze(0).clone()
                else:
                    with repeatable_modules():
                        for i, (enc, proj) in enumerate(coded):
                            mels[i], attns[i] = self.decode_torch(enc, proj, steps)
                lins = self.postprocess_list(mels, cbhg='hip', cbhg_budget=budget)
                return [self._numpy(m, l, a) for m, l, a in zip(mels, lins, attns)]
        finally:
            self.train()


# the reference's hparams.py:67-77; an hparams object's own tts_* values take precedence
TTS_DEFAULTS = dict(tts_embed_dims=256, tts_encoder_dims=128, tts_decoder_dims=256, tts_postnet_dims=128, tts_encoder_K=16,
                    tts_lstm_dims=512, tts_postnet_K=8, tts_num_highways=4, tts_dropout=0.5, tts_stop_threshold=-3.4,
                    num_mels=80)


def build_tacotron(hp=None, num_chars: Optional[int] = None, weights: Union[str, Path, None] = None,
                   device=None) -> Tacotron:
    """The reference's gen_tacotron.py:99-111 constructor call (fft_bins = num_mels there). `num_chars` is
    the size of the caller's symbol table; with `weights` it is read off the checkpoint's embedding."""
    v = {k: getattr(hp, k, d) if hp is not None else d for k, d in TTS_DEFAULTS.items()}
    state = None
    if weights is not None:
        state = torch.load(weights, map_location='cpu', weights_only=True)
        num_chars = int(state['encoder.embedding.weight'].shape[0])
    if num_chars is None:
        raise ValueError('build_tacotron needs num_chars or a checkpoint')
    m = Tacotron(embed_dims=v['tts_embed_dims'], num_chars=num_chars, encoder_dims=v['tts_encoder_dims'],
                 decoder_dims=v['tts_decoder_dims'], n_mels=v['num_mels'], fft_bins=v['num_mels'],
                 postnet_dims=v['tts_postnet_dims'], encoder_K=v['tts_encoder_K'], lstm_dims=v['tts_lstm_dims'],
                 postnet_K=v['tts_postnet_K'], num_highways=v['tts_num_highways'], dropout=v['tts_dropout'],
                 stop_threshold=v['tts_stop_threshold'])
    if device is not None:
        m = m.to(device)
    if weights is not None:
        m.load(weights)
    return m
