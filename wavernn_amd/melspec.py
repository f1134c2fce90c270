"""The mel front end on the GPU (C-ABI wrnn_melspec*, csrc/melspec.hip): wav → the normalised mel
generate() takes, for whole signals, lists of unequal signals, and the frames of a stream as they
become final.  Host-only pieces (the tables, the frame count, the streaming plan) work without a
GPU; a launch without one raises — the host float32 path lives in wavernn_amd.dsp, and is never
substituted silently."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from . import dsp


def _cfg(p: dict) -> nat.MelSpecCfg:
    return nat.MelSpecCfg(int(p["sample_rate"]), int(p["n_fft"]), int(p["hop_length"]), int(p["win_length"]),
                          int(p["num_mels"]), float(p["fmin"]), float(p["min_level_db"]))


def _raise(rc: int):
    msg = (nat.lib().wrnn_cond_last_error() or b"").decode(errors="replace")
    if rc == -6:   # WRNN_EUNSUPPORTED
        raise NotImplementedError(msg)
    if rc == -1:   # WRNN_EINVAL
        raise nat.WrnnInvalid(rc, msg)
    raise nat.WrnnError(rc, msg)


def frames(p: dict, n_samples: int) -> int:
    """wrnn_melspec_frames: 1 + n_samples // hop (ValueError below n_fft//2 + 1 samples)."""
    r = nat.lib().wrnn_melspec_frames(ctypes.byref(_cfg(p)), int(n_samples))
    if r < 0:
        _raise(int(r))
    return int(r)


def plan(p: dict, received: int, final: bool = False) -> Tuple[int, int]:
    """wrnn_melspec_plan → (frames that are final with `received` samples in, the first sample a
    later frame may still read)."""
    ready, keep = ctypes.c_int64(), ctypes.c_int64()
    rc = nat.lib().wrnn_melspec_plan(ctypes.byref(_cfg(p)), int(received), int(bool(final)), ctypes.byref(ready),
                                     ctypes.byref(keep))
    if rc:
        _raise(rc)
    return int(ready.value), int(keep.value)


def tables(p: dict) -> np.ndarray:
    """wrnn_melspec_tables: the float32 tables the kernel reads, as one host array."""
    cfg = _cfg(p)
    n = nat.lib().wrnn_melspec_table_floats(ctypes.byref(cfg))
    if n < 0:
        _raise(n)
    out = np.empty(n, dtype=np.float32)
    rc = nat.lib().wrnn_melspec_tables(ctypes.byref(cfg), out.ctypes.data)
    if rc:
        _raise(rc)
    return out


def unpack_tables(p: dict, tab: np.ndarray) -> dict:
    """The named parts of tables(p) (layout: include/wavernn_amd.h), the filterbank made dense again."""
    N, B = int(p["n_fft"]), int(p["num_mels"])
    M = N // 2
    o = 8
    out = {"first_tap": int(tab[0]), "taps": int(tab[1]), "n_weights": int(tab[2]), "window": tab[o:o + N]}
    o += N
    out["twiddle_m"] = tab[o:o + 2 * M].reshape(M, 2)
    o += 2 * M
    out["twiddle_n"] = tab[o:o + 2 * (M + 1)].reshape(M + 1, 2)
    o += 2 * (M + 1)
    start, length, off = (tab[o + i * B:o + (i + 1) * B].astype(np.int64) for i in range(3))
    o += 3 * B
    w = tab[o:]
    assert len(w) == out["n_weights"] == int(length.sum())
    basis = np.zeros((B, M + 1), dtype=np.float32)
    for i in range(B):
        basis[i, start[i]:start[i] + length[i]] = w[off[i]:off[i] + length[i]]
    out.update(start=start, length=length, basis=basis)
    return out


class MelSpec:
    """One geometry's front end on one GPU: the tables, uploaded once."""
    _cache: dict = {}

    def __init__(self, p: dict, device):
        self.p = dict(p)
        self.cfg = _cfg(p)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MelSpec runs the HIP kernel: it needs a GPU (dsp.melspectrogram has the host path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_mels = int(p["num_mels"])
        self.hop = int(p["hop_length"])
        self.tables = torch.from_numpy(tables(p)).to(self.device)

    @classmethod
    def get(cls, p: dict, device) -> "MelSpec":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (tuple(sorted((k, float(v)) for k, v in p.items() if k in dsp.MELSPEC_KEYS)), str(device))
        if key not in cls._cache:
            cls._cache[key] = cls(p, device)
        return cls._cache[key]

    def _wav(self, y) -> torch.Tensor:
        if isinstance(y, np.ndarray) and not y.flags.writeable:
            y = y.copy()
        t = torch.as_tensor(y)
        if t.dim() != 1:
            raise ValueError("a signal is 1-D")
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def run(self, wavs: Sequence, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """Whole signals (1-D tensors or arrays of any lengths) → their mels [num_mels][T_u] on the
        GPU, ONE launch (wrnn_melspec).  `out`: tensors [num_mels][ld_u >= T_u] to write into (their
        columns beyond T_u stay untouched); the returned mels are then views of them."""
        ws = [self._wav(y) for y in wavs]
        U = len(ws)
        if not U:
            raise ValueError("melspectrogram needs at least one signal")
        T = [frames(self.p, len(w)) for w in ws]
        if out is None:
            out = [torch.empty(self.n_mels, t, dtype=torch.float32, device=self.device) for t in T]
        for o, t in zip(out, T):
            if not (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.dim() == 2
                    and o.shape[0] == self.n_mels and o.shape[1] >= t):
                raise ValueError("out holds contiguous fp32 GPU tensors [num_mels][>= frames]")
        vps, ints = ctypes.c_void_p * U, ctypes.c_int * U
        scratch = torch.empty(nat.MELSPEC_SCRATCH_PER_SIGNAL * U, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = nat.lib().wrnn_melspec(ctypes.byref(self.cfg), self.tables.data_ptr(), vps(*[w.data_ptr() for w in ws]),
                                        ints(*[len(w) for w in ws]), U, vps(*[o.data_ptr() for o in out]),
                                        ints(*[o.shape[1] for o in out]), scratch.data_ptr(), self._stream())
        if rc:
            _raise(rc)
        scratch.record_stream(torch.cuda.current_stream(self.device))
        return [o[:, :t] for o, t in zip(out, T)]

    def windows(self, jobs: Sequence[tuple]) -> List[torch.Tensor]:
        """jobs: (wav_tail 1-D GPU fp32, s0, total or None, t0, nt) per signal → mel [num_mels][nt]
        each, ONE launch (wrnn_melspec_windows): frames t0 .. t0 + nt − 1 of a signal whose samples
        [s0, s0 + len(wav_tail)) are resident."""
        U = len(jobs)
        tails = [self._wav(j[0]) for j in jobs]
        mels = [torch.empty(self.n_mels, int(j[4]), dtype=torch.float32, device=self.device) for j in jobs]
        vps, ints, longs = ctypes.c_void_p * U, ctypes.c_int * U, ctypes.c_int64 * U
        scratch = torch.empty(nat.MELSPEC_SCRATCH_PER_SIGNAL * U, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = nat.lib().wrnn_melspec_windows(
                ctypes.byref(self.cfg), self.tables.data_ptr(), vps(*[t.data_ptr() for t in tails]),
                longs(*[int(j[1]) for j in jobs]), ints(*[len(t) for t in tails]),
                longs(*[-1 if j[2] is None else int(j[2]) for j in jobs]), ints(*[int(j[3]) for j in jobs]),
                ints(*[int(j[4]) for j in jobs]), U, vps(*[m.data_ptr() for m in mels]),
                ints(*[max(1, int(j[4])) for j in jobs]), scratch.data_ptr(), self._stream())
        if rc:
            _raise(rc)
        scratch.record_stream(torch.cuda.current_stream(self.device))
        return mels

    def window(self, wav_tail, s0: int, total: Optional[int], t0: int, nt: int) -> torch.Tensor:
        """One signal's frames t0 .. t0 + nt − 1 (wrnn_melspec_window's job)."""
        return self.windows([(wav_tail, s0, total, t0, nt)])[0]


class AudioFeed:
    """The PCM side of a streaming session: U signals in lock step, their tail kept on the GPU from
    the plan's keep_from, the frames that became final computed by one windows launch."""

    def __init__(self, front: MelSpec, n_streams: int, total_samples: Optional[int] = None):
        self.front, self.U, self.total = front, int(n_streams), total_samples
        self.received, self.done, self.s0 = 0, 0, 0
        self.tail = torch.empty(self.U, 0, dtype=torch.float32, device=front.device)
        self.finished = False

    def _pcm(self, pcm) -> torch.Tensor:
        if isinstance(pcm, np.ndarray) and not pcm.flags.writeable:
            pcm = pcm.copy()
        t = torch.as_tensor(pcm).to(device=self.front.device, dtype=torch.float32)
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2 or t.shape[0] != self.U:
            raise ValueError(f"pcm must be [{self.U}][n] (or [n] for one stream)")
        return t

    def stage(self, pcm, final: bool = False):
        """→ (state to commit(), the jobs of the frames that became final, their count); nothing
        changes until commit()."""
        if self.finished:
            raise RuntimeError("audio after finish_audio(): the session has ended")
        tail = self.tail if pcm is None else torch.cat([self.tail, self._pcm(pcm)], 1).contiguous()
        received = self.s0 + tail.shape[1]
        if self.total is not None and received > self.total:
            raise ValueError(f"{received} samples pushed, total_samples was {self.total}")
        if final and self.total is not None and received != self.total:
            raise ValueError(f"finish_audio() after {received} samples, total_samples was {self.total}")
        ready, keep = plan(self.front.p, received, final)
        nt = ready - self.done
        jobs = [(tail[u], self.s0, received if final else None, self.done, nt) for u in range(self.U)] if nt > 0 else []
        keep = max(keep, self.s0)
        return (tail[:, keep - self.s0:].contiguous(), keep, received, ready, bool(final)), jobs, max(nt, 0)

    def commit(self, state) -> None:
        self.tail, self.s0, self.received, self.done, self.finished = state
