"""Python handle on the persistent HIP sample loop (C-ABI in include/wavernn_amd.h).

`FatchordLoop` is the device-side replacement for the per-step loop of
`WaveRNN.generate()` (models/fatchord_version.py:192-241 in the reference): one call runs
all L steps for B rows in a single persistent-kernel launch per row chunk.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Mapping, Optional, Tuple

import numpy as np
import torch

from . import _native as nat

LOOP_KEYS = ("I.weight", "I.bias", "rnn1.weight_ih_l0", "rnn1.weight_hh_l0", "rnn1.bias_ih_l0",
             "rnn1.bias_hh_l0", "rnn2.weight_ih_l0", "rnn2.weight_hh_l0", "rnn2.bias_ih_l0",
             "rnn2.bias_hh_l0", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight",
             "fc3.bias")


DM_KEYS = ("R.weight", "O1.weight", "O1.bias", "O2.weight", "O2.bias", "O3.weight", "O3.bias", "O4.weight",
           "O4.bias", "I_coarse.weight", "I_fine.weight", "bias_u", "bias_r", "bias_e")


def fingerprint_host(a: np.ndarray) -> int:
    """wrnn_fingerprint of one tensor, restated in numpy (uint64 arithmetic wraps): the sum over j of
    (bits of element j + 1) · (splitmix64(j) | 1) modulo 2^64, as a signed 64-bit integer."""
    bits = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.arange(bits.size, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = (z ^ (z >> np.uint64(31))) | np.uint64(1)
        h = np.add.reduce((bits + np.uint64(1)) * z, dtype=np.uint64)
    return int(np.array(h, dtype=np.uint64).astype(np.int64))


def _fingerprint_args(ts):
    """What a wrnn_fingerprint call over the floating-point tensors of `ts` needs: None (no such
    tensor), ("host", arrays) for CPU tensors, or (n, device, pointers, sizes, out, keep, direct) —
    `direct`: every tensor is read in place (fp32, contiguous), no converted copy was made."""
    fl = [t.detach() for t in ts if t.is_floating_point() and t.numel()]
    if not fl:
        return None
    if not fl[0].is_cuda:
        return ("host", fl)
    keep = [t if t.dtype is torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous() for t in fl]
    n, dev = len(keep), keep[0].device
    return (n, dev, (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep]),
            (ctypes.c_int64 * n)(*[t.numel() for t in keep]), torch.empty(n, dtype=torch.int64, device=dev), keep,
            all(k is t for k, t in zip(keep, fl)))


def content_key(tensors, plan: Optional[dict] = None) -> tuple:
    """Cache key of a set of tensors: (data_ptr, _version) of each, plus a fingerprint of what each
    floating-point one holds.  An in-place operation through `.data` (`p.data.mul_(mask)`, the
    reference pruner's idiom; `conv.weight.data.fill_`) changes neither the pointer nor the version
    counter, so those alone miss it.  The fingerprints come from the device (C-ABI wrnn_fingerprint:
    one launch over all tensors, one small readback); exact integer arithmetic on the fp32 bit
    patterns, so a change of any single element always shows.  CPU tensors: fingerprint_host.
    `plan`: a dict the caller keeps between calls; it holds the call's argument arrays while the
    same tensor objects sit at the same addresses (then their dtype and size are the same too)."""
    ts = list(tensors)
    ident = tuple((t.data_ptr(), t._version) for t in ts)
    ptr = tuple(p for p, _ in ident)
    if plan is not None and plan.get("ptr") == ptr and len(plan["ts"]) == len(ts) and \
            all(a is b for a, b in zip(plan["ts"], ts)):
        args = plan["args"]
    else:
        args = _fingerprint_args(ts)
        if plan is not None:
            plan.clear()
            if args is not None and args[0] != "host" and args[-1]:
                plan.update(ts=ts, ptr=ptr, args=args)
    if args is None:
        return ident
    if args[0] == "host":
        return ident + tuple(fingerprint_host(t.numpy()) for t in args[1])
    n, dev, ptrs, numel, out = args[:5]
    with torch.cuda.device(dev):
        nat.check_cond(nat.lib().wrnn_fingerprint(ptrs, numel, n, out.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream))
        return ident + tuple(out.tolist())


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


def pad_loop_state(state: Mapping[str, np.ndarray], R: int, F: int, A: int, M: int, Rp: int, Fp: int,
                   Ap: int) -> dict:
    """Zero-pad the loop tensors of a WaveRNN with rnn / fc / aux dims R, F, A to Rp, Fp, Ap (the
    kernels' float4 layouts need multiples of 4).  Exact: a padded GRU unit has zero weights and
    biases, so r = z = ½, n = tanh(0) = 0 and h' = h / 2 stays 0 from h = 0; a padded fc row is
    relu(0) = 0; every padded column multiplies such a zero (or a zero-padded aux channel), so the
    real units, rows and logits see only added zero terms (fatchord_version.py:97-123 shapes)."""
    def gates(w, rows, rows_p, cols_map, ncols_p):
        out = np.zeros((3 * rows_p, ncols_p), np.float32)
        for g in range(3):
            for (c0, c1, d0) in cols_map:
                out[g * rows_p:g * rows_p + rows, d0:d0 + c1 - c0] = w[g * rows:(g + 1) * rows, c0:c1]
        return out

    def vec3(b, n, n_p):
        out = np.zeros(3 * n_p, np.float32)
        for g in range(3):
            out[g * n_p:g * n_p + n] = b[g * n:(g + 1) * n]
        return out

    def mat(w, rows_p, cols_map, ncols_p):
        out = np.zeros((rows_p, ncols_p), np.float32)
        for (c0, c1, d0) in cols_map:
            out[:w.shape[0], d0:d0 + c1 - c0] = w[:, c0:c1]
        return out

    def vec(b, n_p):
        out = np.zeros(n_p, np.float32)
        out[:b.shape[0]] = b
        return out

    st = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32)
          for k, v in state.items() if k in LOOP_KEYS}
    o = dict(st)
    o["I.weight"] = mat(st["I.weight"], Rp, [(0, 1 + M, 0), (1 + M, 1 + M + A, 1 + M)], 1 + M + Ap)
    o["I.bias"] = vec(st["I.bias"], Rp)
    for k in ("rnn1.weight_ih_l0", "rnn1.weight_hh_l0", "rnn2.weight_hh_l0"):
        o[k] = gates(st[k], R, Rp, [(0, R, 0)], Rp)
    o["rnn2.weight_ih_l0"] = gates(st["rnn2.weight_ih_l0"], R, Rp, [(0, R, 0), (R, R + A, Rp)], Rp + Ap)
    for k in ("rnn1.bias_ih_l0", "rnn1.bias_hh_l0", "rnn2.bias_ih_l0", "rnn2.bias_hh_l0"):
        o[k] = vec3(st[k], R, Rp)
    o["fc1.weight"] = mat(st["fc1.weight"], Fp, [(0, R, 0), (R, R + A, Rp)], Rp + Ap)
    o["fc1.bias"] = vec(st["fc1.bias"], Fp)
    o["fc2.weight"] = mat(st["fc2.weight"], Fp, [(0, F, 0), (F, F + A, Fp)], Fp + Ap)
    o["fc2.bias"] = vec(st["fc2.bias"], Fp)
    o["fc3.weight"] = mat(st["fc3.weight"], st["fc3.weight"].shape[0], [(0, F, 0)], Fp)
    return o


def noise_width(mode: str, n_classes: int) -> int:
    """K of the injected-noise layout [L][B][K] (reference draw order)."""
    return 11 if mode == "MOL" else n_classes


def philox_draws(seed: int, row_offset: int, rows: int, steps: int, K: int, mode: str, step0: int = 0,
                 device: int = 0, stream=None) -> torch.Tensor:
    """The draws a loop launch takes with noise=None (C-ABI wrnn_philox_draws): [steps][rows][K]
    fp32 on cuda:`device`, row j keyed row_offset + j, step s keyed step0 + s — usable as the
    `noise` of the same launch (bit-identical audio).  mode "MOL": U(1e-5, 1 − 1e-5) (K = 11);
    "RAW" / "DM": Exp(1)."""
    m = {"RAW": nat.MODE_RAW, "MOL": nat.MODE_MOL, "DM": nat.MODE_DM}[mode]
    dev = torch.device("cuda", device)
    out = torch.empty(steps, rows, K, dtype=torch.float32, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = nat.lib().wrnn_philox_draws(ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, rows, step0, steps, K, m,
                                     out.data_ptr(), stream)
    if rc != 0:
        raise nat.WrnnError(rc, nat.lib().wrnn_cond_last_error().decode())
    return out


class FatchordLoop:
    keys = LOOP_KEYS

    def __init__(self, mode: str, rnn_dims: int, fc_dims: int, aux_dims: int, feat_dims: int,
                 n_classes: int, device: int = 0, grid: int = 0, timeout_ms: int = 0):
        if mode not in ("RAW", "MOL"):
            raise RuntimeError("Unknown model mode value - ", mode)
        self.mode, self.rnn_dims, self.fc_dims = mode, rnn_dims, fc_dims
        self.aux_dims, self.feat_dims, self.n_classes = aux_dims, feat_dims, n_classes
        self.device = device
        self.cond_dims = feat_dims + 4 * aux_dims
        self.noise_k = noise_width(mode, n_classes)
        # dims that are not multiples of 4 run zero-padded (pad_loop_state; exact)
        self._dims_p = (_round4(rnn_dims), _round4(fc_dims), _round4(aux_dims))
        self._padded = self._dims_p != (rnn_dims, fc_dims, aux_dims)
        Rp, Fp, Ap = self._dims_p
        self._create(nat.Config(nat.ABI_VERSION, nat.MODE_MOL if mode == "MOL" else nat.MODE_RAW, Rp,
                                Fp, Ap, feat_dims, n_classes, grid, timeout_ms), device)

    def _create(self, cfg, device: int) -> None:
        L = nat.lib()
        self._sessions = weakref.WeakSet()   # open FatchordStream sessions
        h = ctypes.c_void_p()
        rc = L.wrnn_create(ctypes.byref(cfg), device, ctypes.byref(h))
        self._h = h
        if rc != 0:
            msg = L.wrnn_last_error(h) if h else b""
            if h:
                L.wrnn_destroy(h)
            self._h = None
            raise nat.WrnnError(rc, (msg or b"").decode())

    # ------------------------------------------------------------------ weights
    def set_weights(self, state: Mapping[str, object]) -> None:
        """Pack the loop's tensors (reference state_dict names) into the kernel layout."""
        if getattr(self, "_padded", False):
            state = pad_loop_state(state, self.rnn_dims, self.fc_dims, self.aux_dims, self.feat_dims, *self._dims_p)
        keep = []
        arr = (nat.Tensor * len(self.keys))()
        n = 0
        for k in self.keys:
            if k not in state:
                raise KeyError(f"missing weight {k!r}")
            v = state[k]
            if isinstance(v, torch.Tensor):
                v = v.detach()
                if v.is_cuda:
                    v = v.to(torch.float32).contiguous()
                    keep.append(v)
                    arr[n] = nat.Tensor(k.encode(), v.data_ptr(), v.numel(), 1)
                    n += 1
                    continue
                v = v.cpu().numpy()
            a = np.ascontiguousarray(v, dtype=np.float32)
            keep.append(a)
            arr[n] = nat.Tensor(k.encode(), a.ctypes.data, a.size, 0)
            n += 1
        nat.check(self._h, nat.lib().wrnn_set_weights(self._h, arr, n))

    # --------------------------------------------------------------------- run
    def generate(self, cond: torch.Tensor, noise: Optional[torch.Tensor] = None, seed: int = 0,
                 row_offset: int = 0, want_labels: bool = False, stream=None,
                 out: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                 check: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """cond [L][B][feat+4·aux] fp32 on this GPU → samples [B][L] (+ labels [B][L] for RAW)."""
        if not (cond.is_cuda and cond.dtype == torch.float32 and cond.is_contiguous()):
            raise ValueError("cond must be a contiguous fp32 CUDA tensor [L][B][C]")
        L, B, C = cond.shape
        if C != self.cond_dims:
            raise ValueError(f"cond has {C} features, expected {self.cond_dims}")
        if getattr(self, "_padded", False) and self._dims_p[2] != self.aux_dims:   # aux chunks a1..a4 zero-padded
            A, Ap, M = self.aux_dims, self._dims_p[2], self.feat_dims
            cp = torch.zeros(L, B, M + 4 * Ap, dtype=cond.dtype, device=cond.device)
            cp[:, :, :M] = cond[:, :, :M]
            for j in range(4):
                cp[:, :, M + j * Ap:M + j * Ap + A] = cond[:, :, M + j * A:M + (j + 1) * A]
            cond = cp
        if noise is not None:
            if not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()):
                raise ValueError("noise must be a contiguous fp32 CUDA tensor [L][B][K]")
            if tuple(noise.shape) != (L, B, self.noise_k):
                raise ValueError(f"noise shape {tuple(noise.shape)} != {(L, B, self.noise_k)}")
        if out is None:
            out = torch.empty(B, L, dtype=torch.float32, device=cond.device)
        if want_labels and labels is None and self.mode == "RAW":
            labels = torch.empty(B, L, dtype=torch.int32, device=cond.device)
        if stream is None:
            stream = torch.cuda.current_stream(cond.device).cuda_stream
        rc = nat.lib().wrnn_generate(self._h, cond.data_ptr(), B, L,
                                     noise.data_ptr() if noise is not None else None,
                                     ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, out.data_ptr(),
                                     labels.data_ptr() if labels is not None else None, stream)
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return out, labels

    def generate_frames(self, spec, mel: torch.Tensor, aux: torch.Tensor, target: int = 0, overlap: int = 0,
                        noise: Optional[torch.Tensor] = None, seed: int = 0, row_offset: Optional[int] = None,
                        want_labels: bool = False, stream=None, check: bool = True,
                        rows: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The loop from the generate() inputs at frame rate (C-ABI wrnn_generate_frames):
        mel [U][feat][T], aux [U][4·aux][T] (MelResNet of the padded mel) fp32 on this GPU, with
        `spec` the UpsampleNetwork's condition.UpsampleSpec → samples [rows][steps] (+ labels),
        rows / steps as condition.upsample_pack would lay them out (target <= 0: unbatched).
        `rows=(begin, count)`: only those rows of the launch (wrnn_generate_frames_rows; e.g. a
        block of one utterance's folds), keyed row_offset + j.  row_offset=None keys launch row
        j as its place in the whole launch (begin + j), so a block reproduces the same rows of
        the whole launch; pass the global row id of `begin` when the launch is itself a shard."""
        for name, t in (("mel", mel), ("aux", aux)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3):
                raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor [U][C][T]")
        U, feat, T = mel.shape
        if feat != self.feat_dims or tuple(aux.shape) != (U, 4 * self.aux_dims, T):
            raise ValueError(f"mel {tuple(mel.shape)} / aux {tuple(aux.shape)} do not match the loop dims")
        if getattr(self, "_padded", False) and self._dims_p[2] != self.aux_dims:   # aux quarters zero-padded
            A, Ap = self.aux_dims, self._dims_p[2]
            ap = torch.zeros(U, 4 * Ap, T, dtype=aux.dtype, device=aux.device)
            for j in range(4):
                ap[:, j * Ap:j * Ap + A] = aux[:, j * A:(j + 1) * A]
            aux = ap
            spec = spec.with_res_out(4 * Ap)
        steps, n_rows = spec.shape(U, T, target, overlap)
        r0, rows = (0, n_rows) if rows is None else (int(rows[0]), int(rows[1]))
        if r0 < 0 or rows < 1 or r0 + rows > n_rows:
            raise ValueError(f"rows [{r0}, {r0 + rows}) outside the launch's {n_rows}")
        if row_offset is None:
            row_offset = r0
        if noise is not None:
            if not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()):
                raise ValueError("noise must be a contiguous fp32 CUDA tensor [L][B][K]")
            if tuple(noise.shape) != (steps, rows, self.noise_k):
                raise ValueError(f"noise shape {tuple(noise.shape)} != {(steps, rows, self.noise_k)}")
        out = torch.empty(rows, steps, dtype=torch.float32, device=mel.device)
        labels = None
        if want_labels and self.mode == "RAW":
            labels = torch.empty(rows, steps, dtype=torch.int32, device=mel.device)
        if stream is None:
            stream = torch.cuda.current_stream(mel.device).cuda_stream
        rc = nat.lib().wrnn_generate_frames_rows(self._h, ctypes.byref(spec.cfg), mel.data_ptr(), aux.data_ptr(), U,
                                                 T, target, overlap, r0, rows,
                                                 noise.data_ptr() if noise is not None else None,
                                                 ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, out.data_ptr(),
                                                 labels.data_ptr() if labels is not None else None, stream)
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return out, labels

    def generate_list(self, spec, mels, auxs, lanes: Optional[int] = None, noise=None, seed: int = 0,
                      row_offset: int = 0, stream=None, check: bool = True) -> list:
        """Whole utterances of unequal length in one call (C-ABI wrnn_generate_list): mels[i]
        [1][feat][T_i] and auxs[i] [1][4·aux][T_i] (its MelResNet output) fp32 on this GPU → the loop
        samples of each, [hop·T_i] fp32 on the GPU, bit for bit what generate_frames(spec, mels[i],
        auxs[i], row_offset=row_offset + i) gives.  The XCDs are `lanes` (1..8, default
        min(8, len(mels))) lanes, each running a queue of utterances back to back inside the
        persistent launch.  `noise`: per-utterance [hop·T_i][11] draws.  Refusals before anything is
        queued raise ValueError (bad arguments) or NotImplementedError (modes / dims without a list
        kernel) and leave the handle as it was."""
        if getattr(self, "_padded", False):
            raise NotImplementedError("lists need rnn / fc / aux dims that are multiples of 4")
        U = len(mels)
        if U < 1 or len(auxs) != U or (noise is not None and len(noise) != U):
            raise ValueError("mels, auxs (and noise) must be non-empty sequences of one length")
        for name, ts, C in (("mel", mels, self.feat_dims), ("aux", auxs, 4 * self.aux_dims)):
            for t in ts:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                        and t.dim() == 3 and t.shape[0] == 1 and t.shape[1] == C):
                    raise ValueError(f"every {name} must be a contiguous fp32 CUDA tensor [1][{C}][T]")
        T = [int(m.shape[2]) for m in mels]
        if any(a.shape[2] != t for a, t in zip(auxs, T)):
            raise ValueError("an aux has another frame count than its mel")
        steps, _ = zip(*[spec.shape(1, max(t, 1), 0, 0) for t in T])
        if noise is not None:
            for i, z in enumerate(noise):
                if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()) or \
                        tuple(z.shape) != (steps[i], self.noise_k):
                    raise ValueError(f"noise[{i}] must be a contiguous fp32 CUDA tensor [{steps[i]}][{self.noise_k}]")
        if lanes is None:
            lanes = min(8, U)
        dev = mels[0].device
        outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in steps]
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        vps = ctypes.c_void_p * U
        rc = nat.lib().wrnn_generate_list(
            self._h, ctypes.byref(spec.cfg), vps(*[m.data_ptr() for m in mels]), vps(*[a.data_ptr() for a in auxs]),
            (ctypes.c_int * U)(*T), U, int(lanes), vps(*[z.data_ptr() for z in noise]) if noise is not None else None,
            ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, vps(*[o.data_ptr() for o in outs]), stream)
        if rc == -6:   # WRNN_EUNSUPPORTED
            raise NotImplementedError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        if rc == -1:   # WRNN_EINVAL: nothing was queued
            raise ValueError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return outs

    def generate_list_wide(self, spec, mels, auxs, slots: Optional[int] = None, noise=None, seed: int = 0,
                           row_offset: int = 0, stream=None, check: bool = True) -> list:
        """generate_list on the many-row kernel (C-ABI wrnn_generate_list_wide): up to 128 slots (16
        per XCD; `slots` 1..128, default min(128, len(mels))), each running a queue of whole
        utterances back to back through the grouped launches of wide sessions; MoL and RAW (9 bits).
        Arguments and result as generate_list; `noise`: per-utterance [hop·T_i][K] draws by the
        utterance's own step (K = 11 MoL, 512 Exp(1) RAW).  Utterance i's samples do not depend on
        the other utterances, their order, `slots` or WRNN_TERMS_MB: they are bit-identical to the
        wide list of utterance i alone with row_offset + i.  MoL: within 2e-5 of the oracle on the
        same draws (not bit-identical to generate_list / generate_frames: another kernel).  RAW: the
        class labels are generate()'s on the same draws bit for bit.  Refusals before anything is
        queued raise ValueError (bad arguments) or NotImplementedError (a loop without the grouped
        many-row form, with wrnn_stream_open_wide's messages) and leave the handle as it was."""
        if getattr(self, "_padded", False):
            raise NotImplementedError("lists need rnn / fc / aux dims that are multiples of 4")
        U = len(mels)
        if U < 1 or len(auxs) != U or (noise is not None and len(noise) != U):
            raise ValueError("mels, auxs (and noise) must be non-empty sequences of one length")
        if slots is not None and not 1 <= int(slots) <= WIDE_ROWS:
            raise ValueError(f"slots is 1..{WIDE_ROWS} (16 per XCD), not {slots!r}")
        for name, ts, C in (("mel", mels, self.feat_dims), ("aux", auxs, 4 * self.aux_dims)):
            for t in ts:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                        and t.dim() == 3 and t.shape[0] == 1 and t.shape[1] == C):
                    raise ValueError(f"every {name} must be a contiguous fp32 CUDA tensor [1][{C}][T]")
        T = [int(m.shape[2]) for m in mels]
        if any(a.shape[2] != t for a, t in zip(auxs, T)):
            raise ValueError("an aux has another frame count than its mel")
        steps, _ = zip(*[spec.shape(1, max(t, 1), 0, 0) for t in T])
        if noise is not None:
            for i, z in enumerate(noise):
                if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()) or \
                        tuple(z.shape) != (steps[i], self.noise_k):
                    raise ValueError(f"noise[{i}] must be a contiguous fp32 CUDA tensor [{steps[i]}][{self.noise_k}]")
        dev = mels[0].device
        outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in steps]
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        vps = ctypes.c_void_p * U
        rc = nat.lib().wrnn_generate_list_wide(
            self._h, ctypes.byref(spec.cfg), vps(*[m.data_ptr() for m in mels]), vps(*[a.data_ptr() for a in auxs]),
            (ctypes.c_int * U)(*T), U, 0 if slots is None else int(slots),
            vps(*[z.data_ptr() for z in noise]) if noise is not None else None,
            ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, vps(*[o.data_ptr() for o in outs]), stream)
        if rc == -6:   # WRNN_EUNSUPPORTED
            raise NotImplementedError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        if rc == -1:   # WRNN_EINVAL: nothing was queued
            raise ValueError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return outs

    def generate_list_folds(self, spec, mels, auxs, target: int = 11000, overlap: int = 550,
                            slots: Optional[int] = None, noise=None, seed: int = 0, row_offset: int = 0, stream=None,
                            check: bool = True) -> list:
        """A list of unequal utterances fold-batched on the many-row kernel (C-ABI
        wrnn_generate_list_folds): every utterance is cut into folds of target + 2·overlap steps and
        the folds of all utterances, numbered utterance-major, run as the rows of the grouped launches
        — fold g in round g // slots as launch row g % slots (`slots` 1..128, default min(128, folds)).
        mels / auxs as generate_list_wide → per utterance the fold outputs [folds_i][target + 2·overlap]
        fp32 on the GPU, the rows generate_frames(spec, mels[i], auxs[i], target, overlap,
        row_offset=row_offset + first_row[i]) runs (RAW: bit for bit on the same draws; MoL: another
        instantiation of the kernel, within the wide bound).  `noise`: per-utterance
        [target + 2·overlap][folds_i][K] draws, generate_frames' layout for that utterance alone.
        Utterance i's output does not depend on the other utterances, their order, `slots` or
        WRNN_TERMS_MB.  Refusals before anything is queued raise ValueError (bad arguments) or
        NotImplementedError (a loop without the grouped many-row form) and leave the handle as it was."""
        if getattr(self, "_padded", False):
            raise NotImplementedError("lists need rnn / fc / aux dims that are multiples of 4")
        U = len(mels)
        if U < 1 or len(auxs) != U or (noise is not None and len(noise) != U):
            raise ValueError("mels, auxs (and noise) must be non-empty sequences of one length")
        if slots is not None and not 1 <= int(slots) <= WIDE_ROWS:
            raise ValueError(f"slots is 1..{WIDE_ROWS} (16 per XCD), not {slots!r}")
        for name, ts, C in (("mel", mels, self.feat_dims), ("aux", auxs, 4 * self.aux_dims)):
            for t in ts:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                        and t.dim() == 3 and t.shape[0] == 1 and t.shape[1] == C):
                    raise ValueError(f"every {name} must be a contiguous fp32 CUDA tensor [1][{C}][T]")
        T = [int(m.shape[2]) for m in mels]
        if any(a.shape[2] != t for a, t in zip(auxs, T)):
            raise ValueError("an aux has another frame count than its mel")
        target, overlap = int(target), int(overlap)
        try:
            folds, _, _ = list_folds_plan(T, spec.hop, target, overlap, slots, raw=self.mode == "RAW")
        except nat.WrnnError as e:
            raise ValueError(str(e)) from None
        Lf = target + 2 * overlap
        if noise is not None:
            for i, z in enumerate(noise):
                if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()) or \
                        tuple(z.shape) != (Lf, folds[i], self.noise_k):
                    raise ValueError(f"noise[{i}] must be a contiguous fp32 CUDA tensor [{Lf}][{folds[i]}][{self.noise_k}]")
        dev = mels[0].device
        outs = [torch.empty(n, Lf, dtype=torch.float32, device=dev) for n in folds]
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        vps = ctypes.c_void_p * U
        rc = nat.lib().wrnn_generate_list_folds(
            self._h, ctypes.byref(spec.cfg), vps(*[m.data_ptr() for m in mels]), vps(*[a.data_ptr() for a in auxs]),
            (ctypes.c_int * U)(*T), U, target, overlap, 0 if slots is None else int(slots),
            vps(*[z.data_ptr() for z in noise]) if noise is not None else None,
            ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, vps(*[o.data_ptr() for o in outs]), stream)
        if rc == -6:   # WRNN_EUNSUPPORTED
            raise NotImplementedError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        if rc == -1:   # WRNN_EINVAL: nothing was queued
            raise ValueError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return outs

    def push_streams(self, pushes, stream=None, check: bool = True) -> list:
        """Advance several sessions of this loop in one call (C-ABI wrnn_stream_push_group): `pushes`
        is a sequence of (FatchordStream, mel or None, final), each member with its own frames and
        its own end — what FatchordStream.push gives for each, bit for bit, but with one persistent
        launch per time chunk for all of them, every row on its own XCD.  The members' rows together
        are at most 8 — or, when every member is a wide session (FatchordStream(wide=True)), at
        most 128, 16 per XCD on the many-row kernel; wide and narrow members do not mix.  → the new
        audio per member, float64 [U_i][m_i] on the GPU.  Refusals (ValueError with the library's
        message) leave every member unchanged."""
        members = []
        for item in pushes:
            if not isinstance(item, (tuple, list)) or len(item) != 3:
                raise ValueError("pushes holds (FatchordStream, mel or None, final) tuples")
            s, mel, final = item
            if not isinstance(s, FatchordStream):
                raise ValueError("pushes holds (FatchordStream, mel or None, final) tuples")
            if s._s is None:
                raise ValueError("a member session is closed")
            if s.loop is not self:
                raise ValueError("a member session belongs to another loop")
            if s.finished:
                raise ValueError("push after finish(): a member session has ended")
            members.append((s, mel, s._frames_of(mel), bool(final)))
        if not members:
            raise ValueError("push_streams needs at least one member")
        if any(getattr(s, "rows", False) for s, _, _, _ in members):
            raise ValueError("a rows session advances alone: its kernel steps all rows in lock step")
        if any(s.wide != members[0][0].wide for s, _, _, _ in members):
            raise ValueError("a group holds wide sessions or narrow ones, not both: they run different loop kernels")
        rows = sum(s.n_streams for s, _, _, _ in members)
        if members[0][0].wide and rows > WIDE_ROWS:
            raise ValueError(f"a wide group has at most {WIDE_ROWS} rows (16 per XCD): these members have {rows}")
        waves, plan = [], []
        for s, mel, n, final in members:
            try:
                m = s.plan(s.frames + n, final) - s.plan(s.frames)
            except nat.WrnnError as e:
                raise ValueError(str(e)) from None
            plan.append(m)
            waves.append(torch.empty(s.n_streams, m, dtype=torch.float64, device=s.device))
        count = len(members)
        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        vps, ints = ctypes.c_void_p * count, ctypes.c_int * count
        got = ints()
        rc = nat.lib().wrnn_stream_push_group(
            vps(*[s._s.value for s, _, _, _ in members]), count,
            vps(*[mel.data_ptr() if n else None for _, mel, n, _ in members]), ints(*[n for _, _, n, _ in members]),
            ints(*[int(f) for _, _, _, f in members]), vps(*[w.data_ptr() if m else None for w, m in zip(waves, plan)]),
            ints(*plan), got, stream)
        if rc == -1:   # WRNN_EINVAL: nothing was queued, every member is as before
            raise ValueError((nat.lib().wrnn_last_error(self._h) or b"").decode(errors="replace"))
        nat.check(self._h, rc)
        assert list(got) == plan, (list(got), plan)
        for s, _, n, final in members:
            s.frames += n
            s.finished = final
        if check:
            self.check(stream)
        return waves

    def check(self, stream=None) -> None:
        """Synchronise and raise if the persistent kernel aborted (timeout)."""
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        nat.check(self._h, nat.lib().wrnn_check(self._h, stream))

    def elapsed_ms(self) -> float:
        """Device time of the persistent loop launch(es) of the last generate() (HIP events)."""
        ms = ctypes.c_float()
        nat.check(self._h, nat.lib().wrnn_elapsed_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    @property
    def info(self) -> dict:
        i = nat.Info()
        nat.check(self._h, nat.lib().wrnn_query(self._h, ctypes.byref(i)))
        return {f: getattr(i, f) for f, _ in nat.Info._fields_}

    def close(self) -> None:
        for s in list(getattr(self, "_sessions", ())):   # a session must not outlive its handle
            s.close()
        if getattr(self, "_h", None):
            nat.lib().wrnn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_plan(spec, frames_received: int, final: bool = False, total_frames: Optional[int] = None) -> Tuple[int, int]:
    """(steps_done, audio_done) of a streaming session after `frames_received` mel frames (C-ABI
    wrnn_stream_plan, host only): the emission rule of include/wavernn_amd.h.  `spec` is the
    condition.UpsampleSpec (only its scales and pad count).  Raises WrnnError(WRNN_EINVAL) where a
    push would: final with fewer than 21 frames, or a count other than total_frames."""
    steps, audio = ctypes.c_int64(), ctypes.c_int64()
    nat.check_cond(nat.lib().wrnn_stream_plan(ctypes.byref(spec.cfg), frames_received, int(final),
                                              -1 if total_frames is None else int(total_frames),
                                              ctypes.byref(steps), ctypes.byref(audio)))
    return steps.value, audio.value


WIDE_ROWS = 128   # rows of a wide session or group: 16 per XCD (csrc/fatchord_xcdm.h: kMRowsMax)


def wide_plan(steps, rows, steps_per_launch: int) -> list:
    """The round plan of a wide group push (C-ABI wrnn_wide_plan, host only): members with
    `steps[i]` runnable steps and `rows[i]` rows are cut into rounds at the distinct step counts in
    ascending order, every round into launches of at most `steps_per_launch` steps → one
    (first launch-local step, steps, [(member, utterance, xcd, slot) per launch row]) per persistent
    launch: the surviving members' rows in member order, launch row r on XCD r % 8, slot r // 8.
    Raises WrnnError(WRNN_EINVAL) on negative steps, rows < 1 or more than 128 rows."""
    steps, rows = [int(x) for x in steps], [int(x) for x in rows]
    if len(steps) != len(rows):
        raise ValueError("steps and rows have one entry per member")
    n = max(len(steps), 1)
    ints = ctypes.c_int * n
    args = (ints(*steps), ints(*rows), len(steps), int(steps_per_launch))
    count = nat.lib().wrnn_wide_plan(*args, None, None, None, 0)
    if count < 0:
        nat.check_cond(count)
    cap = max(count, 1)
    first, ls, lr = (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    nat.check_cond(min(0, nat.lib().wrnn_wide_plan(*args, first, ls, lr, cap)))
    plan = []
    for j in range(count):
        live = [(i, u) for i in range(len(steps)) if steps[i] > first[j] for u in range(rows[i])]
        assert len(live) == lr[j], (j, len(live), lr[j])
        plan.append((first[j], ls[j], [(i, u, r % 8, r // 8) for r, (i, u) in enumerate(live)]))
    return plan


def wide_steps_per_launch(rows: int, longest_steps: int, raw: bool = False) -> int:
    """Steps per persistent launch of a wide push with `rows` rows to run, the longest member
    `longest_steps` steps (C-ABI wrnn_wide_steps_per_launch, host only; reads WRNN_TERMS_MB as the
    push does): the terms budget over rows · 4608 floats per step, for a RAW loop over
    rows · (4608 + 512) — its draws share the budget.  The steps_per_launch of wide_plan."""
    n = nat.lib().wrnn_wide_steps_per_launch(int(rows), int(longest_steps), int(bool(raw)))
    if n < 0:
        nat.check_cond(n)
    return n


def list_plan(frames, lanes: Optional[int] = None) -> Tuple[list, list, list]:
    """The lane schedule of a list call (C-ABI wrnn_list_plan, host only): (lane_of, pos_in_lane,
    lane_frames) for utterances of `frames` frames on `lanes` lanes (default min(8, len(frames))):
    longest first, each to the least loaded lane, ties to the lower index / lowest lane.
    lane_frames[k] is lane k's timeline in frames (× hop: steps).  Raises WrnnError(WRNN_EINVAL)
    for an empty list, lanes outside 1..8 or an utterance under 21 frames."""
    frames = [int(f) for f in frames]
    U = len(frames)
    if lanes is None:
        lanes = min(8, U)
    n = max(U, 1)
    lane_of, pos = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    steps = (ctypes.c_int64 * max(int(lanes), 8))()
    nat.check_cond(nat.lib().wrnn_list_plan((ctypes.c_int * n)(*frames), U, int(lanes), lane_of, pos, steps))
    return list(lane_of)[:U], list(pos)[:U], list(steps)[:lanes]


def list_wide_plan(frames, slots: Optional[int] = None, hop: int = 275, raw: bool = False) -> Tuple[list, list, list, list]:
    """The schedule of a wide list call (C-ABI wrnn_list_wide_plan, host only): (slot_of, pos_in_slot,
    slot_frames, launches) for utterances of `frames` frames on `slots` many-row slots (1..128,
    default min(128, len(frames))) at `hop` steps per frame.  The assignment is list_plan's rule;
    `launches` holds one (first timeline step, steps, rows) per persistent launch: the common timeline
    cut at every utterance end on any slot and again at wide_steps_per_launch(rows, longest timeline,
    raw) steps, the rows of a launch the slots that still have a step to run, in slot order.  Raises
    WrnnError(WRNN_EINVAL) for an empty list, slots outside 1..128, hop < 1 or an utterance under 21
    frames."""
    frames = [int(f) for f in frames]
    U = len(frames)
    if slots is None:
        slots = min(WIDE_ROWS, max(U, 1))
    slots = int(slots)
    n = max(U, 1)
    slot_of, pos = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    sf = (ctypes.c_int64 * max(slots, WIDE_ROWS))()
    args = ((ctypes.c_int * n)(*frames), U, slots, int(hop), int(bool(raw)), slot_of, pos, sf)
    count = nat.lib().wrnn_list_wide_plan(*args, None, None, None, 0)
    if count < 0:
        nat.check_cond(count)
    first, ls, lr = (ctypes.c_int * count)(), (ctypes.c_int * count)(), (ctypes.c_int * count)()
    nat.check_cond(min(0, nat.lib().wrnn_list_wide_plan(*args, first, ls, lr, count)))
    return list(slot_of)[:U], list(pos)[:U], list(sf)[:slots], list(zip(first, ls, lr))


def list_folds_plan(frames, hop: int = 275, target: int = 11000, overlap: int = 550, slots: Optional[int] = None,
                    raw: bool = False) -> Tuple[list, list, list]:
    """The schedule of a folded list call (C-ABI wrnn_list_folds_plan, host only): (folds, first_row,
    launches) for utterances of `frames` frames at `hop` steps per frame, cut into folds of
    target + 2·overlap steps.  folds[i] is utterance i's fold count (what UpsampleSpec.shape gives),
    first_row[i] the number of its first fold in the utterance-major numbering; fold g runs in round
    g // slots as launch row g % slots (`slots` 1..128, default min(128, all folds)).  `launches`
    holds one (first step on the common timeline, steps, rows) per persistent launch: round q covers
    steps [q·Lf, (q + 1)·Lf) with Lf = target + 2·overlap, cut at wide_steps_per_launch(rows of the
    round, Lf, raw) steps.  Raises WrnnError(WRNN_EINVAL) for an empty list, slots outside 1..128,
    hop < 1, target < 1, overlap < 0, an utterance under 21 frames or shorter than the overlap, or
    counts past 32 bits."""
    if slots is not None and int(slots) == 0:     # the C entry's 0 is this function's None
        raise nat.WrnnError(-1, f"slots is 1..{WIDE_ROWS} (16 per XCD)")
    frames = [int(f) for f in frames]
    U = len(frames)
    n = max(U, 1)
    folds, first = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    args = ((ctypes.c_int * n)(*frames), U, int(hop), int(target), int(overlap), 0 if slots is None else int(slots),
            int(bool(raw)), folds, first)
    count = nat.lib().wrnn_list_folds_plan(*args, None, None, None, 0)
    if count < 0:
        nat.check_cond(count)
    lf, ls, lr = (ctypes.c_int * count)(), (ctypes.c_int * count)(), (ctypes.c_int * count)()
    nat.check_cond(min(0, nat.lib().wrnn_list_folds_plan(*args, lf, ls, lr, count)))
    return list(folds)[:U], list(first)[:U], list(zip(lf, ls, lr))


def stream_lookahead(spec) -> int:
    """Frames a session holds back before it runs a frame's samples (pad + 1)."""
    n = nat.lib().wrnn_stream_lookahead(ctypes.byref(spec.cfg))
    if n < 0:
        nat.check_cond(n)
    return n


class FatchordStream:
    """A streaming session on a FatchordLoop (C-ABI wrnn_stream_*): `n_streams` utterances in lock
    step (the same frames in the same push, one total, one end; FatchordLoop.push_streams advances
    several sessions at once, each at its own pace), mel frames pushed as they arrive, float64 audio
    returned as soon as it is final.  The
    recurrent state, frame-term stores and mel tail live on the GPU in the session, so one-shot
    generate() calls and other sessions on the same loop may run between pushes.  Dims or modes
    the session kernels do not cover raise NotImplementedError with the library's message.

    `wide=True` opens the session on the many-row kernel (C-ABI wrnn_stream_open_wide, last_path
    7): `n_streams` 1..128, and groups of wide sessions hold up to 128 rows.  A wide member's audio
    is bit-identical whatever its company (every wide launch is the kernel's four-quad form, whose
    batch rows are independent MFMA columns) and lies within the project's bound of the oracle; it
    is NOT bit-identical to the same session opened narrow, which runs another kernel.

    A RAW loop (9 bits, rnn / fc 512) opens wide sessions only: `noise` is then
    [steps][n_streams][512] Exp(1) draws by absolute step (generate()'s layout), the class labels
    are those of generate() on the same draws bit for bit, and `mu_law=True` expands the emitted
    samples (C-ABI wrnn_stream_mu_law; ignored on a MoL loop; set_mu_law() changes it before the
    first push).

    `rows=True` opens the session on the multi-row kernel (C-ABI wrnn_stream_open_rows, last_path 2,
    or 9 with streamed weights): any MoL or RAW loop the kernel runs, whatever its rnn / fc dims and
    class count, `n_streams` up to one row block of it (the library states the limit).  `noise` is
    [steps][n_streams][loop.noise_k] by absolute step; `mu_law` as for wide RAW sessions.  A rows
    session advances alone: push_streams refuses it."""

    def __init__(self, loop: FatchordLoop, spec, mr_cfg, mr_packed: torch.Tensor, n_streams: int = 1,
                 total_frames: Optional[int] = None, noise: Optional[torch.Tensor] = None, seed: int = 0,
                 row_offset: int = 0, wide: bool = False, mu_law: bool = False, rows: bool = False):
        self._s = None
        self.wide = bool(wide)
        self.rows = bool(rows)
        if self.rows and self.wide:
            raise ValueError("rows=True and wide=True name two kernels: a session runs on one")
        if self.wide and not 1 <= int(n_streams) <= WIDE_ROWS:
            raise ValueError(f"a wide session has 1..{WIDE_ROWS} utterances, not {n_streams!r}")
        if getattr(loop, "_padded", False):
            raise NotImplementedError("streaming sessions need rnn / fc / aux dims that are multiples of 4")
        if noise is not None:
            if not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()) or \
                    noise.dim() != 3 or tuple(noise.shape[1:]) != (n_streams, loop.noise_k):
                raise ValueError(f"noise must be a contiguous fp32 CUDA tensor [steps][{n_streams}][{loop.noise_k}]")
        if not (mr_packed.is_cuda and mr_packed.dtype == torch.float32 and mr_packed.is_contiguous()):
            raise ValueError("the packed MelResNet weights must be a contiguous fp32 CUDA tensor")
        self.loop, self.spec, self.n_streams, self.total_frames = loop, spec, n_streams, total_frames
        self._keep = (mr_packed, noise, mr_cfg)        # the session reads them until close()
        self.device = torch.device("cuda", loop.device)
        self.frames, self.finished = 0, False
        self.lookahead_frames = stream_lookahead(spec)
        s = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            opener = nat.lib().wrnn_stream_open_rows if self.rows else \
                nat.lib().wrnn_stream_open_wide if self.wide else nat.lib().wrnn_stream_open
            rc = opener(loop._h, ctypes.byref(spec.cfg), ctypes.byref(mr_cfg), mr_packed.data_ptr(),
                                            n_streams, -1 if total_frames is None else int(total_frames),
                                            noise.data_ptr() if noise is not None else None,
                                            noise.shape[0] if noise is not None else 0,
                                            ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, ctypes.byref(s))
        if rc == -6:   # WRNN_EUNSUPPORTED
            raise NotImplementedError((nat.lib().wrnn_last_error(loop._h) or b"").decode(errors="replace"))
        if rc == -1:   # WRNN_EINVAL
            raise ValueError((nat.lib().wrnn_last_error(loop._h) or b"").decode(errors="replace"))
        nat.check(loop._h, rc)
        self._s = s
        loop._sessions.add(self)
        if mu_law and loop.mode == "RAW":
            self.set_mu_law(True)

    def set_mu_law(self, on: bool) -> None:
        """Mu-law expansion of the emitted samples (C-ABI wrnn_stream_mu_law): a RAW session, before
        its first push.  ValueError (the session unchanged) on a MoL session or after a push."""
        if self._s is None:
            raise RuntimeError("the session is closed")
        rc = nat.lib().wrnn_stream_mu_law(self._s, int(bool(on)))
        if rc == -1:   # WRNN_EINVAL
            raise ValueError((nat.lib().wrnn_last_error(self.loop._h) or b"").decode(errors="replace"))
        nat.check(self.loop._h, rc)

    def plan(self, frames: int, final: bool = False) -> int:
        """Samples per utterance the session will have emitted in all once `frames` frames are in."""
        return stream_plan(self.spec, frames, final, self.total_frames)[1]

    def _frames_of(self, mel: Optional[torch.Tensor]) -> int:
        """The frame count of a push's mel (None: 0), after checking its layout."""
        if mel is None:
            return 0
        if not (isinstance(mel, torch.Tensor) and mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous()
                and mel.dim() == 3) or tuple(mel.shape[:2]) != (self.n_streams, self.loop.feat_dims):
            raise ValueError(f"mel must be a contiguous fp32 CUDA tensor [{self.n_streams}][{self.loop.feat_dims}][n]")
        return mel.shape[2]

    def push(self, mel: Optional[torch.Tensor], final: bool = False, stream=None, check: bool = True) -> torch.Tensor:
        """mel [U][feat][n] fp32 on the loop's GPU (None: no frames) → the new audio, float64 [U][m]
        on the GPU (m may be 0).  Asynchronous on `stream` when check=False."""
        if self._s is None:
            raise RuntimeError("the session is closed")
        if self.finished:
            raise RuntimeError("push after finish(): the session has ended")
        n = self._frames_of(mel)
        try:
            m = self.plan(self.frames + n, final) - self.plan(self.frames)
        except nat.WrnnError as e:
            raise ValueError(str(e)) from None
        wave = torch.empty(self.n_streams, m, dtype=torch.float64, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        got = ctypes.c_int()
        rc = nat.lib().wrnn_stream_push(self._s, mel.data_ptr() if n else None, n, int(final),
                                        wave.data_ptr() if m else None, m, ctypes.byref(got), stream)
        nat.check(self.loop._h, rc)
        assert got.value == m, (got.value, m)
        self.frames += n
        self.finished = bool(final)
        if check:
            self.loop.check(stream)
        return wave

    def close(self) -> None:
        if getattr(self, "_s", None) is not None:
            nat.lib().wrnn_stream_close(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeepmindLoop(FatchordLoop):
    """Handle on the dual-softmax kernels replacing the per-step loop of
    models/deepmind_version.py:generate (:98-156) for B independent rows: deepmind_xcd.hip
    (hidden 896 / quantisation 256: 4 rows per XCD, 32 per launch, info["last_path"] 8) or
    deepmind_rows.hip (other dims, or WRNN_PATH=rows: path 3)."""
    keys = DM_KEYS

    def __init__(self, hidden_size: int = 896, quantisation: int = 256, device: int = 0, grid: int = 0,
                 timeout_ms: int = 0):
        self.mode, self.hidden_size, self.n_classes = "DM", hidden_size, quantisation
        self.device = device
        self.noise_k = 2 * quantisation
        self._create(nat.Config(nat.ABI_VERSION, nat.MODE_DM, hidden_size, 0, 0, 0, quantisation, grid, timeout_ms),
                     device)

    def generate(self, B: int, L: int, noise: Optional[torch.Tensor] = None, seed: int = 0, row_offset: int = 0,
                 stream=None, check: bool = True,
                 device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """→ (samples [B][L] fp32, combined int32 [B][L]): coarse·256 + fine − 2^15 per step."""
        dev = device or torch.device("cuda", self.device)
        if noise is not None:
            if not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()):
                raise ValueError("noise must be a contiguous fp32 CUDA tensor [L][B][2Q]")
            if tuple(noise.shape) != (L, B, self.noise_k):
                raise ValueError(f"noise shape {tuple(noise.shape)} != {(L, B, self.noise_k)}")
        out = torch.empty(B, L, dtype=torch.float32, device=dev)
        labels = torch.empty(B, L, dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        rc = nat.lib().wrnn_generate(self._h, None, B, L, noise.data_ptr() if noise is not None else None,
                                     ctypes.c_uint64(seed & (2 ** 64 - 1)), row_offset, out.data_ptr(),
                                     labels.data_ptr(), stream)
        nat.check(self._h, rc)
        if check:
            self.check(stream)
        return out, labels
