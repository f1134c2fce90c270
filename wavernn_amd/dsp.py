"""Audio helpers of the reference's utils/dsp.py: everything generate(), gen_wavernn.py and the
training data path touch without librosa (mu-law, labels, 16-bit split, wav I/O, dB scaling,
emphasis filters), and its melspectrogram(): on a GPU the HIP kernel of csrc/melspec.hip, without
one a float32 numpy/scipy path of the same definition.  That definition is librosa's published
one restated (pinned to tests/melspec_ref.py, not to librosa's output, which no
build of this project can run).  Griffin-Lim and spectrogram() stay out of scope (SURVEY.md §2
row 4)."""
from __future__ import annotations

import math
from pathlib import Path
from typing import Union

import numpy as np


def label_2_float(x, bits):
    """utils/dsp.py:8-9: class label in [0, 2**bits) → [-1, 1]."""
    return 2 * x / (2 ** bits - 1.) - 1.


def float_2_label(x, bits):
    """utils/dsp.py:12-15."""
    assert abs(x).max() <= 1.0
    x = (x + 1.) * (2 ** bits - 1) / 2
    return x.clip(0, 2 ** bits - 1)


def encode_mu_law(x, mu):
    """utils/dsp.py:92-95."""
    mu = mu - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    return np.floor((fx + 1) / 2 * mu + 0.5)


def decode_mu_law(y, mu, from_labels=True):
    """utils/dsp.py:98-103 (float64 like the reference's post-processing)."""
    if from_labels:
        y = label_2_float(y, math.log2(mu))
    mu = mu - 1
    return np.sign(y) / mu * ((1 + mu) ** np.abs(y) - 1)


def split_signal(x):
    """utils/dsp.py:26-30: 16-bit → (coarse, fine) 8-bit halves."""
    unsigned = x + 2 ** 15
    return unsigned // 256, unsigned % 256


def combine_signal(coarse, fine):
    """utils/dsp.py:33-34 (deepmind dual-softmax output)."""
    return coarse * 256 + fine - 2 ** 15


def save_wav(x: np.ndarray, path: Union[str, Path, None], sample_rate: int = 22050) -> None:
    """utils/dsp.py:22-23 wrote float32 samples with librosa.output.write_wav (removed in
    librosa >= 0.8); the same IEEE-float WAV is written with scipy.  path None → no file."""
    if path is None:
        return
    from scipy.io import wavfile
    wavfile.write(str(path), int(sample_rate), np.asarray(x, dtype=np.float32))


def load_wav(path: Union[str, Path], sample_rate: int = 22050) -> np.ndarray:
    """utils/dsp.py:18-19 (librosa.load(path, sr)[0]): float32 mono in [-1, 1].  Integer PCM is
    scaled by its full-scale value and channels are averaged, as librosa does; a file at another
    rate raises (librosa's resampler is not in this image, so a resampled result would be
    unpinned)."""
    from scipy.io import wavfile
    sr, x = wavfile.read(str(path))
    if sr != sample_rate:
        raise ValueError(f"{path}: sample rate {sr} != {sample_rate} (resampling not supported)")
    if np.issubdtype(x.dtype, np.integer):
        if x.dtype == np.uint8:
            x = (x.astype(np.float32) - 128.0) / 128.0
        else:
            x = x.astype(np.float32) / float(-np.iinfo(x.dtype).min)
    x = np.asarray(x, dtype=np.float32)
    return x.mean(axis=1, dtype=np.float32) if x.ndim == 2 else x


def encode_16bits(x):
    """utils/dsp.py:37-38."""
    return np.clip(x * 2 ** 15, -2 ** 15, 2 ** 15 - 1).astype(np.int16)


def normalize(S, min_level_db: float = -100):
    """utils/dsp.py:50-51 (min_level_db = hp.min_level_db)."""
    return np.clip((S - min_level_db) / -min_level_db, 0, 1)


def denormalize(S, min_level_db: float = -100):
    """utils/dsp.py:54-55."""
    return (np.clip(S, 0, 1) * -min_level_db) + min_level_db


def amp_to_db(x):
    """utils/dsp.py:58-59."""
    return 20 * np.log10(np.maximum(1e-5, x))


def db_to_amp(x):
    """utils/dsp.py:62-63."""
    return np.power(10.0, x * 0.05)


def pre_emphasis(x, preemphasis: float = 0.97):
    """utils/dsp.py:84-85 (first-order FIR 1 - p·z⁻¹).  The reference reads hp.preemphasis,
    which its hparams.py does not define: callers pass the coefficient."""
    from scipy.signal import lfilter
    return lfilter([1, -preemphasis], [1], x)


def de_emphasis(x, preemphasis: float = 0.97):
    """utils/dsp.py:88-89 (the inverse IIR)."""
    from scipy.signal import lfilter
    return lfilter([1], [1, -preemphasis], x)


# ------------------------------------------------------------------ mel front end (utils/dsp.py:41-81)
MELSPEC_KEYS = ("sample_rate", "n_fft", "hop_length", "win_length", "num_mels", "fmin", "min_level_db")


def melspec_params(hp=None, **overrides) -> dict:
    """The front end's seven parameters from an HParams, a mapping or None (hparams.DEFAULTS)."""
    from .hparams import DEFAULTS
    out = {k: DEFAULTS[k] for k in MELSPEC_KEYS}
    if hp is not None:
        for k in MELSPEC_KEYS:
            if isinstance(hp, dict):
                out[k] = hp.get(k, out[k])
            else:
                out[k] = getattr(hp, k, out[k])
    out.update({k: v for k, v in overrides.items() if v is not None})
    return out


def stft_window(n_fft: int = 2048, win_length: int = 1100) -> np.ndarray:
    """float64 [n_fft]: scipy.signal.get_window('hann', win_length, fftbins=True) (periodic), centred
    in n_fft as librosa's pad_center does: (n_fft − win_length)//2 zeros on the left."""
    n = np.arange(win_length, dtype=np.float64)
    left = (n_fft - win_length) // 2
    return np.pad(0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length), (left, n_fft - win_length - left))


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, (200.0 / 3.0) * m, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_basis(sample_rate: int = 22050, n_fft: int = 2048, num_mels: int = 80, fmin: float = 40.0) -> np.ndarray:
    """float64 [num_mels][n_fft//2 + 1]: librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax=sr/2,
    htk=False, norm='slaney') from its definition — triangles between num_mels + 2 points equally
    spaced on the Slaney mel scale, each scaled by 2 / (its width in Hz)."""
    fmax = sample_rate / 2.0
    mf = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), num_mels + 2))
    freqs = np.linspace(0.0, fmax, n_fft // 2 + 1)
    fdiff = np.diff(mf)
    ramps = mf[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mf[2:] - mf[:-2]))[:, None]


def melspec_frames(n_samples: int, hop_length: int = 275) -> int:
    return 1 + int(n_samples) // int(hop_length)


def _melspectrogram_host(y: np.ndarray, p: dict) -> np.ndarray:
    """The definition in float32 on the host (scipy.fft keeps single precision)."""
    import scipy.fft
    n_fft, hop = int(p["n_fft"]), int(p["hop_length"])
    y = np.asarray(y, dtype=np.float32)
    if y.ndim != 1 or len(y) < n_fft // 2 + 1:
        raise ValueError(f"melspectrogram needs a 1-D signal of at least n_fft//2 + 1 = {n_fft // 2 + 1} samples")
    yp = np.pad(y, n_fft // 2, mode="reflect")
    T = melspec_frames(len(y), hop)
    frames = np.lib.stride_tricks.sliding_window_view(yp, n_fft)[::hop][:T]
    D = np.abs(scipy.fft.rfft(frames * stft_window(n_fft, int(p["win_length"])).astype(np.float32), axis=1))
    W = mel_basis(int(p["sample_rate"]), n_fft, int(p["num_mels"]), float(p["fmin"])).astype(np.float32)
    S = W @ D.astype(np.float32).T
    db = np.float32(20.0) * np.log10(np.maximum(np.float32(1e-5), S))
    mdb = np.float32(p["min_level_db"])
    return np.clip((db - mdb) / -mdb, 0, 1).astype(np.float32)


def melspectrogram(y, hp=None, device=None) -> np.ndarray:
    """utils/dsp.py:75-78: wav (1-D, float) → normalised mel float32 (num_mels, 1 + len(y)//hop), what
    generate() and gen_wavernn's load_mel take.  `hp`: an HParams, a mapping, or None for the
    defaults.  With a GPU (device None: when torch sees one) the HIP kernel computes it
    (wavernn_amd.melspec.MelSpec); without one, or with device='cpu', the float32 host path of the
    same definition.  The two agree to float32 rounding of the definition, not bit for bit."""
    p = melspec_params(hp)
    if device is None:
        import torch
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if str(device).startswith("cpu"):
        return _melspectrogram_host(np.asarray(y), p)
    from .melspec import MelSpec
    return MelSpec.get(p, device).run([y])[0].cpu().numpy()
