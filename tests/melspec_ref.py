"""The mel front end's definition, restated in float64 (the pin of wavernn_amd/csrc/melspec.hip and
wavernn_amd.dsp.melspectrogram).  The reference's utils/dsp.py:41-81 calls librosa, which is not
available to this project's builds: this file states librosa's published definitions (reflect-padded
centred STFT, periodic Hann window zero-padded to n_fft, Slaney-scale area-normalised mel filterbank)
with numpy and scipy.fft only, one step per function, frame by frame.  It is the reference of the
tests, written apart from wavernn_amd.dsp's table builders, which the tests compare with it.

`dtype=np.float32` runs the same steps in single precision (tables rounded once, float32 FFT and
sums): the float32 error of the definition itself, from which the GPU tests derive their tolerance."""
import math

import numpy as np
import scipy.fft

DEFAULT = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=40.0,
               min_level_db=-100.0)
SMALL = dict(sample_rate=8000, n_fft=256, hop_length=64, win_length=200, num_mels=20, fmin=0.0, min_level_db=-100.0)


def n_frames(n_samples, hop_length):
    return 1 + n_samples // hop_length


def reflect_pad(y, p):
    """yp[-k] = y[k], yp[N - 1 + k] = y[N - 1 - k]: the edge sample is not repeated."""
    y = np.asarray(y)
    assert y.ndim == 1 and len(y) >= p + 1
    return np.concatenate([y[1:p + 1][::-1], y, y[-p - 1:-1][::-1]])


def window(n_fft, win_length):
    """Periodic Hann of win_length, (n_fft - win_length)//2 zeros on its left, the rest on its right."""
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    for n in range(win_length):
        w[left + n] = 0.5 - 0.5 * math.cos(2.0 * math.pi * n / win_length)
    return w


def stft_mag(y, n_fft, hop_length, win_length, dtype=np.float64):
    """|rfft(frame · window)| → (n_fft//2 + 1, T)."""
    yp = reflect_pad(np.asarray(y, dtype=dtype), n_fft // 2)
    w = window(n_fft, win_length).astype(dtype)
    T = n_frames(len(y), hop_length)
    out = np.empty((n_fft // 2 + 1, T), dtype=dtype)
    for t in range(T):
        frame = yp[t * hop_length:t * hop_length + n_fft] * w
        out[:, t] = np.abs(scipy.fft.rfft(frame)).astype(dtype)
    return out


def hz_to_mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m):
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_filterbank(sample_rate, n_fft, num_mels, fmin):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax=sr/2, htk=False, norm='slaney') → (num_mels, n_fft//2 + 1)."""
    fmax = sample_rate / 2.0
    mels = np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), num_mels + 2)
    mf = np.array([mel_to_hz(m) for m in mels])
    freqs = np.linspace(0.0, fmax, n_fft // 2 + 1)
    W = np.zeros((num_mels, len(freqs)))
    for i in range(num_mels):
        lower = (freqs - mf[i]) / (mf[i + 1] - mf[i])
        upper = (mf[i + 2] - freqs) / (mf[i + 2] - mf[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mf[i + 2] - mf[i]))
    return W


def melspectrogram(y, sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=40.0,
                   min_level_db=-100.0, dtype=np.float64):
    """→ (num_mels, T) in [0, 1]; float64 unless dtype says otherwise.  ref_level_db is not applied on
    this path (the reference applies it in spectrogram() only)."""
    D = stft_mag(y, n_fft, hop_length, win_length, dtype)
    W = mel_filterbank(sample_rate, n_fft, num_mels, fmin).astype(dtype)
    S = W @ D
    db = dtype(20.0) * np.log10(np.maximum(dtype(1e-5), S))
    return np.clip((db - dtype(min_level_db)) / dtype(-min_level_db), 0, 1).astype(dtype)


def weighted_samples(t, n_samples_or_none, n_fft, hop_length, win_length):
    """The sample indices frame t reads with a non-zero (float32) weight, reflection applied — at the
    right edge only when the length is known: what a streaming plan must have received and kept."""
    taps = np.nonzero(window(n_fft, win_length).astype(np.float32))[0]
    j = np.abs(t * hop_length + taps - n_fft // 2)
    if n_samples_or_none is not None:
        j = np.where(j >= n_samples_or_none, 2 * (n_samples_or_none - 1) - j, j)
    return j
