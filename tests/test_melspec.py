"""The mel front end without a GPU: the float64 restatement (tests/melspec_ref.py) against
scipy.signal.stft, wavernn_amd.dsp's table builders and float32 host path against the restatement,
the library's host functions (wrnn_melspec_tables / _frames / _plan and the refusals), and the CLI's
wav branch up to the point where it needs a GPU.  The kernel itself: tests/test_gpu_melspec.py."""
import ctypes

import numpy as np
import pytest
import scipy.signal
import torch

from tests import melspec_ref as ref
from wavernn_amd import _native as nat
from wavernn_amd import build as hbuild
from wavernn_amd import dsp, melspec

HOP = 275
N_REPLAY = 12 * HOP + 137
ODD = dict(ref.SMALL, win_length=201)               # n_fft − win_length odd: the two halves of the padding differ
FULL = dict(ref.SMALL, n_fft=512, win_length=512)   # no zero padding at all
GEOMETRIES = [ref.DEFAULT, ref.SMALL, ODD, FULL]


@pytest.fixture(scope="module")
def lib():
    hbuild.build(verbose=False)
    return nat.lib()


def _noise(n, seed=0, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("p", [ref.DEFAULT, ref.SMALL], ids=["default", "small"])
def test_restatement_matches_scipy_stft(p):
    n_fft, hop = p["n_fft"], p["hop_length"]
    y = _noise(N_REPLAY, 1).astype(np.float64)
    w = ref.window(n_fft, p["win_length"])
    _, _, Z = scipy.signal.stft(ref.reflect_pad(y, n_fft // 2), window=w, nperseg=n_fft, noverlap=n_fft - hop,
                                boundary=None, padded=False)
    mine = ref.stft_mag(y, n_fft, hop, p["win_length"])
    assert Z.shape == mine.shape == (n_fft // 2 + 1, 1 + len(y) // hop)
    assert np.abs(np.abs(Z) * w.sum() - mine).max() <= 1e-12
    left = (n_fft - p["win_length"]) // 2
    hann = scipy.signal.get_window("hann", p["win_length"], fftbins=True)
    np.testing.assert_allclose(w, np.pad(hann, (left, n_fft - p["win_length"] - left)), rtol=0, atol=1e-15)


@pytest.mark.parametrize("p", [ref.DEFAULT, ref.SMALL], ids=["default", "small"])
def test_mel_basis_matches_restatement(p):
    W = dsp.mel_basis(p["sample_rate"], p["n_fft"], p["num_mels"], p["fmin"])
    R = ref.mel_filterbank(p["sample_rate"], p["n_fft"], p["num_mels"], p["fmin"])
    assert W.dtype == np.float64 and W.shape == R.shape == (p["num_mels"], p["n_fft"] // 2 + 1)
    np.testing.assert_allclose(W, R, rtol=1e-12, atol=0)
    assert np.array_equal(W > 0, R > 0)
    assert (W > 0).sum(1).min() >= 1                      # every band non-empty
    assert (W > 0).sum(0).max() <= 2                      # at most two bands per bin
    np.testing.assert_allclose(dsp.stft_window(p["n_fft"], p["win_length"]), ref.window(p["n_fft"], p["win_length"]),
                               rtol=1e-12, atol=1e-16)


def test_default_filterbank_figures():
    W = dsp.mel_basis()
    assert int((W > 0).sum()) == 1995
    assert f"{W[0].max():.5g}" == "0.021471" and f"{W[79].max():.5g}" == "0.0022576"


@pytest.mark.parametrize("p", GEOMETRIES, ids=["default", "small", "odd", "full"])
def test_library_tables_are_the_float64_tables_rounded(lib, p):
    t = melspec.unpack_tables(p, melspec.tables(p))
    N, M = p["n_fft"], p["n_fft"] // 2
    win = dsp.stft_window(N, p["win_length"]).astype(np.float32)
    assert np.array_equal(t["window"], win)
    nz = np.nonzero(win)[0]
    assert (t["first_tap"], t["taps"]) == (int(nz[0]), int(nz[-1] - nz[0] + 1))
    W = dsp.mel_basis(p["sample_rate"], N, p["num_mels"], p["fmin"])
    assert np.array_equal(t["basis"], W.astype(np.float32))
    assert t["n_weights"] >= int((W > 0).sum()) and t["n_weights"] <= 2 * (M + 1)
    # float64 cos / sin of the C library (math.*: the libm the tables were built with), rounded once
    import math
    tw_m = np.array([[math.cos(2.0 * math.pi * n / M), -math.sin(2.0 * math.pi * n / M)] for n in range(M)])
    tw_n = np.array([[math.cos(2.0 * math.pi * k / N), -math.sin(2.0 * math.pi * k / N)] for k in range(M + 1)])
    np.testing.assert_array_equal(t["twiddle_m"], tw_m.astype(np.float32))
    np.testing.assert_array_equal(t["twiddle_n"], tw_n.astype(np.float32))


def test_frames(lib):
    for n in (1025, 1099, 1100, N_REPLAY, 13 * HOP, 10 ** 7):
        assert melspec.frames(ref.DEFAULT, n) == 1 + n // HOP == ref.n_frames(n, HOP)
    with pytest.raises(ValueError):
        melspec.frames(ref.DEFAULT, 1024)                  # the reflect padding's own limit
    assert melspec.frames(ref.SMALL, 129) == 3


@pytest.mark.parametrize("p", GEOMETRIES, ids=["default", "small", "odd", "full"])
@pytest.mark.parametrize("push", [1, 275, 549, 550, 551, 1100])
def test_plan_replay(lib, p, push):
    """Every frame ready exactly once, in order, never before its last weighted sample (mirror images
    included) is in; keep_from never drops a sample a later frame weights, whatever the final length."""
    n_fft, hop, win = p["n_fft"], p["hop_length"], p["win_length"]
    N = N_REPLAY
    T = 1 + N // hop
    last = [int(ref.weighted_samples(t, None, n_fft, hop, win).max()) for t in range(T)]
    done, got, keep_prev, first = 0, 0, 0, True
    while got < N:
        got = min(N, got + push)
        ready, keep = melspec.plan(p, got)
        # in order and exactly once (the count only grows), and exactly the frames whose last
        # weighted sample — frame 0's mirror images included — is in
        want = 0
        while want < T and last[want] < got and last[0] < got:
            want += 1
        assert ready == want and ready >= done, (got, ready, want)
        assert keep_prev <= keep <= got
        if ready != done or first:
            # frames still to come read nothing before keep_from, whatever the final length: the
            # shortest signal in which the next frame exists mirrors the furthest back
            for total in {N, max(got, ready * hop, n_fft // 2 + 1)}:
                for t in range(ready, min(1 + total // hop, ready + n_fft // hop + 3)):
                    assert int(ref.weighted_samples(t, total, n_fft, hop, win).min()) >= keep, (t, total, keep)
        done, keep_prev, first = ready, keep, False
    ready, keep = melspec.plan(p, N, final=True)
    assert (ready, keep) == (T, N) and ready >= done
    if p is ref.DEFAULT:
        assert [melspec.plan(p, r)[0] for r in (549, 550, 824, 825)] == [0, 1, 1, 2]   # t·hop + 550


def test_refusals(lib):
    def code(fn, **kw):
        cfg = melspec._cfg(dict(ref.DEFAULT, **kw))
        return fn(ctypes.byref(cfg))
    frames = lambda c: int(lib.wrnn_melspec_frames(c, 4000))
    floats = lambda c: lib.wrnn_melspec_table_floats(c)
    for fn in (frames, floats):
        assert code(fn) > 0
        for kw in (dict(n_fft=2000), dict(n_fft=128), dict(n_fft=8192), dict(win_length=0), dict(win_length=2049),
                   dict(hop_length=0), dict(num_mels=129), dict(fmin=-1.0), dict(fmin=11025.0)):
            assert code(fn, **kw) == -6, kw               # WRNN_EUNSUPPORTED, no launch
        assert code(fn, min_level_db=0.0) == -1
    assert int(lib.wrnn_melspec_frames(ctypes.byref(melspec._cfg(ref.DEFAULT)), 1024)) == -1      # WRNN_EINVAL
    assert b"n_fft/2 + 1" in lib.wrnn_cond_last_error()
    with pytest.raises(NotImplementedError, match="power of two"):
        melspec.tables(dict(ref.DEFAULT, n_fft=2000))
    with pytest.raises(ValueError):
        melspec.plan(ref.DEFAULT, 1000, final=True)
    # launches refuse their arguments before they touch the GPU
    cfg = melspec._cfg(ref.DEFAULT)
    one = (ctypes.c_void_p * 1)(8)
    assert lib.wrnn_melspec(ctypes.byref(cfg), 8, one, (ctypes.c_int * 1)(1024), 1, one, (ctypes.c_int * 1)(4), 8, None) == -1
    assert lib.wrnn_melspec(ctypes.byref(cfg), 8, one, (ctypes.c_int * 1)(4000), 1, one, (ctypes.c_int * 1)(3), 8, None) == -1
    # a frame whose samples are not resident: frame 3 reads up to sample 3·275 + 549
    assert lib.wrnn_melspec_window(ctypes.byref(cfg), 8, 8, 0, 3 * 275 + 549, -1, 0, 4, 8, 4, 8, None) == -1
    assert b"resident" in lib.wrnn_cond_last_error()


SIGNALS = {
    "noise": lambda: _noise(N_REPLAY, 2),
    "quiet": lambda: _noise(N_REPLAY, 3, 1e-4),
    "sine": lambda: (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(N_REPLAY) / 22050)).astype(np.float32),
    "shortest": lambda: _noise(1025, 4),
}


@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("p", [ref.DEFAULT, ODD], ids=["default", "odd"])
def test_host_path_matches_restatement(name, p):
    """dsp.melspectrogram(device='cpu') is the definition in float32: it deviates from the float64
    restatement by float32 rounding, i.e. by no more than a few times what the restatement itself
    deviates by when it is run in float32 (the same rule the GPU test applies to the kernel)."""
    y = SIGNALS[name]()
    r64 = ref.melspectrogram(y, **p)
    d32 = float(np.abs(ref.melspectrogram(y, **p, dtype=np.float32) - r64).max())
    got = dsp.melspectrogram(y, p, device="cpu")
    assert got.dtype == np.float32 and got.shape == r64.shape == (p["num_mels"], 1 + len(y) // p["hop_length"])
    err = float(np.abs(got - r64).max())
    print(f"HOST MELSPEC {name}: d32 {d32:.3g} err {err:.3g}")
    assert err <= max(1e-6, 8 * d32)
    assert got.min() >= 0 and got.max() <= 1


def test_host_path_refuses_short_signals():
    with pytest.raises(ValueError, match="n_fft"):
        dsp.melspectrogram(np.zeros(1024, np.float32), device="cpu")


def test_gpu_entry_points_exist_and_refuse_the_cpu():
    from wavernn_amd import synthetic as syn
    from wavernn_amd.fatchord_version import WaveRNN, WaveRNNStream
    m = WaveRNN(**syn.TINY_MOL.ctor_kwargs())
    for name in ("melspectrogram", "generate_from_wav", "generate_list_from_wavs"):
        assert callable(getattr(m, name))
    assert callable(WaveRNNStream.push_audio) and callable(WaveRNNStream.finish_audio)
    with pytest.raises(RuntimeError, match="GPU"):
        m.melspectrogram(np.zeros(4000, np.float32))       # no silent host substitute on the model path


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the path up to the no-GPU error")
def test_cli_wav_branch_up_to_the_gpu(tmp_path):
    from wavernn_amd import gen_wavernn
    wav = tmp_path / "x.wav"
    dsp.save_wav(_noise(30 * HOP, 5), wav)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        gen_wavernn.main(["-f", str(wav), "-u", "--out_dir", str(tmp_path)])
    assert not list(tmp_path.glob("__*"))


def test_cli_wav_branch_refusals(tmp_path):
    """What the wav branch refuses before it looks for a GPU, and without leaving a file behind."""
    from wavernn_amd import gen_wavernn
    wav = tmp_path / "x.wav"
    dsp.save_wav(_noise(30 * HOP, 5), wav)
    short = tmp_path / "short.wav"
    dsp.save_wav(_noise(1000, 6), short)
    with pytest.raises(ValueError, match="n_fft"):
        gen_wavernn.main(["-f", str(short), "-u", "--out_dir", str(tmp_path)])
    other = tmp_path / "r.wav"
    dsp.save_wav(_noise(8000, 7), other, 16000)
    with pytest.raises(ValueError, match="sample rate"):
        gen_wavernn.main(["-f", str(other), "-u", "--out_dir", str(tmp_path)])
    with pytest.raises(ValueError, match=".npy"):
        gen_wavernn.load_mel(wav, 80)                       # the wav branch lives beside load_mel, not in it
    for bad in (["-b", "--stream-chunk", "4"], ["-u", "--stream-chunk", "0"]):
        with pytest.raises(SystemExit):                     # argument errors come before anything is written
            gen_wavernn.main(["-f", str(wav), "--out_dir", str(tmp_path)] + bad)
    assert not list(tmp_path.glob("__*"))


def test_cli_wav_loader(tmp_path):
    from wavernn_amd import gen_wavernn
    from wavernn_amd.hparams import HParams
    y = _noise(30 * HOP, 5)
    dsp.save_wav(y, tmp_path / "x.wav")
    got = gen_wavernn.load_target_wav(tmp_path / "x.wav", HParams().configure(None))
    assert got.dtype == np.float32 and np.array_equal(got, y)
