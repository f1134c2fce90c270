"""The mel front end on the GPU (csrc/melspec.hip through wrnn_melspec / wrnn_melspec_windows,
WaveRNN.melspectrogram, push_audio, the CLI's wav branch).

Accuracy: every output cell against the float64 restatement (tests/melspec_ref.py), in normalised
units.  The bound is not one number: per input, d32 is the deviation of the restatement run in
float32 on the CPU from the float64 one — the float32 error of the definition itself, never
anything the GPU produced — and the kernel is allowed max(1e-6, 8·d32); the factor 8 covers the
rounding of another FFT factorisation.  Broadband inputs sit at the 1e-6 floor (d32 ≈ 1e-7); a sine
or a chirp has leakage bins next to the 1e-5 amplitude floor under a 120 dB range, where float32
rounding of the FFT moves the logarithm (d32 ≈ 2.5e-4 … 3.3e-4 at the default geometry).

Identity: a frame's bits depend on nothing but its own samples, so the same signal alone, inside a
list, chunked through wrnn_melspec_window and streamed through push_audio gives equal arrays
(np.array_equal), and audio generated from a wav equals audio generated from its mel on the same
seed.  No audio is compared across different mels: the MoL loop amplifies a 1e-7 mel difference over
thousands of steps.

Measured on MI355X, max |Δ| (allowed), default geometry: noise 0.1 8.6e-8 (1e-6), noise 1e-4 1.2e-7
(1.3e-6), sine 2.1e-4 (2.0e-3), chirp 7.8e-4 (2.6e-3), zeros then noise 1.1e-7 (1.1e-6), 1 025 samples
7.5e-8 (1e-6), 13·hop samples 8.5e-8 (1e-6); the other geometries ≤ 1.7e-7 broadband, ≤ 1.4e-4 on the
sine and the chirp (allowed ≥ 2.1e-4); n_fft 4096 / win 4000 / hop 512: ≤ 1.3e-7 broadband, sine 7.5e-4 (3.6e-3), chirp 1.3e-3 (6.8e-3);
n_fft 1024 / win 800 / hop 200: ≤ 1.3e-7, sine 1.9e-4 (1.2e-3), chirp 2.7e-4 (1.7e-3); every identity check equal."""
import functools

import numpy as np
import pytest
import torch

from tests import melspec_ref as ref
from wavernn_amd import dsp, melspec
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ODD = dict(ref.SMALL, win_length=201)               # odd window: the zero padding's halves differ
FULL = dict(ref.SMALL, n_fft=512, win_length=512)   # win_length == n_fft: no zero padding
# the largest n_fft: log2(n_fft/2) odd (a radix-2 stage of four passes per thread, then radix-4 stages
# of two passes), 33 KB of LDS; and n_fft 1024, also odd, one pass of 128 busy threads per stage
LARGE = dict(ref.DEFAULT, n_fft=4096, win_length=4000, hop_length=512)
MID = dict(ref.DEFAULT, n_fft=1024, win_length=800, hop_length=200)
GEOMETRIES = {"default": ref.DEFAULT, "small": ref.SMALL, "full": FULL, "odd": ODD, "large": LARGE, "mid": MID}
NAMES = ("noise", "quiet", "sine", "chirp", "zeros_then_noise", "shortest", "hop_multiple")


@functools.lru_cache(maxsize=None)
def _signals(geom):
    p = GEOMETRIES[geom]
    sr, hop, n_fft = p["sample_rate"], p["hop_length"], p["n_fft"]
    n = 12 * hop + 137
    g = np.random.default_rng(20)
    t = np.arange(n) / sr
    f0, f1 = 50.0, min(10000.0, 0.45 * sr)
    nz = min(1500, n // 2)
    tail = g.standard_normal(n - nz) * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n - nz) / (n - nz))) * 0.2
    sig = {
        "noise": 0.1 * g.standard_normal(n),
        "quiet": 1e-4 * g.standard_normal(n),
        "sine": 0.5 * np.sin(2 * np.pi * 440.0 * t),
        "chirp": 0.8 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / t[-1] * t * t)),
        "zeros_then_noise": np.concatenate([np.zeros(nz), tail]),
        "shortest": 0.1 * g.standard_normal(n_fft // 2 + 1),
        "hop_multiple": 0.1 * g.standard_normal(13 * hop),
    }
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sig.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(geom, name):
    """(float64 restatement, d32) of one signal, computed once and shared (read-only)."""
    p, y = GEOMETRIES[geom], _signals(geom)[name]
    r64 = ref.melspectrogram(y, **p)
    d32 = float(np.abs(ref.melspectrogram(y, **p, dtype=np.float32).astype(np.float64) - r64).max())
    r64.setflags(write=False)
    return r64, d32


def _front(geom="default"):
    return melspec.MelSpec.get(dsp.melspec_params(GEOMETRIES[geom]), DEV)


@functools.lru_cache(maxsize=None)
def _one_shot(geom):
    """All seven signals of a geometry in ONE launch → {name: mel on the host}."""
    sig = _signals(geom)
    mels = _front(geom).run([sig[k] for k in NAMES])
    torch.cuda.synchronize()
    return {k: m.cpu().numpy() for k, m in zip(NAMES, mels)}


# ---- 1. accuracy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_matches_restatement(geom, name):
    p = GEOMETRIES[geom]
    r64, d32 = _expected(geom, name)
    got = _one_shot(geom)[name]
    assert got.dtype == np.float32 and got.shape == r64.shape == (p["num_mels"], 1 + len(_signals(geom)[name]) // p["hop_length"])
    err = float(np.abs(got.astype(np.float64) - r64).max())
    allowed = max(1e-6, 8 * d32)
    print(f"MELSPEC {geom}/{name}: max|d| {err:.3g}  d32 {d32:.3g}  allowed {allowed:.3g}")
    assert err <= allowed
    assert got.min() >= 0.0 and got.max() <= 1.0
    if name == "zeros_then_noise":
        # log of an all-zero frame, the floor clip: every frame that weights only the leading zeros
        y = _signals(geom)[name]
        nz = int(np.nonzero(y)[0][0])
        silent = [t for t in range(got.shape[1])
                  if ref.weighted_samples(t, len(y), p["n_fft"], p["hop_length"], p["win_length"]).max() < nz]
        assert np.all(got[:, silent] == 0.0) and (silent or geom == "large")


def test_dsp_entry_uses_the_kernel():
    y = _signals("default")["noise"]
    assert np.array_equal(dsp.melspectrogram(y), _one_shot("default")["noise"])
    assert np.array_equal(dsp.melspectrogram(y, device=DEV), _one_shot("default")["noise"])


# ---- 2. independence and bit-identity -------------------------------------------------------------
def test_member_of_a_list_equals_alone():
    sig, f = _signals("default"), _front()
    lens = (3437, 2000, 1025, 3000, 3575, 1500, 2750)        # seven signals of unequal length
    g = np.random.default_rng(3)
    for slot in (0, 3, 6):
        for name in ("noise", "chirp"):
            y = sig[name]
            alone = f.run([y])[0].cpu().numpy()
            others = [(0.1 * g.standard_normal(n)).astype(np.float32) for n in lens]
            others[slot] = y
            assert np.array_equal(f.run(others)[slot].cpu().numpy(), alone), (slot, name)
            assert np.array_equal(alone, _one_shot("default")[name])


@pytest.mark.parametrize("chunk", [1, 2, 5, 13])
def test_window_chunks_equal_one_shot(chunk):
    f = _front()
    y = torch.from_numpy(_signals("default")["chirp"].copy()).to(DEV)
    T = melspec.frames(f.p, len(y))
    assert T == 13
    parts = [f.window(y, 0, len(y), t0, min(chunk, T - t0)) for t0 in range(0, T, chunk)]
    assert np.array_equal(torch.cat(parts, 1).cpu().numpy(), _one_shot("default")["chirp"])


def test_window_of_a_resident_tail():
    """Only the samples the plan says are still needed are resident, the length not yet known."""
    f = _front()
    y = _signals("default")["noise"]
    ready, _ = melspec.plan(f.p, 2000)
    _, keep = melspec.plan(f.p, 1400)
    done = melspec.plan(f.p, 1400)[0]
    tail = torch.from_numpy(y[keep:2000].copy()).to(DEV)
    got = f.window(tail, keep, None, done, ready - done).cpu().numpy()
    assert ready > done and np.array_equal(got, _one_shot("default")["noise"][:, done:ready])
    with pytest.raises(ValueError, match="resident"):
        f.window(tail, keep, None, done, ready - done + 1)   # the next frame's samples are not in yet
    with pytest.raises(ValueError, match="resident"):
        f.window(tail[5:], keep + 5, None, done, ready - done)


def test_ld_padding_is_untouched():
    f, sig = _front(), _signals("default")
    ys = [sig["noise"], sig["shortest"]]
    outs = [torch.full((80, 40), -7.0, device=DEV), torch.full((80, 9), -7.0, device=DEV)]
    mels = f.run(ys, out=outs)
    for y, o, m, name in zip(ys, outs, mels, ("noise", "shortest")):
        T = 1 + len(y) // 275
        assert m.shape == (80, T) and np.array_equal(o[:, :T].cpu().numpy(), _one_shot("default")[name])
        assert bool((o[:, T:] == -7.0).all())
    with pytest.raises(ValueError):
        f.run([sig["noise"]], out=[torch.empty(80, 12, device=DEV)])     # ld below the 13 frames


def test_short_and_unsupported_are_refused_without_a_launch():
    f = _front()
    with pytest.raises(ValueError, match="n_fft"):
        f.run([np.zeros(1024, np.float32)])
    with pytest.raises(NotImplementedError, match="power of two"):
        melspec.MelSpec(dict(f.p, n_fft=2000), DEV)


# ---- 3. through the vocoder -----------------------------------------------------------------------
HOP = 275


@functools.lru_cache(maxsize=None)
def _model():
    from wavernn_amd.fatchord_version import WaveRNN
    d = syn.DEFAULT_MOL
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, 0).items()})
    return m.eval()


def _wav(frames, seed, extra=100):
    """A signal of `frames` mel frames: (frames − 1)·hop + extra samples of shaped noise."""
    n = (frames - 1) * HOP + extra
    g = np.random.default_rng(seed)
    return (0.2 * g.standard_normal(n) * (0.6 + 0.4 * np.sin(np.arange(n) / 300.0))).astype(np.float32)


@pytest.mark.parametrize("push", [1, 275, 550, 551])
def test_push_audio_frames_equal_one_shot(push):
    """push_audio's own code with the vocoder's push() replaced by a recorder: the frames handed to
    push(), in order, are the one-shot mel bit for bit."""
    m = _model()
    y = _signals("default")["chirp"]
    got = []
    with m.stream(1, seed=1) as s:
        s.push = lambda mel: (got.append(mel.cpu().numpy()), np.zeros((1, 0)))[1]
        s.finish = lambda: np.zeros((1, 0))
        for i in range(0, len(y), push):
            before = sum(g.shape[2] for g in got)
            s.push_audio(y[i:i + push])
            ready = melspec.plan(_front().p, min(len(y), i + push))[0]
            assert sum(g.shape[2] for g in got) == ready >= before
        s.finish_audio()
        with pytest.raises(RuntimeError, match="ended"):
            s.push_audio(y[:10])
    mel = np.concatenate(got, 2)
    assert mel.shape == (1, 80, 13) and np.array_equal(mel[0], _one_shot("default")["chirp"])


def test_generate_from_wav_equals_generate_on_its_mel():
    m = _model()
    y = _wav(30, 1)
    mel = m.melspectrogram(y)[0]
    assert mel.shape == (1, 80, 30) and mel.is_cuda
    assert np.array_equal(mel[0].cpu().numpy(), m.melspectrogram([y, _wav(22, 2)])[0][0].cpu().numpy())
    a = m.generate_from_wav(y, None, False, 11000, 550, False, seed=5, verbose=False)
    b = m.generate(mel, None, False, 11000, 550, False, seed=5, verbose=False)
    assert a.shape == (29 * HOP,) and np.array_equal(a, b)
    a = m.generate_from_wav(torch.from_numpy(y), None, True, 2750, 275, False, seed=6, verbose=False)
    b = m.generate(mel, None, True, 2750, 275, False, seed=6, verbose=False)
    assert np.array_equal(a, b)


def _mel_fed(m, mel, n_samples, push, **kw):
    """The session fed the one-shot mel in exactly the frame groups wrnn_melspec_plan yields for
    pushes of `push` samples, ending as finish_audio() does."""
    p = _front().p
    out, done = [], 0
    U = mel.shape[0]
    with m.stream(U, total_samples=n_samples, **kw) as s:
        for got in range(push, n_samples + push, push):
            ready = melspec.plan(p, min(got, n_samples))[0]
            if ready > done:
                out.append(s.push(mel[:, :, done:ready]))
                done = ready
        T = melspec.plan(p, n_samples, final=True)[0]
        if T > done:
            out.append(s.push(mel[:, :, done:T]))
        out.append(s.finish())
    return np.concatenate(out, 1)


def test_narrow_session_fed_audio_equals_fed_mel():
    m = _model()
    y = _wav(30, 3)
    mel = m.melspectrogram(y)[0]
    with m.stream(1, total_samples=len(y), seed=9) as s:
        chunks = [s.push_audio(y[i:i + 550]) for i in range(0, len(y), 550)]
        chunks.append(s.finish_audio())
    a = np.concatenate(chunks, 1)
    b = _mel_fed(m, mel, len(y), 550, seed=9)
    assert a.shape == (1, 29 * HOP) and np.array_equal(a, b)
    assert any(c.shape[1] for c in chunks[:-1])              # audio came out before the end
    with pytest.raises(ValueError, match="total"):
        m.stream(1, total_frames=30, total_samples=len(y))


def test_wide_session_fed_audio_equals_fed_mel():
    m = _model()
    ys = np.stack([_wav(30, 4), _wav(30, 5)])
    mel = torch.cat(m.melspectrogram(ys), 0)
    assert mel.shape == (2, 80, 30)
    with m.stream(2, seed=11, wide=True) as s:               # length not announced: neither total given
        chunks = [s.push_audio(ys[:, i:i + 550]) for i in range(0, ys.shape[1], 550)]
        chunks.append(s.finish_audio())
    a = np.concatenate(chunks, 1)
    p, out, done = _front().p, [], 0
    with m.stream(2, seed=11, wide=True) as s:
        for got in range(550, ys.shape[1] + 550, 550):
            ready = melspec.plan(p, min(got, ys.shape[1]))[0]
            if ready > done:
                out.append(s.push(mel[:, :, done:ready]))
                done = ready
        out.append(s.push(mel[:, :, done:]))
        out.append(s.finish())
    assert a.shape == (2, 29 * HOP) and np.array_equal(a, np.concatenate(out, 1))


def test_group_audio_pushes_equal_sessions_alone():
    """push_streams with (session, pcm) members: one front-end launch for both, the group push as it
    is — each member's audio is what the same session gives alone through push_audio."""
    m = _model()
    ya, yb = _wav(30, 6), _wav(26, 7, extra=20)
    alone = []
    for y, seed in ((ya, 21), (yb, 22)):
        with m.stream(1, seed=seed) as s:
            alone.append(np.concatenate([s.push_audio(y[i:i + 1100]) for i in range(0, len(y), 1100)]
                                        + [s.finish_audio()], 1))
    with m.stream(1, seed=21) as sa, m.stream(1, seed=22) as sb:
        outs = [[], []]
        for i in range(0, len(ya), 1100):
            pushes = [(sa, ya[i:i + 1100])] + ([(sb, yb[i:i + 1100])] if i < len(yb) else [])
            for k, w in enumerate(m.push_streams(pushes)):
                outs[k].append(w)
        outs[0].append(sa.finish_audio())
        outs[1].append(sb.finish_audio())
    for k in range(2):
        assert np.array_equal(np.concatenate(outs[k], 1), alone[k]), k


def test_group_members_of_two_geometries():
    """Sessions of one model opened with different hp= (another n_fft and window) in one push_streams
    call: each member's frames come from its own tables, and its audio is the session's alone."""
    m = _model()
    hp_b = dict(n_fft=1024, win_length=800)
    ya, yb = _wav(27, 14), _wav(27, 15)
    alone = []
    for y, seed, hp in ((ya, 31, None), (yb, 32, hp_b)):
        with m.stream(1, seed=seed, hp=hp) as s:
            alone.append(np.concatenate([s.push_audio(y[i:i + 1650]) for i in range(0, len(y), 1650)]
                                        + [s.finish_audio()], 1))
    with m.stream(1, seed=31) as sa, m.stream(1, seed=32, hp=hp_b) as sb:
        assert sa._audio_feed().front is not sb._audio_feed().front
        outs = [[], []]
        for i in range(0, len(ya), 1650):
            for k, w in enumerate(m.push_streams([(sa, ya[i:i + 1650]), (sb, yb[i:i + 1650])])):
                outs[k].append(w)
        outs[0].append(sa.finish_audio())
        outs[1].append(sb.finish_audio())
    for k in range(2):
        assert np.array_equal(np.concatenate(outs[k], 1), alone[k]), k
    # the two geometries give different mels: the members were not computed with one set of tables
    assert not np.array_equal(m.melspectrogram(yb)[0].cpu().numpy(), m.melspectrogram(yb, hp_b)[0].cpu().numpy())


def test_generate_list_from_wavs_equals_generate_list():
    m = _model()
    ys = [_wav(30, 8), _wav(24, 9, extra=0), _wav(27, 10, extra=274)]
    mels = m.melspectrogram(ys)
    assert [x.shape[2] for x in mels] == [30, 24, 27]
    a = m.generate_list_from_wavs(ys, seed=13)
    b = m.generate_list(mels, seed=13)
    assert len(a) == 3
    for x, y, T in zip(a, b, (30, 24, 27)):
        assert x.shape == ((T - 1) * HOP,) and np.array_equal(x, y)


# ---- 4. the CLI -----------------------------------------------------------------------------------
def test_cli_wav_end_to_end(tmp_path):
    from scipy.io import wavfile
    from wavernn_amd import gen_wavernn
    y = _wav(30, 12)
    src = tmp_path / "utt.wav"
    dsp.save_wav(y, src)
    lengths = {}
    for sub, extra in (("w", []), ("s", ["--stream-chunk", "4"])):
        out = tmp_path / sub
        out.mkdir()
        torch.manual_seed(0)
        gen_wavernn.main(["-f", str(src), "-u", "--out_dir", str(out), "--seed", "3"] + extra)
        target, gen = out / "__utt__0k_steps_target.wav", out / "__utt__0k_steps_gen_NOT_BATCHED.wav"
        assert target.exists() and gen.exists()
        assert np.array_equal(wavfile.read(str(target))[1], y)
        lengths[sub] = wavfile.read(str(gen))[1].shape
    # the .npy route on the saved mel gives the same (T − 1)·hop samples
    mel = dsp.melspectrogram(y)
    np.save(tmp_path / "utt.npy", mel)
    out = tmp_path / "m"
    out.mkdir()
    torch.manual_seed(0)
    gen_wavernn.main(["-f", str(tmp_path / "utt.npy"), "-u", "--out_dir", str(out), "--seed", "3"])
    lengths["m"] = wavfile.read(str(out / "__utt__0k_steps_gen_NOT_BATCHED.wav"))[1].shape
    assert lengths["w"] == lengths["s"] == lengths["m"] == ((mel.shape[1] - 1) * HOP,) == (29 * HOP,)
