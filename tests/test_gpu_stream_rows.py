"""Rows sessions (WaveRNN.stream(rows=True), C-ABI wrnn_stream_open_rows): streaming on the multi-row
kernel for the models no XCD-resident session kernel covers — small and large MoL dims, dense rnn 896,
rnn 1024 / fc 768, 8- and 10-bit RAW, RAW rnn 896.

The inputs are built as regimes.stream_inputs builds them (geometries.geom_dims, perturbed taps, draws
by absolute step) and every expectation is `oracle.generate` (unbatched), one call per utterance alone
with its own column of the draws.  Bounds: MoL within 2·MOL_TOL of the oracle, the bound of every
streaming test; RAW labels exact with mu_law off and the audio at rtol 1e-12 with it on
(tests/raw_streams.py `check`).  Each push must return exactly the count `stream_plan` announces
(`_run_session` of tests/test_gpu_streaming.py).  Against the one-shot call on the same kernel
(WRNN_PATH=rows), under time chunking and with other work on the handle between pushes the audio
must be bit-identical.

Measured on MI355X: MoL max |Δ| against the oracle (bound 2e-5) tinymol 2.3e-8 (U = 1) / 2.6e-8 (U = 3),
mol256 2.6e-8, dense896 2.8e-8 / 3.5e-8 (U = 2), mol1024 2.9e-8, total unknown and announced alike; RAW: 0
labels differ, mu-law audio within 3.5e-15 relative (bound 1e-12); session against generate() with
WRNN_PATH=rows, injected draws and Philox, MoL and RAW: 0 samples differ (rocBLAS gave the push-sized terms
GEMM the bits of the whole-utterance one, so the bit equality the issue expects is what is asserted); one
step per launch: 0; the CLI 1.2e-7 (bound 1e-5)."""
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import raw_streams as rs
from tests import regimes as rg
from tests.golden import fixtures as gf
from tests.test_gpu_streaming import _run_session
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2 * gf.MOL_TOL
OVERRIDES = ("WRNN_PATH", "WRNN_TERMS_MB", "WRNN_ROW_GROUPS", "WRNN_ROWS_GRANULES")
SEED = rg.STREAM_STD_SEED
UNEVEN = [1, 5, 2, 7]           # then the rest
# name: (dims beyond the geometry's, geometry, wrnn_info.last_path: 2, or 9 where the weights exceed LDS)
MODELS = {
    "tinymol": (dict(rnn_dims=64, fc_dims=96, res_out_dims=16), "hop12", 2),
    "mol256": (dict(rnn_dims=256, fc_dims=256), "hop4", 2),
    "dense896": (dict(rnn_dims=896), "hop12", 9),
    "mol1024": (dict(rnn_dims=1024, fc_dims=768), "hop12", 9),
    "tinyraw": (dict(rnn_dims=64, fc_dims=96, res_out_dims=16, bits=8, mode="RAW"), "hop12", 2),
    "raw10": (dict(bits=rg.RAW10.bits, mode="RAW"), "hop12", None),
    "raw896": (dict(rnn_dims=896, mode="RAW"), "hop12", None),
}
_BUILT = {}


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _inputs(name, n_utt, frames):
    """(dims, state, mels [U][feat][T], draws [T·hop][U][K]); computed once and shared (read-only)."""
    kw, geom, _ = MODELS[name]
    d = geo.geom_dims(geom, **kw)
    state = {k: np.array(v, copy=True) for k, v in syn.make_fatchord_state(d, SEED).items()}
    geo.perturb_taps(state, d, SEED)
    mels = np.stack([syn.make_mel(d.feat_dims, frames, 1000 * SEED + 40 + i) for i in range(n_utt)])
    noise = syn.make_noise(d.mode, n_utt, frames * d.hop_length, d.n_classes, 1000 * SEED + 21)
    for a in (mels, noise):
        a.setflags(write=False)
    return d, state, mels, noise


@functools.lru_cache(maxsize=None)
def _oracle(name, n_utt, frames, u, mu_law=False):
    from oracle import oracle
    d, state, mels, noise = _inputs(name, n_utt, frames)
    ref = oracle.generate(state, d, mels[u], False, 0, 0, mu_law, np.ascontiguousarray(noise[:, u:u + 1]))
    assert ref.shape == ((frames - 1) * d.hop_length,) and ref.dtype == np.float64
    ref.setflags(write=False)
    return ref


def _model(name, n_utt, frames):
    from wavernn_amd.fatchord_version import WaveRNN
    d, state, mels, noise = _inputs(name, n_utt, frames)
    if name not in _BUILT:
        m = WaveRNN(**d.ctor_kwargs()).to(DEV)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
        _BUILT[name] = m.eval()
    return _BUILT[name], d, mels, noise


def _rest(frames):
    return UNEVEN + [frames - sum(UNEVEN)]


def _labels(wave, hop, nc):
    """raw_streams.labels_of with the model's own class count."""
    body = (wave[..., :-rs.FADE_FRAMES * hop] + 1.0) * (nc - 1) / 2.0
    lab = np.rint(body)
    assert np.abs(body - lab).max() <= 1e-4, "not a mu_law-off RAW waveform"
    return lab.astype(np.int64)


# ---- 1. MoL against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("name,U,frames", [("tinymol", 1, 24), ("tinymol", 3, 24), ("mol256", 2, 24), ("dense896", 1, 22),
                                           ("dense896", 2, 22), ("mol1024", 1, 21)])
def test_mol_sessions_against_the_oracle(name, U, frames):
    """Uneven pushes with the total unknown and an empty finish(); the total announced and the last
    frames in the final push itself.  Every row against its own oracle run."""
    m, d, mels, noise = _model(name, U, frames)
    ref = np.stack([_oracle(name, U, frames, u) for u in range(U)])
    for total, final_last in ((None, False), (frames, True)):
        chunks, path = _run_session(m, mels.copy(), _rest(frames), total, noise=noise.copy(), final_last=final_last, rows=True)
        assert path == MODELS[name][2], (name, path)
        out = np.concatenate(chunks, 1)
        assert out.shape == ref.shape
        diff = np.abs(out - ref)
        print(f"ROWS STREAM {name} U={U} total={total}: max |Δ| {diff.max():.3g} over {diff.size} samples")
        assert diff.max() <= TOL, f"{name} U={U} total={total}: max |Δ| {diff.max():.3g} at {tuple(np.argwhere(diff > TOL)[0])}"


# ---- 2. RAW labels -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tinyraw", "raw10", "raw896"])
def test_raw_sessions_give_the_oracles_labels(name):
    """mu_law off, U = 2: the labels before the fade are the oracle's exactly (and so is every sample
    there; the fade at rtol 1e-12).  mu_law on, U = 1: the audio at rtol 1e-12.  40 frames: 228 samples of
    every row lie before the 20-frame fade."""
    frames = 40
    m, d, mels, noise = _model(name, 2, frames)
    hop, nc = d.hop_length, d.n_classes
    assert noise.shape[2] == nc
    ref = np.stack([_oracle(name, 2, frames, u) for u in range(2)])
    chunks, path = _run_session(m, mels.copy(), _rest(frames), None, noise=noise.copy(), rows=True, mu_law=False)
    assert path in (2, 9) and (MODELS[name][2] is None or path == MODELS[name][2])
    out = np.concatenate(chunks, 1)
    got, want = _labels(out, hop, nc), _labels(ref, hop, nc)
    print(f"ROWS STREAM {name}: {int((got != want).sum())} of {got.size} labels differ, {len(np.unique(want))} classes drawn")
    assert np.array_equal(got, want)
    rs.check(out, ref, hop, False, f"{name} U=2 mu_law off")
    ref1 = _oracle(name, 2, frames, 0, True)[None]
    chunks, _ = _run_session(m, mels[:1].copy(), _rest(frames), frames, noise=np.ascontiguousarray(noise[:, :1]),
                             final_last=True, rows=True, mu_law=True)
    rs.check(np.concatenate(chunks, 1), ref1, hop, True, f"{name} U=1 mu_law on")


# ---- 3. against the one-shot call on the same kernel -----------------------------------------------
@pytest.mark.parametrize("name", ["tinymol", "tinyraw"])
@pytest.mark.parametrize("draws", ["injected", "philox"])
def test_session_concatenates_to_the_one_shot_call(name, draws, monkeypatch):
    """One utterance: the session's records, packers, partition and kernel are generate()'s on the
    multi-row kernel; only the column count of the terms GEMM differs.  Expected bit-identical."""
    frames = 24
    m, d, mels, noise = _model(name, 2, frames)
    mel = mels[:1]
    kw = dict(noise=np.ascontiguousarray(noise[:, :1])) if draws == "injected" else dict(seed=20240611, row_offset=5)
    monkeypatch.setenv("WRNN_PATH", "rows")
    want = m.generate(torch.from_numpy(mel.copy()), None, False, 0, 0, False, verbose=False, **kw)
    one_shot_path = m.loop_handle().info["last_path"]
    monkeypatch.delenv("WRNN_PATH")
    chunks, path = _run_session(m, mel.copy(), _rest(frames), None, rows=True, mu_law=False, **kw)
    assert path == one_shot_path and path in (2, 9)
    got = np.concatenate(chunks, 1)[0]
    assert got.shape == want.shape
    print(f"ROWS STREAM {name} {draws} vs generate(): max |Δ| {np.abs(got - want).max():.3g}, "
          f"{int((got != want).sum())} of {got.size} samples differ")
    assert np.array_equal(got, want)
    if draws == "philox":   # another row offset is another utterance's draws
        other, _ = _run_session(m, mel.copy(), [frames], frames, rows=True, mu_law=False, seed=20240611, row_offset=6)
        assert np.abs(np.concatenate(other, 1)[0] - want).max() > 1e-3


# ---- 4. chunking ---------------------------------------------------------------------------------
def test_one_step_per_launch_is_bit_identical(monkeypatch):
    frames = 24
    m, d, mels, noise = _model("tinymol", 3, frames)
    ref, _ = _run_session(m, mels.copy(), _rest(frames), None, noise=noise.copy(), rows=True)
    monkeypatch.setenv("WRNN_TERMS_MB", rg.ONE_STEP_BUDGET_MB)
    got, path = _run_session(m, mels.copy(), _rest(frames), None, noise=noise.copy(), rows=True)
    assert path == 2
    a, b = np.concatenate(got, 1), np.concatenate(ref, 1)
    print(f"ROWS STREAM one step per launch: max |Δ| {np.abs(a - b).max():.3g}")
    assert np.array_equal(a, b)


# ---- 5. isolation --------------------------------------------------------------------------------
def test_one_shot_calls_and_other_sessions_between_pushes(monkeypatch):
    frames = 24
    m, d, mels, noise = _model("tinymol", 3, frames)
    mel_a, mel_c = mels[:2].copy(), mels[2:].copy()
    mel_b = torch.from_numpy(syn.make_mel(d.feat_dims, 23, 91)[None])
    monkeypatch.setenv("WRNN_PATH", "rows")     # the one-shot call on the same kernel and hop areas

    def one_shot():
        return m.generate(mel_b, None, False, 0, 0, False, seed=3, verbose=False)

    ref_a, _ = _run_session(m, mel_a, [5, 19], None, rows=True, seed=1)
    ref_c, _ = _run_session(m, mel_c, [10, 14], frames, rows=True, seed=2, row_offset=4)
    ref_b = one_shot()
    assert m.loop_handle().info["last_path"] == 2
    with m.stream(2, None, seed=1, rows=True) as a, m.stream(1, frames, seed=2, row_offset=4, rows=True) as c:
        got_a = [a.push(mel_a[:, :, :5])]
        got_c = [c.push(mel_c[:, :, :10])]
        got_a.append(a.push(mel_a[:, :, 5:]))
        got_b = one_shot()
        got_c.append(c.push(mel_c[:, :, 10:]))
        got_a.append(a.finish())
        got_b2 = one_shot()
        got_c.append(c.finish())
    assert np.array_equal(got_b, ref_b) and np.array_equal(got_b2, ref_b)
    for got, ref in ((got_a, ref_a), (got_c, ref_c)):
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and np.array_equal(g, r)


# ---- 6. refusals ---------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from wavernn_amd import _native as nat
    frames = 24
    m, d, mels, noise = _model("tinymol", 3, frames)
    mels = mels.copy()
    loop = m.loop_handle()
    hop = d.hop_length
    with pytest.raises(ValueError, match="rows=True and wide=True"):
        m.stream(1, None, rows=True, wide=True)
    with pytest.raises(ValueError, match=r"a rows session has 1\.\.(\d+) utterances") as e:
        m.stream(257, None, rows=True)
    lim = int(e.value.args[0].split("1..")[1].split()[0])
    assert 1 <= lim <= 256
    with pytest.raises(ValueError, match="noise must be"):                      # MoL draws are 11 wide
        m.stream(1, None, rows=True, noise=np.zeros((frames * hop, 1, 12), np.float32))
    with m.stream(1, None, rows=True, noise=np.ascontiguousarray(noise[:5 * hop, :1])) as s:
        assert s.push(mels[:1, :, :d.pad + 1 + 5]).shape == (1, 0)            # 5 frames of steps: the draws just reach
        with pytest.raises(nat.WrnnError, match="injected draws cover"):
            s.push(mels[:1, :, d.pad + 6:d.pad + 7])
        out = s.push(None)                                                      # the refused push changed nothing
        assert out.shape == (1, 0)
    # a rows member of a group: refused before anything is queued, the other member goes on to its oracle's audio
    ref = _oracle("tinymol", 3, frames, 0)
    with m.stream(1, frames, rows=True, noise=np.ascontiguousarray(noise[:, :1])) as a, \
            m.stream(1, frames, rows=True, noise=np.ascontiguousarray(noise[:, 1:2])) as b:
        got = [a.push(mels[:1, :, :9])]
        with pytest.raises(ValueError, match="a rows session advances alone"):
            m.push_streams([(a, mels[:1, :, 9:], False), (b, mels[1:2], False)])
        got += [a.push(mels[:1, :, 9:]), a.finish()]
        assert np.abs(np.concatenate(got, 1)[0] - ref).max() <= TOL
        out_b = np.concatenate([b.push(mels[1:2]), b.finish()], 1)[0]
        assert np.abs(out_b - _oracle("tinymol", 3, frames, 1)).max() <= TOL
    # a push after a weight reload
    with m.stream(1, None, rows=True, seed=1) as s:
        s.push(mels[:1, :, :8])
        state = _inputs("tinymol", 3, frames)[1]
        loop.set_weights({k: torch.from_numpy(np.array(v)) for k, v in state.items() if k in loop.keys})
        with pytest.raises(nat.WrnnError, match="weights were loaded again"):
            s.push(mels[:1, :, 8:9])
    # a deepmind handle has no conditioning to stream
    dm = syn.TINY_DM
    from wavernn_amd.loop import DeepmindLoop, FatchordStream
    dloop = DeepmindLoop(dm.hidden_size, dm.quantisation)
    dloop.set_weights(syn.make_deepmind_state(dm, 0))
    dloop.feat_dims = d.feat_dims
    cfg, packed = m._melresnet_packed()
    with pytest.raises(NotImplementedError, match="deepmind"):
        FatchordStream(dloop, m._upsample_spec(), cfg, packed, 1, rows=True)
    assert dloop.info["last_path"] == 0
    dloop.close()


# ---- 7. the CLI ----------------------------------------------------------------------------------
def test_cli_stream_chunk_falls_to_a_rows_session(tmp_path):
    """A TINY_MOL-sized model has no narrow session kernel: --stream-chunk opens a rows session and
    writes generate()'s samples."""
    from scipy.io import wavfile
    from wavernn_amd import gen_wavernn
    t = syn.TINY_MOL
    hp = tmp_path / "hp.py"
    hp.write_text(f"voc_rnn_dims = {t.rnn_dims}\nvoc_fc_dims = {t.fc_dims}\nvoc_compute_dims = {t.compute_dims}\n"
                  f"voc_res_out_dims = {t.res_out_dims}\nvoc_res_blocks = {t.res_blocks}\nvoc_mode = 'MOL'\n")
    mel = tmp_path / "m.npy"
    np.save(mel, syn.make_mel(t.feat_dims, 24, 5).clip(0, 1).astype(np.float32))
    waves = []
    for extra, sub in ((["--stream-chunk", "5"], "s"), ([], "g")):
        out = tmp_path / sub
        out.mkdir()
        torch.manual_seed(0)                      # the same fresh weights for both runs
        gen_wavernn.main(["-f", str(mel), "-u", "--hp_file", str(hp), "--out_dir", str(out), "--seed", "7"] + extra)
        (wav,) = list(out.glob("*.wav"))
        waves.append(wavfile.read(str(wav))[1])
    assert waves[0].shape == waves[1].shape == (23 * t.hop_length,)
    diff = np.abs(waves[0].astype(np.float64) - waves[1].astype(np.float64)).max()
    print(f"ROWS STREAM CLI: max |Δ| {diff:.3g}")
    assert diff <= gf.MOL_TOL
