"""Streaming sessions (WaveRNN.stream / generate_stream, C-ABI wrnn_stream_*) against the
reference's recorded generate() outputs.

The fixtures were written by the reference's own `WaveRNN.generate()` with injected sampler draws
(tests/golden/make_golden.py).  A session gets the same weights, mel and draws, the mel in pushes
of a few frames; the concatenated audio must be the fixture's to the project's MoL tolerance
(`gf.MOL_TOL`) — never compared with the streamed code itself — and each push must
return exactly the sample count `wrnn_stream_plan` announces.  Under Philox the streamed audio is
compared with generate() at the same seed and row offset (the draws are keyed identically; only
the batch of the frame-terms GEMM differs, so the bound is MOL_TOL, not bit equality).  Interleaved
one-shot calls and sessions on the same handle must leave every output bit-identical.

Measured on MI355X (max |Δ|, bound 1e-5): gen_mol_unbatched 5.9e-8 (total unknown and known),
gen_mol_5s_unbatched 7.3e-8 (8-frame and uneven pushes), gen_sparse896_8utt 6.9e-8 (worst
utterance); the Philox comparisons came out bit-identical on that build (not asserted)."""
import numpy as np
import pytest
import torch

from tests.golden import fixtures as gf
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import stream_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(d, state):
    from wavernn_amd.fatchord_version import WaveRNN
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def cache():
    return {}


def _case(name, cache):
    """(fixture, dims, model, mel(s), noise), the model shared by the tests of one dims record."""
    if name not in cache:
        fx = gf.load(name)
        d, state, mel, noise = gf.gen_many_inputs(fx) if "n_utt" in fx else gf.gen_inputs(fx)
        key = "model:" + str(fx["dims"]) + str(fx.get("prune", 0))
        if key not in cache:
            cache[key] = _build(d, state)
        cache[name] = (fx, d, cache[key], mel, noise)
    return cache[name]


def _close(got, ref, what):
    diff = np.abs(got - ref)
    print(f"{what}: max |Δ| {diff.max():.3g} over {diff.size} samples")
    assert diff.max() <= gf.MOL_TOL, f"{what}: max |Δ| {diff.max():.3g}, first over at {np.argwhere(diff > gf.MOL_TOL)[0]}"


def _run_session(model, mel, pushes, total, noise=None, final_last=False, **kw):
    """Push `mel` [U][feat][T] by the frame counts `pushes`, then finish(): (chunks, last_path).
    A count of None is a push without a mel (the C-ABI's n = 0, mel = NULL).  `final_last`: the
    last count's frames go in the final call itself (push(mel, final=True) of the loop-level
    session; the model-level wrapper always ends with an empty finish())."""
    spec = model._upsample_spec()
    chunks, f = [], 0
    with model.stream(mel.shape[0], total, noise=noise, **kw) as s:
        assert s.lookahead_frames == model.pad + 1
        for i, n in enumerate(pushes):
            last = final_last and i == len(pushes) - 1
            if n is None:
                n, out = 0, s._session.push(None).cpu().numpy()
            elif last:
                out = s._session.push(torch.from_numpy(mel[:, :, f:f + n].copy()).to(s.device), final=True).cpu().numpy()
            else:
                out = s.push(mel[:, :, f:f + n])
            f += n
            want = stream_plan(spec, f, last, total)[1] - stream_plan(spec, f - n, False, total)[1]
            assert out.dtype == np.float64 and out.shape == (mel.shape[0], want), (f, out.shape, want)
            chunks.append(out)
        assert f == mel.shape[2]
        if not final_last:
            out = s.finish()
            assert out.shape == (mel.shape[0], stream_plan(spec, f, True, total)[1] - stream_plan(spec, f, False, total)[1])
            chunks.append(out)
        with pytest.raises(RuntimeError):
            s.push(mel[:, :, :1])
    return chunks, model.loop_handle().info["last_path"]


@pytest.mark.parametrize("total,pushes", [(None, [1, 2, 1, 5, 13]), (22, [22])])
def test_short_utterance_in_uneven_pushes(total, pushes, cache):
    fx, d, m, mel, noise = _case("gen_mol_unbatched", cache)
    assert int(fx["T"]) == 22 and noise.shape[0] == 22 * d.hop_length
    chunks, path = _run_session(m, mel[None], pushes, total, noise=noise)
    assert path == 5
    if total is None:   # nothing is final before frame 21 has been seen
        assert [c.shape[1] for c in chunks[:4]] == [0, 0, 0, 0]
    out = np.concatenate(chunks, 1)[0]
    assert out.shape == fx["output"].shape == (21 * d.hop_length,)      # this fixture stores every sample
    _close(out, fx["output"], f"gen_mol_unbatched total={total}")


@pytest.mark.parametrize("pushes", [8, [1] * 12 + [37] * 11])
def test_headline_utterance_streamed(pushes, cache):
    fx, d, m, mel, noise = _case("gen_mol_5s_unbatched", cache)
    assert int(fx["T"]) == 401
    chunks = list(m.generate_stream(mel[None], pushes, noise=noise))
    assert m.loop_handle().info["last_path"] == 5
    out = np.concatenate(chunks)
    assert out.dtype == np.float64 and out.shape == (int(fx["out_len"]),)
    assert int(fx["out_stride"]) == 4
    _close(out[::4], fx["output"], f"gen_mol_5s_unbatched pushes={pushes if isinstance(pushes, int) else 'uneven'}")
    assert abs(out.sum() - float(fx["out_sum"])) <= gf.MOL_TOL * out.size


def test_eight_utterances_in_one_sparse_session(cache):
    fx, d, m, mels, noise = _case("gen_sparse896_8utt", cache)
    assert int(fx["T"]) == 41 and len(mels) == 8
    chunks, path = _run_session(m, np.stack(mels), [7, 1, 13, 20], None, noise=noise)
    assert path == 6
    out = np.concatenate(chunks, 1)
    assert out.shape == (8, int(fx["out_len"]))
    s = int(fx["out_stride"])
    for i in range(8):
        _close(out[i, ::s], fx["output"][i], f"gen_sparse896_8utt utterance {i}")


@pytest.mark.parametrize("name", ["gen_mol_unbatched", "gen_sparse896_8utt"])
def test_philox_streamed_equals_one_shot(name, cache):
    fx, d, m, mel, _ = _case(name, cache)
    mel = (mel[0] if isinstance(mel, list) else mel)[None]
    seed = 20240611
    want = m.generate(torch.from_numpy(mel), None, False, 11000, 550, False, seed=seed, row_offset=5, verbose=False)
    got = np.concatenate(list(m.generate_stream(mel, 8, seed=seed, row_offset=5)))
    assert got.shape == want.shape
    _close(got, want, f"{name} Philox streamed vs generate()")
    # another row offset is another utterance's draws
    other = np.concatenate(list(m.generate_stream(mel, 8, seed=seed, row_offset=6)))
    assert np.abs(other - want).max() > 1e-3


def test_sessions_and_one_shot_calls_do_not_disturb_each_other(cache):
    fx, d, m, mel, _ = _case("gen_mol_unbatched", cache)
    mel_a = mel[None]
    mel_b = syn.make_mel(d.feat_dims, 23, 91)[None]
    mel_c = syn.make_mel(d.feat_dims, 25, 92)[None]
    one_shot = lambda: m.generate(torch.from_numpy(mel_b), None, False, 11000, 550, False, seed=3, verbose=False)
    ref_a, _ = _run_session(m, mel_a, [5, 17], None, seed=1)
    ref_c, _ = _run_session(m, mel_c, [10, 15], 25, seed=2, row_offset=4)
    ref_b = one_shot()
    with m.stream(1, None, seed=1) as a, m.stream(1, 25, seed=2, row_offset=4) as c:
        got_a = [a.push(mel_a[:, :, :5])]
        got_b = one_shot()
        got_c = [c.push(mel_c[:, :, :10])]
        got_a.append(a.push(mel_a[:, :, 5:]))
        got_c.append(c.push(mel_c[:, :, 10:]))
        got_a.append(a.finish())
        got_c.append(c.finish())
    assert np.array_equal(got_b, ref_b)
    for got, ref in ((got_a, ref_a), (got_c, ref_c)):
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and np.array_equal(g, r)
    assert np.concatenate(got_a, 1).shape[1] == 21 * d.hop_length


def test_unsupported_and_misused_sessions_raise(cache):
    """None of these launches the persistent kernel."""
    for d in (syn.DEFAULT_RAW, syn.TINY_MOL):
        m = _build(d, syn.make_fatchord_state(d, 0))
        with pytest.raises(NotImplementedError) as e:
            m.stream()
        assert str(e.value)        # the library's message
        with pytest.raises(NotImplementedError):
            next(m.generate_stream(syn.make_mel(d.feat_dims, 22, 1)[None]))
    fx, d, m, mel, _ = _case("gen_mol_unbatched", cache)
    look = m.pad + 1
    with m.stream(1, None, seed=1) as s:
        assert s.push(mel[None, :, :look]).shape == (1, 0)   # within the look-ahead: no loop step runs
        with pytest.raises(ValueError):          # generate() fails the same way below 21 frames
            s.finish()
    with m.stream(1, 30, seed=1) as s:
        s.push(mel[None, :, :look])
        with pytest.raises(ValueError):          # these frames are not the 30 announced
            s.finish()
        with pytest.raises(ValueError):
            s.push(np.concatenate([mel, mel], 1)[None])   # 3 + 44 > 30
    with pytest.raises(ValueError):
        m.stream(1, 20)                          # an announced total below the fade
    with pytest.raises(ValueError):
        m.stream(9)                              # one utterance per XCD: at most 8
