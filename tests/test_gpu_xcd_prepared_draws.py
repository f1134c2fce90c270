"""The XCD-resident kernel's prepared sampler terms (fatchord_xcd.hip: xcd_draws_kernel, ring_draws).

The one-shot launches (generate / generate_many up to 8 rows per launch) no longer form the 11 MoL
sampler terms of a step inside the loop: a fill kernel writes them per time chunk as 16-float
records [chunk step][launch row], Philox or injected draws alike, and wave 7 loads the record of
step t + 2 in the ring's load batch.  What can go wrong, and the smallest shapes that show it:

  * the record of another row or step: row index k of the launch against the injected layout's
    (t·Bt + b0 + k) — 11 rows make a second launch with b0 = 8, nb = 3 — and the Philox key's
    row_offset + b0 + k (row offsets 0 and 5); 40 steps wrap the 4-slot ring ten times;
  * the horizon: L = 1..4 — the prologue fills three slots under t < L, the look-ahead stops at L;
  * the chunk's origin t0 and the two records past a chunk's end: 96 steps at no more than 11
    steps per launch (>= 9 launches; the library does not report its launch count, the budget
    rule is tests/geometries.py's), 1 and 8 rows, bitwise against one launch;
  * the windowed instantiation, which still forms its draws in the loop: one streamed call.

References: the C oracle fed the same draws (|Δ| <= MOL_TOL, the bound of the other XCD tests,
tests/test_gpu_xcd.py), computed once per case; the Philox route against the injected route and
chunked against unchunked launches bit for bit — they differ in where the terms were read, not in
any arithmetic."""
import functools

import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests.golden import fixtures as gf
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 40
SEED = 0xD1B54A32D192ED03
OVERRIDES = ("WRNN_PATH", "WRNN_TERMS_MB", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES")


@pytest.fixture(autouse=True)
def _xcd_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WRNN_PATH", "xcd")


def _loop(d, state):
    from wavernn_amd.loop import FatchordLoop
    loop = FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0)
    assert loop.info["xcd_rows"] == 8, loop.info
    loop.set_weights(state)
    return loop


def _cond(mels, aux):
    return torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(B, L, seed):
    d = syn.DEFAULT_MOL
    state = syn.make_fatchord_state(d, seed)
    mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, seed + 1)
    for a in (mels, aux):
        a.setflags(write=False)
    return d, state, mels, aux


def _philox_and_injected(B, L, r0, wseed):
    """(Philox audio, audio of the same draws injected, the oracle's on those draws)."""
    from oracle import oracle
    from wavernn_amd.loop import philox_draws
    d, state, mels, aux = _inputs(B, L, wseed)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    y0, _ = loop.generate(cond, seed=SEED, row_offset=r0)
    assert loop.info["last_path"] == 5, loop.info
    draws = philox_draws(SEED, r0, B, L, 11, "MOL")
    assert draws.shape == (L, B, 11)
    y1, _ = loop.generate(cond, noise=draws)
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    ref, _ = oracle.fatchord_loop(state, "MOL", mels, aux, draws.cpu().numpy())
    return y0, y1, ref


@pytest.mark.parametrize("B,r0", [(1, 0), (1, 5), (8, 0), (8, 5), (11, 5)])
def test_philox_route_equals_injected_route(B, r0):
    """40 steps: noise = NULL with a seed gives the audio of the same call fed wrnn_philox_draws of
    that seed and row offset, bit for bit, and both are the oracle's on those draws."""
    y0, y1, ref = _philox_and_injected(B, STEPS, r0, 510 + B)
    nd = int((y0 != y1).sum().item())
    err = np.abs(y0.cpu().numpy() - ref).max()
    print(f"PREPARED {B} row(s), row_offset {r0}: {nd} of {y0.numel()} samples differ; vs oracle max |Δ| {err:.3g}")
    assert torch.equal(y0, y1)
    assert err <= gf.MOL_TOL


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_short_loops(L):
    """One row, L = 1..4 steps: fewer steps than the prologue's three slots, and the first length
    at which wave 7 loads a record in the loop."""
    y0, y1, ref = _philox_and_injected(1, L, 3, 530)
    assert y0.shape == (1, L)
    err = np.abs(y0.cpu().numpy() - ref).max()
    print(f"PREPARED L = {L}: vs oracle max |Δ| {err:.3g}")
    assert torch.equal(y0, y1)
    assert err <= gf.MOL_TOL


@pytest.mark.parametrize("B", [1, 8])
def test_time_chunks_bitwise(B, monkeypatch):
    """96 steps in launches of at most 11 steps (>= 9 launches) against the same call in one launch,
    bit for bit, Philox and injected.

    8 rows also pin the terms GEMM's fixed panel shape (csrc/capi_loops.cpp: generate_xcd_rows): with
    one GEMM over the chunk's columns, 8 x 12 of them did not sum like 8 x 97 and 647 of 768 samples
    differed by up to 3.7e-08."""
    from wavernn_amd.loop import philox_draws
    L = 96
    d, state, mels, aux = _inputs(B, L, 540 + B)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    draws = philox_draws(SEED, 2, B, L, 11, "MOL")
    whole_p, _ = loop.generate(cond, seed=SEED, row_offset=2)
    whole_i, _ = loop.generate(cond, noise=draws)
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(11, B, geo.N_TERMS))
    chunk_p, _ = loop.generate(cond, seed=SEED, row_offset=2)
    chunk_i, _ = loop.generate(cond, noise=draws)
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    print(f"PREPARED chunked {B} row(s): Philox max |Δ| {(chunk_p - whole_p).abs().max().item():.3g}, "
          f"injected {(chunk_i - whole_i).abs().max().item():.3g}, routes {(whole_p - whole_i).abs().max().item():.3g}")
    assert torch.equal(whole_p, whole_i)
    assert torch.equal(chunk_p, whole_p)
    assert torch.equal(chunk_i, whole_i)


def test_against_reference_fixture():
    """tests/golden/loop_mol_b1.npz (the reference's own loop, injected draws, 4400 steps)."""
    fx = gf.load("loop_mol_b1")
    d, state, mels, aux, noise = gf.loop_inputs(fx)
    loop = _loop(d, state)
    out, _ = loop.generate(_cond(mels, aux), noise=torch.from_numpy(noise).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    err = np.abs(out.cpu().numpy() - fx["samples"])
    print(f"PREPARED loop_mol_b1: max |Δ| {err.max():.3g}")
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


def test_windowed_launch_unchanged(monkeypatch):
    """The windowed instantiation (streaming sessions) keeps its in-loop draws: a 22-frame utterance
    pushed in one call under Philox is generate()'s audio at the same seed and row offset, bit for
    bit."""
    from wavernn_amd.fatchord_version import WaveRNN
    monkeypatch.delenv("WRNN_PATH", raising=False)
    fx = gf.load("gen_mol_unbatched")
    d, state, mel, _ = gf.gen_inputs(fx)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    m.eval()
    mel = mel[None]
    T = mel.shape[2]
    want = m.generate(torch.from_numpy(mel), None, False, 11000, 550, False, seed=20240611, row_offset=5, verbose=False)
    assert m.loop_handle().info["last_path"] == 5
    with m.stream(1, T, seed=20240611, row_offset=5) as s:
        got = np.concatenate([s.push(mel), s.finish()], 1)[0]
    assert m.loop_handle().info["last_path"] == 5
    assert got.shape == want.shape
    print(f"PREPARED streamed vs generate(): max |Δ| {np.abs(got - want).max():.3g}")
    np.testing.assert_array_equal(got, want)
