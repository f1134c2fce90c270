"""The XCD-resident kernel's wave roles (fatchord_xcd.h): GRU2 on waves 0, 5, 6, 7 with two units
per engine, fc1 / fc2 waves that hold no W_ih2, W_hh2 rows spread over waves 1..7 and LDS.

Shapes are the smallest at which that mapping can go wrong: a wrong unit -> wave -> slab row, or a
wrong W_hh2 row holder, reaches the logits within two steps, so 40 steps of one row (and of eight
rows, one per XCD) against the C oracle; 96 steps in many launches for the carried state's slots.
The synthetic weights are i.i.d. uniform, every unit distinct: a swap of two units cannot cancel.

Tolerances as tests/test_gpu_xcd.py: |Δ| <= MOL_TOL against the oracle under injected noise,
2·MOL_TOL between launch splits under Philox; in-kernel draws against their injected restatement
bit for bit (tests/test_gpu_philox.py)."""
import functools

import numpy as np
import pytest
import torch

from tests.golden import fixtures as gf
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 40


def _loop(d, state):
    from wavernn_amd.loop import FatchordLoop
    loop = FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0)
    assert loop.info["xcd_rows"] == 8, loop.info
    loop.set_weights(state)
    return loop


def _cond(mels, aux):
    return torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _oracle_case(B, L, seed):
    """Inputs and the oracle's samples, computed once per (B, L, seed) and never modified."""
    from oracle import oracle
    d = syn.DEFAULT_MOL
    state = syn.make_fatchord_state(d, seed)
    mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, seed + 1)
    noise = syn.make_noise("MOL", B, L, d.n_classes, seed + 2)
    ref, _ = oracle.fatchord_loop(state, "MOL", mels, aux, noise)
    for a in (mels, aux, noise, ref):
        a.setflags(write=False)
    return d, state, mels, aux, noise, ref


@pytest.mark.parametrize("B", [1, 8])
def test_wave_roles_rows_vs_oracle(B, monkeypatch):
    """One row, and eight rows in one launch (one per XCD: membership and the per-XCD hop areas with
    the new publishers), 40 steps each, every sample against the oracle."""
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref = _oracle_case(B, STEPS, 210 + B)
    loop = _loop(d, state)
    out, _ = loop.generate(_cond(mels, aux), noise=torch.from_numpy(np.array(noise)).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    err = np.abs(out.cpu().numpy() - ref)
    print(f"{B} row(s) x {STEPS} steps: max |Δ| {err.max():.3g}")
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    loop.close()


def test_wave_roles_carried_state(monkeypatch):
    """h2 of the GRU2 lanes and W_hh2·h2 through the carried state: 1 row x 96 steps with a terms
    budget of 0.25 MiB — 65 536 floats against 5 120 terms per step and row, so at most 11 steps
    per launch and at least 9 launches — against the same call in one launch (Philox, the
    tolerance of test_xcd_time_chunks_carry_state), and against the oracle under injected noise."""
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref = _oracle_case(1, 96, 230)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    whole, _ = loop.generate(cond, seed=5)
    monkeypatch.setenv("WRNN_TERMS_MB", "0.25")
    chunked, _ = loop.generate(cond, seed=5)
    out, _ = loop.generate(cond, noise=torch.from_numpy(np.array(noise)).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    diff = (chunked - whole).abs().max().item()
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"chunked vs one launch max |Δ| {diff:.3g}; chunked vs oracle max |Δ| {err:.3g}")
    assert diff <= 2 * gf.MOL_TOL
    assert err <= gf.MOL_TOL
    loop.close()


def test_wave_roles_philox_equals_restated_injection(monkeypatch):
    """1 row x 40 steps: the in-kernel draws give the audio of the same call with the draws
    injected from oracle/philox.py's restatement, bit for bit."""
    from oracle import philox as ph
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, _, _ = _oracle_case(1, STEPS, 211)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    seed, r0 = 0x9E3779B97F4A7C15, 3
    y0, _ = loop.generate(cond, seed=seed, row_offset=r0)
    assert loop.info["last_path"] == 5, loop.info
    noise = ph.philox_draws(seed, r0, 1, 0, STEPS, 11, mol=True)
    y1, _ = loop.generate(cond, noise=torch.from_numpy(noise).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    diff = (y0 - y1).abs().max().item()
    print(f"Philox vs restated injection max |Δ| {diff:.3g}")
    assert torch.equal(y0, y1), diff
    loop.close()
