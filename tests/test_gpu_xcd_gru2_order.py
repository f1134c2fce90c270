"""The XCD-resident kernel's GRU2 gate order (fatchord_xcd.hip): the r and z rows of an engine's
two units reduce-scattered to its lanes 0..3 (one sigmoid pass), the n rows reduced under it, tanh
and h' in lanes 0 and 2 — so h2, y and the carried h2 slots come from lanes 0 and 2 — and the fc3
partial logits of the fc2 waves (lane l: logit l & 31 over the workgroup's f2 rows).

Shapes are the smallest at which a wrong lane -> unit -> gate mapping reaches the logits within two
steps: 40 steps of one row (and of eight rows, one per XCD) against the C oracle; 96 steps in many
launches for the carried state.  The synthetic weights are i.i.d. uniform: every unit, every fc3
row and column distinct, so neither two swapped units nor a swapped logit half can cancel.

Tolerances as tests/test_gpu_xcd_wave_roles.py: |Δ| <= MOL_TOL against the oracle under injected
noise, 2·MOL_TOL between launch splits under Philox; in-kernel draws against their injected
restatement bit for bit."""
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


def _rows_vs_oracle(B, seed, monkeypatch):
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref = _oracle_case(B, STEPS, seed)
    loop = _loop(d, state)
    out, _ = loop.generate(_cond(mels, aux), noise=torch.from_numpy(np.array(noise)).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    err = np.abs(out.cpu().numpy() - ref)
    print(f"{B} row(s) x {STEPS} steps: max |Δ| {err.max():.3g}")
    return err


@pytest.mark.parametrize("B", [1, 8])
def test_gru2_order_rows_vs_oracle(B, monkeypatch):
    """One row, and eight rows in one launch (one per XCD), 40 steps each, every sample against
    the oracle: the gates of unit 4·g + 2j + e from lanes 2j, 2j + 1 of engine e, y from lanes 0, 2."""
    err = _rows_vs_oracle(B, 310 + B, monkeypatch)
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


def test_gru2_order_carried_state(monkeypatch):
    """h2own through the state record from lanes 0 and 2: 1 row x 96 steps with a terms budget of
    0.25 MiB — 65 536 floats against 5 120 terms per step and row, so at most 11 steps per launch
    and at least 9 launches — against the same call in one launch (Philox), and against the oracle
    under injected noise."""
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref = _oracle_case(1, 96, 330)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    whole, _ = loop.generate(cond, seed=7)
    monkeypatch.setenv("WRNN_TERMS_MB", "0.25")
    chunked, _ = loop.generate(cond, seed=7)
    out, _ = loop.generate(cond, noise=torch.from_numpy(np.array(noise)).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    diff = (chunked - whole).abs().max().item()
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"chunked vs one launch max |Δ| {diff:.3g}; chunked vs oracle max |Δ| {err:.3g}")
    assert diff <= 2 * gf.MOL_TOL
    assert err <= gf.MOL_TOL
    loop.close()


def test_gru2_order_philox_equals_restated_injection(monkeypatch):
    """1 row x 40 steps: the in-kernel draws give the audio of the same call with the draws
    injected from oracle/philox.py's restatement, bit for bit."""
    from oracle import philox as ph
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, _, _ = _oracle_case(1, STEPS, 311)
    loop = _loop(d, state)
    cond = _cond(mels, aux)
    seed, r0 = 0xD1B54A32D192ED03, 5
    y0, _ = loop.generate(cond, seed=seed, row_offset=r0)
    assert loop.info["last_path"] == 5, loop.info
    noise = ph.philox_draws(seed, r0, 1, 0, STEPS, 11, mol=True)
    y1, _ = loop.generate(cond, noise=torch.from_numpy(noise).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    diff = (y0 - y1).abs().max().item()
    print(f"Philox vs restated injection max |Δ| {diff:.3g}")
    assert torch.equal(y0, y1), diff
    loop.close()


def test_fc3_partials_distinct_rows(monkeypatch):
    """8 rows x 40 steps on a weight state whose fc3 rows (logits) and columns (f2 rows) are all
    distinct, so logits exchanged between lanes < 16 and >= 16, or f2 rows between the DPP rows
    that hold them, cannot cancel: every sample against the oracle."""
    _, state, *_ = _oracle_case(8, STEPS, 318)
    w3 = np.asarray(state["fc3.weight"])
    assert len(np.unique(w3, axis=0)) == w3.shape[0] and len(np.unique(w3, axis=1).T) == w3.shape[1]
    err = _rows_vs_oracle(8, 318, monkeypatch)
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
