"""The XCD-resident kernel's row-packed dot products (fatchord_xcd.hip, xcd_device.h: e32part2,
fc8_rows_rp): every packed FMA of the three on-chain segments — GRU2's W_ih2 rows, fc1, fc2 —
multiplies the weights of TWO rows at one K index by one input value, so the register-resident
weights are loaded as interleaved row pairs ((a_r, a_z), (b_r, b_z), (a_n, b_n) on the GRU2 waves,
rows (2p, 2p + 1) on the fc waves) and each accumulator half is a whole in-lane row sum.

What goes wrong if the pairing is off: a row's weights meet another row's accumulator half (two
gates, two units or two fc rows exchanged), or a weight meets the wrong input of the lane's eight
(fc) or sixteen (GRU2).  With i.i.d. weights none of these can cancel, and each reaches the logits
within two steps.  The five instantiations of the kernel are compiled separately (their register
allocation differs), so each is run: one launch (1 and 8 rows), the windowed form (chunked
launches), the grouped form (group pushes) and the list form (generate_list).

Shapes are the smallest that do this: 40 steps wrap the 4-step ring ten times and both hop
parities; 8 rows put one row on every XCD; 96 steps at 11 steps per launch are 9 launches.
References are the C oracle's, computed once per process and shared with the files whose helpers are used here (tests/test_gpu_xcd_gru2_order.py, tests/test_gpu_stream_group.py,
tests/regimes.py).

Measured on MI355X (max |Δ| against the oracle): 1 row 3.4e-8, 8 rows 4.8e-8; 96 steps under
Philox 3.7e-8, chunked and one launch bit-identical; grouped 3.2e-8, list 3.5e-8; hot state
7.8e-7 with 405 clamped samples.

Tolerances are the project's: |Δ| <= MOL_TOL against the oracle's loop under injected noise,
2·MOL_TOL between launch splits under Philox and for whole generate() comparisons."""
import numpy as np
import pytest
import torch

from tests import geometries as geo
from tests import regimes as rg
from tests import test_gpu_stream_group as sg
from tests import test_gpu_xcd_gru2_order as g2o
from tests.golden import fixtures as gf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 40


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in sg.OVERRIDES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("B", [1, 8])
def test_row_packed_rows_vs_oracle(B, monkeypatch):
    """One row, and eight rows in one launch (one per XCD), 40 steps, every sample against the
    oracle under injected noise."""
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref = g2o._oracle_case(B, STEPS, 410 + B)
    loop = g2o._loop(d, state)
    out, _ = loop.generate(g2o._cond(mels, aux), noise=torch.from_numpy(np.array(noise)).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    err = np.abs(out.cpu().numpy() - ref)
    print(f"ROW-PACKED {B} row(s) x {STEPS} steps: max |Δ| {err.max():.3g}")
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


def test_row_packed_chunked_launches_philox(monkeypatch):
    """1 row x 96 steps under Philox with the terms budget that tests/geometries.py works out for 11
    steps per launch — 9 launches of the windowed instantiation with the state carried between them
    (the library does not report its launch count; the budget rule is the one the chunking tests
    of tests/test_gpu_stream_group.py and tests/test_gpu_generate_list.py rely on) — against the
    same call in one launch (2·MOL_TOL), and against the oracle fed the restated draws (MOL_TOL)."""
    from oracle import oracle
    from oracle import philox as ph
    monkeypatch.setenv("WRNN_PATH", "xcd")
    L, per_launch = 96, 11   # ⌈96 / 11⌉ = 9 launches
    d, state, mels, aux, _, _ = g2o._oracle_case(1, L, 430)
    seed, r0 = 0x9E3779B97F4A7C15, 3
    draws = ph.philox_draws(seed, r0, 1, 0, L, 11, mol=True)
    ref, _ = oracle.fatchord_loop(state, "MOL", mels, aux, draws)
    loop = g2o._loop(d, state)
    cond = g2o._cond(mels, aux)
    whole, _ = loop.generate(cond, seed=seed, row_offset=r0)
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(per_launch, 1, geo.N_TERMS))
    chunked, _ = loop.generate(cond, seed=seed, row_offset=r0)
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    diff = (chunked - whole).abs().max().item()
    err_w = np.abs(whole.cpu().numpy() - ref).max()
    err_c = np.abs(chunked.cpu().numpy() - ref).max()
    print(f"ROW-PACKED chunked vs one launch max |Δ| {diff:.3g}; vs oracle: one launch {err_w:.3g}, chunked {err_c:.3g}")
    assert diff <= 2 * gf.MOL_TOL
    assert err_w <= gf.MOL_TOL and err_c <= gf.MOL_TOL


def test_row_packed_grouped_launch():
    """The grouped instantiation at the group tests' smallest dense shape: two U = 1 sessions of 21
    and 24 frames at hop 12 with uneven pushes, each against oracle.generate of its utterance."""
    inp, m = sg._case(*sg.RAGGED)
    members = [sg.Member(sg.RAGGED, 0, 1, 21, sg.sched([5] + [1] * 16)),
               sg.Member(sg.RAGGED, 1, 1, 24, sg.sched([11, 3, 3, 3, 3, 1]))]
    sg._check(m, members, "row-packed grouped 21/24", alone=False)


def test_row_packed_list_launch():
    """The list instantiation: three utterances of 21, 24 and 30 frames at hop 12 queued on two
    lanes (one lane runs two pieces), injected draws, each against oracle.generate of its utterance
    (the group tests' references)."""
    inp, m = sg._case(*sg.RAGGED)
    hop = inp.dims.hop_length
    Ts = (21, 24, 30)
    mels = [np.array(inp.mels[u][None, :, :T], order="C") for u, T in enumerate(Ts)]
    noise = [np.array(inp.noise[:T * hop, u], order="C") for u, T in enumerate(Ts)]
    got = m.generate_list(mels, noise=noise, lanes=2)
    assert m.loop_handle().info["last_path"] == 5
    for u, T in enumerate(Ts):
        ref = sg._alone(sg.RAGGED, u, T)
        assert got[u].shape == ref.shape == ((T - 1) * hop,)
        err = float(np.abs(got[u] - ref).max())
        print(f"ROW-PACKED list utterance {u} ({T} frames): max |Δ| {err:.3g}")
        assert err <= 2 * gf.MOL_TOL


def test_row_packed_full_amplitude(monkeypatch):
    """Saturated gates and sampler clamps: the hot rnn-512 state of tests/regimes.py (gates pinned
    to 0 / 1 / ±1, x = ±1 fed back; its CPU preconditions are tests/test_regimes.py's), 8 rows x
    120 steps, every sample against the oracle, the clamp bounds exact."""
    from wavernn_amd.loop import FatchordLoop
    monkeypatch.setenv("WRNN_PATH", "xcd")
    d, state, mels, aux, noise, ref, _, _ = rg.fatchord_inputs("mol512", 8, 120)
    assert (ref == 1.0).any() and (ref == -1.0).any()
    loop = FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0)
    loop.set_weights(state)
    out, _ = loop.generate(g2o._cond(mels, aux), noise=torch.from_numpy(noise.copy()).to(DEV))
    assert loop.info["last_path"] == 5, loop.info
    loop.close()
    out = out.cpu().numpy()
    err = np.abs(out - ref)
    print(f"ROW-PACKED hot 8 x 120: max |Δ| {err.max():.3g}, {int((np.abs(ref) == 1.0).sum())} clamped samples")
    assert np.isfinite(out).all()
    assert err.max() <= gf.MOL_TOL, f"max |Δ| {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    assert np.abs(out).max() <= 1.0
