"""GPU parity in the full-amplitude regime (tests/regimes.py): every loop kernel through the C-ABI
with its WRNN_PATH forced, injected noise, wrnn_info.last_path asserted, against the C oracle.
MoL |Δ| <= MOL_TOL (1e-5) per sample; RAW and deepmind labels bit-exact.

What these inputs reach and the standard generator never does — the sampler's [-1, 1] clamp on
about a fifth of the samples each side, selected log-scales below the log(1e-14) floor on over a
third of the steps and above -1 on some, means outside +-1, x = +-1 fed back into GRU1's rank-1
form, gates pinned to 0 / 1 / +-1 with exp at inf, 0 and denormal, RAW heads where over half the
classes underflow and both end labels are drawn — is asserted on the CPU, for the same seeds and
shapes, in tests/test_regimes.py, together with the spread of the two CPU references (<= 2e-6).

The floor's value itself cannot show under an absolute bound (exp(-32.236) = 1e-14 beside a mean of
order 1); test_mol_log_scale_floor_value checks it relatively on a state whose floor components
have mean exactly 0.

A case over tolerance prints the first row-step with |Δ| > 1e-6 and the oracle's sampler trace
there (component, raw log-scale, pre-clamp sample): a jump at one step is a wrong operation, smooth
growth from 1e-7 is amplified gate rounding."""
import numpy as np
import pytest
import torch

from tests import regimes as rg
from tests.golden import fixtures as gf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDES = ("WRNN_PATH", "WRNN_TERMS_MB", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_SPARSE")


def _cond(mels, aux):
    return torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)


def _env(case, monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    if case.path:
        monkeypatch.setenv("WRNN_PATH", case.path)
    if case.budget is not None:
        monkeypatch.setenv("WRNN_TERMS_MB", case.budget)


def _run_fatchord(case, monkeypatch):
    from wavernn_amd.loop import FatchordLoop
    d, state, mels, aux, noise, ref, ref_lab, logits = rg.fatchord_inputs(*case.input_key)
    _env(case, monkeypatch)
    loop = FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0)
    if case.path == "xcdm" and loop.info["xcdm_rows"] == 0:
        pytest.skip("many-row XCD kernel unavailable on this device")
    loop.set_weights(state)
    out, lab = loop.generate(_cond(mels, aux), noise=torch.from_numpy(noise.copy()).to(DEV),
                             want_labels=d.mode == "RAW")
    info = loop.info
    loop.close()
    if case.want_path == 6 and info["last_path"] != 6:
        pytest.skip(f"sparse XCD kernel not selected (path {info['last_path']})")
    want = 9 if case.path == "rows" and info["last_path"] == 9 else case.want_path   # streamed-weights rows
    assert info["last_path"] == want, (case.id, info["last_path"])
    return out.cpu().numpy(), (lab.cpu().numpy() if lab is not None else None), ref, ref_lab, logits, noise


def _mol_report(case, out, ref, logits, noise) -> str:
    err = np.abs(out - ref)
    bad = np.argwhere(err > 1e-6)
    msg = f"{case.id}: max |Δ| {err.max():.3g}"
    if len(bad):
        order = np.lexsort((bad[:, 0], bad[:, 1]))            # earliest step first
        b, t = (int(v) for v in bad[order[0]])
        tr = rg.mol_trace(logits, noise)
        msg += (f"; first |Δ| > 1e-6 at row {b} step {t}: got {out[b, t]!r} want {ref[b, t]!r}, component "
                f"{int(tr['comp'][b, t])}, raw log-scale {float(tr['raw_ls'][b, t]):.4f}, pre-clamp sample "
                f"{float(tr['pre'][b, t])!r}; {len(bad)} of {err.size} over 1e-6")
    return msg


@pytest.mark.parametrize("case", rg.MOL_CASES, ids=lambda c: c.id)
def test_mol_hot_regime_vs_oracle(case, monkeypatch):
    out, _, ref, _, logits, noise = _run_fatchord(case, monkeypatch)
    assert out.shape == ref.shape
    msg = _mol_report(case, out, ref, logits, noise)
    print("REGIME " + msg)
    assert np.isfinite(out).all(), msg
    assert np.abs(out - ref).max() <= gf.MOL_TOL, msg
    assert np.abs(out).max() <= 1.0, msg          # the clamp's bounds are exact, not a rounding matter


@pytest.mark.parametrize("case", rg.FLOOR_CASES, ids=lambda c: c.id)
def test_mol_log_scale_floor_value(case, monkeypatch):
    """Where the selected component has mean 0 and a log-scale below the floor the sample is
    exp(floor) · u = ±1e-14 · u: the only place the floor's value shows (beside a mean of order 1
    it is lost to rounding, and under MOL_TOL it is invisible at any value).  There the kernel must
    agree with the oracle relatively, within regimes.FLOOR_REL_TOL = 1e-5 (derived there from the
    roundings of the two sides); MOL_TOL holds on every sample as everywhere."""
    out, _, ref, _, logits, noise = _run_fatchord(case, monkeypatch)
    msg = _mol_report(case, out, ref, logits, noise)
    mask = rg.floor_only_mask(rg.mol_trace(logits, noise))
    assert mask.sum() >= 10
    rel = rg.floor_rel_error(out, ref, mask)
    print(f"REGIME {msg}; {int(mask.sum())} floor-only row-steps, relative error {rel:.3g}")
    assert np.abs(out - ref).max() <= gf.MOL_TOL, msg
    assert rel <= rg.FLOOR_REL_TOL, f"{case.id}: floor-only samples off by {rel:.3g} relative"


@pytest.mark.parametrize("case", rg.RAW_CASES, ids=lambda c: c.id)
def test_raw_hot_regime_labels_bit_exact(case, monkeypatch):
    out, lab, ref, ref_lab, _, _ = _run_fatchord(case, monkeypatch)
    eq = lab == ref_lab
    print(f"REGIME {case.id}: {int((~eq).sum())} label mismatches of {eq.size}")
    assert eq.all(), f"{case.id}: {eq.mean():.6f} equal, first mismatch (row, step) {tuple(np.argwhere(~eq)[0])}"
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("case", rg.DM_CASES, ids=lambda c: c.id)
def test_deepmind_hot_regime_labels_bit_exact(case, monkeypatch):
    from wavernn_amd.loop import DeepmindLoop
    d, state, noise, ref = rg.deepmind_inputs(*case.input_key)
    _env(case, monkeypatch)
    loop = DeepmindLoop(d.hidden_size, d.quantisation)
    loop.set_weights(state)
    _, comb = loop.generate(case.B, case.L, noise=torch.from_numpy(noise.copy()).to(DEV))
    path = loop.info["last_path"]
    loop.close()
    assert path in (case.want_path, 10 if case.want_path == 3 else case.want_path), (case.id, path)
    eq = comb.cpu().numpy().astype(np.int64) == ref
    print(f"REGIME {case.id}: {int((~eq).sum())} label mismatches of {eq.size}")
    assert eq.all(), f"{case.id}: {eq.mean():.6f} equal, first mismatch (row, step) {tuple(np.argwhere(~eq)[0])}"


@pytest.mark.parametrize("batched", [False, True], ids=["unbatched", "batched"])
def test_dropin_generate_hot_regime(batched, monkeypatch):
    """The drop-in WaveRNN.generate() with no override on the hot rnn-512 MoL state, 24 frames,
    unbatched (one row) and folded with target 1500 / overlap 200 (4 rows, one per XCD): the XCD
    kernel both times, against oracle.generate within 2·MOL_TOL — the bound of the whole-generate()
    comparison in tests/test_torch_cpu_baseline.py.  This entry forms the conditioning terms at
    frame rate with a GEMM on the scaled, composed weights: another fp32 rounding of the
    conditioning than wrnn_generate sees."""
    from wavernn_amd.fatchord_version import WaveRNN
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    d, state, mel, noise, ref = rg.generate_inputs(batched)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    got = m.generate(torch.from_numpy(mel.copy())[None], None, batched, rg.GEN_TARGET, rg.GEN_OVERLAP, False,
                     noise=noise.copy(), verbose=False)
    path = m.loop_handle().info["last_path"]
    assert path == 5, path
    assert got.shape == ref.shape
    diff = np.abs(got - ref)
    print(f"REGIME generate-{'batched' if batched else 'unbatched'}: max |Δ| {diff.max():.3g}")
    first = int(np.argmax(diff > 1e-6)) if (diff > 1e-6).any() else None
    assert diff.max() <= 2 * gf.MOL_TOL, f"max |Δ| {diff.max():.3g}, first sample over 1e-6: {first}"
