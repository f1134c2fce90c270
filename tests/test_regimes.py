"""CPU conditions on the full-amplitude cases of tests/regimes.py, for exactly the seeds and shapes
tests/test_gpu_regimes.py runs on the GPU:

  * the two independent fp32 CPU restatements (the C oracle in the reference's operation order,
    and oracle/torch_cpu.py through ATen) agree: MoL max |Δ| <= 2e-6, RAW / deepmind labels equal.
    This keeps a chaotic input out of the suite (GRU gain 8 diverges to |Δ| = 2 within 400 steps)
    and leaves MOL_TOL = 1e-5 a 5x margin over the reference's own spread.  A seed that fails it is
    replaced or its gain lowered, the bound stays.
  * the regime is reached, asserted on the oracle's output and its logits trace, so a later change
    to the generator cannot quietly stop these cases from testing it.

The share conditions (each clamp on >= 3 % of row-steps, every mixture component selected five
times, ...) are statistics and need a sample to hold: they are asserted on every case of at least
FULL_ROW_STEPS = 300 row-steps.  The smaller cases of the GPU matrix (one row x 120 steps, the
one-step-per-launch cases of 12 steps, 2 x 60 and 3 x 60 at rnn 896) cannot meet counts such as
10 components x 5 selections; they run the same state as a full case (dense rnn 896: the same
construction) and assert that each event occurs at all: both clamps, a log-scale below the floor, a
mean outside +-1, and x = +-1 fed back."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle, torch_cpu
from tests import regimes as rg
from wavernn_amd import synthetic as syn

PAIR_TOL = 2e-6
GEN_PAIR_TOL = 4e-6
FULL_ROW_STEPS = 300
SLOW_ROW_STEPS = 2500          # the C oracle costs about 0.8 ms per row-step at rnn 512


def _params(cases):
    return [pytest.param(c, id=f"{c.model}-{c.B}x{c.L}",
                         marks=[pytest.mark.slow] if c.B * c.L >= SLOW_ROW_STEPS else [])
            for c in rg.distinct_inputs(cases)]


@pytest.mark.parametrize("case", _params(rg.MOL_CASES))
def test_mol_references_agree_and_regime_reached(case):
    d, state, mels, aux, noise, ref, _, logits = rg.fatchord_inputs(*case.input_key)
    got = torch_cpu.loop(state, "MOL", torch.from_numpy(mels.copy()), torch.from_numpy(aux.copy()), noise.copy())
    pair = float(np.abs(got - ref).max())
    tr = rg.mol_trace(logits, noise)
    n = ref.size
    hi, lo = float(np.mean(ref == 1.0)), float(np.mean(ref == -1.0))
    inside = float(np.mean(np.abs(ref) < 1.0))
    below = float(np.mean(tr["raw_ls"] < rg.LOG_SCALE_MIN))
    wide = int(np.sum(tr["raw_ls"] > -1.0))
    mean_out = int(np.sum(np.abs(tr["mean"]) > 1.0))
    comps = np.bincount(tr["comp"].ravel(), minlength=10)
    fed_back = int(np.sum(np.abs(ref[:, :-1]) == 1.0))
    print(f"{case.id}: C oracle vs torch max |Δ| {pair:.3g}; x=+1 {hi:.3f}, x=-1 {lo:.3f}, inside {inside:.3f}, "
          f"raw log-scale below floor {below:.3f}, above -1: {wide}, mean outside ±1: {mean_out}, "
          f"selections per component {comps.tolist()}, x(t-1)=±1: {fed_back} of {n}")
    assert pair <= PAIR_TOL
    # the numpy trace restates the oracle's sampler: same clamp decisions
    assert np.array_equal(np.clip(tr["pre"], -1.0, 1.0) == 1.0, ref == 1.0)
    assert np.array_equal(np.clip(tr["pre"], -1.0, 1.0) == -1.0, ref == -1.0)
    assert inside >= 0.5
    assert below >= 0.10
    assert mean_out >= 1 and fed_back >= 1
    if n >= FULL_ROW_STEPS:
        share = 0.02 if case.model == "sparse896" else 0.03
        assert hi >= share and lo >= share
        assert comps.min() >= 5
        assert wide >= 1
    else:
        assert hi > 0 and lo > 0


@pytest.mark.parametrize("case", _params(rg.FLOOR_CASES))
def test_floor_value_cases(case):
    """The cases that show the value of the log-scale floor (regimes.FLOOR_REL_TOL): enough
    row-steps whose sample is exp(floor) · u alone, and the two CPU references agree on them
    relatively as well as absolutely."""
    d, state, mels, aux, noise, ref, _, logits = rg.fatchord_inputs(*case.input_key)
    got = torch_cpu.loop(state, "MOL", torch.from_numpy(mels.copy()), torch.from_numpy(aux.copy()), noise.copy())
    mask = rg.floor_only_mask(rg.mol_trace(logits, noise))
    rel = rg.floor_rel_error(got, ref, mask)
    pair = float(np.abs(got - ref).max())
    print(f"{case.id}: {int(mask.sum())} of {ref.size} row-steps are exp(floor)·u alone (|x| <= "
          f"{np.abs(ref[mask]).max():.3g}); C oracle vs torch there: relative {rel:.3g}; everywhere: max |Δ| {pair:.3g}")
    assert mask.sum() >= max(10, ref.size // 10)
    assert (np.abs(ref[mask]) < 1e-12).all() and (ref[mask] != 0).all()
    assert pair <= PAIR_TOL and rel <= rg.FLOOR_REL_TOL


@pytest.mark.parametrize("case", [c for c in rg.MOL_CASES if c.budget], ids=lambda c: c.id)
def test_clamped_sample_crosses_a_launch_boundary(case):
    """One step per launch: every step boundary is a launch boundary, so a clamped x at any step
    but the last is carried into the next launch.  Both signs must occur."""
    ref = rg.fatchord_inputs(*case.input_key)[5]
    assert (ref[:, :-1] == 1.0).any() and (ref[:, :-1] == -1.0).any()


@pytest.mark.parametrize("case", _params(rg.RAW_CASES))
def test_raw_references_agree_and_regime_reached(case):
    d, state, mels, aux, noise, ref, lab, logits = rg.fatchord_inputs(*case.input_key)
    got = torch_cpu.loop(state, "RAW", torch.from_numpy(mels.copy()), torch.from_numpy(aux.copy()), noise.copy())
    mism = int((got != ref).sum())
    uf = float(np.mean(rg.raw_underflow_share(logits) > 0.5))
    n0, n1 = int((lab == 0).sum()), int((lab == d.n_classes - 1).sum())
    print(f"{case.id}: {mism} label mismatches C oracle vs torch; label 0: {n0}, label {d.n_classes - 1}: {n1}, "
          f"{len(np.unique(lab))} distinct labels; steps with over half the classes at exp = 0: {uf:.3f}")
    assert mism == 0
    assert n0 >= 3 and n1 >= 3
    assert uf >= 0.10
    assert (ref[lab == 0] == -1.0).all() and (ref[lab == d.n_classes - 1] == 1.0).all()


@pytest.mark.parametrize("case", _params(rg.DM_CASES))
def test_deepmind_references_agree(case):
    d, state, noise, ref = rg.deepmind_inputs(*case.input_key)
    got = torch_cpu.deepmind_loop(state, case.B, noise.copy(), case.L)
    mism = int((got != ref).sum())
    print(f"{case.id}: {mism} label mismatches C oracle vs torch, {len(np.unique(ref))} distinct outputs")
    assert mism == 0


def test_pinned_units_reach_every_slice_and_saturate():
    """Three pinned units in every 16-unit slice, every pattern used, and the pinned values do what
    their comment says in fp32 (the libm the C oracle calls)."""
    for H in (64, 512, 896):
        pins = rg.pinned_units(H)
        assert {u // rg.PIN_SLICE for u, _ in pins} == set(range(H // rg.PIN_SLICE))
        assert {p for _, p in pins} == set(rg.PIN_PATTERNS)
    for s0 in range(0, 896, 28):                      # the 28-unit slices of an rnn-896 workgroup
        assert sum(s0 <= u < s0 + 28 for u, _ in rg.pinned_units(896)) >= 4
    f = np.float32
    with np.errstate(over="ignore"):
        sig = lambda x: f(1) / (f(1) + np.exp(f(-x), dtype=f))          # noqa: E731
        assert sig(20.0) == 1 and sig(90.0) == 1 and sig(100.0) == 1 and np.tanh(f(20.0)) == 1
        assert np.isinf(np.exp(f(90.0))) and sig(-90.0) == 0 and sig(-104.0) == 0
        assert 0 < np.exp(f(-100.0)) < np.finfo(f).tiny                    # denormal
    st = rg.hot_state("mol512")
    base = syn.make_fatchord_state(syn.DEFAULT_MOL, rg.STATE_SEED)
    R = 512
    changed = np.flatnonzero(st["rnn1.bias_ih_l0"] != base["rnn1.bias_ih_l0"])
    assert set(changed % R) <= {u for u, _ in rg.pinned_units(R)} and len(changed) >= len(rg.pinned_units(R))


def test_standard_generator_stays_narrow():
    """Why tests/regimes.py exists: under the standard generator no sample reaches the clamp and no
    selected log-scale reaches the floor (DEFAULT_MOL, state seed 7, 4 rows x 400 steps)."""
    d = syn.DEFAULT_MOL
    state = syn.make_fatchord_state(d, 7)
    mels, aux = syn.make_conditioning(4, 400, d.feat_dims, d.res_out_dims, 8)
    noise = syn.make_noise("MOL", 4, 400, d.n_classes, 9)
    ref, _, logits = oracle.fatchord_loop(state, "MOL", mels, aux, noise, want_logits=True)
    tr = rg.mol_trace(logits, noise)
    print(f"standard generator: max |x| {np.abs(ref).max():.3f}, raw log-scale in "
          f"[{tr['raw_ls'].min():.2f}, {tr['raw_ls'].max():.2f}], selected |mean| max {np.abs(tr['mean']).max():.3f}")
    assert not (np.abs(ref) == 1.0).any() and np.abs(ref).max() < 0.5
    assert tr["raw_ls"].min() > rg.LOG_SCALE_MIN and np.abs(tr["mean"]).max() < 1.0


def test_want_logits_leaves_the_samples_unchanged():
    d, state, mels, aux, noise, ref, _, logits = rg.fatchord_inputs("tinymol", 3, 200)
    plain, lab = oracle.fatchord_loop(state, "MOL", mels, aux, noise)
    assert lab is None and np.array_equal(plain, ref)
    assert logits.shape == (3, 200, 30) and np.isfinite(logits).all()


@pytest.mark.slow
@pytest.mark.parametrize("batched", [False, True], ids=["unbatched", "batched"])
def test_generate_references_agree(batched):
    """The end-to-end input of the GPU generate() case: torch_cpu.timed_generate vs oracle.generate."""
    d, state, mel, noise, ref = rg.generate_inputs(batched)
    r = torch_cpu.timed_generate(state, d, mel.copy(), batched, rg.GEN_TARGET, rg.GEN_OVERLAP, False, noise.copy())
    pair = float(np.abs(r["wave"] - ref).max())
    out = r["out"]
    print(f"generate batched={batched}: {r['rows']} rows x {r['L']} steps, max |Δ| {pair:.3g}, "
          f"x=+1 {np.mean(out == 1.0):.3f}, x=-1 {np.mean(out == -1.0):.3f}")
    assert r["rows"] == (4 if batched else 1)
    assert pair <= GEN_PAIR_TOL
    assert np.mean(out == 1.0) >= 0.03 and np.mean(out == -1.0) >= 0.03


def _stream_param(key):
    from tests import geometries as geo
    model, geom, n_utt, frames, seed = key
    row_steps = n_utt * frames * geo.geom_dims(geom).hop_length
    return pytest.param(key, id=f"{model}-{geom}-{n_utt}x{frames}",
                        marks=[pytest.mark.slow] if row_steps >= SLOW_ROW_STEPS else [])


@pytest.mark.parametrize("key", [_stream_param(k) for k in rg.STREAM_HOT])
def test_stream_hot_inputs_agree_and_reach_both_clamps(key):
    """The hot streaming inputs of tests/test_gpu_streaming_shapes.py (the hop-275 one is
    generate_inputs(False): test_generate_references_agree[unbatched]).  Per utterance,
    torch_cpu.timed_generate against the oracle.generate output the GPU tests expect; over the whole
    input, the loop output at x = +1 and x = −1 on >= 3 % of row-steps each (every input here has at
    least FULL_ROW_STEPS), and regimes.stream_clamps reads the same events off the oracle's audio.
    Seeds: dense hop12 state seed 7 (pair 8.3e-7, x=+1 0.035, x=−1 0.104), sparse hop12 state seed
    12 (pair 6.6e-7, x=+1 0.110, x=−1 0.326): the first seed tried met every condition."""
    inp = rg.stream_inputs(*key)
    d, n_utt = inp.dims, key[2]
    outs, pair = [], 0.0
    for u in range(n_utt):
        r = torch_cpu.timed_generate(inp.state, d, inp.mels[u].copy(), False, 0, 0, False,
                                     np.ascontiguousarray(inp.noise[:, u:u + 1]))
        assert r["rows"] == 1 and r["wave"].shape == inp.ref[u].shape
        pair = max(pair, float(np.abs(r["wave"] - inp.ref[u]).max()))
        outs.append(r["out"])
    out = np.concatenate(outs, 0)
    hi, lo = float(np.mean(out == 1.0)), float(np.mean(out == -1.0))
    print(f"stream {key}: {out.shape[0]} rows x {out.shape[1]} steps, max |Δ| {pair:.3g}, x=+1 {hi:.3f}, x=-1 {lo:.3f}")
    assert pair <= GEN_PAIR_TOL
    if out.size >= FULL_ROW_STEPS:
        assert hi >= 0.03 and lo >= 0.03
    else:
        assert hi > 0 and lo > 0
    # the events as the GPU tests read them off the oracle's audio: the same steps, the fade included
    pos, neg = rg.stream_clamps(inp.ref, d.hop_length)
    n = pos.shape[1]
    assert np.array_equal(pos, out[:, :n] == 1.0) and np.array_equal(neg, out[:, :n] == -1.0)
    assert pos.any() and neg.any()


def test_stream_inputs_follow_the_geometry_table():
    """Every geometry's standard input: the frame weights the table states (asserted inside
    stream_inputs on the state the GPU sees), one expectation per utterance, different utterances."""
    from tests import geometries as geo
    for geom in geo.ODD:
        inp = rg.stream_inputs("std512", geom, 3, 24, rg.STREAM_STD_SEED)
        d = inp.dims
        assert (d.feat_dims, d.upsample_factors, d.pad) == geo.GEOMS[geom][:3] and d.rnn_dims == 512
        assert inp.mels.shape == (3, d.feat_dims, 24) and inp.noise.shape == (24 * d.hop_length, 3, 11)
        assert inp.ref.shape == (3, 23 * d.hop_length) and np.isfinite(inp.ref).all()
        assert np.abs(inp.ref[0] - inp.ref[1]).max() > 1e-3 and np.abs(inp.ref[1] - inp.ref[2]).max() > 1e-3
        assert np.abs(inp.ref).max() < 1.0            # the narrow regime: the hot inputs are the others


def test_oracle_build_follows_its_source(tmp_path, monkeypatch):
    """oracle.build() rebuilds when the recorded digest differs from the source's (a stale library
    with the old orc_fatchord_loop signature would be called with one argument too many), and not
    otherwise.  Runs on a copy of the source in a temporary directory."""
    src = os.path.join(oracle.HERE, "wavernn_oracle.c")
    work = tmp_path / "oracle"
    work.mkdir()
    with open(src, "rb") as f:
        (work / "wavernn_oracle.c").write_bytes(f.read())
    lib_path = str(work / "_build" / "liboracle.so")
    monkeypatch.setattr(oracle, "HERE", str(work))
    monkeypatch.setattr(oracle, "LIB_PATH", lib_path)
    monkeypatch.setattr(oracle, "STAMP_PATH", lib_path + ".sha256")
    oracle.build()
    first = os.stat(lib_path).st_ino, os.stat(lib_path).st_mtime_ns
    oracle.build()
    assert (os.stat(lib_path).st_ino, os.stat(lib_path).st_mtime_ns) == first       # up to date: untouched
    with open(work / "wavernn_oracle.c", "ab") as f:
        f.write(b"\n/* changed */\n")
    os.utime(work / "wavernn_oracle.c", ns=(0, 0))                                  # older than the library
    oracle.build()
    assert (os.stat(lib_path).st_ino, os.stat(lib_path).st_mtime_ns) != first
