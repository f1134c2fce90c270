"""Full-amplitude ("hot") inputs for the parity tests, and the traces that prove a run reached them.

`synthetic.make_fatchord_state` / `make_deepmind_state` keep every run in a narrow range
(DEFAULT_MOL, seed 7, 4 rows × 400 steps: max |x| = 0.18, no sample at ±1, gate pre-activations
below 2), so the suite built on them alone never executes the MoL sampler's [-1, 1] clamp, its
log-scale floor log(1e-14) (utils/distribution.py:96-97, 114-115 in the reference), a selected
mean outside ±1, x = ±1 fed back into the rank-1 GRU1 form, a saturated gate, or a softmax head
whose classes underflow to probability 0.  This module builds states that do, from the standard
generator's output (which it leaves untouched: the golden fixtures store digests of it), and
lists the cases the CPU condition tests (tests/test_regimes.py) and the GPU parity tests
(tests/test_gpu_regimes.py) share, so the conditions are checked on exactly what the GPU sees.

Plain module: no test in here."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from wavernn_amd import synthetic as syn
from wavernn_amd.pruning import prune_state

LOG_SCALE_MIN = np.float32(-32.23619130191664)    # float(np.log(1e-14)), distribution.py:114-115
# fc3.bias of the ten log-scales: four components below, at or just above the floor, then narrow
# (a trained vocoder's −9 … −3) to wide ones whose draw leaves [-1, 1]
HOT_LOG_SCALE_BIAS = (-40.0, -36.0, -33.0, -32.0, -9.0, -7.0, -5.0, -3.0, -1.0, 0.5)
LOGIT_GAIN, MEAN_GAIN = 8.0, 6.0
RAW_HEAD_GAIN = 8.0                               # on top of the generator's × 16
# Classes 0 and n_classes − 1 (x = ∓1 exactly).  With the head at × 128 the logits spread over
# about 75 (measured: std 12, max − min 75), and expf(l − max) is 0 only below −103.97, so no class
# underflows; the two end rows get a further gain, which makes their logit swing over ±100: where
# it is high most other classes underflow and the end label is drawn, where it is low the rest of
# the head decides as before.  Tuned on the CPU (tests/test_regimes.py asserts the outcome).
RAW_END_ROW_GAIN = 24.0
# fc3.bias added to (class 0, class n − 1): centres each end logit, which the x = ∓1 feedback
# drives far negative, near −55 (its swing is ±100 to ±150)
RAW_END_BIAS = {"raw512": (88.0, 383.0), "tinyraw": (214.0, 138.0), "raw10": (88.0, 170.0)}
DM_R_GAIN = 4.0

# Gate-bias extremes (r, z, n) of one pinned unit; None leaves the generator's value.
#   ±20   the gate is 0 / 1 / ±1 in fp32 once the exponential is below half an ulp of 1
#   ±90   exp overflows to inf on one side (1 / (1 + inf) = 0) and vanishes on the other
#   −104  the issue's r / z entry (exp(104) = inf); +100: exp(−100) = 3.8e-44 is denormal in libm
#         and flushed to zero by the hardware exponential, 1 + e is 1 either way
PIN_PATTERNS = (
    (20.0, None, None), (-20.0, None, None), (None, 20.0, None), (None, -20.0, None),
    (None, None, 20.0), (None, None, -20.0), (90.0, None, 90.0), (-90.0, -90.0, None),
    (None, 90.0, -90.0), (-104.0, -104.0, None), (100.0, 100.0, None),
)
PIN_SLICE, PIN_OFFSETS = 16, (1, 6, 11)


def pinned_units(H: int):
    """(unit, pattern) pairs: three units in every 16-unit slice (so at least four in every
    28-unit slice an rnn-896 workgroup owns), the patterns taken in turn so every workgroup gets
    several kinds and eleven consecutive pins cover all of them."""
    out, n = [], 0
    for s0 in range(0, H, PIN_SLICE):
        for off in PIN_OFFSETS:
            if s0 + off < H:
                out.append((s0 + off, PIN_PATTERNS[n % len(PIN_PATTERNS)]))
                n += 1
    return out


def _pin_gates(r: np.ndarray, z: np.ndarray, n: np.ndarray) -> None:
    for u, (pr, pz, pn) in pinned_units(r.shape[0]):
        for vec, p in ((r, pr), (z, pz), (n, pn)):
            if p is not None:
                vec[u] = np.float32(p)


def hot_fatchord_state(d: syn.FatchordDims, seed: int, gru_gain: float, pinned: bool = True,
                       sparsity: Optional[float] = None, raw_end_bias=None,
                       zero_floor_means: bool = False) -> Dict[str, np.ndarray]:
    """`syn.make_fatchord_state(d, seed)` moved into the full-amplitude regime (module docstring).
    `sparsity`: prune the GRU weights (pruning.prune_state) after scaling them.
    `zero_floor_means`: the four components whose log-scale lies at or below the floor get a mean of
    exactly 0 (zero fc3 row and bias), so their sample is exp(floor) · u alone and shows the
    floor's value; beside a mean of order 1 that term, 1e-14, is lost to fp32 rounding."""
    st = {k: np.array(v, copy=True) for k, v in syn.make_fatchord_state(d, seed).items()}
    f32 = np.float32
    if d.mode == "MOL":
        w, b = st["fc3.weight"], st["fc3.bias"]
        w[0:10] *= f32(LOGIT_GAIN)
        w[10:20] *= f32(MEAN_GAIN)
        b[20:30] = np.asarray(HOT_LOG_SCALE_BIAS, f32)
        if zero_floor_means:
            w[10:14] = 0
            b[10:14] = 0
    else:
        st["fc3.weight"] = (st["fc3.weight"] * f32(RAW_HEAD_GAIN)).astype(f32)
        for c, bias in zip((0, -1), raw_end_bias or (0.0, 0.0)):
            st["fc3.weight"][c] *= f32(RAW_END_ROW_GAIN)
            st["fc3.bias"][c] += f32(bias)
    for name in ("rnn1", "rnn2"):
        for k in ("weight_ih_l0", "weight_hh_l0"):
            st[f"{name}.{k}"] = (st[f"{name}.{k}"] * f32(gru_gain)).astype(f32)
    if sparsity is not None:
        st = {k: np.array(v, copy=True) for k, v in prune_state(st, sparsity).items()}
    if pinned:
        R = d.rnn_dims
        for name in ("rnn1", "rnn2"):
            b = st[f"{name}.bias_ih_l0"]           # [r | z | n] (torch GRUCell layout)
            _pin_gates(b[0:R], b[R:2 * R], b[2 * R:3 * R])
    return st


def hot_deepmind_state(d: syn.DeepmindDims, seed: int, pinned: bool = True) -> Dict[str, np.ndarray]:
    """`syn.make_deepmind_state(d, seed)` with R.weight × 4 and the same pinned extremes on
    bias_r / bias_u / bias_e (r, update and candidate gates, deepmind_version.py:122-125)."""
    st = {k: np.array(v, copy=True) for k, v in syn.make_deepmind_state(d, seed).items()}
    st["R.weight"] = (st["R.weight"] * np.float32(DM_R_GAIN)).astype(np.float32)
    if pinned:
        _pin_gates(st["bias_r"], st["bias_u"], st["bias_e"])
    return st


# ------------------------------------------------------------------------------- traces
def mol_trace(logits: np.ndarray, noise: np.ndarray) -> Dict[str, np.ndarray]:
    """What the MoL sampler did at every row-step, recomputed in fp32 numpy from the oracle's
    logits [B][L][30] and the injected draws [L][B][11] (distribution.py:87-123): the selected
    component, its mean, its raw log-scale and the sample before the [-1, 1] clamp."""
    u = np.ascontiguousarray(noise.transpose(1, 0, 2), np.float32)           # [B][L][11]
    v = logits[..., :10] - np.log(-np.log(u[..., :10]))
    comp = v.argmax(axis=-1)                                                   # first max on ties
    mean = np.take_along_axis(logits[..., 10:20], comp[..., None], -1)[..., 0]
    raw_ls = np.take_along_axis(logits[..., 20:30], comp[..., None], -1)[..., 0]
    ls = np.maximum(raw_ls, LOG_SCALE_MIN)
    u2 = u[..., 10]
    pre = (mean + np.exp(ls) * (np.log(u2) - np.log(np.float32(1.0) - u2))).astype(np.float32)
    return {"comp": comp, "mean": mean, "raw_ls": raw_ls, "pre": pre,
            "u": (np.log(u2) - np.log(np.float32(1.0) - u2)).astype(np.float32)}


# The floor's value is visible only where nothing else is: the sample exp(floor) · u of a component
# with mean 0.  Both sides form it from the same draws, so they differ by rounding alone: the
# hardware exponential takes exp2(ls · log2 e), whose fp32 product at |ls · log2 e| = 46.5 carries
# half an ulp = 1.9e-6, i.e. 1.3e-6 relative after the exponential; v_exp_f32, libm's expf and the
# product with u add an ulp (1.2e-7) each; u = log u2 − log(1 − u2) differs by the two logs' ulps
# (6e-8 each, at values near 0.7), 1.2e-6 relative once |u| >= 0.1 is required (it cancels to 0 at
# u2 = 1/2).  Together under 3e-6; the bound leaves 3x, and a floor of −30 for −32.236 is a factor 9.4.
FLOOR_REL_TOL = 1e-5
FLOOR_MIN_U = 0.1


def floor_only_mask(trace: Dict[str, np.ndarray]) -> np.ndarray:
    """Row-steps whose sample is exp(floor) · u and nothing else (mean exactly 0, raw log-scale
    below the floor, |u| >= FLOOR_MIN_U)."""
    return (trace["mean"] == 0) & (trace["raw_ls"] < LOG_SCALE_MIN) & (np.abs(trace["u"]) >= FLOOR_MIN_U)


def floor_rel_error(out: np.ndarray, ref: np.ndarray, mask: np.ndarray) -> float:
    return float(np.abs(out[mask].astype(np.float64) / ref[mask].astype(np.float64) - 1.0).max())


def raw_underflow_share(logits: np.ndarray) -> np.ndarray:
    """Per row-step, the share of classes whose softmax numerator expf(l − max) is 0 in fp32."""
    z = (logits - logits.max(axis=-1, keepdims=True)).astype(np.float32)
    return (np.exp(z) == 0).mean(axis=-1)


# -------------------------------------------------------------------------------- cases
DENSE896_MOL = syn.SPARSE896_MOL                      # the same dims, unpruned
RAW10 = syn.FatchordDims(bits=10, mode="RAW")
MODELS = {
    # name: (dims, GRU gain, sparsity)
    "mol512": (syn.DEFAULT_MOL, 4.0, None),
    "mol512floor": (syn.DEFAULT_MOL, 4.0, None),          # zero_floor_means
    "sparse896": (syn.SPARSE896_MOL, 12.0, 0.95),
    "dense896": (DENSE896_MOL, 4.0, None),
    "tinymol": (syn.TINY_MOL, 4.0, None),
    "raw512": (syn.DEFAULT_RAW, 4.0, None),
    "tinyraw": (syn.TINY_RAW, 4.0, None),
    "raw10": (RAW10, 4.0, None),
}
DM_MODELS = {"dm896": syn.DEFAULT_DM, "dmtiny": syn.TINY_DM}
STATE_SEED = 7
ONE_STEP_BUDGET_MB = "0.0001"                         # WRNN_TERMS_MB: every launch one step


@dataclass(frozen=True)
class Case:
    model: str
    path: str             # WRNN_PATH ("" = the default entry)
    B: int
    L: int
    want_path: int        # wrnn_info.last_path
    budget: Optional[str] = None
    seed: int = STATE_SEED

    @property
    def id(self) -> str:
        return f"{self.model}-{self.path or 'default'}-{self.B}x{self.L}" + ("-1step" if self.budget else "")

    @property
    def input_key(self):
        return (self.model, self.B, self.L, self.seed)


# wrnn_info.last_path: latency 1, rows 2 (deepmind rows 3), split 4, xcd 5, sparse xcd 6,
# many-row xcd 7, deepmind xcd 8, streamed-weights rows 9
MOL_CASES = [
    Case("mol512", "xcd", 1, 120, 5), Case("mol512", "xcd", 8, 120, 5),
    Case("mol512", "xcdm", 10, 120, 7),      # one quad: every workgroup samples
    Case("mol512", "xcdm", 40, 80, 7),       # two quads: row-owner sampler + x hop
    Case("mol512", "xcdm", 72, 60, 7),       # three quads: the 16x16x4 form
    Case("mol512", "split", 1, 120, 4), Case("mol512", "latency", 1, 120, 1),
    Case("mol512", "rows", 3, 120, 2),
    Case("mol512", "xcd", 3, 12, 5, ONE_STEP_BUDGET_MB), Case("mol512", "xcdm", 10, 12, 7, ONE_STEP_BUDGET_MB),
    Case("mol512", "rows", 3, 12, 2, ONE_STEP_BUDGET_MB),
    # state seed 12: at seed 7 one component is selected 3 times in 3 × 100 (5 are required)
    Case("sparse896", "", 3, 100, 6, seed=12), Case("sparse896", "rows", 3, 60, 2, seed=12),
    Case("dense896", "", 2, 60, 9),
    Case("tinymol", "rows", 3, 200, 2),
]
# the floor's value (FLOOR_REL_TOL): one case per sampler form — mol_sample_pairs (xcd, xcdm),
# mol_sample_reg (split), mol_sample (rows)
FLOOR_CASES = [
    Case("mol512floor", "xcd", 8, 120, 5), Case("mol512floor", "xcdm", 10, 120, 7),
    Case("mol512floor", "split", 1, 120, 4), Case("mol512floor", "rows", 3, 120, 2),
]
RAW_CASES = [
    Case("raw512", "xcdm", 1, 150, 7), Case("raw512", "xcdm", 10, 150, 7), Case("raw512", "xcdm", 72, 60, 7),
    Case("raw512", "rows", 3, 150, 2), Case("raw512", "latency", 1, 150, 1),
    Case("tinyraw", "rows", 3, 150, 2), Case("raw10", "rows", 3, 150, 2),
]
DM_CASES = [
    Case("dm896", "", 3, 150, 8), Case("dm896", "", 32, 60, 8), Case("dm896", "rows", 3, 150, 3),
    Case("dmtiny", "rows", 3, 150, 3),
]


def distinct_inputs(cases):
    seen, out = set(), []
    for c in cases:
        if c.input_key not in seen:
            seen.add(c.input_key)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def hot_state(model: str, seed: int = STATE_SEED):
    if model in DM_MODELS:
        return hot_deepmind_state(DM_MODELS[model], seed)
    d, gain, sparsity = MODELS[model]
    return hot_fatchord_state(d, seed, gain, sparsity=sparsity, raw_end_bias=RAW_END_BIAS.get(model),
                              zero_floor_means=model == "mol512floor")


@functools.lru_cache(maxsize=None)
def fatchord_inputs(model: str, B: int, L: int, seed: int = STATE_SEED):
    """(dims, state, mels, aux, noise, oracle samples, oracle labels, oracle logits) of a case;
    computed once per process and shared (treat as read-only)."""
    from oracle import oracle
    d = MODELS[model][0]
    state = hot_state(model, seed)
    mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, 1000 * seed + 10 * B + 1)
    noise = syn.make_noise(d.mode, B, L, d.n_classes, 1000 * seed + 10 * B + 2)
    ref, lab, logits = oracle.fatchord_loop(state, d.mode, mels, aux, noise, want_logits=True)
    for a in (mels, aux, noise, ref, logits):
        a.setflags(write=False)
    return d, state, mels, aux, noise, ref, lab, logits


@functools.lru_cache(maxsize=None)
def deepmind_inputs(model: str, B: int, L: int, seed: int = STATE_SEED):
    """(dims, state, noise, oracle combined output [B][L] int64) of a deepmind case."""
    from oracle import oracle
    d = DM_MODELS[model]
    state = hot_state(model, seed)
    noise = syn.make_dm_noise(B, L, d.quantisation, 1000 * seed + 10 * B + 3)
    _, _, ref = oracle.deepmind_loop(state, B, L, noise)
    noise.setflags(write=False)
    return d, state, noise, ref


GEN_FRAMES, GEN_TARGET, GEN_OVERLAP = 24, 1500, 200


@functools.lru_cache(maxsize=None)
def generate_inputs(batched: bool, seed: int = STATE_SEED):
    """(dims, state, mel, noise, oracle.generate output) of the end-to-end case: the hot rnn-512
    MoL state, 24 frames, unbatched or folded with target 1500 / overlap 200."""
    from oracle import oracle
    d = MODELS["mol512"][0]
    state = hot_state("mol512", seed)
    mel = syn.make_mel(d.feat_dims, GEN_FRAMES, 1000 * seed + 5)
    L = GEN_FRAMES * d.hop_length
    rows, steps = (oracle.fold_with_overlap(np.zeros((1, L, 1), np.float32), GEN_TARGET, GEN_OVERLAP).shape[:2]
                   if batched else (1, L))
    noise = syn.make_noise(d.mode, rows, steps, d.n_classes, 1000 * seed + 6 + int(batched))
    ref = oracle.generate(state, d, mel, batched, GEN_TARGET, GEN_OVERLAP, False, noise)
    for a in (mel, noise, ref):
        a.setflags(write=False)
    return d, state, mel, noise, ref


# ------------------------------------------------------------------- streaming sessions
# Inputs of tests/test_gpu_streaming_shapes.py: a model at one of the geometries of
# tests/geometries.py, mels for U utterances, injected draws by absolute step, and what
# oracle.generate (unbatched) makes of each utterance alone with its own column of the draws.
STREAM_MODELS = {
    # name: (rnn dims, GRU gain of hot_fatchord_state or None for the standard narrow state, sparsity)
    "std512": (512, None, None),
    "stdsparse896": (896, None, 0.95),
    "mol512": (512, MODELS["mol512"][1], None),
    "sparse896": (896, MODELS["sparse896"][1], MODELS["sparse896"][2]),
}
STREAM_STD_SEED = 3        # geometries.TAP_SEED: the states tests/test_gpu_frame_geometry.py runs
# The hot sessions (CPU conditions: tests/test_regimes.py): (model, geometry, U, frames, state seed).
# Dense: 2 × 24 × 12 = 576 row-steps; sparse: 2 × 30 × 12 = 720 (≤ 800 at rnn 896).
STREAM_HOT_DENSE = ("mol512", "hop12", 2, 24, STATE_SEED)
STREAM_HOT_SPARSE = ("sparse896", "hop12", 2, 30, 12)
STREAM_HOT_275 = ("mol512", "hop275", 1, GEN_FRAMES, STATE_SEED)      # generate_inputs(False)
STREAM_HOT = [STREAM_HOT_DENSE, STREAM_HOT_SPARSE]


@dataclass(frozen=True)
class StreamInput:
    dims: syn.FatchordDims
    state: Dict[str, np.ndarray]
    mels: np.ndarray      # [U][feat][T]
    noise: np.ndarray     # [T·hop][U][11]
    ref: np.ndarray       # [U][(T − 1)·hop] float64, oracle.generate per utterance


def upsample_spec(d: syn.FatchordDims, state):
    from wavernn_amd import condition
    taps = [state[f"upsample.up_layers.{2 * i + 1}.weight"] for i in range(len(d.upsample_factors))]
    return condition.UpsampleSpec(d.feat_dims, d.res_out_dims, d.pad, d.upsample_factors, taps)


@functools.lru_cache(maxsize=None)
def stream_inputs(model: str, geom: str, n_utt: int, frames: int, seed: int) -> StreamInput:
    """A streaming case's inputs and expectation; computed once per process and shared (read-only).
    ("mol512", "hop275", 1, 24, seed) is generate_inputs(False, seed), so its oracle run is shared
    with tests/test_gpu_regimes.py."""
    from oracle import oracle
    from tests import geometries as geo
    from wavernn_amd import condition
    if geom == "hop275":
        assert (model, n_utt, frames) == STREAM_HOT_275[:1] + STREAM_HOT_275[2:4]
        d, state, mel, noise, ref = generate_inputs(False, seed)
        mels, ref = mel[None], ref[None]
    else:
        rnn, gain, sparsity = STREAM_MODELS[model]
        d = geo.geom_dims(geom, rnn_dims=rnn)
        if gain is None:
            state = syn.make_fatchord_state(d, seed)
            if sparsity is not None:
                state = {k: np.array(v, copy=True) for k, v in prune_state(state, sparsity).items()}
        else:
            state = hot_fatchord_state(d, seed, gain, sparsity=sparsity)
        geo.perturb_taps(state, d, seed)
        mels = np.stack([syn.make_mel(d.feat_dims, frames, 1000 * seed + 40 + i) for i in range(n_utt)])
        noise = syn.make_noise(d.mode, n_utt, frames * d.hop_length, d.n_classes, 1000 * seed + 21)
        ref = np.stack([oracle.generate(state, d, mels[u], False, 0, 0, False, np.ascontiguousarray(noise[:, u:u + 1]))
                        for u in range(n_utt)])
    assert condition.frame_weights(upsample_spec(d, state))[:2] == geo.GEOMS[geom][3:5], geom
    assert ref.shape == (n_utt, (frames - 1) * d.hop_length) and ref.dtype == np.float64
    for a in (mels, noise, ref):
        a.setflags(write=False)
    return StreamInput(d, state, mels, noise, ref)


def stream_clamps(ref: np.ndarray, hop: int):
    """(x = +1, x = −1) per audio position of oracle.generate's output [..][(T − 1)·hop].  Its post
    multiplies the float64 copy of the last 20·hop loop samples by linspace(1, 0, 20·hop), and a
    product with ±1 is exact, so a clamped sample is ± that envelope and nothing else is (an
    unclamped fp32 sample times the envelope does not land on the envelope).  The last position,
    where the envelope is 0, is left out: every position kept is followed by another loop step."""
    env = np.ones(ref.shape[-1])
    env[-20 * hop:] = np.linspace(1, 0, 20 * hop)
    return (ref == env)[..., :-1], (ref == -env)[..., :-1]
