"""Inputs, expectations and the driver of the RAW wide-session tests (tests/test_gpu_stream_wide_raw.py):
a RAW 9-bit rnn / fc 512 model at one of the geometries of tests/geometries.py, mels for U utterances,
injected Exp(1) draws [steps][U][512] by absolute step, and what oracle.generate (unbatched) makes of
ONE utterance alone — its own mel truncated to its own length, its own column of the draws.

The bound (`check`).  The RAW head promises labels, and a label fixes the sample: x = label_to_x(label)
is one fp32 value per class, the float64 post is a widening, so with mu_law off every sample outside
the fade-out equals the oracle's bit for bit (np.array_equal), and inside it (the last 20·hop samples:
one float64 product with numpy's linspace element) within rtol 1e-12, atol 0.  With mu_law on every
sample passes pow() in float64, whose last bits differ between libm and the device: rtol 1e-12
throughout, the project's existing RAW post bound.  Labels are recovered from the mu_law-off body as
round((x + 1)·511 / 2) (`labels_of`: the body is integral to 1.5e-5).

Plain module: no test in here."""
import functools
from dataclasses import dataclass
from typing import Dict

import numpy as np

from tests import geometries as geo
from tests import regimes as rg
from wavernn_amd import synthetic as syn

NC = 512                       # kMRawNC: the classes of the many-row kernel's softmax head (bits = 9)
N_RAW = 32 * 144 + NC          # terms + draws of one row-step: the RAW share of the WRNN_TERMS_MB budget
FADE_FRAMES = 20
DEV = "cuda:0"


@dataclass(frozen=True)
class RawInput:
    dims: syn.FatchordDims
    state: Dict[str, np.ndarray]
    mels: np.ndarray      # [U][feat][T]
    noise: np.ndarray     # [T·hop][U][512] Exp(1)


@functools.lru_cache(maxsize=None)
def inputs(geom: str, n_utt: int, frames: int, seed: int, hot: bool = False, draws: bool = True, **dims_kw) -> RawInput:
    """key = (geom, n_utt, frames, seed[, hot[, draws]]): computed once per process and shared
    (read-only).  hot: rg.hot_fatchord_state at the raw512 regime's gain and end-class biases (full
    amplitude).  draws=False: no injected draws (Philox cases; noise is empty)."""
    kw = dict(rnn_dims=512, mode="RAW")
    kw.update(dims_kw)
    d = geo.geom_dims(geom, **kw)
    if hot:
        state = rg.hot_fatchord_state(d, seed, rg.MODELS["raw512"][1], raw_end_bias=rg.RAW_END_BIAS["raw512"])
    else:
        state = {k: np.array(v, copy=True) for k, v in syn.make_fatchord_state(d, seed).items()}
    geo.perturb_taps(state, d, seed)
    mels = np.stack([syn.make_mel(d.feat_dims, frames, 1000 * seed + 40 + i) for i in range(n_utt)])
    noise = syn.make_noise("RAW", n_utt, frames * d.hop_length if draws else 0, d.n_classes, 1000 * seed + 21)
    for a in (mels, noise):
        a.setflags(write=False)
    return RawInput(d, state, mels, noise)


@functools.lru_cache(maxsize=None)
def alone(key, u: int, T: int, mu_law: bool) -> np.ndarray:
    """oracle.generate of utterance u of inputs(*key) alone on its first T frames: float64 [(T − 1)·hop]."""
    from oracle import oracle
    inp = inputs(*key)
    hop = inp.dims.hop_length
    ref = oracle.generate(inp.state, inp.dims, np.ascontiguousarray(inp.mels[u][:, :T]), False, 0, 0, mu_law,
                          np.ascontiguousarray(inp.noise[:T * hop, u:u + 1]))
    assert ref.shape == ((T - 1) * hop,) and ref.dtype == np.float64
    ref.setflags(write=False)
    return ref


def labels_of(wave: np.ndarray, hop: int) -> np.ndarray:
    """Class labels of the samples before the fade-out of a mu_law-off waveform [..][(T − 1)·hop]."""
    body = (wave[..., :-FADE_FRAMES * hop] + 1.0) * (NC - 1) / 2.0
    lab = np.rint(body)
    assert np.abs(body - lab).max() <= 1e-4, "not a mu_law-off RAW waveform"
    return lab.astype(np.int64)


def check(out: np.ndarray, ref: np.ndarray, hop: int, mu_law: bool, what: str) -> None:
    """The bound of the module docstring; prints the figures before it asserts."""
    assert out.shape == ref.shape and out.dtype == np.float64, (what, out.shape, ref.shape, out.dtype)
    cut = out.shape[-1] - FADE_FRAMES * hop
    neq = out != ref
    denom = np.where(ref == 0, 1.0, np.abs(ref))
    rel = float((np.abs(out - ref) / denom).max())
    print(f"RAW WIDE {what}: {int(neq[..., :cut].sum())} of {neq[..., :cut].size} body samples differ, "
          f"{int(neq[..., cut:].sum())} in the fade, max rel {rel:.3g} (mu_law {mu_law})")
    if not mu_law:
        if neq[..., :cut].any():
            at = tuple(np.argwhere(neq[..., :cut])[0])
            raise AssertionError(f"{what}: first differing sample before the fade at {at}: {out[at]!r} vs oracle {ref[at]!r}")
        np.testing.assert_allclose(out[..., cut:], ref[..., cut:], rtol=1e-12, atol=0, err_msg=what)
    else:
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0, err_msg=what)


def model(inp: RawInput, key, _cache={}):
    """One WaveRNN on the GPU per input key, shared by the tests."""
    import torch
    from wavernn_amd.fatchord_version import WaveRNN
    if key not in _cache:
        m = WaveRNN(**inp.dims.ctor_kwargs()).to(DEV)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in inp.state.items()}, strict=True)
        _cache[key] = m.eval()
    return _cache[key]


class Member:
    """One wide RAW session of a group: the utterances `rows` of an input (an index may repeat)
    truncated to T frames, its schedule (one entry per tick: None = not listed, else (frames, final)),
    whether the total is announced, injected draws or a Philox key, mu_law."""

    def __init__(self, key, rows, T, sched, total=None, philox=None, mu_law=False):
        inp = inputs(*key)
        hop = inp.dims.hop_length
        rows = [rows] if isinstance(rows, int) else list(rows)
        self.key, self.rows, self.U, self.T, self.sched, self.total = key, rows, len(rows), T, sched, total
        self.hop, self.mu_law = hop, mu_law
        self.mel = np.ascontiguousarray(inp.mels[rows][:, :, :T])
        self.kw = {"wide": True, "mu_law": mu_law}
        if philox is None:
            self.kw["noise"] = np.ascontiguousarray(inp.noise[:T * hop][:, rows])
        else:
            self.kw.update(seed=philox[0], row_offset=philox[1])
        assert sum(e[0] for e in sched if e) == T and [e[1] for e in sched if e].count(True) == 1 and sched[-1][1]

    def ref(self):
        return np.stack([alone(self.key, u, self.T, self.mu_law) for u in self.rows])


def sched(counts, start=0, final_with_frames=False):
    """A schedule: not listed for `start` ticks, then one push per count (0: an empty push), the
    final flag on the last count's push or on an empty push after it."""
    s = [None] * start + [(n, False) for n in counts]
    if final_with_frames:
        s[-1] = (counts[-1], True)
    else:
        s.append((0, True))
    return s


def run(m, members, grouped=True, between=None):
    """Drive the members through their schedules: per tick one push_streams over the members listed
    (grouped), or every member's whole session alone through push().  Every push must return exactly
    the count stream_plan announces.  → ([U][(T − 1)·hop] per member, last_path)."""
    import torch
    from wavernn_amd.loop import stream_plan
    spec = m._upsample_spec()

    def want(mb, f, n, final):
        return stream_plan(spec, f + n, final, mb.total)[1] - stream_plan(spec, f, False, mb.total)[1]

    def chunk(mb, f, n):
        return mb.mel[:, :, f:f + n] if n else None

    chunks = [[] for _ in members]
    if not grouped:
        for i, mb in enumerate(members):
            with m.stream(mb.U, mb.total, **mb.kw) as s:
                f = 0
                for e in mb.sched:
                    if e is None:
                        continue
                    n, final = e
                    t = torch.from_numpy(chunk(mb, f, n).copy()).to(DEV) if n else None
                    out = s._session.push(t, final=final).cpu().numpy()
                    assert out.shape == (mb.U, want(mb, f, n, final)), (i, f, out.shape)
                    chunks[i].append(out)
                    f += n
        return [np.concatenate(c, 1) for c in chunks], m.loop_handle().info["last_path"]
    sess, f = [None] * len(members), [0] * len(members)
    try:
        for tick in range(max(len(mb.sched) for mb in members)):
            listed = [i for i, mb in enumerate(members) if tick < len(mb.sched) and mb.sched[tick] is not None]
            for i in listed:
                if sess[i] is None:
                    sess[i] = m.stream(members[i].U, members[i].total, **members[i].kw)
            pushes = [(sess[i], chunk(members[i], f[i], members[i].sched[tick][0]), members[i].sched[tick][1]) for i in listed]
            outs = m.push_streams(pushes) if pushes else []
            assert len(outs) == len(listed)
            for i, out in zip(listed, outs):
                n, final = members[i].sched[tick]
                assert out.dtype == np.float64 and out.shape == (members[i].U, want(members[i], f[i], n, final)), (tick, i, out.shape)
                chunks[i].append(out)
                f[i] += n
            if between:
                between(tick)
        path = m.loop_handle().info["last_path"]
    finally:
        for s in sess:
            if s is not None:
                s.close()
    return [np.concatenate(c, 1) for c in chunks], path


def launch_plan(m, members):
    """The persistent launches of every tick of a grouped run under the WRNN_TERMS_MB in force: per
    tick (rows with a step to run, steps per launch the library takes for them, launches wide_plan
    cuts the members' runnable steps into at that count)."""
    from wavernn_amd.loop import stream_plan, wide_plan, wide_steps_per_launch
    spec = m._upsample_spec()
    f = [0] * len(members)
    ticks = []
    for tick in range(max(len(mb.sched) for mb in members)):
        steps, rows = [], []
        for i, mb in enumerate(members):
            if tick < len(mb.sched) and mb.sched[tick] is not None:
                n, final = mb.sched[tick]
                steps.append(stream_plan(spec, f[i] + n, final, mb.total)[0] - stream_plan(spec, f[i], False, mb.total)[0])
                rows.append(mb.U)
                f[i] += n
        live = sum(r for s, r in zip(steps, rows) if s > 0)
        if live == 0:
            ticks.append((0, 0, 0))
            continue
        per = wide_steps_per_launch(live, max(steps), raw=True)
        ticks.append((live, per, len(wide_plan(steps, rows, per))))
    return ticks
