"""One handle through every host-side store the list, streaming and one-shot entry points share
(csrc/host_ctx.h: StagedTable; capi_loops.cpp: upload_coef; capi_lists.cpp: ListArena,
wide_list_front): the staged piece and row tables (device table, pinned staging copy, upload event), the cached frame weights, the list arena and the grow-only
workspaces.

One MoL rnn / fc 512 model at the smallest geometry of the list tests (tests/geometries.py "hop2") runs,
on ONE handle: the lane list, the wide list and the folded list of 3 utterances of 21 … 24 frames, a
wide group push of two sessions (and their final push), a plain generate(), then the three lists again
in the reverse order with 9 utterances of 21 … 40 frames — so every grow-only workspace and both staged
tables are reallocated while an earlier upload's event exists, and the frame weights one entry point
uploaded serve the next.  Every output must be np.array_equal to the same call on a handle of its own
(a fresh model), with injected draws and a fixed seed: what a stale pointer, a table rewritten under an
upload in flight, an arena offset of the earlier list or a frame-weight table of another call would
change."""
import numpy as np
import pytest
import torch

from tests import geometries as geo
from wavernn_amd import synthetic as syn
from wavernn_amd.loop import list_folds_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOM = "hop2"
HOP = 2
TARGET, OVERLAP = geo.GEOMS[GEOM][6][1:]          # (10, 2)
FRAMES_A = (21, 24, 22)
FRAMES_B = (40, 21, 33, 27, 38, 24, 30, 21, 36)
SESSION = ((30, 12), (26, 9))                     # (total frames, frames of the first push) per session
SEED, ROW0 = 20250301, 3
STATE_SEED = geo.TAP_SEED


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("WRNN_PATH", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_MR_FRAMES", "WRNN_TERMS_MB"):
        monkeypatch.delenv(k, raising=False)


class Inputs:
    def __init__(self):
        self.dims = geo.geom_dims(GEOM, rnn_dims=512)
        assert self.dims.hop_length == HOP and self.dims.mode == "MOL"
        self.state = geo.perturb_taps(syn.make_fatchord_state(self.dims, STATE_SEED), self.dims, STATE_SEED)
        self.mels = [syn.make_mel(self.dims.feat_dims, 40, 500 + i) for i in range(len(FRAMES_B))]

    def model(self):
        from wavernn_amd.fatchord_version import WaveRNN
        m = WaveRNN(**self.dims.ctor_kwargs()).to(DEV)
        m.load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in self.state.items()}, strict=True)
        return m.eval()

    def mel(self, i, T):
        return np.array(self.mels[i][None, :, :T], order="C")

    def draws(self, i, T):
        return syn.make_noise("MOL", 1, T * HOP, self.dims.n_classes, 900 + i)[:, 0]

    def fold_draws(self, i, T):
        folds = list_folds_plan([T], HOP, TARGET, OVERLAP)[0][0]
        return syn.make_noise("MOL", folds, TARGET + 2 * OVERLAP, self.dims.n_classes, 700 + i)


def _calls(inp):
    """name → callable(model) → list of arrays, in the order the shared handle runs them."""
    def lanes(frames):
        def run(m):
            return m.generate_list([inp.mel(i, T) for i, T in enumerate(frames)], seed=SEED, row_offset=ROW0,
                                   noise=[inp.draws(i, T) for i, T in enumerate(frames)])
        return run

    def wide(frames):
        def run(m):
            return m.generate_list([inp.mel(i, T) for i, T in enumerate(frames)], wide=True, seed=SEED, row_offset=ROW0,
                                   noise=[inp.draws(i, T) for i, T in enumerate(frames)])
        return run

    def folds(frames):
        def run(m):
            return m.generate_list([inp.mel(i, T) for i, T in enumerate(frames)], wide=True, batched=True, target=TARGET,
                                   overlap=OVERLAP, seed=SEED, row_offset=ROW0,
                                   noise=[inp.fold_draws(i, T) for i, T in enumerate(frames)])
        return run

    def sessions(m):
        ss = [m.stream(1, T, noise=inp.draws(4 + k, T)[:, None], seed=SEED, row_offset=ROW0 + 20 + k, wide=True)
              for k, (T, _) in enumerate(SESSION)]
        try:
            mels = [inp.mel(4 + k, T) for k, (T, _) in enumerate(SESSION)]
            first = m.push_streams([(s, x[:, :, :n], False) for s, x, (_, n) in zip(ss, mels, SESSION)])
            last = m.push_streams([(s, x[:, :, n:], True) for s, x, (_, n) in zip(ss, mels, SESSION)])
        finally:
            for s in ss:
                s.close()
        assert all(a.shape[1] > 0 for a in first), "the first push emitted nothing: the group ran no step"
        return list(first) + list(last)

    def one(m):
        T = 23
        return [m.generate(inp.mel(8, T), None, False, 0, 0, False, noise=inp.draws(8, T)[:, None], seed=SEED,
                           row_offset=ROW0, verbose=False)]

    return [("lane list of 3", lanes(FRAMES_A)), ("wide list of 3", wide(FRAMES_A)), ("folded list of 3", folds(FRAMES_A)),
            ("wide group push of two sessions", sessions), ("generate", one),
            ("folded list of 9", folds(FRAMES_B)), ("wide list of 9", wide(FRAMES_B)), ("lane list of 9", lanes(FRAMES_B))]


def test_one_handle_against_fresh_handles():
    inp = Inputs()
    calls = _calls(inp)
    shared = inp.model()
    got = [(name, run(shared)) for name, run in calls]
    handle = shared.loop_handle()
    for name, run in calls:
        fresh = inp.model()
        want = run(fresh)
        fresh.loop_handle().close()
        mine = dict(got)[name]
        assert len(mine) == len(want) and len(want) > 0, name
        for i, (a, b) in enumerate(zip(mine, want)):
            assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and a.size > 0, (name, i, a.shape, b.shape)
            assert np.array_equal(a, b), f"{name}, output {i}: the shared handle differs from a fresh one, " \
                                         f"max |Δ| {np.abs(a - b).max():.3g}"
            assert len(np.unique(a)) > 8, f"{name}, output {i}: a constant waveform"
    assert shared.loop_handle() is handle, "the shared model repacked its handle on the way"
