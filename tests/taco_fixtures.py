"""What the Tacotron tests share: the recorded fixtures (tests/golden/taco_*.npz), the seeded models
they were recorded with, and the bound of a forced step."""
import functools
import os

import numpy as np
import torch

from wavernn_amd import synthetic as syn
from wavernn_amd.tacotron import Tacotron

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = syn.DEFAULT_TACOTRON
REGIMES = {"tame": 1.0, "lively": 2.0, "saturated": 3.5}
SEED = 11
FIELDS = ("attn_hidden", "rnn1_hidden", "rnn1_cell", "rnn2_hidden", "rnn2_cell", "context", "cumulative", "attention",
          "frame")


@functools.lru_cache(maxsize=None)
def load_steps(regime):
    with np.load(os.path.join(GOLDEN, f"taco_steps_{regime}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    assert str(fx["state_sha256"]) == syn.state_digest(_state(regime)), "the seeded weights changed"
    return fx


@functools.lru_cache(maxsize=None)
def load_runs():
    with np.load(os.path.join(GOLDEN, "taco_runs.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _state(regime):
    return syn.make_tacotron_state(DIMS, seed=SEED, scale=REGIMES[regime])


def make_model(regime, r=2, stop_threshold=None, device=None):
    m = Tacotron(**DIMS.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _state(regime).items()})
    m.r = r
    if stop_threshold is not None:
        m.stop_threshold.fill_(stop_threshold)
    return m.to(device) if device is not None else m


def decoder_weights(regime):
    return {k[len("decoder."):]: v for k, v in _state(regime).items() if k.startswith("decoder.") and k != "decoder.r"}


def step_cases(fx):
    """(case, T, r, k, enc, proj) for every recorded step; the inputs are regenerated and their digest checked."""
    for case in [str(c) for c in fx["cases"]]:
        T, r = int(case[1:case.index("_")]), int(case[case.index("_r") + 2:])
        enc, proj = syn.make_encoder_seq(T, DIMS.decoder_dims, seed=100 + T)
        assert syn.digest(enc, proj) == str(fx[f"{case}.inputs_sha256"])
        for k in [int(k) for k in fx["record_at"]]:
            yield case, T, r, k, enc, proj


def step_bound(fx, case, k):
    """max(1e-6, 8 d1): d1 is the reference's own float32-against-float64 deviation on this step."""
    return max(1e-6, 8.0 * float(fx[f"{case}.{k}.d1"]))
