"""Upsample geometries other than the reference's (5, 5, 11) / pad 2, shared by
tests/test_gpu_frame_geometry.py (one-shot frame terms) and the streaming cases of tests/regimes.py
(tests/test_gpu_streaming_shapes.py): hop below the 32 steps a workgroup interpolates, 3 and 7
frame weights, pad·hop exactly the cascade's reach, four stages, an odd feature count.

Plain module: no test in here."""
import numpy as np

from wavernn_amd import synthetic as syn

# name: (feat, factors, pad, jlo, nJ, frames unbatched, (frames, target, overlap) fold-batched,
#        steps per chunk)
GEOMS = {
    # hop 12 < 32 steps per workgroup, odd feat (terms-GEMM depth 30 + 128 + 4 = 162); E = 16 < 36
    "hop12": (30, (3, 4), 3, -2, 5, 24, (60, 150, 20), 77),
    # pad·hop = 4 = E, the exactness boundary; 3 frame weights
    "hop4": (20, (4,), 1, -1, 3, 24, (24, 20, 4), 37),
    # pad·hop = 6 = E; 7 frame weights; 16 frames per workgroup
    "hop2": (80, (1, 1, 2), 3, -3, 7, 24, (24, 10, 2), 13),
    # four stages; E = 16 + 8 + 4 + 2 = 30 < 32
    "hop16": (80, (2, 2, 2, 2), 2, -2, 5, 21, (21, 70, 10), 101),
    # the reference's own geometry (chunked only: its other cases are tests/test_gpu_frame_terms.py)
    "hop275": (80, (5, 5, 11), 2, -2, 5, 21, None, 1801),
}
ODD = [g for g in GEOMS if g != "hop275"]
N_TERMS = 32 * 160            # kXcdWgs · kXTerms floats per row and step (csrc/fatchord_xcd.h)
TAP_SEED = 3                  # the state seed of every geometry model


def dims(feat, factors, pad, **kw):
    return syn.FatchordDims(feat_dims=feat, upsample_factors=tuple(factors), hop_length=int(np.prod(factors)),
                            pad=pad, compute_dims=16, res_blocks=1, **kw)


def geom_dims(name, **kw):
    feat, factors, pad = GEOMS[name][:3]
    return dims(feat, factors, pad, **kw)


def perturb_taps(state, d, seed):
    """The box taps scaled by factors in [0.5, 1.5], in place, so tap order matters."""
    rng = np.random.default_rng(100 + seed)
    for i in range(len(d.upsample_factors)):
        k = f"upsample.up_layers.{2 * i + 1}.weight"
        state[k] = (np.asarray(state[k]) * rng.uniform(0.5, 1.5, np.shape(state[k]))).astype(np.float32)
    return state


def terms_budget_mb(steps, rows, record):
    """WRNN_TERMS_MB that makes a launch loop take exactly `steps` steps: the loops take
    ⌊budget / (rows · record) − 1⌋ (budget in floats), so (steps + 1.5) · rows · record floats."""
    return repr((steps + 1.5) * rows * record * 4 / 2 ** 20)
