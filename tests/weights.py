"""Weight states for the loading tests (tests/test_weights.py proves each is what its name says on
the CPU; tests/test_gpu_weights.py loads exactly these): states on either side of every decision
wrnn_set_weights takes, the orders they are loaded in on one live handle, and the updates applied
to a live drop-in model.  No test lives here.

`block_stats` restates capi.cpp's: 4x4 blocks of W_ih2[:, :R], W_hh1, W_hh2; density over all gate
block-rows; nbmax the largest nonzero-block count of a row.  density <= 1/2 selects the sparse rows
layout (sized by nbmax); at rnn 896 nbmax <= XCDS_NB selects the XCD-resident sparse kernel.
"""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np

from wavernn_amd import synthetic as syn
from wavernn_amd.pruning import GRU_KEYS, block_mask, prune_state

SEED_A, SEED_B = 7, 8
XCDS_NB = 32                       # kSNB: block slots per gate block-row of the XCD sparse kernel
LOOP_MATS = ("rnn2.weight_ih_l0", "rnn1.weight_hh_l0", "rnn2.weight_hh_l0")   # SparseMat order
DIMS = {"tinymol": syn.TINY_MOL, "tinyraw": syn.TINY_RAW, "mol512": syn.DEFAULT_MOL, "raw512": syn.DEFAULT_RAW,
        "mol896": syn.SPARSE896_MOL}
DM_DIMS = {"dm896": syn.DEFAULT_DM, "dmtiny": syn.TINY_DM}

# nb32[k] / nb33[k]: restored blocks are the unpruned state's times NB_GAIN, in gate NB_GATE (the
# candidate gate n), block-row NB_ROW.  Measured (2 rows x 60 steps, oracle): zeroing the last
# block in column order moves some sample by 9.6e-3 / 9.1e-3 (W_ih2, 32nd / 33rd block), 2.3e-3 /
# 2.8e-3 (W_hh1) and 5.9e-3 / 4.2e-3 (W_hh2) at gain 1024 (tests/test_weights.py prints each); at
# gain 64 the W_hh1 blocks move it by 4.7e-4 only, under 100 * MOL_TOL, at gain 256 by 1.15e-3.
NB_GAIN = 1024.0
NB_GATE, NB_ROW = 2, 5
# dens_over's extra block and one_dense_row's restored row carry the same gain, so that the update
# pairs (dens_over -> dens_eq, hh_only -> one_dense_row) are visible in the output
EDGE_GAIN = 64.0
ODR_GATE, ODR_ROW = 2, 3           # one_dense_row: this gate block-row of W_hh2 restored in full


# ----------------------------------------------------------------------------- statistics
def loop_mats(state) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    R = state["rnn1.weight_hh_l0"].shape[1]
    return state[LOOP_MATS[0]][:, :R], state[LOOP_MATS[1]], state[LOOP_MATS[2]]


def block_map(W: np.ndarray) -> np.ndarray:
    """bool [rows/4][cols/4]: the 4x4 block holds a nonzero."""
    r, c = W.shape
    return (W.reshape(r // 4, 4, c // 4, 4) != 0).any(axis=(1, 3))


def block_stats(state) -> Dict[str, float]:
    maps = [block_map(m) for m in loop_mats(state)]
    per_row = np.concatenate([m.sum(1) for m in maps])
    nz, tot = int(sum(m.sum() for m in maps)), int(sum(m.size for m in maps))
    return {"nbmax": int(per_row.max()), "nbmin": int(per_row.min()), "nz": nz, "total": tot,
            "density": nz / tot}


def expect_sparse_blocks(state, sparse_env: bool = True) -> int:
    """wrnn_info.sparse_blocks after loading `state` where the sparse layout fits: nbmax (at least
    1) when density <= 1/2, else 0."""
    s = block_stats(state)
    return max(s["nbmax"], 1) if sparse_env and s["nz"] * 2 <= s["total"] else 0


LDS_BYTES = 160 * 1024             # per workgroup on MI355X
LDS_ROW_RESERVE = 16 * 1024        # one row of state, the hop buffers and the slab's small vectors


def sparse_slab_bytes(d, nbmax: int) -> int:
    """The large parts of the sparse rows slab of one workgroup (capi.cpp make_rows_slab with
    G = R / 4): nine gate block-rows of nbmax blocks and columns, the workgroup's fc1 / fc2 rows,
    and the MoL head (RAW: its share of fc3).  The sparse layout is taken only where it fits
    beside one row of state; otherwise the weights run dense (resident or streamed)."""
    R, F, G = d.rnn_dims, d.fc_dims, d.rnn_dims // 4
    uf = -(-F // G)
    head = d.n_classes * (F + 1) if d.mode == "MOL" else -(-d.n_classes // G) * (F + 1)
    return 4 * (9 * nbmax * 17 + uf * (R + F) + head)


def sparse_must_fit(d, nbmax: int) -> bool:
    """True where the sparse slab leaves LDS_ROW_RESERVE: there the 1/2 rule alone decides."""
    return sparse_slab_bytes(d, nbmax) <= LDS_BYTES - LDS_ROW_RESERVE


# ------------------------------------------------------------------------------- builders
def _copy(state):
    return {k: np.array(v, copy=True) for k, v in state.items()}


def _blk(W, br, cb):
    return W[4 * br:4 * br + 4, 4 * cb:4 * cb + 4]


def _restore(st, dense, key, br, cb, gain=1.0):
    _blk(st[key], br, cb)[...] = _blk(dense[key], br, cb) * np.float32(gain)


def _zero_blocks(st, key):
    """(block-row, block-col) of the zero blocks of the loop part of st[key], row-major."""
    R = st["rnn1.weight_hh_l0"].shape[1]
    return np.argwhere(~block_map(st[key][:, :R]))


def dens_eq(dense) -> dict:
    """prune_state(0.5) lands just under 1/2 (ties are kept per gate, the aux columns of W_ih2 are
    ranked with the rest); blocks of W_hh1 are put back, spread over its rows, until nz * 2 == total."""
    st = _copy(prune_state(dense, 0.5))
    s = block_stats(st)
    need = s["total"] // 2 - s["nz"]
    assert s["total"] % 2 == 0 and need >= 0, s
    zeros = _zero_blocks(st, "rnn1.weight_hh_l0")
    for br, cb in zeros[:: max(1, len(zeros) // max(need, 1))][:need]:
        _restore(st, dense, "rnn1.weight_hh_l0", br, cb)
    return st


def dens_over(dense) -> dict:
    st = dens_eq(dense)
    R = dense["rnn1.weight_hh_l0"].shape[1]
    zeros = _zero_blocks(st, "rnn2.weight_hh_l0")
    br, cb = zeros[zeros[:, 0] >= 2 * R // 4][0]          # a block of the candidate gate
    _restore(st, dense, "rnn2.weight_hh_l0", br, cb, EDGE_GAIN)
    return st


def hh_only(dense, z: float = 0.95) -> dict:
    """The reference pruner with prune_rnn_input off: W_hh pruned, W_ih dense."""
    st = _copy(dense)
    for k in ("rnn1.weight_hh_l0", "rnn2.weight_hh_l0"):
        st[k] = (dense[k] * block_mask(dense[k], z)).astype(np.float32)
    return st


def one_dense_row(dense, z: float = 0.95) -> dict:
    st = _copy(prune_state(dense, z))
    R = dense["rnn1.weight_hh_l0"].shape[1]
    r0 = ODR_GATE * R + 4 * ODR_ROW
    st["rnn2.weight_hh_l0"][r0:r0 + 4] = dense["rnn2.weight_hh_l0"][r0:r0 + 4] * np.float32(EDGE_GAIN)
    return st


def elementwise_mask(W: np.ndarray, z: float, splits: int = 3) -> np.ndarray:
    """The notebook's PruneMask rule on single elements: per gate slice, threshold
    sorted_abs[int(numel * z)], mask |W| >= threshold."""
    out = np.empty_like(W, dtype=np.float32)
    gs = W.shape[0] // splits
    for g in range(splits):
        a = np.abs(W[g * gs:(g + 1) * gs])
        thr = np.sort(a.reshape(-1))[min(int(a.size * z), a.size - 1)]
        out[g * gs:(g + 1) * gs] = a >= thr
    return out


def elementwise(dense, z: float) -> dict:
    st = _copy(dense)
    for k in GRU_KEYS:
        st[k] = (dense[k] * elementwise_mask(dense[k], z)).astype(np.float32)
    return st


def all_zero(dense) -> dict:
    st = _copy(dense)
    R = dense["rnn1.weight_hh_l0"].shape[1]
    st["rnn2.weight_ih_l0"][:, :R] = 0
    st["rnn1.weight_hh_l0"][...] = 0
    st["rnn2.weight_hh_l0"][...] = 0
    return st


def nb_row(R: int) -> int:
    return NB_GATE * R // 4 + NB_ROW


def nb_state(dense, k: int, count: int, gain: float = NB_GAIN) -> dict:
    """The 0.95-pruned state with blocks of one gate block-row of loop matrix k restored (from the
    highest column down, so the last block in column order is a restored one) until the row holds
    exactly `count`; every other row is untouched."""
    st = _copy(prune_state(dense, 0.95))
    key, R = LOOP_MATS[k], dense["rnn1.weight_hh_l0"].shape[1]
    br = nb_row(R)
    have = block_map(st[key][4 * br:4 * br + 4, :R])[0]
    assert not have[-1] and have.sum() < count, (k, int(have.sum()))
    for cb in np.flatnonzero(~have)[::-1][:count - int(have.sum())]:
        _restore(st, dense, key, br, cb, gain)
    return st


def cut_last_block(st, k: int) -> dict:
    """`st` with the last nonzero block (column order) of the nb row of matrix k zeroed: what a
    packer that truncates one slot early would run."""
    out = _copy(st)
    key, R = LOOP_MATS[k], st["rnn1.weight_hh_l0"].shape[1]
    br = nb_row(R)
    cb = int(np.flatnonzero(block_map(out[key][4 * br:4 * br + 4, :R])[0])[-1])
    _blk(out[key], br, cb)[...] = 0
    return out


@functools.lru_cache(maxsize=None)
def state(model: str, name: str) -> Dict[str, np.ndarray]:
    """A named state of DIMS[model] (or DM_DIMS[model]: "dense" / "denseB" only); computed once per
    process and shared (read-only)."""
    if model in DM_DIMS:
        st = syn.make_deepmind_state(DM_DIMS[model], {"dense": SEED_A, "denseB": SEED_B}[name])
    else:
        d = DIMS[model]
        if name == "denseB" or name == "pB90":
            dense = syn.make_fatchord_state(d, SEED_B)
        else:
            dense = syn.make_fatchord_state(d, SEED_A)
        if name in ("dense", "denseB"):
            st = dense
        elif name in ("p90", "pB90", "p95", "p99"):
            st = prune_state(dense, {"p90": 0.9, "pB90": 0.9, "p95": 0.95, "p99": 0.99}[name])
        elif name in ("ew95", "ew97", "ew99"):
            st = elementwise(dense, int(name[2:]) / 100.0)
        elif name[:4] in ("nb32", "nb33"):       # nb32_k, nb33_k, and nb32_k_cut, nb33_k_cut
            parts = name.split("_")
            st = nb_state(dense, int(parts[1]), int(parts[0][2:]))
            if parts[-1] == "cut":
                st = cut_last_block(st, int(parts[1]))
        else:
            st = {"dens_eq": dens_eq, "dens_over": dens_over, "hh_only": hh_only, "one_dense_row": one_dense_row,
                  "all_zero": all_zero}[name](dense)
    st = {k: np.ascontiguousarray(v) for k, v in st.items()}
    for v in st.values():
        v.setflags(write=False)
    return st


# ------------------------------------------------------------------------- runs and ladders
@functools.lru_cache(maxsize=None)
def inputs(model: str, B: int, L: int):
    """(mels, aux, noise) of a loop run, or the noise alone for a deepmind model; read-only."""
    if model in DM_DIMS:
        nz = syn.make_dm_noise(B, L, DM_DIMS[model].quantisation, 7300 + 10 * B)
        nz.setflags(write=False)
        return nz
    d = DIMS[model]
    mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, 7100 + 10 * B)
    noise = syn.make_noise(d.mode, B, L, d.n_classes, 7200 + 10 * B)
    for a in (mels, aux, noise):
        a.setflags(write=False)
    return mels, aux, noise


@functools.lru_cache(maxsize=None)
def oracle_run(model: str, name: str, B: int, L: int):
    """The oracle on state(model, name): MoL samples [B][L] fp32, RAW / deepmind labels [B][L]."""
    from oracle import oracle
    if model in DM_DIMS:
        out = oracle.deepmind_loop(state(model, name), B, L, inputs(model, B, L))[2]
    else:
        d = DIMS[model]
        ref, lab = oracle.fatchord_loop(state(model, name), d.mode, *inputs(model, B, L))
        out = ref if d.mode == "MOL" else lab
    out.setflags(write=False)
    return out


def pair_distance(a: np.ndarray, b: np.ndarray, mol: bool) -> float:
    """How far two oracle runs are apart: MoL max |delta|; labels the share that differs."""
    return float(np.abs(a - b).max()) if mol else float((a != b).mean())


MOL_PAIR_MIN = 100 * 1e-5          # 100 * MOL_TOL: no rounding hides a stale slab under the 1e-5 bound
LABEL_PAIR_MIN = 0.10

# One live handle, these loads in this order.  (model, (B, L) the pairs are checked at, names)
LADDERS = {
    "mol512": ("mol512", (3, 60), ("dense", "denseB", "pB90", "dens_over", "dens_eq", "dense")),
    "raw512": ("raw512", (3, 60), ("dense", "denseB", "pB90", "dense")),
    "tinymol": ("tinymol", (3, 100), ("dense", "p90", "all_zero", "p99", "hh_only", "dense")),
    # RAW: hh_only and dense differ in 5 % of the labels only (3.7 .. 6.7 % over six input seeds), so
    # the other dense state is loaded between them: every adjacent pair then moves >= 10 %
    "tinyraw": ("tinyraw", (3, 100), ("dense", "p90", "all_zero", "p99", "hh_only", "denseB", "dense")),
    # rnn 896: dense, 0.95, nb32[k], nb33[k] per matrix k, then the rest of the order from nb33[0] on
    "mol896-nb0": ("mol896", (2, 60), ("dense", "p95", "nb32_0", "nb33_0")),
    "mol896-nb1": ("mol896", (2, 60), ("dense", "p95", "nb32_1", "nb33_1")),
    "mol896-nb2": ("mol896", (2, 60), ("dense", "p95", "nb32_2", "nb33_2")),
    "mol896-rest": ("mol896", (2, 60), ("nb33_0", "hh_only", "one_dense_row", "ew97", "dense", "p95")),
    "dm896": ("dm896", (3, 60), ("dense", "denseB", "dense")),
    "dmtiny": ("dmtiny", (3, 100), ("dense", "denseB", "dense")),
}


def is_mol(model: str) -> bool:
    return model in DIMS and DIMS[model].mode == "MOL"


# ------------------------------------------------------------- updates under a live drop-in
# Each update is (name, how, {state key: array or scalar}); `how` is the torch idiom the GPU test
# uses on the live model, apply_update its numpy restatement (the same single fp32 operation per
# element, so the model's state_dict afterwards equals the numpy state bit for bit):
#   "add_"      with torch.no_grad(): p.add_(delta)
#   "load"      model.load_state_dict(..., strict=False)
#   "assign"    p.data = tensor
#   "data_mul"  p.data.mul_(mask)            (PruneMask.apply_mask)
#   "data_add"  p.data.add_(delta)
#   "data_fill" p.data.fill_(value)          (the reference's tap initialisation)
MODEL_FRAMES = 24
DATA_HOWS = ("data_mul", "data_add", "data_fill")      # invisible to (data_ptr, _version)


def apply_update(st: dict, how: str, args: dict) -> dict:
    out = dict(st)
    for k, v in args.items():
        a = np.asarray(st[k])
        if how in ("add_", "data_add"):
            out[k] = (a + np.asarray(v, np.float32)).astype(np.float32)
        elif how in ("load", "assign"):
            out[k] = np.array(v, dtype=a.dtype)
        elif how == "data_mul":
            out[k] = (a * np.asarray(v, np.float32)).astype(np.float32)
        elif how == "data_fill":
            out[k] = np.full(a.shape, v, np.float32)
        else:
            raise ValueError(how)
    return out


def model_dims(rnn: int):
    from tests import geometries as geo
    return geo.geom_dims("hop12", rnn_dims=rnn)


@functools.lru_cache(maxsize=None)
def model_state(rnn: int, seed: int = SEED_A):
    from tests import geometries as geo
    d = model_dims(rnn)
    return geo.perturb_taps(syn.make_fatchord_state(d, seed), d, seed)


def _mol_bias_delta(st):
    delta = np.zeros_like(st["fc3.bias"])
    delta[10:20] = np.linspace(-0.5, 0.5, 10, dtype=np.float32)      # the ten means
    return delta


@functools.lru_cache(maxsize=None)
def model_updates(rnn: int):
    """The updates of one live model, in order.  rnn 512: every idiom; rnn 896: dense -> sparse
    through .data (0.95 block masks on the four GRU matrices), then a .data bias update."""
    a, b = model_state(rnn, SEED_A), model_state(rnn, SEED_B)
    if rnn == 896:
        return (("gru_data_mul_p95", "data_mul", {k: block_mask(a[k], 0.95) for k in GRU_KEYS}),
                ("fc3_bias_data_add", "data_add", {"fc3.bias": _mol_bias_delta(a)}))
    d = model_dims(rnn)
    tap = "upsample.up_layers.1.weight"
    return (
        ("rnn1_hh_add_", "add_", {"rnn1.weight_hh_l0": b["rnn1.weight_hh_l0"]}),
        ("load_state_dict", "load", {k: b[k] for k in b}),
        ("fc1_assign", "assign", {"fc1.weight": a["fc1.weight"]}),
        ("gru_data_mul_p90", "data_mul", {k: block_mask(b[k], 0.9) for k in GRU_KEYS}),
        ("fc3_bias_data_add", "data_add", {"fc3.bias": _mol_bias_delta(a)}),
        ("taps_data_fill", "data_fill", {tap: 1.0 / (2 * d.upsample_factors[0] + 1)}),
        ("melresnet_conv_data_mul", "data_mul", {"upsample.resnet.conv_in.weight": np.float32(1.5)}),
        ("bn_running_var_data_mul", "data_mul", {"upsample.resnet.batch_norm.running_var": np.float32(4.0)}),
    )


@functools.lru_cache(maxsize=None)
def model_run(rnn: int):
    """(mel [feat][T], noise [T * hop][1][11], [state after 0, 1, .. updates], [oracle.generate of
    each]); computed once per process and shared."""
    from oracle import oracle
    d = model_dims(rnn)
    mel = syn.make_mel(d.feat_dims, MODEL_FRAMES, 7400 + rnn)
    noise = syn.make_noise(d.mode, 1, MODEL_FRAMES * d.hop_length, d.n_classes, 7500 + rnn)
    states = [model_state(rnn)]
    for _, how, args in model_updates(rnn):
        states.append(apply_update(states[-1], how, args))
    refs = [oracle.generate(st, d, mel, False, 0, 0, False, noise) for st in states]
    return mel, noise, states, refs


DM_STEPS, DM_BATCH = 100, 3


@functools.lru_cache(maxsize=None)
def dm_updates(model: str):
    a = state(model, "dense")
    H = a["bias_u"].shape[0]
    return (("R_data_mul", "data_mul", {"R.weight": block_mask(a["R.weight"], 0.9)}),
            ("bias_u_data_add", "data_add", {"bias_u": np.linspace(-1, 1, H, dtype=np.float32)}))


@functools.lru_cache(maxsize=None)
def dm_run(model: str):
    """(noise, [state after 0, 1, 2 updates], [oracle labels [3][100] of each])."""
    from oracle import oracle
    noise = inputs(model, DM_BATCH, DM_STEPS)
    states = [state(model, "dense")]
    for _, how, args in dm_updates(model):
        states.append(apply_update(states[-1], how, args))
    return noise, states, [oracle.deepmind_loop(st, DM_BATCH, DM_STEPS, noise)[2] for st in states]
