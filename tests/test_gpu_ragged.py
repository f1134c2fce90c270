"""The generic kernels (fatchord_loop.hip, fatchord_rows.hip in its resident, rnn/fc-512, and
streamed-weights forms, deepmind_rows.hip) at ragged partitions, at the edges of a row block and where
LDS shrinks a block.

Every expectation is `oracle.fatchord_loop` / `oracle.deepmind_loop` on the same injected draws, inputs
built as tests/test_gpu_parity.py builds them (fresh seeds); bounds are the project's: MoL |Δ| <=
MOL_TOL per sample, RAW and deepmind labels bit-exact.  What ran is asserted from wrnn_info — the
partition (`grid`, `units_*`, `rows_*` against tests/partitions.py: a case that is not ragged on the
device fails), `last_path`, and the launch choices `last_row_groups`, `last_row_blocks`,
`last_block_rows`, `last_tile_rows` — never from the environment the test set: a handle whose group
partition does not fit runs one group whatever WRNN_ROW_GROUPS says.

A mismatch names the first (row, step) and, for labels, the workgroup that owns the class row
(`j // UC`), so a wrong tail shows as "last workgroup".

Row blocks.  B in {193, 256, 257, 258, 300, 513} at the tiny dims: the fourth x-gather slot per lane
(more than 192 rows in a group), a second and third row block with their `b0` offsets into noise,
output and Philox keys, and the one-row remainder that two groups must never see (257 = 255 + 2,
513 = 256 + 255 + 2: before the host cut blocks that way the last block's second group had no rows,
its conditioning kernels were launched with a grid of no blocks and the call failed with WRNN_EHIP).

LDS shrink.  The 10-bit RAW rnn-512 model on its default path (rows kernel, two groups of 128 workgroups
with 4 units and 8 of the 1 024 class rows each): the shrink loop of rows_block runs, the first block is
180 rows (90 per group) at B = 256 (180 + 76) and at B = 300 (180 + 120), tile 1.  9-bit RAW rnn 512
forced onto the rows kernel still holds 128 rows per group: one block of 256, tile 1.

Measured on MI355X (last_path, row groups, row blocks, rows and tile rows of the first block):
  tiny grid 24: latency B = 2 MoL 4.4e-8 (1, 0, 0, 0, 0); rows one group B = 3 3.6e-8 (2, 1, 1, 3, 3),
  B = 40 5.2e-8 (2, 1, 1, 40, 16), bulk and granules alike; two groups B = 5 3.6e-8 (2, 2, 1, 5, 3), B = 40
  5.2e-8 (2, 2, 1, 40, 16); RAW: 0 labels differ, the same launches.
  rnn 512 grid 200, rows, B = 3: 3.7e-8 (2, 1, 1, 3, 3); RAW 0 labels differ.
  rnn 520 / fc 388 (max_rows 0: the latency kernel holds no row, every count runs the rows kernel):
  B = 1 3.0e-8 (2, 1, 1, 1, 1), B = 3 3.5e-8 (2, 2, 1, 3, 2), B = 20 4.1e-8 (2, 2, 1, 20, 6), forced two
  groups the same; RAW 7-bit B = 3 0 labels differ (2, 2, 1, 3, 2).  Before wrnn_create asked for the
  residency of the group slab WITHOUT the MoL head, the MoL model ran (2, 1, 1, 20, 20) with or without
  WRNN_ROW_GROUPS=2: its group partition was dropped.
  rnn 1028 / fc 772, B = 2: 5.2e-8 (9, 1, 1, 2, 2).
  deepmind 136 grid 12: 0 labels differ; B = 3 (3, 1, 1, 3, 3) / (3, 2, 1, 3, 2), B = 20 (3, 1, 1, 20, 16) /
  (3, 2, 1, 20, 10).  deepmind 1048, B = 3: 0 labels differ (3, 1, 1, 3, 3).
  row blocks, tiny dims, tile 16 throughout: MoL 4.5e-8 up to 300 rows, 6.0e-8 at 513; RAW and deepmind 0
  labels differ; blocks 1 up to 256 rows, 257: 256 + 1 / 255 + 2 (one group / two), 258 and 300: 2 blocks of
  256 first, 513: 3 blocks.  Philox rows 255, 256, 299 of 300 equal the rows alone.
"""
import functools

import numpy as np
import pytest
import torch

from tests import partitions as pt
from tests.golden import fixtures as gf
from wavernn_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDES = ("WRNN_PATH", "WRNN_TERMS_MB", "WRNN_ROW_GROUPS", "WRNN_ROWS_GRANULES", "WRNN_SPARSE", "WRNN_REPLICAS")
L_RAGGED, L_BLOCKS, L_SHRINK = 60, 8, 6
BLOCK_ROWS = (193, 256, 257, 258, 300, 513)
RAW10 = syn.FatchordDims(bits=10, mode="RAW")


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


# ------------------------------------------------------------------------------------ inputs (shared)
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _fat_state(d, seed):
    return syn.make_fatchord_state(d, seed)


@functools.lru_cache(maxsize=None)
def _fat_inputs(d, B, L, seed):
    """(state, cond [L][B][C], noise [L][B][K], oracle samples, oracle labels); computed once, read-only."""
    from oracle import oracle
    state = _fat_state(d, seed)
    mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, seed + 1)
    noise = syn.make_noise(d.mode, B, L, d.n_classes, seed + 2)
    ref, ref_lab = oracle.fatchord_loop(state, d.mode, mels, aux, noise)
    cond = np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()
    return (state,) + _frozen(cond, noise, ref, ref_lab)


@functools.lru_cache(maxsize=None)
def _dm_inputs(d, B, L, seed):
    from oracle import oracle
    state = syn.make_deepmind_state(d, seed)
    noise = syn.make_dm_noise(B, L, d.quantisation, seed + 1)
    _, _, ref = oracle.deepmind_loop(state, B, L, noise)
    return (state,) + _frozen(noise, ref)


def _rows(a, B):
    """The first B rows of a [L][Bmax][K] input (rows are independent: the oracle ran them once)."""
    return torch.from_numpy(np.array(a[:, :B])).to(DEV)       # a writable, contiguous copy


# ------------------------------------------------------------------------------------------- handles
@pytest.fixture(scope="module")
def handles():
    """One handle per (model, grid, weights) for the module: the environment is read per call."""
    from wavernn_amd.loop import DeepmindLoop, FatchordLoop
    made = {}

    def get(d, grid, seed):
        key = (d, grid, seed)
        if key not in made:
            if isinstance(d, syn.DeepmindDims):
                loop = DeepmindLoop(d.hidden_size, d.quantisation, grid=grid)
                loop.set_weights(syn.make_deepmind_state(d, seed))
            else:
                loop = FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0,
                                    grid=grid)
                loop.set_weights(_fat_state(d, seed))
            made[key] = loop
        return made[key]

    yield get
    for loop in made.values():
        loop.close()


def _check_partition(loop, case):
    """wrnn_info against tests/partitions.py: the device runs the ragged partition the case is about."""
    i, w = loop.info, case.want
    flat, _ = pt.partitions(case, i["num_cus"])
    got = dict(num_cus=i["num_cus"], grid=i["grid"], units_rnn=i["units_rnn"], units_fc=i["units_fc"],
               units_cls=i["units_cls"], rows_grid=i["rows_grid"], rows_units_rnn=i["rows_units_rnn"])
    want = dict(num_cus=pt.CUS, grid=w["G"], units_rnn=w["units"][0], units_fc=w["fc"][0],
                units_cls=w["cls"][0] if w["cls"] else 0, rows_grid=w["G"], rows_units_rnn=w["units"][0])
    assert got == want, (case.id, got, want)
    assert pt.triple(flat.units) == w["units"] and flat.units.last < flat.units.per, case.id
    return flat


def _launch_info(loop):
    i = loop.info
    return i["last_path"], i["last_row_groups"], i["last_row_blocks"], i["last_block_rows"], i["last_tile_rows"]


# ------------------------------------------------------------------------------------------- compare
def _owner(split, j):
    w = split.owner(int(j))
    return f"workgroup {w} of {split.G}" + (" (last workgroup with rows)" if w == split.busy - 1 else "")


def _assert_mol(what, out, ref, launch):
    diff = np.abs(out - ref)
    print(f"RAGGED {what}: max |Δ| {diff.max():.3g}; path/groups/blocks/rows/tile {launch}")
    if diff.max() > gf.MOL_TOL:
        r, t = np.argwhere(diff > 1e-6)[0]
        pytest.fail(f"{what}: max |Δ| {diff.max():.3g} > {gf.MOL_TOL}; first (row, step) over 1e-6: ({r}, {t}), "
                    f"got {out[r, t]!r} want {ref[r, t]!r}; launch {launch}")


def _assert_labels(what, got, ref, cls, launch, split_label=lambda v: (v,)):
    eq = got == ref
    print(f"RAGGED {what}: {int((~eq).sum())} of {eq.size} labels differ; path/groups/blocks/rows/tile {launch}")
    if not eq.all():
        r, t = np.argwhere(~eq)[0]
        own = "; ".join(f"class row {g} (got) in {_owner(cls, g)}, {w} (want) in {_owner(cls, w)}"
                        for g, w in zip(split_label(got[r, t]), split_label(ref[r, t])) if g != w)
        pytest.fail(f"{what}: {eq.mean():.6f} equal; first mismatch (row, step) ({r}, {t}): {own}; launch {launch}")


def _dm_split(v):
    u = int(v) + 2 ** 15
    return u // 256, u % 256


def _run_fat(loop, d, B, inputs, flat, what):
    _, cond, noise, ref, ref_lab = inputs
    out, lab = loop.generate(_rows(cond, B), noise=_rows(noise, B), want_labels=True)
    launch = _launch_info(loop)
    if d.mode == "RAW":
        _assert_labels(what, lab.cpu().numpy(), ref_lab[:B], flat.cls, launch)
        x = (2.0 * ref_lab[:B].astype(np.float32)) / np.float32(d.n_classes - 1.0) - np.float32(1.0)
        assert np.array_equal(out.cpu().numpy(), x.astype(np.float32)), what
    else:
        _assert_mol(what, out.cpu().numpy(), ref[:B], launch)
    return launch


def _run_dm(loop, d, B, L, inputs, flat, what):
    _, noise, ref = inputs
    out, comb = loop.generate(B, L, noise=_rows(noise, B))
    launch = _launch_info(loop)
    got = comb.cpu().numpy().astype(np.int64)
    _assert_labels(what, got, ref[:B], flat.cls, launch, _dm_split)
    np.testing.assert_array_equal(out.cpu().numpy(), got.astype(np.float32))
    return launch


def _tile_ok(tile, rows_in_group, mol):
    return 1 <= tile <= min(rows_in_group, 32 if mol else 16)


# -------------------------------------------------------------------------------- ragged partitions
TINY24 = ("tiny24-mol", "tiny24-raw")
SEED = {"tiny24-mol": 1100, "tiny24-raw": 1110, "r512g200-mol": 1120, "r512g200-raw": 1130, "m520-mol": 1140,
        "m520-raw7": 1150, "m1028-mol": 1160, "dm136g12": 1170, "dm1048": 1180}
# the most rows any test of a case runs: the oracle runs them once (rows are independent)
ROWS_OF = {"tiny24-mol": 40, "tiny24-raw": 40, "r512g200-mol": 3, "r512g200-raw": 3, "m520-mol": 20, "m520-raw7": 3,
           "m1028-mol": 2, "dm136g12": 20, "dm1048": 3}
STEPS_OF = {"m1028-mol": 40, "dm1048": 40}


def _case_inputs(cid):
    c = pt.CASES[cid]
    L = STEPS_OF.get(cid, L_RAGGED)
    if c.family == "deepmind":
        return c, L, _dm_inputs(c.dims, ROWS_OF[cid], L, SEED[cid])
    return c, L, _fat_inputs(c.dims, ROWS_OF[cid], L, SEED[cid])


@pytest.mark.parametrize("cid", TINY24)
def test_tiny_grid24_latency_kernel(cid, handles, monkeypatch):
    """fatchord_loop.hip, 22 workgroups of 3 units with ONE in the last, two workgroups without an fc
    row, 2 rows; MoL too (tests/test_gpu_parity.py::test_grid_sizes_agree is RAW only)."""
    c, L, inp = _case_inputs(cid)
    _env(monkeypatch, WRNN_PATH="latency")
    loop = handles(c.dims, c.grid, SEED[cid])
    flat = _check_partition(loop, c)
    assert loop.info["max_rows"] >= 2
    launch = _run_fat(loop, c.dims, 2, inp, flat, f"{cid} latency B=2")
    assert launch == (1, 0, 0, 0, 0), launch


@pytest.mark.parametrize("gran", [0, 1], ids=["bulk", "granules"])
@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("cid", TINY24)
def test_tiny_grid24_rows_one_group(cid, B, gran, handles, monkeypatch):
    """fatchord_rows.hip on the same partition, one group, bulk and granule hand-offs."""
    c, L, inp = _case_inputs(cid)
    _env(monkeypatch, WRNN_PATH="rows", WRNN_ROW_GROUPS=1, WRNN_ROWS_GRANULES=gran)
    loop = handles(c.dims, c.grid, SEED[cid])
    flat = _check_partition(loop, c)
    path, groups, blocks, rows, tile = _run_fat(loop, c.dims, B, inp, flat, f"{cid} rows B={B} gran={gran}")
    assert (path, groups, blocks, rows) == (2, 1, 1, B) and _tile_ok(tile, B, c.dims.mode == "MOL"), tile


@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("cid", TINY24)
def test_tiny_grid24_rows_two_groups(cid, B, handles, monkeypatch):
    """Two groups of 11 workgroups, 6 units each and 4 in the last; fc 9 per workgroup, last 6."""
    c, L, inp = _case_inputs(cid)
    _env(monkeypatch, WRNN_PATH="rows", WRNN_ROW_GROUPS=2)
    loop = handles(c.dims, c.grid, SEED[cid])
    _check_partition(loop, c)
    _, grp = pt.partitions(c)
    path, groups, blocks, rows, tile = _run_fat(loop, c.dims, B, inp, grp, f"{cid} rows two groups B={B}")
    assert (path, groups, blocks, rows) == (2, 2, 1, B) and _tile_ok(tile, (B + 1) // 2, c.dims.mode == "MOL"), tile


@pytest.mark.parametrize("cid", ["r512g200-mol", "r512g200-raw"])
def test_rnn512_grid200_rows(cid, handles, monkeypatch):
    """The rows kernel's rnn/fc-512 instantiation on 171 workgroups of 3 units, 2 in the last; G is odd:
    one group although three rows would otherwise run as two."""
    c, L, inp = _case_inputs(cid)
    _env(monkeypatch, WRNN_PATH="rows")
    loop = handles(c.dims, c.grid, SEED[cid])
    flat = _check_partition(loop, c)
    path, groups, blocks, rows, tile = _run_fat(loop, c.dims, 3, inp, flat, f"{cid} rows B=3")
    assert (path, groups, blocks, rows) == (2, 1, 1, 3) and _tile_ok(tile, 3, c.dims.mode == "MOL"), tile


# wrnn_info.last_path of the rnn 520 / fc 388 model by row count with nothing forced: the latency kernel
# holds no row of these dims (wrnn_info.max_rows is 0), so every row count runs the rows kernel
M520_PATHS = {1: 2, 3: 2, 20: 2}


@pytest.mark.parametrize("B", [1, 3, 20])
def test_m520_mol_default_path(B, handles):
    """rnn 520 / fc 388 / res_out 48 / feat 37: 174 workgroups of 3 units with ONE in the last, 44
    workgroups without an fc row, a conditioning record 85 wide."""
    c, L, inp = _case_inputs("m520-mol")
    loop = handles(c.dims, c.grid, SEED[c.id])
    flat = _check_partition(loop, c)
    max_rows = loop.info["max_rows"]
    _, grp = pt.partitions(c)
    launch = _run_fat(loop, c.dims, B, inp, flat, f"m520-mol default B={B} (max_rows {max_rows})")
    assert launch[0] == (1 if B <= max_rows else 2) == M520_PATHS[B], (launch, max_rows)
    groups = 2 if B >= 2 else 1          # two groups by default from two rows on
    assert launch[1:4] == (groups, 1, B) and _tile_ok(launch[4], (B + groups - 1) // groups, True), launch


def test_m520_mol_forced_two_groups(handles, monkeypatch):
    """87 workgroups of 6 units, 4 in the last; fc 5 per workgroup on 78 of them, 3 in the last.  The
    group slab and the MoL head together exceed LDS: the head stays in HBM.  (wrnn_create asked for the
    residency of slab + head, got none and dropped the group partition: WRNN_ROW_GROUPS=2 then ran one
    group without a word, which last_row_groups showed.)"""
    c, L, inp = _case_inputs("m520-mol")
    _env(monkeypatch, WRNN_PATH="rows", WRNN_ROW_GROUPS=2)
    loop = handles(c.dims, c.grid, SEED[c.id])
    _check_partition(loop, c)
    path, groups, blocks, rows, tile = _run_fat(loop, c.dims, 20, inp, pt.partitions(c)[1], "m520-mol two groups B=20")
    assert (path, groups, blocks, rows) == (2, 2, 1, 20) and _tile_ok(tile, 10, True), tile


def test_m520_raw7_default_path(handles):
    """The same dims with a 7-bit head: one class row per workgroup, 46 workgroups without one."""
    c, L, inp = _case_inputs("m520-raw7")
    loop = handles(c.dims, c.grid, SEED[c.id])
    flat = _check_partition(loop, c)
    max_rows = loop.info["max_rows"]
    launch = _run_fat(loop, c.dims, 3, inp, flat, f"m520-raw7 default B=3 (max_rows {max_rows})")
    assert launch[0] == (1 if 3 <= max_rows else 2) == M520_PATHS[3], (launch, max_rows)
    assert launch[1:4] == (2, 1, 3) and _tile_ok(launch[4], 2, False), launch


def test_m1028_mol_streamed_weights(handles):
    """rnn 1028 / fc 772: weights beyond LDS, streamed (path 9); 206 workgroups of 5 units, 3 in the last."""
    c, L, inp = _case_inputs("m1028-mol")
    loop = handles(c.dims, c.grid, SEED[c.id])
    flat = _check_partition(loop, c)
    path, groups, blocks, rows, tile = _run_fat(loop, c.dims, 2, inp, flat, "m1028-mol B=2")
    # a streamed slab has no two-group partition
    assert (path, groups, blocks, rows) == (9, 1, 1, 2) and _tile_ok(tile, 2, True), tile


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("B", [3, 20])
def test_dm136_grid12(B, groups, handles, monkeypatch):
    """deepmind_rows.hip, S = 68: 12 workgroups of 6 units with 2 in the last, O2 / O4 22 rows with 14
    in the last; two groups: 6 workgroups of 12 units, 8 in the last."""
    c, L, inp = _case_inputs("dm136g12")
    _env(monkeypatch, WRNN_ROW_GROUPS=1 if groups == 1 else None)
    loop = handles(c.dims, c.grid, SEED[c.id])
    _check_partition(loop, c)
    part = pt.partitions(c)[groups - 1]
    path, g, blocks, rows, tile = _run_dm(loop, c.dims, B, L, inp, part, f"dm136g12 B={B} groups={groups}")
    assert (path, g, blocks, rows) == (3, groups, 1, B) and _tile_ok(tile, (B + groups - 1) // groups, False), tile


def test_dm1048(handles):
    """S = 524: 175 workgroups of 3 units with 2 in the last, 47 workgroups without a class row; G odd."""
    c, L, inp = _case_inputs("dm1048")
    loop = handles(c.dims, c.grid, SEED[c.id])
    flat = _check_partition(loop, c)
    path, g, blocks, rows, tile = _run_dm(loop, c.dims, 3, L, inp, flat, "dm1048 B=3")
    assert (path, g, blocks, rows) == (3, 1, 1, 3) and _tile_ok(tile, 3, False), tile


def test_ragged_rows_philox_row_keyed(handles, monkeypatch):
    """Philox on the ragged tiny partition (rows kernel): row 2 of a 5-row call equals that row alone
    with row_offset 2, as test_gpu_parity.py::test_philox_deterministic_and_shard_invariant checks it."""
    c = pt.CASES["tiny24-mol"]
    _env(monkeypatch, WRNN_PATH="rows")
    loop = handles(c.dims, c.grid, SEED[c.id])
    _check_partition(loop, c)
    mels, aux = syn.make_conditioning(5, L_RAGGED, c.dims.feat_dims, c.dims.res_out_dims, 1190)
    cond = torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)
    a, _ = loop.generate(cond, seed=1234)
    assert loop.info["last_path"] == 2 and loop.info["last_row_groups"] == 2
    b, _ = loop.generate(cond, seed=1234)
    assert torch.equal(a, b)
    r2, _ = loop.generate(cond[:, 2:3].contiguous(), seed=1234, row_offset=2)
    assert loop.info["last_path"] == 2 and loop.info["last_row_groups"] == 1
    assert (r2[0] - a[2]).abs().max().item() <= gf.MOL_TOL
    assert float(a.abs().max()) <= 1.0 and torch.isfinite(a).all()


def test_ragged_dm_philox_row_keyed(handles):
    c = pt.CASES["dm136g12"]
    loop = handles(c.dims, c.grid, SEED[c.id])
    _check_partition(loop, c)
    _, a = loop.generate(5, L_RAGGED, seed=99)
    assert _launch_info(loop)[:4] == (3, 2, 1, 5)
    _, r2 = loop.generate(1, L_RAGGED, seed=99, row_offset=2)
    assert _launch_info(loop)[:4] == (3, 1, 1, 1)
    assert torch.equal(r2[0], a[2])


# ---------------------------------------------------------------------------------------- row blocks
BLOCK_MODELS = {"tinymol": syn.TINY_MOL, "tinyraw": syn.TINY_RAW, "tinydm": syn.TINY_DM}
BLOCK_SEED = {"tinymol": 1200, "tinyraw": 1210, "tinydm": 1220}
BLOCK_PATH = {"tinymol": 2, "tinyraw": 2, "tinydm": 3}


def _block_inputs(model):
    d = BLOCK_MODELS[model]
    if model == "tinydm":
        return d, _dm_inputs(d, max(BLOCK_ROWS), L_BLOCKS, BLOCK_SEED[model])
    return d, _fat_inputs(d, max(BLOCK_ROWS), L_BLOCKS, BLOCK_SEED[model])


def _flat_of(d):
    if isinstance(d, syn.DeepmindDims):
        return pt.deepmind_partition(d.hidden_size, d.quantisation)
    return pt.fatchord_partition(d.rnn_dims, d.fc_dims, d.n_classes, d.mode == "MOL")


@pytest.mark.parametrize("force_one", [False, True], ids=["grouped", "one-group"])
@pytest.mark.parametrize("B", BLOCK_ROWS)
@pytest.mark.parametrize("model", list(BLOCK_MODELS))
def test_row_blocks_vs_oracle(model, B, force_one, handles, monkeypatch):
    """Every row of B rows against the oracle, the blocks the host cut asserted from wrnn_info: 2 blocks
    of 256 + 1 at B = 257 with one group; 255 + 2 with two."""
    d, inp = _block_inputs(model)
    _env(monkeypatch, WRNN_PATH=None if model == "tinydm" else "rows", WRNN_ROW_GROUPS=1 if force_one else None)
    loop = handles(d, 0, BLOCK_SEED[model])
    assert loop.info["num_cus"] == pt.CUS
    groups = 1 if force_one else 2
    want = pt.row_blocks(B, groups == 2)
    what = f"{model} B={B} groups={groups}"
    if model == "tinydm":
        launch = _run_dm(loop, d, B, L_BLOCKS, inp, _flat_of(d), what)
    else:
        launch = _run_fat(loop, d, B, inp, _flat_of(d), what)
    path, g, blocks, rows, tile = launch
    assert (path, g, blocks, rows) == (BLOCK_PATH[model], groups, len(want), want[0]), (launch, want)
    assert _tile_ok(tile, (rows + groups - 1) // groups, model == "tinymol"), launch
    if B == 257:
        assert (blocks, rows) == ((2, 256) if force_one else (2, 255))


@pytest.mark.parametrize("force_one", [False, True], ids=["grouped", "one-group"])
@pytest.mark.parametrize("model", list(BLOCK_MODELS))
def test_row_blocks_philox_rows_keyed_by_global_row(model, force_one, handles, monkeypatch):
    """Philox at B = 300 (blocks 256 + 44): the last row of the first block, the first of the second
    and the last row equal those rows generated alone with their row_offset."""
    d = BLOCK_MODELS[model]
    _env(monkeypatch, WRNN_PATH=None if model == "tinydm" else "rows", WRNN_ROW_GROUPS=1 if force_one else None)
    loop = handles(d, 0, BLOCK_SEED[model])
    B, L = 300, L_BLOCKS
    if model == "tinydm":
        whole = loop.generate(B, L, seed=77)[1]
    else:
        mels, aux = syn.make_conditioning(B, L, d.feat_dims, d.res_out_dims, 1230)
        cond = torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)
        out, lab = loop.generate(cond, seed=77, want_labels=True)
        whole = lab if d.mode == "RAW" else out
    assert _launch_info(loop)[:4] == (BLOCK_PATH[model], 1 if force_one else 2, 2, 256)
    for r in (255, 256, 299):
        if model == "tinydm":
            one = loop.generate(1, L, seed=77, row_offset=r)[1]
        else:
            out, lab = loop.generate(cond[:, r:r + 1].contiguous(), seed=77, row_offset=r, want_labels=True)
            one = lab if d.mode == "RAW" else out
        if model == "tinymol":     # the terms GEMM may tile differently per row count: the fp tolerance
            assert (one[0] - whole[r]).abs().max().item() <= gf.MOL_TOL, r
        else:
            assert torch.equal(one[0], whole[r]), r


# ---------------------------------------------------------------------------------------- LDS shrink
SHRINK_ROWS = 300
RAW10_BLOCK_ROWS = 180      # measured: 90 rows per group fit beside the two-group slab of the 10-bit model


@pytest.mark.parametrize("B", [256, 300])
def test_raw10_rnn512_default_path_shrinks_its_blocks(B, handles):
    """10-bit RAW rnn 512 runs the rows kernel by default, in two groups of 128 workgroups whose slab
    (4 units, 8 of the 1 024 class rows each) leaves LDS for fewer than 128 rows per group: the shrink
    loop of rows_block runs.  Labels exact."""
    inp = _fat_inputs(RAW10, SHRINK_ROWS, L_SHRINK, 1300)
    loop = handles(RAW10, 0, 1300)
    flat = pt.fatchord_partition(512, 512, 1024, False)
    path, groups, blocks, rows, tile = launch = _run_fat(loop, RAW10, B, inp, flat, f"raw10 default B={B}")
    assert path == 2 and groups == 2, launch
    assert rows == RAW10_BLOCK_ROWS < pt.ROWS_MAX and blocks == len(pt.row_blocks(B, True, fit=rows)) == 2, launch
    assert _tile_ok(tile, (rows + 1) // 2, False), launch


def test_raw9_rnn512_rows_256(handles, monkeypatch):
    """9-bit RAW rnn 512 forced onto the rows kernel at a full block of 256 rows."""
    d = syn.DEFAULT_RAW
    inp = _fat_inputs(d, 256, L_SHRINK, 1310)
    _env(monkeypatch, WRNN_PATH="rows")
    loop = handles(d, 0, 1310)
    flat = pt.fatchord_partition(512, 512, 512, False)
    path, groups, blocks, rows, tile = launch = _run_fat(loop, d, 256, inp, flat, "raw9 rows B=256")
    assert (path, groups, blocks, rows) == (2, 2, 1, 256), launch       # 128 rows per group still fit


# ------------------------------------------------------------------------------- a rows session's push
def test_rows_session_push_reports_its_block(monkeypatch):
    """A rows session fills the same wrnn_info fields at every push (three tiny MoL rows: two groups,
    one block of 3), a call on another kernel clears them."""
    from tests.test_gpu_stream_rows import _model, _rest
    from tests.test_gpu_streaming import _run_session
    frames = 24
    m, d, mels, noise = _model("tinymol", 3, frames)
    _, path = _run_session(m, mels.copy(), _rest(frames), None, noise=noise.copy(), rows=True)
    launch = _launch_info(m.loop_handle())
    assert path == 2 and launch[:4] == (2, 2, 1, 3) and _tile_ok(launch[4], 2, True), launch
    _env(monkeypatch, WRNN_PATH="latency")
    m.generate(torch.from_numpy(mels[:1].copy()), None, False, 0, 0, False, seed=1, verbose=False)
    assert _launch_info(m.loop_handle()) == (1, 0, 0, 0, 0)
