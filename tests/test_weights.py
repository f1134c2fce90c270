"""CPU conditions of tests/weights.py: every named state is what its name says under the numpy
restatement of capi.cpp's block_stats, the 32nd / 33rd block and every update pair move the oracle's
output by at least 100 * MOL_TOL (labels: 10 %), so that tests/test_gpu_weights.py cannot pass on a
stale slab or a dropped block."""
import numpy as np
import pytest
import torch

from tests import weights as wt
from tests.golden import fixtures as gf
from wavernn_amd.pruning import GRU_KEYS, block_density, prune_state

SIZES = ("tinymol", "mol512", "raw512", "mol896")


def test_pair_minimum_is_100_mol_tol():
    assert wt.MOL_PAIR_MIN == pytest.approx(100 * gf.MOL_TOL)


def test_block_stats_matches_pruning_block_density():
    """The restatement against pruning.block_density on each loop matrix, and by hand on a toy."""
    st = wt.state("tinymol", "p90")
    mats = wt.loop_mats(st)
    s = wt.block_stats(st)
    assert s["nz"] == sum(round(block_density(m) * m.size / 16) for m in mats)
    toy = {k: np.zeros((12, 4 + (4 if k == wt.LOOP_MATS[0] else 0)), np.float32) for k in wt.LOOP_MATS}
    toy["rnn1.weight_hh_l0"][5, 2] = 1          # one element makes its block count
    toy["rnn2.weight_ih_l0"][0, 6] = 1          # the aux columns do not
    assert wt.block_stats(toy) == {"nbmax": 1, "nbmin": 0, "nz": 1, "total": 9, "density": 1 / 9}


@pytest.mark.parametrize("model", SIZES)
def test_density_states_sit_on_the_boundary(model):
    eq, over = wt.block_stats(wt.state(model, "dens_eq")), wt.block_stats(wt.state(model, "dens_over"))
    plain = wt.block_stats(prune_state(wt.state(model, "dense"), 0.5))
    print(f"WEIGHTS {model}: prune_state(0.5) density {plain['density']:.6f}, dens_eq {eq['nz']}/{eq['total']}")
    assert plain["nz"] * 2 < plain["total"]                     # what the builder starts from
    assert eq["nz"] * 2 == eq["total"]                           # exactly 1/2: the sparse side
    assert over["nz"] == eq["nz"] + 1                            # one block over: the dense side
    assert wt.expect_sparse_blocks(wt.state(model, "dens_eq")) == eq["nbmax"] > 0
    assert wt.expect_sparse_blocks(wt.state(model, "dens_over")) == 0
    assert wt.expect_sparse_blocks(wt.state(model, "dens_eq"), sparse_env=False) == 0


@pytest.mark.parametrize("model", SIZES)
def test_pruning_variants(model):
    dense = wt.state(model, "dense")
    R = dense["rnn1.weight_hh_l0"].shape[1]
    hh = wt.state(model, "hh_only")
    for k in ("rnn1.weight_ih_l0", "rnn2.weight_ih_l0"):
        assert np.array_equal(hh[k], dense[k])
    for k in ("rnn1.weight_hh_l0", "rnn2.weight_hh_l0"):
        assert abs(block_density(hh[k]) - 0.05) < 0.01
    s = wt.block_stats(hh)
    assert s["nbmax"] == R // 4 and s["nz"] * 2 <= s["total"], s         # sparse by density, one full row
    assert abs(s["density"] - 0.367) < 0.002, s

    odr, p95 = wt.state(model, "one_dense_row"), wt.state(model, "p95")
    s = wt.block_stats(odr)
    assert s["nbmax"] == R // 4 and s["density"] < 0.06, s
    r0 = wt.ODR_GATE * R + 4 * wt.ODR_ROW
    rest = np.ones(3 * R, bool)
    rest[r0:r0 + 4] = False
    assert (odr["rnn2.weight_hh_l0"][r0:r0 + 4] != 0).all()
    assert np.array_equal(odr["rnn2.weight_hh_l0"][rest], p95["rnn2.weight_hh_l0"][rest])
    for k in GRU_KEYS[:3]:
        assert np.array_equal(odr[k], p95[k])

    for name, want in (("ew95", 0.56), ("ew97", 0.39), ("ew99", 0.15)):
        st, z = wt.state(model, name), int(name[2:]) / 100
        s = wt.block_stats(st)
        assert abs(s["density"] - want) < 0.01, (name, s)
        for k in GRU_KEYS:                                               # the element rule itself
            assert abs((st[k] == 0).mean() - z) < 1e-3, (name, k)
    assert wt.expect_sparse_blocks(wt.state(model, "ew95")) == 0
    assert wt.expect_sparse_blocks(wt.state(model, "ew97")) > 0
    if model == "mol896":       # sparse, but too crowded for the XCD-resident sparse kernel
        assert wt.expect_sparse_blocks(wt.state(model, "ew97")) > wt.XCDS_NB

    z0 = wt.state(model, "all_zero")
    assert wt.block_stats(z0)["nz"] == 0 and wt.expect_sparse_blocks(z0) == 1
    assert np.array_equal(z0["rnn2.weight_ih_l0"][:, R:], dense["rnn2.weight_ih_l0"][:, R:])
    assert np.array_equal(z0["rnn1.weight_ih_l0"], dense["rnn1.weight_ih_l0"])

    s = wt.block_stats(wt.state(model, "p99"))
    assert s["nbmin"] == 0 and s["nbmax"] > 0, s                          # empty block-rows beside full ones


@pytest.mark.parametrize("k", (0, 1, 2))
def test_nb32_nb33_sit_on_the_xcd_sparse_boundary(k):
    p95 = wt.state("mol896", "p95")
    assert wt.block_stats(p95)["nbmax"] == 25
    R, br = 896, wt.nb_row(896)
    for count in (32, 33):
        st = wt.state("mol896", f"nb{count}_{k}")
        s = wt.block_stats(st)
        assert s["nbmax"] == count and s["nz"] * 2 <= s["total"], s
        for j, key in enumerate(wt.LOOP_MATS):
            m, m0 = st[key], p95[key]
            rows = np.ones(3 * R, bool)
            if j == k:
                rows[4 * br:4 * br + 4] = False
                assert wt.block_map(m[4 * br:4 * br + 4, :R]).sum() == count
            assert np.array_equal(m[rows], m0[rows])                     # every other row unchanged
        cut = wt.state("mol896", f"nb{count}_{k}_cut")
        assert wt.block_stats(cut)["nz"] == s["nz"] - 1
        last = np.flatnonzero(wt.block_map(st[wt.LOOP_MATS[k]][4 * br:4 * br + 4, :R])[0])[-1]
        assert not wt.block_map(cut[wt.LOOP_MATS[k]][4 * br:4 * br + 4, :R])[0][last]
        # the block truncation would drop is visible: 2 rows x 60 steps, 100 * MOL_TOL
        d = wt.pair_distance(wt.oracle_run("mol896", f"nb{count}_{k}", 2, 60),
                             wt.oracle_run("mol896", f"nb{count}_{k}_cut", 2, 60), True)
        print(f"WEIGHTS nb{count}[{k}] gain {wt.NB_GAIN:g}: block {count} moves the output by {d:.3g}")
        assert d >= wt.MOL_PAIR_MIN, (k, count, d)
    assert wt.expect_sparse_blocks(wt.state("mol896", f"nb32_{k}")) == wt.XCDS_NB
    assert wt.expect_sparse_blocks(wt.state("mol896", f"nb33_{k}")) == wt.XCDS_NB + 1


@pytest.mark.parametrize("ladder", sorted(wt.LADDERS))
def test_ladder_pairs_are_visible(ladder):
    model, (B, L), names = wt.LADDERS[ladder]
    mol = wt.is_mol(model)
    for a, b in zip(names, names[1:]):
        d = wt.pair_distance(wt.oracle_run(model, a, B, L), wt.oracle_run(model, b, B, L), mol)
        print(f"WEIGHTS {ladder}: {a} -> {b} {d:.3g}")
        assert d >= (wt.MOL_PAIR_MIN if mol else wt.LABEL_PAIR_MIN), (ladder, a, b, d)


@pytest.mark.parametrize("rnn", (512, 896))
def test_model_updates_are_visible(rnn):
    _, _, states, refs = wt.model_run(rnn)
    ups = wt.model_updates(rnn)
    assert len(states) == len(ups) + 1
    for (name, how, args), a, b, sa, sb in zip(ups, refs, refs[1:], states, states[1:]):
        d = float(np.abs(a - b).max())
        print(f"WEIGHTS model {rnn}: {name} {d:.3g}")
        assert d >= wt.MOL_PAIR_MIN, (name, d)
        assert all(np.asarray(sb[k]).shape == np.asarray(sa[k]).shape for k in args)
    if rnn == 896:      # dense -> sparse on a live model: over 1/2 before, XCD-sparse after
        assert wt.expect_sparse_blocks(states[0]) == 0
        assert 0 < wt.expect_sparse_blocks(states[1]) <= wt.XCDS_NB
    assert {u[1] for u in wt.model_updates(512)} == {"add_", "load", "assign", "data_mul", "data_add", "data_fill"}


@pytest.mark.parametrize("model", sorted(wt.DM_DIMS))
def test_deepmind_updates_are_visible(model):
    _, _, refs = wt.dm_run(model)
    for (name, _, _), a, b in zip(wt.dm_updates(model), refs, refs[1:]):
        d = float((a != b).mean())
        print(f"WEIGHTS {model}: {name} {d:.3g} of the labels")
        assert d >= wt.LABEL_PAIR_MIN, (name, d)


def test_data_updates_keep_pointer_and_version_but_not_content_key():
    """What makes the `.data` idioms invisible to (data_ptr, _version), and that loop.content_key
    sees each of them and every single-element change, and nothing else."""
    from wavernn_amd.loop import content_key
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(3 * 64, 64, generator=g)), torch.nn.Parameter(torch.randn(5000, generator=g)),
          torch.zeros((), dtype=torch.long)]
    ident = lambda: tuple((p.data_ptr(), p._version) for p in ps)      # noqa: E731
    k0, i0 = content_key(ps), ident()
    assert content_key(ps) == k0
    for op in (lambda: ps[0].data.mul_((torch.rand(3 * 64, 64, generator=g) > 0.5).float()),
               lambda: ps[1].data.add_(1e-3), lambda: ps[1].data.fill_(0.25)):
        op()
        k1 = content_key(ps)
        assert ident() == i0 and k1 != k0 and k1[:len(i0)] == i0
        k0 = k1
    ps[1].data.copy_(torch.randn(5000, generator=g))
    k0 = content_key(ps)
    for idx in (0, 4095, 4096, 4999):           # one ulp of one element
        ps[1].data[idx] = torch.nextafter(ps[1].data[idx], torch.tensor(9.0))
        k1 = content_key(ps)
        assert k1 != k0
        k0 = k1
    a, b = ps[1].data[3].item(), ps[1].data[3 + 4096].item()      # a swap of two elements shows
    ps[1].data[3], ps[1].data[3 + 4096] = b, a
    assert content_key(ps) != k0
    with torch.no_grad():
        ps[0].add_(1.0)
    assert ident() != i0 and content_key(ps)[:len(i0)] != i0


def test_sparse_slab_fit_bound():
    """Where the sparse layout must fit (the 1/2 rule alone decides) and where a fall-back to the
    dense layout is legitimate: W_hh pruned alone at rnn 896 sizes the slab by a full block-row,
    9 * 224 * 17 floats of blocks and columns, beyond the whole LDS."""
    d = wt.DIMS["mol896"]
    assert wt.sparse_slab_bytes(d, 224) > wt.LDS_BYTES
    for name in ("hh_only", "one_dense_row"):
        assert not wt.sparse_must_fit(d, wt.expect_sparse_blocks(wt.state("mol896", name)))
    for name in ("p95", "nb32_0", "nb33_0", "ew97", "ew99", "p99", "all_zero"):
        assert wt.sparse_must_fit(d, wt.expect_sparse_blocks(wt.state("mol896", name))), name
    for model in ("tinymol", "tinyraw", "raw512"):       # every state of these dims must fit
        assert wt.sparse_must_fit(wt.DIMS[model], wt.DIMS[model].rnn_dims // 4)
