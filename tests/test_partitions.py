"""CPU conditions on the ragged-partition cases of tests/partitions.py: on a 256-CU device every case is
ragged in the way its comment says — the last workgroup's short share of GRU units, the workgroups
without an fc or class row, G even (a two-group partition exists) or odd (none).  The GPU module
(tests/test_gpu_ragged.py) asserts the same numbers against wrnn_info."""
import pytest

from tests import partitions as pt


@pytest.mark.parametrize("case", pt.CASES.values(), ids=lambda c: c.id)
def test_case_is_ragged_as_stated(case):
    flat, grp = pt.partitions(case)
    w = case.want
    assert flat.G == w["G"]
    assert pt.triple(flat.units) == w["units"] and pt.triple(flat.fc) == w["fc"] and pt.triple(flat.cls) == w["cls"]
    # the point of every case: the last workgroup owns fewer units than the others
    assert 0 < flat.units.last < flat.units.per and flat.units.idle == 0
    assert (flat.G - 1) * flat.units.per + flat.units.last == flat.units.n
    if w["G2"] is None:
        assert grp is None and flat.G % 2 == 1
    else:
        assert flat.G % 2 == 0 and grp.G == w["G2"] == flat.G // 2
        assert pt.triple(grp.units) == w["units2"] and pt.triple(grp.fc) == w["fc2"]
        assert pt.triple(grp.cls) == w.get("cls2")
        assert 0 < grp.units.last < grp.units.per and grp.units.idle == 0
    for s in (flat.units, flat.fc, flat.cls) + ((grp.units, grp.fc, grp.cls) if grp else ()):
        if s is not None:
            assert s.busy + s.idle == s.G and (s.busy - 1) * s.per + s.last == s.n and 0 < s.last <= s.per


def test_the_kinds_of_raggedness_are_all_covered():
    parts = {k: pt.partitions(c) for k, c in pt.CASES.items()}
    flat = {k: p[0] for k, p in parts.items()}
    # a last workgroup of ONE unit and one of several; in the latency, rows (generic and rnn/fc 512) and
    # deepmind kernels; with weights beyond LDS
    assert flat["tiny24-mol"].units.last == 1 and flat["m520-mol"].units.last == 1
    assert flat["r512g200-mol"].units.last == 2 and flat["m1028-mol"].units.last == 3 and flat["dm136g12"].units.last == 2
    # workgroups without an fc row, with a short last fc share, and both at once
    assert flat["tiny24-mol"].fc.idle == 2 and flat["tiny24-mol"].fc.last == 1
    assert flat["m520-mol"].fc.idle == 44 and flat["m520-mol"].fc.last == 1
    # workgroups without a class row (RAW and deepmind), and a short last class share
    assert flat["m520-raw7"].cls.idle == 46 and flat["dm1048"].cls.idle == 47
    assert flat["tiny24-raw"].cls.last == 4 and flat["dm136g12"].cls.last == 14
    # G odd: one group only
    assert parts["r512g200-mol"][1] is None and parts["dm1048"][1] is None
    # the conditioning record of the 520 model: 37 + 48 wide, terms-GEMM depth 89 (no multiple of 4 or 16)
    d = pt.CASES["m520-mol"].dims
    assert d.feat_dims + d.res_out_dims == 85 and d.aux_dims == 12 and d.rnn_dims % 4 == d.fc_dims % 4 == 0


def test_every_dims_of_the_older_suite_divides_evenly():
    """Why this module exists: the dims the rest of the suite runs leave no unit tail on 256 CUs."""
    for R in (64, 256, 512, 896, 1024):
        s = pt.fatchord_partition(R, 512, 30, True).units
        assert s.last == s.per and s.idle == 0, R
    for H in (64, 128, 896, 2048):
        s = pt.deepmind_partition(H, 256).units
        assert s.last == s.per and s.idle == 0, H


def test_owner_names_the_last_workgroup():
    u = pt.partitions(pt.CASES["m520-mol"])[0].units
    assert u.owner(519) == 173 and u.owner(518) == 172 and u.owner(0) == 0


@pytest.mark.parametrize("B,grouped,want", [
    (193, True, [193]), (256, True, [256]), (257, False, [256, 1]), (257, True, [255, 2]), (258, True, [256, 2]),
    (300, True, [256, 44]), (513, False, [256, 256, 1]), (513, True, [256, 255, 2]), (512, True, [256, 256]),
    (1, False, [1]), (2, True, [2]), (3, True, [3])])
def test_row_blocks_never_leave_one_row_to_two_groups(B, grouped, want):
    got = pt.row_blocks(B, grouped)
    assert got == want and sum(got) == B and max(got) <= pt.ROWS_MAX
    if grouped and B >= 2:
        assert min(got) >= 2          # each block gives both groups at least one row


def test_row_blocks_after_a_shrink():
    """Blocks of what fits (say 180 rows): 181 rows are 179 + 2 with two groups."""
    assert pt.row_blocks(181, True, fit=180) == [179, 2]
    assert pt.row_blocks(181, False, fit=180) == [180, 1]
    assert pt.row_blocks(300, True, fit=180) == [180, 120]
