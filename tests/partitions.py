"""Ragged partitions of the generic kernels, and the models that reach them.

The generic kernels (fatchord_loop.hip, fatchord_rows.hip, deepmind_rows.hip) spread the R GRU units,
the F fc rows and the class rows over the G workgroups of a persistent launch, U / UF / UC to each;
the last workgroup takes what is left (`Uv = min(U, R − w·U)`), and where UF·G overshoots F by a
workgroup or more the trailing workgroups own no fc (or class) row at all.  The dims the rest of the
suite runs (64, 256, 512, 896, 1024 on 256 CUs) divide evenly, so those tails never run there.  This
module restates the host's partition arithmetic (capi.cpp: wrnn_create, set_group_partition, the
deepmind branch) in plain Python and lists models whose partitions are ragged in every such way on a
256-CU device.  tests/test_partitions.py asserts on the CPU that each case is ragged as its `want`
says; tests/test_gpu_ragged.py asserts the same numbers against `wrnn_info` on the device and runs
the kernels on them against the oracle.

Plain module: no test in here."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

from wavernn_amd import synthetic as syn

CUS = 256                   # the MI355X's compute units: the grid target when `grid` is 0
ROWS_MAX = 256              # kRowsMax (rows_device.h): rows of one row block


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclass(frozen=True)
class Split:
    """`n` rows dealt `per` to a workgroup, in order, over `G` workgroups."""
    n: int
    per: int
    G: int

    @property
    def busy(self) -> int:          # workgroups that own at least one row
        return ceil_div(self.n, self.per) if self.per else 0

    @property
    def idle(self) -> int:          # trailing workgroups without a row
        return self.G - self.busy

    @property
    def last(self) -> int:          # rows of the last workgroup that owns any
        return self.n - (self.busy - 1) * self.per if self.per else 0

    @property
    def ragged(self) -> bool:
        return self.per > 0 and (self.last < self.per or self.idle > 0)

    def owner(self, j: int) -> int:
        return j // self.per


@dataclass(frozen=True)
class Partition:
    G: int
    units: Split                    # GRU units (deepmind: per half)
    fc: Split                       # fc1 / fc2 rows (deepmind: O1 / O3 rows)
    cls: Optional[Split]            # fc3 rows of a RAW head (deepmind: O2 / O4 rows); None for MoL


def fatchord_partition(R: int, F: int, n_classes: int, mol: bool, grid: int = 0, cus: int = CUS) -> Partition:
    """wrnn_create: U = ⌈R / target⌉, G = ⌈R / U⌉, UF = ⌈F / G⌉, UC = ⌈classes / G⌉ (RAW)."""
    U = ceil_div(R, grid if grid > 0 else cus)
    G = ceil_div(R, U)
    return Partition(G, Split(R, U, G), Split(F, ceil_div(F, G), G),
                     None if mol else Split(n_classes, ceil_div(n_classes, G), G))


def fatchord_group_partition(R: int, F: int, n_classes: int, mol: bool, grid: int = 0,
                             cus: int = CUS) -> Optional[Partition]:
    """set_group_partition: the same weights over rG = G / 2 workgroups, rU = ⌈R / rG⌉ units each (two
    row groups per launch); None where the host forms none (G odd or below 8)."""
    G = fatchord_partition(R, F, n_classes, mol, grid, cus).G
    if G % 2 or G < 8:
        return None
    rG = G // 2
    return Partition(rG, Split(R, ceil_div(R, rG), rG), Split(F, ceil_div(F, rG), rG),
                     None if mol else Split(n_classes, ceil_div(n_classes, rG), rG))


def _dm(S: int, Q: int, target: int) -> Partition:
    U = ceil_div(S, target)
    G = ceil_div(S, U)              # recomputed: the workgroups U units each leave busy
    return Partition(G, Split(S, U, G), Split(S, ceil_div(S, G), G), Split(Q, ceil_div(Q, G), G))


def deepmind_partition(H: int, Q: int, grid: int = 0, cus: int = CUS) -> Partition:
    """The deepmind branch of wrnn_create over the S = H / 2 units of a half."""
    return _dm(H // 2, Q, grid if grid > 0 else cus)


def deepmind_group_partition(H: int, Q: int, grid: int = 0, cus: int = CUS) -> Optional[Partition]:
    G = deepmind_partition(H, Q, grid, cus).G
    if G % 2 or G < 8:
        return None
    return _dm(H // 2, Q, G // 2)


def row_blocks(B: int, grouped: bool, fit: int = ROWS_MAX):
    """The row blocks rows_block / generate_dm cut B rows into when `fit` rows fit one block: at most
    `fit` each, and with two groups never a block of one row (257 rows are 255 + 2)."""
    out = []
    while B > 0:
        bl = min(B, fit)
        if grouped and B - bl == 1 and bl > 2:
            bl -= 1
        out.append(bl)
        B -= bl
    return out


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    """A model and grid; `want`: what its partitions must be, as (per workgroup, idle workgroups, last
    workgroup's share) triples — asserted on the CPU at 256 CUs and against wrnn_info on the device."""
    id: str
    family: str                     # "fatchord" | "deepmind"
    dims: object                    # syn.FatchordDims | syn.DeepmindDims
    grid: int
    want: Dict[str, object]


def _fd(**kw):
    return syn.FatchordDims(compute_dims=16, res_blocks=1, **kw)


TINY = dict(rnn_dims=64, fc_dims=96, res_out_dims=16)
M520 = dict(rnn_dims=520, fc_dims=388, res_out_dims=48, feat_dims=37)

CASES = {c.id: c for c in (
    # 22 workgroups of 3 units, the last holds 1; fc 5 per workgroup over 20, the 20th holds 1, two idle;
    # two groups: 11 workgroups of 6 units (last 4), fc 9 (last 6)
    Case("tiny24-mol", "fatchord", _fd(mode="MOL", **TINY), 24,
         dict(G=22, units=(3, 0, 1), fc=(5, 2, 1), cls=None, G2=11, units2=(6, 0, 4), fc2=(9, 0, 6))),
    # the same with an 8-bit head: 12 class rows per workgroup, the last holds 4
    Case("tiny24-raw", "fatchord", _fd(mode="RAW", bits=8, **TINY), 24,
         dict(G=22, units=(3, 0, 1), fc=(5, 2, 1), cls=(12, 0, 4), G2=11, units2=(6, 0, 4), fc2=(9, 0, 6),
              cls2=(24, 0, 16))),
    # rnn / fc 512 (the kRF = 512 instantiation of the rows kernel): 171 workgroups of 3, the last holds
    # 2; G odd: no two-group partition.  fc 3 per workgroup is exact (171 · 3 = 513 > 512: last 2)
    Case("r512g200-mol", "fatchord", syn.FatchordDims(mode="MOL"), 200,
         dict(G=171, units=(3, 0, 2), fc=(3, 0, 2), cls=None, G2=None)),
    Case("r512g200-raw", "fatchord", syn.FatchordDims(mode="RAW"), 200,
         dict(G=171, units=(3, 0, 2), fc=(3, 0, 2), cls=(3, 0, 2), G2=None)),
    # 174 workgroups of 3 units, the last holds 1; fc 3 per workgroup on 130 workgroups (the 130th
    # holds 1), 44 idle; two groups: 87 of 6 units (last 4), fc 5 on 78 workgroups (last 3), 9 idle;
    # conditioning record 37 + 48 = 85 wide (terms GEMM depth 89)
    Case("m520-mol", "fatchord", _fd(mode="MOL", **M520), 0,
         dict(G=174, units=(3, 0, 1), fc=(3, 44, 1), cls=None, G2=87, units2=(6, 0, 4), fc2=(5, 9, 3))),
    # 7-bit head: one class row per workgroup, 46 workgroups without one
    Case("m520-raw7", "fatchord", _fd(mode="RAW", bits=7, **M520), 0,
         dict(G=174, units=(3, 0, 1), fc=(3, 44, 1), cls=(1, 46, 1), G2=87, units2=(6, 0, 4), fc2=(5, 9, 3),
              cls2=(2, 23, 2))),
    # weights beyond LDS (streamed): 206 workgroups of 5 units, the last holds 3; fc 4 on 193 (all full)
    Case("m1028-mol", "fatchord", syn.FatchordDims(rnn_dims=1028, fc_dims=772, mode="MOL"), 0,
         dict(G=206, units=(5, 0, 3), fc=(4, 13, 4), cls=None, G2=103, units2=(10, 0, 8), fc2=(8, 6, 4))),
    # deepmind, S = 68: 12 workgroups of 6 units (last 2), O1 / O3 6 rows (last 2), O2 / O4 22 rows
    # (last 14); two groups: 6 workgroups of 12 (last 8), O2 / O4 43 (last 41)
    Case("dm136g12", "deepmind", syn.DeepmindDims(hidden_size=136, quantisation=256), 12,
         dict(G=12, units=(6, 0, 2), fc=(6, 0, 2), cls=(22, 0, 14), G2=6, units2=(12, 0, 8), fc2=(12, 0, 8),
              cls2=(43, 0, 41))),
    # deepmind, S = 524: 175 workgroups of 3 (last 2); 2 class rows per workgroup, 47 without one; G odd
    Case("dm1048", "deepmind", syn.DeepmindDims(hidden_size=1048, quantisation=256), 0,
         dict(G=175, units=(3, 0, 2), fc=(3, 0, 2), cls=(2, 47, 2), G2=None)),
)}


def partitions(case: Case, cus: int = CUS):
    """(flat partition, two-group partition or None) of a case on a device of `cus` compute units."""
    d = case.dims
    if case.family == "deepmind":
        return (deepmind_partition(d.hidden_size, d.quantisation, case.grid, cus),
                deepmind_group_partition(d.hidden_size, d.quantisation, case.grid, cus))
    mol = d.mode == "MOL"
    return (fatchord_partition(d.rnn_dims, d.fc_dims, d.n_classes, mol, case.grid, cus),
            fatchord_group_partition(d.rnn_dims, d.fc_dims, d.n_classes, mol, case.grid, cus))


def triple(s: Optional[Split]):
    return None if s is None else (s.per, s.idle, s.last)
