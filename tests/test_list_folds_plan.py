"""The host side of folded lists without a GPU (include/wavernn_amd.h, "Folded lists"):
wrnn_list_folds_plan — fold counts and first rows against wrnn_cond_shape at the geometries of
tests/geometries.py, the round and launch tables at several `slots`, WRNN_TERMS_MB cuts inside a fold
for both heads, every refusal with its message — and the three entry points declared, exported and
bound with the ABI version unchanged."""
import os
import re

import numpy as np
import pytest

from tests import geometries as geo
from tests import raw_streams as rs
from wavernn_amd import _native as nat
from wavernn_amd import condition
from wavernn_amd import loop as wloop
from wavernn_amd.loop import list_folds_plan

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wavernn_amd.h")
N_MOL = 32 * 144


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("WRNN_TERMS_MB", raising=False)


def _spec(geom):
    feat, factors, pad = geo.GEOMS[geom][:3]
    taps = [np.ones(2 * s + 1, np.float32) / (2 * s + 1) for s in factors]
    return condition.UpsampleSpec(feat, 128, pad, factors, taps)


def _expected_launches(folds, slots, Lf, raw):
    """Rounds of `slots` folds, each cut at wide_steps_per_launch(rows of the round, Lf, raw)."""
    F = sum(folds)
    slots = min(128, F) if slots is None else slots
    out = []
    for q in range(-(-F // slots)):
        rows = min(slots, F - q * slots)
        per = wloop.wide_steps_per_launch(rows, Lf, raw)
        out += [(q * Lf + off, min(per, Lf - off), rows) for off in range(0, Lf, per)]
    return out


# ---- fold counts against wrnn_cond_shape ------------------------------------------------------------
@pytest.mark.parametrize("geom", [g for g in geo.GEOMS if geo.GEOMS[g][6]])
def test_folds_and_first_rows_match_cond_shape(geom):
    spec = _spec(geom)
    _, target, overlap = geo.GEOMS[geom][6]
    frames = list(range(21, 70)) + [geo.GEOMS[geom][6][0], 200, 333]
    folds, first, launches = list_folds_plan(frames, spec.hop, target, overlap)
    want = [spec.shape(1, T, target, overlap) for T in frames]
    assert all(steps == target + 2 * overlap for steps, _ in want)
    assert folds == [rows for _, rows in want]
    assert first == [sum(folds[:i]) for i in range(len(folds))]
    assert sum(rows for f, _, rows in launches if f % (target + 2 * overlap) == 0) == sum(folds)


def test_reference_geometry_counts():
    # hop 275, target 11 000, overlap 550: a 5 s utterance (401 frames) is 10 folds of 12 100 steps
    spec = condition.UpsampleSpec(80, 128, 2, (5, 5, 11), [np.ones(2 * s + 1, np.float32) for s in (5, 5, 11)])
    frames = [401, 101, 4800, 21, 44, 45]
    folds, first, launches = list_folds_plan(frames)
    assert folds == [spec.shape(1, T, 11000, 550)[1] for T in frames]
    assert folds[0] == 10 and folds[3] == 1
    # (L − overlap) an exact multiple of target + overlap: no extra fold (44 frames = 12 100 = 11 550 + 550)
    assert folds[4] == 1 and folds[5] == 2
    assert launches == _expected_launches(folds, None, 12100, False)


# ---- rounds and launches ------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("slots", [1, 3, 128, None])
def test_round_and_launch_tables(slots, raw):
    frames = [21 + (7 * i) % 25 for i in range(41)]          # hop 4, (20, 4): 4 … 8 folds each
    folds, first, launches = list_folds_plan(frames, 4, 20, 4, slots, raw=raw)
    F, Lf = sum(folds), 28
    assert F > 128 and F % 3 and F % 128                      # F is no multiple of the slot counts
    n_slots = 128 if slots is None else slots
    rounds = -(-F // n_slots)
    assert launches == [(q * Lf, Lf, min(n_slots, F - q * n_slots)) for q in range(rounds)]
    assert launches[-1][2] == F - (rounds - 1) * n_slots      # the last round is partly filled
    assert sum(r for _, _, r in launches) == F


def test_slots_zero_is_all_folds_up_to_128():
    lib = nat.lib()
    ints = nat.ctypes.c_int * 2
    first, steps, rows = ints(), ints(), ints()
    n = lib.wrnn_list_folds_plan(ints(21, 30), 2, 12, 150, 20, 0, 0, None, None, first, steps, rows, 2)
    assert n == 1 and (first[0], steps[0], rows[0]) == (0, 190, 4)
    assert list_folds_plan([21] * 200, 12, 150, 20)[2] == [(0, 190, 128), (190, 190, 128), (380, 190, 128), (570, 190, 16)]
    # outputs may be NULL and cap may be short: the count is still returned
    assert lib.wrnn_list_folds_plan(ints(21, 30), 2, 12, 150, 20, 1, 0, None, None, None, None, None, 0) == 4


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("steps", [1, 13, 77])
def test_budget_cuts_inside_a_fold(monkeypatch, raw, steps):
    frames, slots, Lf = [60, 21, 36, 30], 5, 190                # hop 12, (150, 20): 5 + 2 + 3 + 2 folds
    folds, first, uncut = list_folds_plan(frames, 12, 150, 20, slots, raw=raw)
    assert folds == [5, 2, 3, 2] and first == [0, 5, 7, 10]
    assert uncut == [(0, 190, 5), (190, 190, 5), (380, 190, 2)]
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, 5, rs.N_RAW if raw else N_MOL))
    assert wloop.wide_steps_per_launch(5, Lf, raw=raw) == steps
    f2, r2, cut = list_folds_plan(frames, 12, 150, 20, slots, raw=raw)
    assert (f2, r2) == (folds, first)
    assert cut == _expected_launches(folds, slots, Lf, raw)
    full = [c for c in cut if c[2] == 5]
    assert full[0] == (0, steps, 5) and all(s == steps or (f + s) % Lf == 0 for f, s, _ in full)
    assert len(full) == 2 * -(-Lf // steps)
    # the partly filled round has its own, larger, budget; every round starts at a multiple of Lf
    assert [c for c in cut if c[2] == 2][0][0] == 2 * Lf
    for q in range(3):
        assert sum(s for f, s, _ in cut if f // Lf == q) == Lf


# ---- refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, msg", [
    (dict(frames=[]), "a list has at least one utterance"),
    (dict(slots=129), r"slots is 1\.\.128"),
    (dict(slots=-1), r"slots is 1\.\.128"),
    (dict(slots=0), r"slots is 1\.\.128"),
    (dict(hop=0), "hop is at least 1"),
    (dict(target=0), "target is at least 1"),
    (dict(overlap=-1), "overlap is at least 0"),
    (dict(frames=[30, 20]), "utterance 1 has 20 frames: fewer than 21"),
    (dict(frames=[21, 22], hop=1, overlap=22), r"utterance 0: hop \* frames \(21\) is less than the overlap"),
    (dict(frames=[21], hop=1, overlap=21), "no fold"),
    (dict(target=2 ** 31 - 10, overlap=8), "exceeds the step counter"),
    (dict(frames=[2 ** 30 // 4 + 1]), r"hop \* frames exceeds the step counter"),
    (dict(frames=[2 ** 27] * 8, target=1, overlap=0, slots=1), "exceeds the step counter|more folds"),
])
def test_refusals(kw, msg):
    args = dict(frames=[24, 45], hop=4, target=20, overlap=4, slots=None)
    args.update(kw)
    with pytest.raises(nat.WrnnError, match=msg) as e:
        list_folds_plan(**args)
    assert e.value.code == -1


def test_null_frames_is_refused():
    assert nat.lib().wrnn_list_folds_plan(None, 1, 4, 20, 4, 0, 0, None, None, None, None, None, 0) == -1
    assert b"frames" in nat.lib().wrnn_cond_last_error()


def test_post_refusals_need_no_gpu():
    lib = nat.lib()
    for args, msg in (((None, 1, 28, 4, 100, 0, 512, 80, None, None), b"need entries"),):
        assert lib.wrnn_postprocess_list_folds(*args) == -1 and msg in lib.wrnn_cond_last_error()
    assert lib.wrnn_generate_list_folds(None, None, None, None, None, 1, 20, 4, 0, None, 0, 0, None, None) == -1


# ---- declarations ---------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(HDR).read()
    lib = nat.lib()
    for name, nargs in (("wrnn_list_folds_plan", 13), ("wrnn_generate_list_folds", 14), ("wrnn_postprocess_list_folds", 10)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes)
    assert "#define WRNN_ABI_VERSION 7" in hdr and nat.ABI_VERSION == 7      # additive: the version stays (7: wrnn_info grew)
    fields = re.search(r"typedef struct \{([^{}]*)\}\s*wrnn_post_fold_entry;", hdr).group(1)
    assert [f.split()[-1] for f in fields.replace(",", ";").split(";") if f.strip()] == ["*y", "dst", "rows", "wave_len"]
    assert condition.POST_FOLD_ENTRY.itemsize == 24 and condition.POST_FOLD_ENTRY.names == ("y", "dst", "rows", "wave_len")
