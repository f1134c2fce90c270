"""The host side of RAW wide sessions without a GPU: the two entry points the feature adds are
declared, exported and bound; the steps-per-launch rule of a wide push (wrnn_wide_steps_per_launch,
the function wide_group_launches itself calls) is pinned for both heads — MoL: the terms alone, as
before; RAW: the terms and the 512 draws of a row-step share the WRNN_TERMS_MB budget."""
import os
import re

import pytest

from tests import geometries as geo
from wavernn_amd import _native as nat
from wavernn_amd import loop as wloop

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wavernn_amd.h")
N_MOL, N_RAW = 32 * 144, 32 * 144 + 512


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(HDR).read()
    lib = nat.lib()
    for name, args in (("wrnn_stream_mu_law", ["wrnn_stream_t *s", "int on"]),
                       ("wrnn_wide_steps_per_launch", ["int rows", "int longest_steps", "int raw"])):
        assert name in nat.EXPORTS and hasattr(lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert [a.strip() for a in m.group(1).split(",")] == args
        assert len(getattr(lib, name).argtypes) == len(args)
    assert "#define WRNN_ABI_VERSION 7" in hdr      # additive: the version stays (7: wrnn_info grew)


def test_mu_law_needs_a_session():
    assert nat.lib().wrnn_stream_mu_law(None, 1) == -1


def test_einval_is_a_value_error():
    with pytest.raises(ValueError) as e:
        nat.check(None, -1)
    assert isinstance(e.value, nat.WrnnError) and e.value.code == -1
    with pytest.raises(nat.WrnnError) as e:
        nat.check(None, -2)
    assert not isinstance(e.value, ValueError)


@pytest.mark.parametrize("rows", [1, 9, 20, 128])
@pytest.mark.parametrize("steps", [1, 37, 77, 1801])
def test_steps_per_launch(monkeypatch, rows, steps):
    """terms_budget_mb(steps, rows, record) makes a head whose row-step costs `record` floats take
    exactly `steps` steps; the other head, on the same budget, takes what its own record gives."""
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, rows, N_RAW))
    assert wloop.wide_steps_per_launch(rows, 10 ** 6, raw=True) == steps
    assert wloop.wide_steps_per_launch(rows, 10 ** 6, raw=False) == int((steps + 1.5) * N_RAW / N_MOL - 1)
    assert wloop.wide_steps_per_launch(rows, max(1, steps - 1), raw=True) == max(1, steps - 1)   # never past the longest member
    monkeypatch.setenv("WRNN_TERMS_MB", geo.terms_budget_mb(steps, rows, N_MOL))
    assert wloop.wide_steps_per_launch(rows, 10 ** 6, raw=False) == steps
    assert wloop.wide_steps_per_launch(rows, 10 ** 6, raw=True) == max(1, int((steps + 1.5) * N_MOL / N_RAW - 1))


def test_steps_per_launch_defaults_and_refusals(monkeypatch):
    monkeypatch.delenv("WRNN_TERMS_MB", raising=False)
    budget = 8192.0 * 2 ** 20 / 4
    assert wloop.wide_steps_per_launch(128, 10 ** 9, raw=True) == int(budget / (128 * N_RAW) - 1)
    assert wloop.wide_steps_per_launch(128, 10 ** 9, raw=False) == int(budget / (128 * N_MOL) - 1)
    monkeypatch.setenv("WRNN_TERMS_MB", "0.0001")
    assert wloop.wide_steps_per_launch(128, 500, raw=True) == 1
    for bad in ((0, 10), (129, 10), (8, 0)):
        with pytest.raises(nat.WrnnError):
            wloop.wide_steps_per_launch(*bad, raw=True)
