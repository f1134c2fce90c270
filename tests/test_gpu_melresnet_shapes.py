"""wrnn_melresnet (csrc/melresnet.hip) at every form it dispatches, against the float64 interpreter
of its packed weights (tests/melresnet_ref.py): each compiled (tile frames, frames per thread)
entry, the scalar weight-staging branch, tile edges with guard floats around `aux`, bit-identity of
the 4- and 16-frame forms, and the contract between wrnn_melresnet_tile_frames and the launch.
WRNN_MR_FRAMES forces the tile form, so nothing here depends on the CU count except the one test
that is about it.  Bound: max |Δ| ≤ 1e-5 · max |want| (tests/test_gpu_melresnet.py's).
Reference: fatchord_version.py:13-48."""
import ctypes

import numpy as np
import pytest
import torch

from tests import melresnet_ref as mr

from wavernn_amd import _native as nat
from wavernn_amd import condition

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RTOL = 1e-5
EUNSUPPORTED = -6

# Every compiled form (F, frames per thread of the compute layers, of the output layer) with dims
# that select it: at F = 4 a channel count ≤ 64 gives 1 frame per thread, 128 → 2, 256 → 4; at
# F = 16: ≤ 16 → 1, 32 → 2, 64 → 4, 128 → 8 (256 → 16 never fits, see the unreachable test).
ENTRIES = [
    (16, 8, 8, 128, 128), (16, 1, 1, 16, 16), (16, 2, 2, 32, 32), (16, 4, 4, 64, 64), (16, 8, 1, 128, 16),
    (16, 8, 2, 128, 32), (16, 8, 4, 128, 64), (16, 8, 16, 128, 256), (16, 1, 8, 16, 128), (16, 2, 8, 32, 128),
    (16, 4, 8, 64, 128),
    (4, 2, 2, 128, 128), (4, 1, 1, 32, 64), (4, 4, 4, 256, 256), (4, 2, 1, 128, 64), (4, 1, 2, 64, 128),
    (4, 4, 2, 256, 128), (4, 2, 4, 128, 256), (4, 4, 1, 256, 64), (4, 1, 4, 64, 256),
]
FORMS = {(F, fc, fr) for F, fc, fr, _, _ in ENTRIES}


def _fpt(cout, F):
    """The kernel's thread layout: frames per thread for cout outputs over F frames and 256 threads."""
    if cout * F <= 256:
        return 1
    f, rem = divmod(cout * F, 256)
    return f if rem == 0 and F % f == 0 else 0


def _force(monkeypatch, F):
    if F is None:
        monkeypatch.delenv("WRNN_MR_FRAMES", raising=False)
    else:
        monkeypatch.setenv("WRNN_MR_FRAMES", str(F))


def _case(blocks, cin, C, R, pad, U, T, seed=0):
    """(cfg, packed on the GPU, x on the GPU, want float64) for a seeded module and mel."""
    res = mr.build(blocks, cin, C, R, pad, seed=seed)
    g = torch.Generator().manual_seed(77 + seed)
    x = torch.rand(U, cin, T + 2 * pad, generator=g)
    cfg, packed, want = mr.reference(res, x)
    return cfg, packed.to(DEV), x.to(DEV), want


def _check(got, want, what):
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: max |Δ| {err:.3g} of {top:.3g} (ratio {err / top:.3g})")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= RTOL * top, (what, err, top)


def _tile_frames(cfg, U, T):
    return nat.lib().wrnn_melresnet_tile_frames(ctypes.byref(cfg), U, T)


@pytest.mark.parametrize("F,fc,fr,C,R", ENTRIES)
def test_every_dispatch_entry(F, fc, fr, C, R, monkeypatch):
    """in 80, pad 2, U = 2, T = 37: 10 tiles of 4 or 3 of 16 per utterance, the last one partial."""
    assert (_fpt(C, F), _fpt(R, F)) == (fc, fr)
    _force(monkeypatch, F)
    cfg, packed, x, want = _case(2, 80, C, R, 2, 2, 37)
    assert _tile_frames(cfg, 2, 37) == F
    got = condition.melresnet(cfg, packed, x).cpu().numpy()
    _check(got, want, f"form ({F}, {fc}, {fr}) C {C} R {R}")


@pytest.mark.parametrize("C,R", [(256, 256), (256, 128), (256, 16)])
def test_sixteen_frame_tiles_never_take_256_compute_channels(C, R, monkeypatch):
    """The 16-frame forms with fc = 16 (C = 256) cannot run: act + tmp are 2·256·16 floats and the
    staged weights 128·max(C, R) = 128·256 floats, (8192 + 32768)·4 bytes = 163 840 = exactly the
    160 KiB of LDS, before the mel tile's in_dims·(16 + K − 1) > 0 floats.  Asked for 16-frame
    tiles, such dims take the 4-frame form (8 KiB + 128 KiB + the mel tile), and say so."""
    assert (2 * 256 * 16 + 128 * 256) * 4 == 160 * 1024
    _force(monkeypatch, 16)
    cfg, packed, x, want = _case(1, 1, C, R, 0, 1, 20)      # the smallest mel tile there is: 16 floats
    assert _tile_frames(cfg, 1, 20) == 4
    _check(condition.melresnet(cfg, packed, x).cpu().numpy(), want, f"C {C} R {R} asked for 16-frame tiles")


def test_channel_counts_no_form_covers_are_refused(monkeypatch):
    """192 channels: 192·4 / 256 = 3 frames per thread does not divide 4, 192·16 / 256 = 12 does not
    divide 16 — both the query and the launch say WRNN_EUNSUPPORTED, in either form."""
    for F in (4, 16, None):
        _force(monkeypatch, F)
        for C, R in ((192, 64), (64, 192)):
            cfg, packed, x, _ = _case(1, 20, C, R, 1, 1, 20)
            aux = torch.empty(1, R, 20, device=DEV)
            assert _tile_frames(cfg, 1, 20) == EUNSUPPORTED
            assert nat.lib().wrnn_melresnet(ctypes.byref(cfg), packed.data_ptr(), x.data_ptr(), 1, 20,
                                            aux.data_ptr(), None) == EUNSUPPORTED


@pytest.mark.parametrize("F", [4, 16])
def test_production_dims(F, monkeypatch):
    _force(monkeypatch, F)
    cfg, packed, x, want = _case(10, 80, 128, 128, 2, 2, 37, seed=2)
    assert _tile_frames(cfg, 2, 37) == F
    _check(condition.melresnet(cfg, packed, x).cpu().numpy(), want, f"80/128/128, 10 blocks, F {F}")


@pytest.mark.parametrize("cin,pad,C,R", [(30, 3, 30, 18), (30, 3, 12, 20)])
def test_scalar_weight_staging(cin, pad, C, R, monkeypatch):
    """Weight blocks the float4 staging cannot take.  30/30/18: the first block's W1 starts at
    float 30·7·30 + 30 = 6330 (≡ 2 mod 4) and conv_out's 30·18 = 540 floats start off 16 bytes too.
    12/20: every matrix and bias is a multiple of 4 floats (C·C = 144, C·R = 240, C = 12), so
    n & 3 == 0 holds everywhere and the address alone decides — vector here, scalar in
    test_misaligned_packed_weights_take_the_scalar_branch — with 48 of the 256 threads owning
    outputs and 36 of them staging a block."""
    _force(monkeypatch, 4)
    cfg, packed, x, want = _case(2, cin, C, R, pad, 2, 37, seed=3)
    assert packed.data_ptr() % 16 == 0
    assert _tile_frames(cfg, 2, 37) == 4
    _check(condition.melresnet(cfg, packed, x).cpu().numpy(), want, f"scalar staging {cin}/{C}/{R}")


def test_misaligned_packed_weights_take_the_scalar_branch(monkeypatch):
    """The same weights at a device address 4 bytes off 16: every block is staged scalar (C = 12,
    R = 20), the output must not change by a bit."""
    _force(monkeypatch, 4)
    cfg, packed, x, want = _case(2, 30, 12, 20, 3, 2, 37, seed=3)
    base = condition.melresnet(cfg, packed, x)
    shifted = torch.empty(packed.numel() + 1, device=DEV)[1:]
    shifted.copy_(packed)
    assert shifted.data_ptr() % 16 == 4
    got = condition.melresnet(cfg, shifted, x)
    _check(got.cpu().numpy(), want, "packed weights 4 bytes off")
    np.testing.assert_array_equal(got.cpu().numpy(), base.cpu().numpy())


GUARD = 64
SENTINEL = 12345.678


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("F", [4, 16])
def test_tile_edges_write_nothing_outside_aux(F, U, monkeypatch):
    """T below, at and one past the tile sizes (1, 3, 4, 5, 15, 16, 17, 33) at C = R = 128: aux lies
    inside a larger allocation, 64 sentinel floats before and after it (the utterances are
    contiguous in the kernel's [U][R][T] layout, so a write past one utterance's tail lands in the
    next one's rows and shows as a mismatch there).  Every aux float is overwritten and no guard
    float changes."""
    _force(monkeypatch, F)
    res = mr.build(2, 80, 128, 128, 2, seed=4)
    cfg = condition.melresnet_cfg(res)
    packed = condition.melresnet_pack(res)
    packed_d = packed.to(DEV)
    g = torch.Generator().manual_seed(8)
    for T in (1, 3, 4, 5, 15, 16, 17, 33):
        x = torch.rand(U, 80, T + 4, generator=g)
        want = mr.run_packed(packed.numpy().astype(np.float64), cfg, x.double().numpy())
        n = U * 128 * T
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        xd = x.to(DEV).contiguous()
        assert _tile_frames(cfg, U, T) == F
        rc = nat.lib().wrnn_melresnet(ctypes.byref(cfg), packed_d.data_ptr(), xd.data_ptr(), U, T,
                                      buf[GUARD:].data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:GUARD] == np.float32(SENTINEL)).all(), f"T {T}: floats before aux were written"
        assert (out[GUARD + n:] == np.float32(SENTINEL)).all(), f"T {T}: floats after aux were written"
        _check(out[GUARD:GUARD + n].reshape(U, 128, T), want, f"F {F} U {U} T {T}")


@pytest.mark.parametrize("blocks,C,R", [(10, 128, 128), (2, 64, 64), (2, 128, 32)])
def test_both_forms_are_bit_identical(blocks, C, R, monkeypatch):
    """include/wavernn_amd.h: both forms sum every output in the same order."""
    cfg, packed, x, want = _case(blocks, 80, C, R, 2, 2, 37, seed=5)
    outs = {}
    for F in (4, 16):
        _force(monkeypatch, F)
        assert _tile_frames(cfg, 2, 37) == F
        outs[F] = condition.melresnet(cfg, packed, x).cpu().numpy()
    _check(outs[4], want, f"C {C} R {R}")
    np.testing.assert_array_equal(outs[4], outs[16])


SWEEP = (12, 16, 30, 32, 48, 64, 128, 192, 256)


def _query_and_launch(cfg, packed, x, U, T, R):
    aux = torch.full((U, R, T), SENTINEL, device=DEV)
    q = _tile_frames(cfg, U, T)
    rc = nat.lib().wrnn_melresnet(ctypes.byref(cfg), packed.data_ptr(), x.data_ptr(), U, T, aux.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return q, rc, aux.cpu().numpy()


@pytest.mark.parametrize("F", [4, 16, None])
def test_query_agrees_with_the_launch(F, monkeypatch):
    """C, R over SWEEP at (U, T) = (1, 20): wrnn_melresnet_tile_frames ≥ 0 ⇔ wrnn_melresnet is
    WRNN_OK, the output then matches the reference, and the reported form is the asked one when
    that form is compiled for the dims, else the other (unset: 4-frame tiles, 2 tiles < any CU
    count).  Only 192 channels are unsupported (see the refusal test)."""
    _force(monkeypatch, F)
    worst = 0.0
    for C in SWEEP:
        for R in SWEEP:
            cfg, packed, x, want = _case(1, 20, C, R, 1, 1, 20, seed=6)
            q, rc, got = _query_and_launch(cfg, packed, x, 1, 20, R)
            assert (q >= 0) == (rc == 0), (C, R, q, rc)
            assert (rc == 0) == (192 not in (C, R)), (C, R, rc)
            if rc != 0:
                assert q == rc == EUNSUPPORTED
                continue
            ask = F or 4
            other = 4 if ask == 16 else 16
            # C = 256 at 16 frames: over the LDS (test_sixteen_frame_tiles_never_take_256_compute_channels)
            has = (ask, _fpt(C, ask), _fpt(R, ask)) in FORMS and not (ask == 16 and C == 256)
            assert q == (ask if has else other), (C, R, q)
            err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
            worst = max(worst, err / top)
            assert err <= RTOL * top, (C, R, q, err, top)
    print(f"asked {F}: worst max |Δ| / max |want| {worst:.3g}")


def test_support_does_not_depend_on_the_grid(monkeypatch):
    """WRNN_MR_FRAMES unset: the 16-frame form is preferred once U·⌈T/16⌉ reaches the CU count.
    Dims only the 4-frame form is compiled for (C 64 R 32, 30 channels, 48 channels …) must run
    there as they do on a small grid."""
    _force(monkeypatch, None)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    U, T = 3, 16 * ((cus + 2) // 3)
    assert U * ((T + 15) // 16) >= cus
    worst = 0.0
    for C in (12, 16, 30, 32, 48, 64):
        for R in (12, 16, 30, 32, 48, 64):
            res = mr.build(1, 20, C, R, 1, seed=7)
            g = torch.Generator().manual_seed(3)
            forms = []
            for u, t in ((1, 20), (U, T)):
                x = torch.rand(u, 20, t + 2, generator=g)
                cfg, packed, want = mr.reference(res, x)
                q, rc, got = _query_and_launch(cfg, packed.to(DEV), x.to(DEV), u, t, R)
                assert rc == 0 and q in (4, 16), (C, R, u, t, q, rc)
                err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
                worst = max(worst, err / top)
                assert err <= RTOL * top, (C, R, u, t, err, top)
                forms.append(q)
            big = (16, _fpt(C, 16), _fpt(R, 16)) in FORMS
            assert forms == [4, 16 if big else 4], (C, R, forms)
    print(f"{U} × {T} frames on {cus} CUs: worst max |Δ| / max |want| {worst:.3g}")
