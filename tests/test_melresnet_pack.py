"""The fused MelResNet's packed weights (condition.melresnet_pack, every BatchNorm folded into its
conv) interpreted on the CPU exactly as csrc/melresnet.hip walks them (tests/melresnet_ref.py),
against the reference-layout torch module in eval mode (fatchord_version.py:13-48).  The kernel
itself: tests/test_gpu_melresnet.py, tests/test_gpu_melresnet_shapes.py."""
import numpy as np
import pytest
import torch

from tests import melresnet_ref as mr

from wavernn_amd import condition
from wavernn_amd import synthetic as syn


def _module(d, seed):
    from wavernn_amd.fatchord_version import WaveRNN
    st = syn.make_fatchord_state(d, seed)
    m = WaveRNN(**d.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
    return m.upsample.resnet.eval()


@pytest.mark.parametrize("d", [syn.DEFAULT_MOL, syn.TINY_MOL])
def test_packed_weights_reproduce_the_module(d):
    res = _module(d, 3)
    # non-trivial running statistics (the synthetic state's are the defaults)
    g = torch.Generator().manual_seed(5)
    mr.randomize_bn(res, g)
    cfg = condition.melresnet_cfg(res)
    packed = condition.melresnet_pack(res).numpy().astype(np.float64)
    x = torch.rand(2, d.feat_dims, 23 + 2 * d.pad, generator=g)
    with torch.no_grad():
        want = res(x).double().numpy()
    got = mr.run_packed(packed, cfg, x.double().numpy())
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


def test_packed_weights_reproduce_an_odd_geometry():
    """in 30, pad 3 (K = 7), C 30, R 18, 2 blocks (the GPU tests' scalar-staging geometry) from the
    shared builder: the float64 module (no fp32 rounding but the packed weights') against the
    interpreter, and the builder's promise of a channel that ReLU kills."""
    res = mr.build(2, 30, 30, 18, 3, seed=1)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 30, 23 + 2 * 3, generator=g)
    assert 1 in mr.dead_channels(res, x)
    cfg, packed, got = mr.reference(res, x)
    assert (cfg.in_dims, cfg.compute_dims, cfg.res_out_dims, cfg.res_blocks, cfg.pad) == (30, 30, 18, 2, 3)
    assert packed.numel() == 30 * 7 * 30 + 30 + 2 * 2 * (30 * 30 + 30) + 30 * 18 + 18
    with torch.no_grad():
        want32 = res(x).double().numpy()
        want64 = res.double()(x.double()).numpy()
    err32, err64 = np.abs(got - want32).max(), np.abs(got - want64).max()
    print(f"max |Δ| vs fp32 module {err32:.3g}, vs float64 module {err64:.3g} of {np.abs(want64).max():.3g}")
    np.testing.assert_allclose(got, want32, rtol=1e-5, atol=1e-5 * np.abs(want32).max())
    # against the module in float64 only the packed weights' fp32 rounding is left
    assert err64 <= 1e-5 * np.abs(want64).max()
