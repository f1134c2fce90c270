"""Shared MelResNet helpers for tests/test_melresnet_pack.py (CPU) and
tests/test_gpu_melresnet_shapes.py (GPU): a seeded module of arbitrary dims with non-trivial
BatchNorm statistics, and the float64 interpreter of condition.melresnet_pack's packed weights that
walks them exactly as csrc/melresnet.hip does (layer order, k-major matrices).  Reference:
fatchord_version.py:13-48."""
import numpy as np
import torch

from wavernn_amd import condition


def run_packed(p, cfg, x):
    """x [U][in][T + 2pad] float64 → [U][R][T], the kernel's layer order and layouts."""
    cin, C, R, K = cfg.in_dims, cfg.compute_dims, cfg.res_out_dims, 2 * cfg.pad + 1
    U, _, Tp = x.shape
    T = Tp - K + 1
    o = 0

    def take(n):
        nonlocal o
        v = p[o:o + n]
        o += n
        return v
    W0, b0 = take(cin * K * C).reshape(cin * K, C), take(C)
    cols = np.stack([x[:, c, tap:tap + T] for c in range(cin) for tap in range(K)], 1)   # [U][cin·K][T]
    a = np.maximum(np.einsum("kc,ukt->uct", W0, cols) + b0[None, :, None], 0.0)
    for _ in range(cfg.res_blocks):
        W1, b1, W2, b2 = take(C * C).reshape(C, C), take(C), take(C * C).reshape(C, C), take(C)
        h = np.maximum(np.einsum("kc,ukt->uct", W1, a) + b1[None, :, None], 0.0)
        a = a + np.einsum("kc,ukt->uct", W2, h) + b2[None, :, None]
    Wo, bo = take(C * R).reshape(C, R), take(R)
    assert o == p.size
    return np.einsum("kr,ukt->urt", Wo, a) + bo[None, :, None]


def randomize_bn(res, g):
    """Non-trivial running statistics on every BatchNorm of `res`: mean ~ 0.1·randn, var ∈ [0.5, 1.5]."""
    with torch.no_grad():
        for mod in res.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                dev = mod.running_mean.device
                mod.running_mean.copy_((torch.randn(mod.num_features, generator=g) * 0.1).to(dev))
                mod.running_var.copy_((torch.rand(mod.num_features, generator=g) + 0.5).to(dev))


def build(res_blocks, in_dims, compute_dims, res_out_dims, pad, seed=0):
    """A MelResNet (eval mode, CPU) of arbitrary dims: seeded weights ~ randn / √fan_in (so the
    activations stay O(1) through the blocks), BatchNorm γ ∈ [0.5, 1.5], β ~ 0.1·randn, running
    statistics as randomize_bn.  Channel 1 of the first BatchNorm and of the first block's
    batch_norm1 has running_mean 1e3: its pre-activations are all negative for the unit-range mels
    the tests feed, so ReLU kills it."""
    from wavernn_amd.fatchord_version import MelResNet
    g = torch.Generator().manual_seed(1000 + seed)
    res = MelResNet(res_blocks, in_dims, compute_dims, res_out_dims, pad).eval()
    with torch.no_grad():
        for mod in res.modules():
            if isinstance(mod, torch.nn.Conv1d):
                fan_in = mod.in_channels * mod.kernel_size[0]
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) / fan_in ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
            elif isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
        randomize_bn(res, g)
        dead = [res.batch_norm] + ([res.layers[0].batch_norm1] if res_blocks else [])
        for bn in dead:
            bn.running_mean[min(1, bn.num_features - 1)] = 1e3
    return res


def dead_channels(res, x):
    """Channels of conv_in → BN that are negative at every frame of x [U][in][T + 2pad] (float64 module math)."""
    with torch.no_grad():
        pre = res.batch_norm(res.conv_in(x.float()))
    return [c for c in range(pre.shape[1]) if bool((pre[:, c] < 0).all())]


def reference(res, x):
    """The float64 MelResNet of the module's packed weights: x [U][in][T + 2pad] (torch, any device) →
    (cfg, packed fp32 tensor on res's device, want float64 ndarray [U][R][T])."""
    cfg = condition.melresnet_cfg(res)
    packed = condition.melresnet_pack(res)
    want = run_packed(packed.cpu().numpy().astype(np.float64), cfg, x.cpu().double().numpy())
    return cfg, packed, want
