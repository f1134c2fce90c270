"""The ragged Tacotron CBHG restated in numpy from its definitions (float64 by default), and what the
CBHG tests share: the recorded fixtures (tests/golden/cbhg_*.npz), the seeded states and inputs.

`cbhg_list(state, which, inputs, dtype)` takes N sentences, packs them end to end on the time axis
as the HIP path does, and returns per sentence every stage and the two outputs."""
import functools
import os

import numpy as np

from wavernn_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = syn.DEFAULT_TACOTRON
SEED = 11
REGIMES = {"tame": 1.0, "hot": 5.0}
POST_SEED = 500
STAGES = ("front", "bank", "pooled", "proj1", "residual", "highway_in", "highway_out", "rnn")


@functools.lru_cache(maxsize=None)
def state(regime):
    return syn.make_tacotron_state(DIMS, seed=SEED, cbhg_gate_scale=REGIMES[regime])


@functools.lru_cache(maxsize=None)
def load(which, regime):
    with np.load(os.path.join(GOLDEN, f"cbhg_{which}_{regime}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    assert str(fx["state_sha256"]) == syn.state_digest(state(regime)), "the seeded weights changed"
    return fx


def enc_input(T):
    return syn.make_text_ids(T, DIMS.num_chars, seed=200 + T)


def post_input(T):
    return syn.make_taco_mel(T, DIMS.n_mels, seed=POST_SEED + T)


def fixture_input(fx, which, T):
    x = enc_input(T) if which == "enc" else post_input(T)
    assert syn.digest(x) == str(fx[f"T{T}.input_sha256"]), "the seeded inputs changed"
    return x


def bound(d):
    """The project's parity bound: 8 × the reference's own float32-against-float64 deviation, at least 1e-6."""
    return max(1e-6, 8.0 * float(d))


# ---------------------------------------------------------------------- the restatement
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _conv_same(x, w, seg):
    """x (P, Cin) packed; w (O, Cin, k) in the PyTorch layout; seg (P, 2) the own sentence's range.
    Tap j reads x[t + j − k // 2]; positions outside the sentence contribute nothing."""
    O, _, k = w.shape
    y = np.zeros((x.shape[0], O), x.dtype)
    p = np.arange(x.shape[0])
    for j in range(k):
        q = p + j - k // 2
        ok = (q >= seg[:, 0]) & (q < seg[:, 1])
        y[ok] += x[q[ok]] @ w[:, :, j].T
    return y


def _bn(y, s, prefix):
    w, b, m, v = (s[prefix + n] for n in (".weight", ".bias", ".running_mean", ".running_var"))
    return (y - m) / np.sqrt(v + 1e-5) * w + b


def cbhg_packed(st, which, x, offsets, dtype=np.float64):
    """`x`: packed ids (P,) for 'enc', packed mel rows (P, 80) for 'post'. Returns a dict of packed stages
    plus 'rnn' and 'proj', every one (P, channels)."""
    s = {k: np.asarray(v, dtype) for k, v in st.items() if v.dtype.kind == "f"}
    p = "encoder.cbhg" if which == "enc" else "postnet"
    P = int(offsets[-1])
    seg = np.zeros((P, 2), np.int64)
    for a, b in zip(offsets[:-1], offsets[1:]):
        seg[a:b] = (a, b)
    out = {}
    if which == "enc":
        e = s["encoder.embedding.weight"][np.asarray(x)]
        h = np.maximum(e @ s["encoder.pre_net.fc1.weight"].T + s["encoder.pre_net.fc1.bias"], 0)
        x0 = np.maximum(h @ s["encoder.pre_net.fc2.weight"].T + s["encoder.pre_net.fc2.bias"], 0)
        out["front"] = x0
    else:
        x0 = np.asarray(x, dtype)
    K = len([k for k in st if k.startswith(p + ".conv1d_bank.") and k.endswith("conv.weight")])
    bank = []
    for k in range(K):
        q = f"{p}.conv1d_bank.{k}"
        bank.append(_bn(np.maximum(_conv_same(x0, s[q + ".conv.weight"], seg), 0), s, q + ".bnorm"))
    bank = np.concatenate(bank, axis=1)
    out["bank"] = bank
    pooled = bank.copy()
    has_left = np.arange(P) > seg[:, 0]
    pooled[has_left] = np.maximum(bank[np.nonzero(has_left)[0] - 1], bank[has_left])
    out["pooled"] = pooled
    y = _bn(np.maximum(_conv_same(pooled, s[p + ".conv_project1.conv.weight"], seg), 0), s, p + ".conv_project1.bnorm")
    out["proj1"] = y
    y = _bn(_conv_same(y, s[p + ".conv_project2.conv.weight"], seg), s, p + ".conv_project2.bnorm") + x0
    out["residual"] = y
    if p + ".pre_highway.weight" in s:
        y = y @ s[p + ".pre_highway.weight"].T
    out["highway_in"] = y
    i = 0
    while f"{p}.highways.{i}.W1.weight" in s:
        q = f"{p}.highways.{i}"
        g = _sigmoid(y @ s[q + ".W2.weight"].T + s[q + ".W2.bias"])
        y = g * np.maximum(y @ s[q + ".W1.weight"].T + s[q + ".W1.bias"], 0) + (1 - g) * y
        i += 1
    out["highway_out"] = y
    C = y.shape[1]
    rnn = np.zeros((P, 2 * C), dtype)
    for d, sfx in enumerate(("", "_reverse")):
        wi, wh = s[f"{p}.rnn.weight_ih_l0{sfx}"], s[f"{p}.rnn.weight_hh_l0{sfx}"]
        bi, bh = s[f"{p}.rnn.bias_ih_l0{sfx}"], s[f"{p}.rnn.bias_hh_l0{sfx}"]
        gi = y @ wi.T + bi
        for a, b in zip(offsets[:-1], offsets[1:]):
            h = np.zeros(C, dtype)
            for t in (range(a, b) if d == 0 else range(b - 1, a - 1, -1)):
                gh = wh @ h + bh
                r = _sigmoid(gi[t, :C] + gh[:C])
                z = _sigmoid(gi[t, C:2 * C] + gh[C:2 * C])
                n = np.tanh(gi[t, 2 * C:] + r * gh[2 * C:])
                h = (1 - z) * n + z * h
                rnn[t, d * C:(d + 1) * C] = h
    out["rnn"] = rnn
    out["proj"] = rnn @ s["encoder_proj.weight" if which == "enc" else "post_proj.weight"].T
    return out


def cbhg_list(st, which, inputs, dtype=np.float64):
    """N sentences (ids (T,) for 'enc', mel (80, T) for 'post') → per sentence a dict of (T, channels) arrays."""
    lens = [len(x) if which == "enc" else x.shape[1] for x in inputs]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    packed = np.concatenate([np.asarray(x) for x in inputs]) if which == "enc" else \
        np.concatenate([np.asarray(x).T for x in inputs], axis=0)
    out = cbhg_packed(st, which, packed, offsets, dtype)
    return [{k: v[a:b] for k, v in out.items()} for a, b in zip(offsets[:-1], offsets[1:])]
