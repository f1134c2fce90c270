"""One Tacotron decoder step (eval mode) restated in float64 numpy from the definitions.

Written from what the layers are (Linear, GRUCell, LSTMCell, Conv1d, the location-sensitive attention
with the smooth normalisation), not from anybody's implementation; the tests pin it to steps the
reference recorded (tests/golden/taco_steps_*.npz), and it serves as an independent statement of what
the HIP decoder loop computes.

`w` maps the decoder's state_dict keys (without the 'decoder.' prefix) to arrays; a state is a dict of
1-D arrays: attn_hidden, rnn1_hidden, rnn1_cell, rnn2_hidden, rnn2_cell, context, cumulative,
attention, frame.
"""
import numpy as np

MAX_R = 20


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def linear(w, name, x):
    y = w[name + ".weight"] @ x
    return y + w[name + ".bias"] if name + ".bias" in w else y


def gru_cell(w, name, x, h):
    gi = w[name + ".weight_ih"] @ x + w[name + ".bias_ih"]
    gh = w[name + ".weight_hh"] @ h + w[name + ".bias_hh"]
    H = h.shape[0]
    r = sigmoid(gi[:H] + gh[:H])
    z = sigmoid(gi[H:2 * H] + gh[H:2 * H])
    n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
    return (1.0 - z) * n + z * h


def lstm_cell(w, name, x, h, c):
    g = w[name + ".weight_ih"] @ x + w[name + ".bias_ih"] + w[name + ".weight_hh"] @ h + w[name + ".bias_hh"]
    H = h.shape[0]
    i, f, cand, o = sigmoid(g[:H]), sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), sigmoid(g[3 * H:])
    c = f * c + i * cand
    return o * np.tanh(c), c


def location_features(w, cumulative, attention):
    """The 2-channel zero-padded conv over [cumulative, attention], then L: (T, attn_dims)."""
    k = w["attn_net.conv.weight"]                 # (filters, 2, taps)
    taps, T = k.shape[2], cumulative.shape[0]
    pad = (taps - 1) // 2
    x = np.zeros((2, T + 2 * pad))
    x[0, pad:pad + T], x[1, pad:pad + T] = cumulative, attention
    conv = np.stack([np.einsum("fck,ck->f", k, x[:, t:t + taps]) for t in range(T)])      # (T, filters)
    return conv @ w["attn_net.L.weight"].T + w["attn_net.L.bias"]


def decoder_step(w, enc, enc_proj, s, r):
    """→ (frames (n_mels, r), scores (T,), new state)."""
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    enc, enc_proj = np.asarray(enc, np.float64), np.asarray(enc_proj, np.float64)
    s = {k: np.asarray(v, np.float64) for k, v in s.items()}
    p = np.maximum(linear(w, "prenet.fc1", s["frame"]), 0.0)
    p = np.maximum(linear(w, "prenet.fc2", p), 0.0)
    h = gru_cell(w, "attn_rnn", np.concatenate([s["context"], p]), s["attn_hidden"])
    q = linear(w, "attn_net.W", h)
    u = np.tanh(q[None, :] + enc_proj + location_features(w, s["cumulative"], s["attention"])) @ w["attn_net.v.weight"][0]
    sg = sigmoid(u)
    scores = sg / sg.sum()
    ctx = scores @ enc
    x = linear(w, "rnn_input", np.concatenate([ctx, h]))
    h1, c1 = lstm_cell(w, "res_rnn1", x, s["rnn1_hidden"], s["rnn1_cell"])
    x = x + h1
    h2, c2 = lstm_cell(w, "res_rnn2", x, s["rnn2_hidden"], s["rnn2_cell"])
    x = x + h2
    frames = (w["mel_proj.weight"] @ x).reshape(-1, MAX_R)[:, :r]
    new = {"attn_hidden": h, "rnn1_hidden": h1, "rnn1_cell": c1, "rnn2_hidden": h2, "rnn2_cell": c2, "context": ctx,
           "cumulative": s["cumulative"] + scores, "attention": scores, "frame": frames[:, -1]}
    return frames, scores, new
