"""Weight loading on live objects: a second wrnn_set_weights on a handle, the sparse / dense and
XCD-sparse decisions at their boundaries, states the reference's pruning workflow produces, the
drop-in's caches under every way a weight can change, and streaming sessions across a reload.

Every state, load order and update comes from tests/weights.py, whose CPU conditions
(tests/test_weights.py) prove that each is what its name says and that consecutive loads differ by
at least 100 * MOL_TOL in the oracle's output (labels: 10 %): a slab left over from the load before
cannot pass.  After every load the handle is compared with the oracle on the weights just loaded
(MoL: MOL_TOL; RAW / deepmind labels bit-exact) and, bit for bit, with a fresh handle that loaded
only that state (the kernels are deterministic), on every path the handle offers; WRNN_PATH and
WRNN_ROW_GROUPS are read per generate call.

Before the fixes of this change (measured on MI355X; see the summary of the change for the list):
rnn 896 `hh_only` and `one_dense_row` were refused ("fit neither kernel's LDS layout") although the
same weights run dense; every `.data` update left generate() on the old weights; a push after a
reload ran on."""
import ctypes

import numpy as np
import pytest
import torch

from tests import weights as wt
from tests.golden import fixtures as gf
from wavernn_amd import _native as nat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OVERRIDES = ("WRNN_PATH", "WRNN_TERMS_MB", "WRNN_NO_FRAME_TERMS", "WRNN_TORCH_MELRESNET", "WRNN_SPARSE",
             "WRNN_ROW_GROUPS", "WRNN_ROWS_GRANULES")
_FRESH = {}          # (model, state, env, B, L) -> what a handle that loaded only that state gives


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------ helpers
def _new_loop(model):
    from wavernn_amd.loop import DeepmindLoop, FatchordLoop
    if model in wt.DM_DIMS:
        d = wt.DM_DIMS[model]
        return DeepmindLoop(d.hidden_size, d.quantisation)
    d = wt.DIMS[model]
    return FatchordLoop(d.mode, d.rnn_dims, d.fc_dims, d.aux_dims, d.feat_dims, d.n_classes, device=0)


def _run(loop, model, B, L, env, monkeypatch):
    """One generate on injected noise under `env` -> (MoL samples | labels as numpy, last_path)."""
    with monkeypatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        if model in wt.DM_DIMS:
            nz = torch.from_numpy(wt.inputs(model, B, L).copy()).to(DEV)
            _, comb = loop.generate(B, L, noise=nz)
            return comb.cpu().numpy().astype(np.int64), loop.info["last_path"]
        mels, aux, noise = wt.inputs(model, B, L)
        cond = torch.from_numpy(np.concatenate([mels, aux], 2).transpose(1, 0, 2).copy()).to(DEV)
        out, lab = loop.generate(cond, noise=torch.from_numpy(noise.copy()).to(DEV), want_labels=not wt.is_mol(model))
        return (out if wt.is_mol(model) else lab).cpu().numpy(), loop.info["last_path"]


def _fresh(model, name, runs, monkeypatch, sparse_env=None):
    """The runs on a handle that loaded state(model, name) alone; shared between the tests."""
    todo = [r for r in runs if (model, name, sparse_env) + r[:3] not in _FRESH]
    if todo:
        loop = _new_loop(model)
        loop.set_weights(wt.state(model, name))
        for env, B, L, _ in todo:
            _FRESH[(model, name, sparse_env, env, B, L)] = _run(loop, model, B, L, env, monkeypatch)
        loop.close()
    return [_FRESH[(model, name, sparse_env) + r[:3]] for r in runs]


def _check_runs(loop, model, name, runs, monkeypatch, tag):
    """Every run of `runs` = (env, B, L, wanted last_path or a tuple of them) on the live handle:
    the path, the oracle on state(model, name), and a fresh handle bit for bit."""
    fresh = _fresh(model, name, runs, monkeypatch)
    for (env, B, L, want), (f_out, f_path) in zip(runs, fresh):
        got, path = _run(loop, model, B, L, env, monkeypatch)
        where = f"{tag} {model}/{name} {dict(env)} {B}x{L}"
        assert path in (want if isinstance(want, tuple) else (want,)), (where, path)
        assert path == f_path, (where, path, f_path)
        ref = wt.oracle_run(model, name, B, L)
        if wt.is_mol(model):
            err = float(np.abs(got - ref).max())
            print(f"WEIGHTS {where}: path {path}, max |delta| {err:.3g}")
            assert np.isfinite(got).all() and err <= gf.MOL_TOL, (where, err)
        else:
            assert np.array_equal(got, ref), (where, float((got != ref).mean()))
        assert np.array_equal(got, f_out), (where, "differs from a fresh handle")


def _check_info(loop, model, name, fits=True, sparse_env=True):
    info = loop.info
    want = wt.expect_sparse_blocks(wt.state(model, name), sparse_env)
    assert fits or not wt.sparse_must_fit(wt.DIMS[model], want), (model, name, want)
    want = want if fits else 0
    assert info["sparse_blocks"] == want, (model, name, info)
    if want > 0:         # one 4-unit block-row per workgroup
        assert info["rows_units_rnn"] == 4 and info["rows_grid"] == wt.DIMS[model].rnn_dims // 4, info
    return info


P = lambda **kw: tuple(sorted(kw.items()))        # noqa: E731  (an environment, hashable)
ROWS1 = P(WRNN_PATH="rows", WRNN_ROW_GROUPS="1")
ROWS2 = P(WRNN_PATH="rows", WRNN_ROW_GROUPS="2")


# -------------------------------------------------------- 2. one handle, many loads
MOL512_RUNS = ((P(WRNN_PATH="xcd"), 3, 60, 5), (P(WRNN_PATH="xcdm"), 10, 40, 7), (P(WRNN_PATH="split"), 1, 60, 4),
               (P(WRNN_PATH="latency"), 1, 60, 1), (ROWS1, 3, 60, 2))


def test_mol512_reloads_on_one_handle(monkeypatch):
    model, _, names = wt.LADDERS["mol512"]
    loop = _new_loop(model)
    assert loop.info["xcd_rows"] == 8 and loop.info["xcdm_rows"] > 0, loop.info
    for i, name in enumerate(names):
        loop.set_weights(wt.state(model, name))
        info = _check_info(loop, model, name)
        assert info["xcd_rows"] == 8, info
        _check_runs(loop, model, name, MOL512_RUNS, monkeypatch, f"load {i}")
        if info["sparse_blocks"] == 0:          # the two-group slab follows dense loads
            _check_runs(loop, model, name, ((ROWS2, 4, 60, 2),), monkeypatch, f"load {i}")
        else:                                    # while sparse the run is not grouped
            one, _ = _run(loop, model, 4, 60, ROWS1, monkeypatch)
            two, path = _run(loop, model, 4, 60, ROWS2, monkeypatch)
            assert path == 2 and np.array_equal(one, two), name
            assert np.abs(one - wt.oracle_run(model, name, 4, 60)).max() <= gf.MOL_TOL, name
    loop.close()


def test_raw512_reloads_on_one_handle(monkeypatch):
    model, _, names = wt.LADDERS["raw512"]
    runs = ((P(WRNN_PATH="xcdm"), 10, 40, 7), (ROWS1, 3, 60, 2), (P(WRNN_PATH="latency"), 1, 60, 1))
    loop = _new_loop(model)
    for i, name in enumerate(names):
        loop.set_weights(wt.state(model, name))
        _check_info(loop, model, name)
        _check_runs(loop, model, name, runs, monkeypatch, f"load {i}")
    loop.close()


@pytest.mark.parametrize("ladder", ("tinymol", "tinyraw"))
def test_tiny_reloads_on_one_handle(ladder, monkeypatch):
    model, (B, L), names = wt.LADDERS[ladder]
    loop = _new_loop(model)
    for i, name in enumerate(names):
        loop.set_weights(wt.state(model, name))
        _check_info(loop, model, name)
        _check_runs(loop, model, name, ((P(WRNN_PATH="rows"), B, L, 2),), monkeypatch, f"load {i}")
    loop.close()


# what each rnn-896 state must select: (default path, WRNN_PATH=rows path, the sparse layout fits)
M896 = {"dense": (9, 9, True), "p95": (6, 2, True), "hh_only": (9, 9, False), "one_dense_row": (9, 9, False),
        "ew97": (2, 2, True)}
for _k in range(3):
    M896[f"nb32_{_k}"] = (6, 2, True)
    M896[f"nb33_{_k}"] = (2, 2, True)            # one block too many for the XCD sparse kernel: not 6


@pytest.mark.parametrize("ladder", ("mol896-nb0", "mol896-nb1", "mol896-nb2", "mol896-rest"))
def test_mol896_reloads_on_one_handle(ladder, monkeypatch):
    model, (B, L), names = wt.LADDERS[ladder]
    loop = _new_loop(model)
    for i, name in enumerate(names):
        loop.set_weights(wt.state(model, name))
        default, rows, fits = M896[name]
        info = _check_info(loop, model, name, fits)
        assert info["xcd_rows"] == (8 if default == 6 else 0), (name, info)
        if default == 6:
            assert info["rows_units_rnn"] == 4 and info["sparse_blocks"] <= wt.XCDS_NB, info
        _check_runs(loop, model, name, ((P(), B, L, default), (P(WRNN_PATH="rows"), B, L, rows)), monkeypatch,
                    f"load {i}")
    loop.close()


@pytest.mark.parametrize("ladder", ("dm896", "dmtiny"))
def test_deepmind_reloads_on_one_handle(ladder, monkeypatch):
    model, (B, L), names = wt.LADDERS[ladder]
    runs = ((P(), B, L, 8), (ROWS1, B, L, (3, 10)), (ROWS2, B, L, (3, 10))) if model == "dm896" else \
        ((P(), B, L, (3, 10)),)
    loop = _new_loop(model)
    for i, name in enumerate(names):
        loop.set_weights(wt.state(model, name))
        _check_runs(loop, model, name, runs, monkeypatch, f"load {i}")
    loop.close()


def _load(loop, tensors):
    """wrnn_set_weights with just these tensors (FatchordLoop.set_weights demands every key)."""
    keep = [np.ascontiguousarray(v, dtype=np.float32) for v in tensors.values()]
    arr = (nat.Tensor * len(keep))()
    for i, (k, a) in enumerate(zip(tensors, keep)):
        arr[i] = nat.Tensor(k.encode(), a.ctypes.data, a.size, 0)
    nat.check(loop._h, nat.lib().wrnn_set_weights(loop._h, arr, len(keep)))


def test_partial_loads(monkeypatch):
    from wavernn_amd.loop import LOOP_KEYS
    model, B, L = "tinymol", 3, 100
    run = (P(WRNN_PATH="rows"), B, L, 2)
    dense, other = wt.state(model, "dense"), wt.state(model, "denseB")
    loop = _new_loop(model)
    _load(loop, {k: dense[k] for k in LOOP_KEYS[:8]})
    with pytest.raises(nat.WrnnError) as e:
        _run(loop, model, B, L, run[0], monkeypatch)
    assert e.value.code == -3, e.value                         # WRNN_ENOWEIGHTS
    _load(loop, {k: dense[k] for k in LOOP_KEYS[8:]})
    _check_runs(loop, model, "dense", (run,), monkeypatch, "two halves")
    # one tensor alone on a loaded handle: the merged state
    _load(loop, {"fc3.bias": other["fc3.bias"]})
    merged = dict(dense)
    merged["fc3.bias"] = other["fc3.bias"]
    fresh = _new_loop(model)
    fresh.set_weights(merged)
    want, _ = _run(fresh, model, B, L, run[0], monkeypatch)
    fresh.close()
    got, _ = _run(loop, model, B, L, run[0], monkeypatch)
    assert np.array_equal(got, want)
    assert np.abs(want - wt.oracle_run(model, "dense", B, L)).max() >= wt.MOL_PAIR_MIN      # the bias shows
    from oracle import oracle
    ref = oracle.fatchord_loop(merged, "MOL", *wt.inputs(model, B, L))[0]
    assert np.abs(got - ref).max() <= gf.MOL_TOL
    # one matrix alone takes the density across 1/2: the layout follows
    assert loop.info["sparse_blocks"] == 0
    eq = wt.state(model, "dens_eq")
    keys = ("rnn1.weight_hh_l0", "rnn2.weight_hh_l0", "rnn2.weight_ih_l0")
    _load(loop, {k: eq[k] for k in keys[1:]})
    half = dict(merged)
    half.update({k: eq[k] for k in keys[1:]})
    assert loop.info["sparse_blocks"] == wt.expect_sparse_blocks(half) == 0                # still over 1/2
    _load(loop, {keys[0]: eq[keys[0]]})
    half[keys[0]] = eq[keys[0]]
    assert loop.info["sparse_blocks"] == wt.expect_sparse_blocks(half) > 0
    got, path = _run(loop, model, B, L, run[0], monkeypatch)
    ref = oracle.fatchord_loop(half, "MOL", *wt.inputs(model, B, L))[0]
    assert path == 2 and np.abs(got - ref).max() <= gf.MOL_TOL
    loop.close()


# ---------------------------------------------------- 3. the decision and its boundaries
@pytest.mark.parametrize("model,B,L", (("tinymol", 3, 100), ("mol512", 3, 60)))
def test_density_boundary(model, B, L, monkeypatch):
    runs = ((ROWS1, B, L, 2),)
    loop = _new_loop(model)
    for name, sparse in (("dens_eq", True), ("dens_over", False), ("dens_eq", True)):
        loop.set_weights(wt.state(model, name))
        info = _check_info(loop, model, name)
        assert (info["sparse_blocks"] > 0) == sparse and (info["rows_units_rnn"] == 4) == sparse, (name, info)
        _check_runs(loop, model, name, runs, monkeypatch, "boundary")
    monkeypatch.setenv("WRNN_SPARSE", "0")
    loop.set_weights(wt.state(model, "dens_eq"))
    monkeypatch.delenv("WRNN_SPARSE")
    assert loop.info["sparse_blocks"] == 0, loop.info
    got, path = _run(loop, model, B, L, ROWS1, monkeypatch)
    assert path == 2 and np.abs(got - wt.oracle_run(model, "dens_eq", B, L)).max() <= gf.MOL_TOL
    loop.close()


PART1 = ("dens_eq", "dens_over", "hh_only", "one_dense_row", "ew95", "ew97", "ew99", "all_zero", "p99")
# rnn 896 packs its slabs on the host: hh_only, one_dense_row, ew97 and nb32 / nb33 load in the ladders above
EVERY = [(m, n) for m in ("tinymol", "tinyraw", "mol512", "raw512") for n in PART1] + \
        [("mol896", n) for n in PART1 if n not in M896]


@pytest.mark.parametrize("model,name", EVERY, ids=lambda v: v)
def test_every_state_loads_and_runs(model, name, monkeypatch):
    """Any weights whose dense form the handle can run must run: on the path the handle picks, and on
    the multi-row kernel, whose layout the statistics decide."""
    R = wt.DIMS[model].rnn_dims
    B, L = {64: (3, 100), 512: (3, 60), 896: (2, 60)}[R]
    loop = _new_loop(model)
    loop.set_weights(wt.state(model, name))
    info, s = loop.info, wt.block_stats(wt.state(model, name))
    want = wt.expect_sparse_blocks(wt.state(model, name))
    # a slab sized by a crowded block-row may not fit beside a row of state: then the dense layout,
    # never a refusal; where it must fit (weights.sparse_must_fit) the 1/2 rule alone decides
    must = wt.sparse_must_fit(wt.DIMS[model], want)
    assert info["sparse_blocks"] in ((want,) if must else (want, 0)), (info, s)
    for env in (P(), P(WRNN_PATH="rows")):
        got, path = _run(loop, model, B, L, env, monkeypatch)
        ref = wt.oracle_run(model, name, B, L)
        if wt.is_mol(model):
            err = float(np.abs(got - ref).max())
            print(f"WEIGHTS every {model}/{name} {dict(env)}: path {path}, sparse_blocks {info['sparse_blocks']}, "
                  f"max |delta| {err:.3g}")
            assert err <= gf.MOL_TOL, (model, name, path, err)
        else:
            assert np.array_equal(got, ref), (model, name, path)
    loop.close()


# ------------------------------------------------------------- 4. the drop-in's caches
def _tensor_state(state):
    return {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def _apply(model, how, args):
    """The torch idiom `how` of tests/weights.py on the live model."""
    named = dict(model.named_parameters())
    named.update(dict(model.named_buffers()))
    if how == "load":
        model.load_state_dict(_tensor_state(args), strict=False)
        return
    for k, v in args.items():
        p = named[k]
        t = torch.from_numpy(np.array(v, dtype=np.float32)).to(p.device)
        if how == "add_":
            with torch.no_grad():
                p.add_(t)
        elif how == "assign":
            p.data = t.clone()
        elif how == "data_mul":
            p.data.mul_(t)
        elif how == "data_add":
            p.data.add_(t)
        elif how == "data_fill":
            p.data.fill_(float(v))
        else:
            raise ValueError(how)


def _same_state(model, state):
    sd = model.state_dict()
    return [k for k, v in state.items() if not np.array_equal(sd[k].cpu().numpy(), np.asarray(v))]


@pytest.mark.parametrize("rnn", (512, 896))
def test_dropin_follows_every_update(rnn):
    """generate() after each update of weights.model_updates against oracle.generate on the
    state_dict as it then reads (the numpy restatement, checked equal bit for bit), 2 * MOL_TOL."""
    from wavernn_amd.fatchord_version import WaveRNN
    d = wt.model_dims(rnn)
    mel, noise, states, refs = wt.model_run(rnn)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict(_tensor_state(states[0]), strict=True)
    paths = {512: [5] * len(states), 896: [9, 6, 6]}[rnn]
    names = ["initial"] + [u[0] for u in wt.model_updates(rnn)]
    failed = []
    for i, (name, st, ref, want_path) in enumerate(zip(names, states, refs, paths)):
        if i:
            _apply(m, *wt.model_updates(rnn)[i - 1][1:])
        assert _same_state(m, st) == [], name
        got = m.generate(torch.from_numpy(mel.copy())[None], None, False, 0, 0, False, noise=noise.copy(), verbose=False)
        path = m.loop_handle().info["last_path"]
        err = float(np.abs(got - ref).max())
        print(f"WEIGHTS dropin {rnn} after {name}: path {path}, max |delta| {err:.3g}")
        if err > 2 * gf.MOL_TOL or path != want_path:
            failed.append((name, path, err))
    assert not failed, failed


@pytest.mark.parametrize("model", ("dmtiny", "dm896"))
def test_deepmind_dropin_follows_data_updates(model):
    from wavernn_amd.deepmind_version import WaveRNN
    noise, states, refs = wt.dm_run(model)
    m = WaveRNN(**wt.DM_DIMS[model].ctor_kwargs()).to(DEV)
    m.load_state_dict(_tensor_state(states[0]), strict=True)
    names = ["initial"] + [u[0] for u in wt.dm_updates(model)]
    failed = []
    for i, (name, st, ref) in enumerate(zip(names, states, refs)):
        if i:
            _apply(m, *wt.dm_updates(model)[i - 1][1:])
        assert _same_state(m, st) == [], name
        out, _, _ = m.generate(wt.DM_STEPS, batch=wt.DM_BATCH, noise=noise.copy())
        if not np.array_equal(out, ref):
            failed.append((name, float((out != ref).mean())))
    assert not failed, failed


def test_fingerprint_kernel_matches_its_numpy_restatement():
    """wrnn_fingerprint against loop.fingerprint_host (exact integers, so equal): one element, sizes
    around a workgroup (256) and around one pass of a tensor's 32 workgroups (8192), 70 tensors (two
    launches of at most 64), a non-contiguous and a half-precision tensor (fingerprinted as their
    contiguous fp32 copies), an integer buffer left out; and that the `.data` idioms, invisible to
    (data_ptr, _version), change it on the device."""
    from wavernn_amd.loop import content_key, fingerprint_host
    g = torch.Generator().manual_seed(3)
    sizes = [1, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5] + [7 + i for i in range(62)]
    ts = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    ts.append(torch.randn(40, 30, generator=g).to(DEV).t())
    ts.append(torch.randn(100, generator=g).to(DEV).half())
    ts.insert(3, torch.zeros((), dtype=torch.long, device=DEV))
    key = content_key(ts)
    fl = [t for t in ts if t.is_floating_point()]
    assert len(fl) == 72 and len(key) == len(ts) + len(fl)
    want = tuple(fingerprint_host(t.float().contiguous().cpu().numpy()) for t in fl)
    assert key[len(ts):] == want
    assert content_key(ts) == key
    p = torch.nn.Parameter(torch.randn(3 * 64, 64, generator=g).to(DEV))
    k0, ident = content_key([p]), (p.data_ptr(), p._version)
    for op in (lambda: p.data.mul_((torch.rand(3 * 64, 64, generator=g) > 0.5).float().to(DEV)),
               lambda: p.data.add_(1e-3), lambda: p.data.fill_(0.25),
               lambda: p.data[191, 63].copy_(torch.nextafter(p.data[191, 63], p.data[191, 63] + 1))):
        op()
        k1 = content_key([p])
        assert (p.data_ptr(), p._version) == ident and k1[0] == ident and k1 != k0
        assert k1[1] == fingerprint_host(p.detach().cpu().numpy())
        k0 = k1


# ------------------------------------------------------ 5. sessions and weight changes
def _session_model():
    from wavernn_amd.fatchord_version import WaveRNN
    d = wt.model_dims(512)
    mel, noise, states, refs = wt.model_run(512)
    m = WaveRNN(**d.ctor_kwargs()).to(DEV)
    m.load_state_dict(_tensor_state(states[0]), strict=True)
    return m, mel, noise, states, refs


def _stream_all(m, sessions, mel, via_group):
    """Push the whole mel 8 frames at a time, then finish -> one waveform per session."""
    T, parts = mel.shape[1], [[] for _ in sessions]
    for f in range(0, T, 8):
        chunk = mel[None, :, f:f + 8]
        outs = m.push_streams([(s, chunk, False) for s in sessions]) if via_group else [s.push(chunk) for s in sessions]
        for p, o in zip(parts, outs):
            p.append(o[0])
    outs = m.push_streams([(s, None, True) for s in sessions]) if via_group else [s.finish() for s in sessions]
    return [np.concatenate(p + [o[0]]) for p, o in zip(parts, outs)]


@pytest.mark.parametrize("via_group", (False, True), ids=("push", "push_streams"))
def test_session_binds_the_weights_it_was_opened_with(via_group):
    m, mel, noise, states, refs = _session_model()
    n = 2 if via_group else 1
    old = [m.stream(1, mel.shape[1], noise=noise.copy()) for _ in range(n)]
    first = m.push_streams([(s, mel[None, :, :8], False) for s in old]) if via_group else [old[0].push(mel[None, :, :8])]
    assert all(o.shape[0] == 1 for o in first)
    # other weights arrive; a one-shot call packs them into the handle the sessions share
    m.load_state_dict(_tensor_state(states[2]), strict=True)
    got = m.generate(torch.from_numpy(mel.copy())[None], None, False, 0, 0, False, noise=noise.copy(), verbose=False)
    assert np.abs(got - refs[2]).max() <= 2 * gf.MOL_TOL
    assert np.abs(refs[2] - refs[0]).max() >= wt.MOL_PAIR_MIN
    with pytest.raises((ValueError, nat.WrnnError), match="loaded again"):
        if via_group:
            m.push_streams([(s, mel[None, :, 8:16], False) for s in old])
        else:
            old[0].push(mel[None, :, 8:16])
    with pytest.raises((ValueError, nat.WrnnError)):          # dead from then on
        old[0].push(mel[None, :, 8:16])
    # one-shot calls and new sessions are unaffected
    got = m.generate(torch.from_numpy(mel.copy())[None], None, False, 0, 0, False, noise=noise.copy(), verbose=False)
    assert np.abs(got - refs[2]).max() <= 2 * gf.MOL_TOL
    new = [m.stream(1, mel.shape[1], noise=noise.copy()) for _ in range(n)]
    for wave in _stream_all(m, new, mel, via_group):
        assert wave.shape == refs[2].shape and np.abs(wave - refs[2]).max() <= 2e-5
    for s in old + new:
        s.close()


def test_stale_session_through_the_c_abi(monkeypatch):
    """wrnn_stream_push itself: WRNN_EINVAL with the cause, the session dead afterwards, while a
    session opened after the reload on the same handle runs."""
    m, mel, noise, states, _ = _session_model()
    s = m.stream(1, mel.shape[1], noise=noise.copy())
    loop = m.loop_handle()
    loop.set_weights({k: v for k, v in _tensor_state(states[2]).items() if k in loop.keys})
    chunk = torch.from_numpy(mel[None, :, :8].copy()).to(DEV)
    got, wave = ctypes.c_int(), torch.empty(1, 512, dtype=torch.float64, device=DEV)
    for _ in range(2):
        rc = nat.lib().wrnn_stream_push(s._session._s, chunk.data_ptr(), 8, 0, wave.data_ptr(), 512, ctypes.byref(got),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and got.value == 0, rc                                     # WRNN_EINVAL, nothing emitted
        assert b"loaded again" in nat.lib().wrnn_last_error(loop._h)
    s.close()
