"""mmoe_layer / tower_layer (layer/interaction.py:429-523) and MMOE
(model/mmoe.py:10-32) on the one-launch kernel (mmoe.hip).

The fp64 restatements (mmoe_layer_ref, mmoe_ref) are composed from the
oracle's Dense and a max-subtracting softmax and pinned by a hand-computed
case.  CPU tests cover the restatements, the Keras weight exchange, the
support / size queries and the argument checks (nothing is launched); the GPU
tests compare mix and tower outputs at the project's tolerance
(tests.helpers.RTOL) and check the bit-exactness contracts of the ABI."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_rel_close, assert_scaled_close

gpu_test = pytest.mark.gpu

TOY = dict(d=4, H=10, E=3, T=3, towers=(20, 10), out=1)         # model/mmoe.py:35-48
TIMING = dict(d=221, H=64, E=8, T=2, towers=(32, 16), out=1)    # scripts/time_mmoe.py
TOY_X = np.array([[1., 1., 1., 3.], [2., 2., 1., 4.]], np.float32)


def softmax_ref(z):
    z = np.asarray(z, np.float64)
    p = np.exp(z - z.max(axis=-1, keepdims=True))
    return p / p.sum(axis=-1, keepdims=True)


def mmoe_layer_ref(x, expert_matrix, expert_bias, gate_matrix, gate_bias, dt=np.float64):
    """mmoe_layer.call: the T mixes [B, H] as one [B, T * H] array (task t at
    columns t * H).  expert_bias / gate_bias None = the use_*_bias flag off."""
    x = np.asarray(x, dt)
    d, H, E = expert_matrix.shape
    eb = np.zeros(H * E) if expert_bias is None else np.asarray(expert_bias).reshape(-1)
    experts = O.dense(x, np.asarray(expert_matrix).reshape(d, H * E), eb, "relu", dt=dt).reshape(-1, H, E)
    mixes = []
    for t, gm in enumerate(gate_matrix):
        gb = np.zeros(E) if gate_bias is None else gate_bias[t]
        gate = softmax_ref(O.dense(x, gm, gb, None, dt=dt))
        mixes.append((experts * gate[:, None, :]).sum(-1))
    return np.concatenate(mixes, axis=1)


def mmoe_ref(x, w, T, n_hidden, act="relu"):
    """MMOE.call from Keras-named weights: (mix [B, T * H], y [T, B, out])."""
    g = lambda n: w.get(n)
    mix = mmoe_layer_ref(x, w["mmoe_layer/expert_matrix"], g("mmoe_layer/expert_bias"),
                         [w[f"mmoe_layer/gate_matrix{t}"] for t in range(T)],
                         [w[f"mmoe_layer/gate_bias{t}"] for t in range(T)] if g("mmoe_layer/gate_bias0") is not None
                         else None)
    H = mix.shape[1] // T
    ys = []
    for t in range(T):
        p = f"tower_layer_{t}/"
        hidden = [(w[p + f"dense_{i}/kernel"], w[p + f"dense_{i}/bias"]) for i in range(n_hidden)]
        ys.append(O.dnn_layer(mix[:, t * H:(t + 1) * H], hidden, (w[p + "dense_out/kernel"], w[p + "dense_out/bias"]),
                              act))
    return mix, np.stack(ys)


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def expected_prepared_size(d, H, E, T, dims):
    """The header's formula: dp N1p + N1p + sum_l T (Kp_l Np_l + Np_l)."""
    up = lambda v: (v + 15) // 16 * 16
    n1p = up((H + T) * E)
    return up(d) * n1p + n1p + sum(T * (up(a) * up(b) + up(b)) for a, b in zip(dims[:-1], dims[1:]))


def rand_weights(rng, d, H, E, T, towers, out, eb=True, gb=True):
    """Keras-named float32 weights: N(0, 0.05) layer weights with the biases
    requested, glorot-sized tower kernels with small non-zero biases."""
    n = lambda *s: rng.normal(0, 0.05, s).astype(np.float32)
    w = {"mmoe_layer/expert_matrix": n(d, H, E)}
    if eb:
        w["mmoe_layer/expert_bias"] = n(H, E)
    for t in range(T):
        w[f"mmoe_layer/gate_matrix{t}"] = rng.normal(0, 0.5, (d, E)).astype(np.float32)  # gates away from uniform
    if gb:
        for t in range(T):
            w[f"mmoe_layer/gate_bias{t}"] = n(E)
    dims = [H] + list(towers) + [out]
    for t in range(T):
        for i, (kin, nout) in enumerate(zip(dims[:-1], dims[1:])):
            name = f"tower_layer_{t}/" + (f"dense_{i}" if i < len(towers) else "dense_out")
            lim = np.sqrt(6.0 / (kin + nout))
            w[name + "/kernel"] = rng.uniform(-lim, lim, (kin, nout)).astype(np.float32)
            w[name + "/bias"] = n(nout)
    return w


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(d, H, E, T, towers, out, B=5, act="relu", eb=True, gb=True, seed=0):
    """Weights, an input with negatives and the fp64 reference, computed once
    per configuration and shared (never modified) by the tests that use it."""
    rng = np.random.default_rng([seed, d, H, E, T, out, B, len(towers)])
    c = Case()
    c.d, c.H, c.E, c.T, c.towers, c.out, c.act, c.B = d, H, E, T, tuple(towers), out, act, B
    c.dims = [H] + list(towers) + [out]
    c.w = rand_weights(rng, d, H, E, T, towers, out, eb, gb)
    c.x = rng.normal(0, 1, (B, d)).astype(np.float32)
    c.mix, c.y = mmoe_ref(c.x, c.w, T, len(towers), act)
    return c


# ------------------------------------------------------------------ CPU
def test_restatement_known_answers():
    """d 2, H 1, E 2, T 2, x = [1, 2], by hand.  Experts: x @ [[1, -1], [0.5,
    0]] + [0, 0.5] = [2, -0.5] -> relu [2, 0].  Gate 0: zeros -> softmax
    [0.5, 0.5] -> mix 1.0.  Gate 1: logits [ln 3, 0] -> softmax [0.75, 0.25]
    -> mix 1.5.  Towers (no hidden layer): 2 * mix - 1 -> 1.0 and 2.0."""
    em = np.array([[[1.0, -1.0]], [[0.5, 0.0]]])  # [d, H, E]
    eb = np.array([[0.0, 0.5]])
    gms = [np.zeros((2, 2)), np.array([[np.log(3.0), 0.0], [0.0, 0.0]])]
    mix = mmoe_layer_ref([[1.0, 2.0]], em, eb, gms, None)
    np.testing.assert_allclose(mix, [[1.0, 1.5]], rtol=1e-15)
    w = {"mmoe_layer/expert_matrix": em, "mmoe_layer/expert_bias": eb,
         "mmoe_layer/gate_matrix0": gms[0], "mmoe_layer/gate_matrix1": gms[1]}
    for t in range(2):
        w[f"tower_layer_{t}/dense_out/kernel"], w[f"tower_layer_{t}/dense_out/bias"] = np.array([[2.0]]), np.array([-1.0])
    mix2, y = mmoe_ref([[1.0, 2.0]], w, 2, 0)
    np.testing.assert_array_equal(mix2, mix)
    np.testing.assert_allclose(y, [[[1.0]], [[2.0]]], rtol=1e-15)
    # E = 1: every gate is exactly 1, the mix is the relu expert output
    rng = np.random.default_rng(0)
    em1, x = rng.normal(size=(3, 4, 1)), rng.normal(size=(6, 3))
    gms1 = [rng.normal(size=(3, 1)) for _ in range(2)]
    want = np.maximum(x @ em1[:, :, 0], 0)
    np.testing.assert_array_equal(mmoe_layer_ref(x, em1, None, gms1, [np.array([5.0]), np.array([-7.0])]),
                                  np.concatenate([want, want], 1))


def test_restatement_softmax_is_stable():
    """Gate bias [90, 0, -90]: exp(90) overflows fp32 and the naive fp32
    softmax is NaN; the restatement's gates are finite and sum to 1."""
    g = softmax_ref(np.array([[90.0, 0.0, -90.0], [0.3, 90.2, -89.0]]))
    assert np.isfinite(g).all() and np.all(g >= 0)
    np.testing.assert_allclose(g.sum(-1), 1.0, rtol=1e-15)
    with np.errstate(over="ignore", invalid="ignore"):
        naive = np.exp(np.float32([90.0, 0.0, -90.0]))
        assert not np.isfinite(naive / naive.sum()).all()
    em = np.zeros((2, 2, 3))
    em[0] = [1.0, 2.0, 3.0]  # x = [1, -1]: both hidden units see the experts [1, 2, 3]
    mix = mmoe_layer_ref([[1.0, -1.0]], em, None, [np.zeros((2, 3))], [np.array([90.0, 0.0, -90.0])])
    np.testing.assert_allclose(mix, [[1.0, 1.0]], rtol=1e-15)  # expert 0 (value 1) takes all the weight


@pytest.mark.parametrize("eb,gb", [(True, True), (True, False), (False, True), (False, False)])
def test_keras_names_shapes_and_round_trip_cpu(eb, gb):
    import recommender_system_amd as rs
    layer = rs.mmoe_layer(5, 3, 2, use_expert_bias=eb, use_gate_bias=gb, device="cpu", seed=1)
    assert not layer.built
    with pytest.raises(RuntimeError):
        layer.keras_weights()
    layer.build(7)
    want = {"expert_matrix": (7, 5, 3)}
    if eb:
        want["expert_bias"] = (5, 3)
    want.update({f"gate_matrix{t}": (7, 3) for t in range(2)})
    if gb:
        want.update({f"gate_bias{t}": (3,) for t in range(2)})
    assert {n: tuple(v.shape) for n, v in layer.keras_weights().items()} == want

    m = rs.MMOE(5, 3, 2, [4, 6], 3, use_expert_bias=eb, use_gate_bias=gb, device="cpu", seed=0, input_dim=7)
    full = {"mmoe_layer/" + n: s for n, s in want.items()}
    for t in range(2):
        p = f"tower_layer_{t}/"
        full.update({p + "dense_0/kernel": (5, 4), p + "dense_0/bias": (4,), p + "dense_1/kernel": (4, 6),
                     p + "dense_1/bias": (6,), p + "dense_out/kernel": (6, 3), p + "dense_out/bias": (3,)})
    assert {n: tuple(v.shape) for n, v in m.keras_weights().items()} == full
    assert not torch.equal(m.tower_layer[0].output_layer.kernel, m.tower_layer[1].output_layer.kernel)
    new = {n: np.full(s, float(i)) for i, (n, s) in enumerate(full.items())}
    m.set_keras_weights(new)
    assert all(float(v.mean()) == i for i, v in enumerate(m.keras_weights().values()))
    with pytest.raises(KeyError):
        m.set_keras_weights({k: v for k, v in new.items() if k != "tower_layer_1/dense_out/kernel"})
    with pytest.raises(KeyError):
        m.set_keras_weights({k: v for k, v in new.items() if k != "mmoe_layer/gate_matrix1"})
    with pytest.raises(KeyError):
        m.set_keras_weights({**new, "tower_layer_2/dense_0/kernel": np.zeros((5, 4))})
    lw = {n: np.full(s, float(i + 1)) for i, (n, s) in enumerate(want.items())}
    layer.set_keras_weights(lw)
    assert all(float(v.mean()) == i + 1 for i, v in enumerate(layer.keras_weights().values()))
    with pytest.raises(KeyError):
        layer.set_keras_weights({k: v for k, v in lw.items() if k != "expert_matrix"})


def test_initialisers_cpu():
    """random_normal_initializer() (mean 0, std 0.05) for all four weight
    kinds of the layer; the towers are Keras Dense: glorot kernels, zero biases."""
    import recommender_system_amd as rs
    m = rs.MMOE(32, 8, 2, [16], 1, device="cpu", seed=3, input_dim=64)
    w = {n: v.detach().numpy() for n, v in m.keras_weights().items()}
    em = w["mmoe_layer/expert_matrix"]
    assert abs(float(em.std()) - 0.05) < 0.002 and abs(float(em.mean())) < 0.002
    gm = np.concatenate([w[f"mmoe_layer/gate_matrix{t}"].ravel() for t in range(2)])
    assert abs(float(gm.std()) - 0.05) < 0.005
    assert abs(float(w["mmoe_layer/expert_bias"].std()) - 0.05) < 0.01
    for t in range(2):
        gb = w[f"mmoe_layer/gate_bias{t}"]
        assert np.all(gb != 0) and float(np.abs(gb).max()) < 0.3
        assert all(float(np.abs(w[n]).max()) == 0 for n in w if n.startswith(f"tower_layer_{t}/") and n.endswith("bias"))
    assert not np.array_equal(w["mmoe_layer/gate_matrix0"], w["mmoe_layer/gate_matrix1"])
    lim = np.sqrt(6.0 / (32 + 16))
    k0 = np.abs(w["tower_layer_0/dense_0/kernel"]).max()
    assert 0.5 * lim < k0 <= lim
    assert isinstance(m.tower_layer[0], rs.DNNLayer) and isinstance(m.tower_layer[0], rs.tower_layer)


def _cfg_args(c):
    return c["d"], c["H"], c["E"], c["T"], len(c["towers"]) + 1, _ints([c["H"], *c["towers"], c["out"]])


def test_abi_queries_cpu():
    lib = _lib.lib()
    for cfg in (TOY, TIMING):
        assert lib.rs_mmoe_ok(*_cfg_args(cfg)) == 1
        assert lib.rs_mmoe_prepared_size(*_cfg_args(cfg)) == expected_prepared_size(
            cfg["d"], cfg["H"], cfg["E"], cfg["T"], [cfg["H"], *cfg["towers"], cfg["out"]])
    # the layer alone, with and without a tower_dims array
    assert lib.rs_mmoe_ok(4, 10, 3, 3, 0, None) == 1 and lib.rs_mmoe_ok(4, 10, 3, 3, 0, _ints([10])) == 1
    assert lib.rs_mmoe_prepared_size(4, 10, 3, 3, 0, None) == expected_prepared_size(4, 10, 3, 3, [10])
    assert lib.rs_mmoe_prepared_size(221, 64, 8, 2, 1, _ints([64, 3])) == expected_prepared_size(221, 64, 8, 2, [64, 3])
    dims = _ints([10, 20, 10, 1])
    bad = {"E = 0": (4, 10, 0, 3, 3, dims), "T = 0": (4, 10, 3, 0, 3, dims), "d = 0": (0, 10, 3, 3, 3, dims),
           "E over the cap": (4, 10, 17, 3, 3, dims), "T over the cap": (4, 10, 3, 9, 3, dims),
           "width over the cap": (4, 10, 3, 3, 3, _ints([10, 1025, 10, 1])),
           "d over the cap": (1025, 10, 3, 3, 3, dims),
           "tower_dims[0] != hidden": (4, 10, 3, 3, 3, _ints([12, 20, 10, 1])),
           "too many tower layers": (4, 10, 3, 3, 5, _ints([10, 8, 8, 8, 8, 1])),
           "N1 over the cap": (4, 64, 16, 8, 1, _ints([64, 1])),
           "towers that do not fit the LDS": (4, 10, 3, 8, 2, _ints([10, 1024, 1])),
           "towers without tower_dims": (4, 10, 3, 3, 1, None)}
    for what, args in bad.items():
        assert lib.rs_mmoe_ok(*args) == 0, what
        assert lib.rs_mmoe_prepared_size(*args) == -1, what
        assert b"rs_mmoe_prepared_size" in lib.rs_last_error_string()


def test_abi_validation_launches_nothing_cpu():
    """Bad arguments return RS_ERR_ARG (-1) with a message before any device
    work: a launch attempt would return RS_ERR_HIP (-2) on this device-less
    process, or fault on the fake pointers."""
    lib = _lib.lib()
    one = C.c_void_p(16)
    dims, acts = _ints([10, 20, 10, 1]), _ints([1, 1, 0])
    fwd = lambda x, prep, L, mix, y, **k: lib.rs_mmoe_fwd(
        x, k.get("xs", 4), 4, 10, 3, 3, L, dims, k.get("acts", acts), prep, mix, 30, y, k.get("yts", 2), 1,
        k.get("batch", 2), None)
    assert fwd(None, one, 3, None, one) == -1 and b"null" in lib.rs_last_error_string()
    assert fwd(one, None, 3, None, one) == -1 and b"null" in lib.rs_last_error_string()
    assert fwd(one, one, 0, None, None) == -1 and b"mix" in lib.rs_last_error_string()
    assert fwd(one, one, 3, None, None) == -1 and b"null" in lib.rs_last_error_string()
    assert fwd(one, one, 3, None, one, acts=None) == -1
    assert fwd(one, one, 3, None, one, xs=3) == -1 and b"stride" in lib.rs_last_error_string()
    assert fwd(one, one, 3, None, one, acts=_ints([2, 1, 0])) == -1 and b"activation" in lib.rs_last_error_string()
    assert fwd(one, one, 3, None, one, batch=-1) == -1
    assert lib.rs_mmoe_fwd(one, 4, 4, 10, 0, 3, 3, dims, acts, one, None, 0, one, 2, 1, 2, None) == -1
    # batch 0: nothing to do, whatever the pointers
    assert fwd(None, None, 3, None, None, batch=0) == 0
    # prepare: shape and pointers first
    gm = (C.c_void_p * 3)(16, 16, 16)
    tw = (C.c_void_p * 9)(*[16] * 9)
    prep = lambda em, g, t, out, E=3: lib.rs_mmoe_prepare(4, 10, E, 3, em, None, g, None, 3, dims, t, None, out, None)
    assert prep(None, gm, tw, one) == -1 and b"null" in lib.rs_last_error_string()
    assert prep(one, None, tw, one) == -1 and prep(one, gm, None, one) == -1 and prep(one, gm, tw, None) == -1
    assert prep(one, (C.c_void_p * 3)(16, None, 16), tw, one) == -1 and b"gate_matrix" in lib.rs_last_error_string()
    assert prep(one, gm, (C.c_void_p * 9)(*([16] * 8 + [None])), one) == -1 and b"kernel" in lib.rs_last_error_string()
    assert prep(one, gm, tw, one, E=0) == -1


def test_no_cpu_fallback():
    import recommender_system_amd as rs
    m = rs.MMOE(10, 3, 3, [20, 10], 1, device="cpu", seed=0)
    with pytest.raises(_lib.RSError, match="device"):
        m(TOY_X)
    assert m.mmoe_layer.built and m.mmoe_layer.input_dim == 4  # built lazily by the call
    with pytest.raises(_lib.RSError, match="device"):
        m.forward_unfused(TOY_X)
    with pytest.raises(_lib.RSError, match="device"):
        rs.mmoe_layer(10, 3, 3, device="cpu", seed=0)(TOY_X)
    # a tower activation the fused towers do not take; the model is still built and exchanged
    assert not rs.MMOE(10, 3, 3, [20], 1, activation="dice", device="cpu", seed=0, input_dim=4).fused_ok()
    assert not rs.MMOE(10, 3, 3, [20], 1, activation="prelu", device="cpu", seed=0, input_dim=4).fused_ok()
    assert rs.MMOE(10, 3, 3, [20, 10], 1, device="cpu", seed=0, input_dim=4).fused_ok()
    assert rs.MMOE(64, 8, 2, [32, 16], 1, device="cpu", seed=0, input_dim=221).fused_ok()
    assert not rs.MMOE(10, 3, 8, [1024], 1, device="cpu", seed=0, input_dim=4).fused_ok()


# ------------------------------------------------------------------ GPU
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


def abi_forward(gpu, c, x=None, with_mix=True, towers=True, x_pad=0, mix_pad=3):
    """rs_mmoe_prepare + rs_mmoe_fwd on case c's weights through the raw ABI:
    (mix [B, T H] or None, y [T, B, out] or None).  x and mix live in wider
    buffers (row strides d + x_pad, T H + mix_pad) whose padding must survive."""
    lib = _lib.lib()
    st = _lib.stream()
    x = c.x if x is None else x
    B = x.shape[0]
    d, H, E, T = c.d, c.H, c.E, c.T
    dims = c.dims if towers else [H]
    L = len(dims) - 1
    w = {n: _dev(v, gpu) for n, v in c.w.items()}
    p = lambda n: _lib.ptr(w.get(n))
    pa = lambda names: (C.c_void_p * len(names))(*[p(n) for n in names])
    tnames = [f"tower_layer_{t}/" + (f"dense_{i}" if i < L - 1 else "dense_out") for t in range(T) for i in range(L)]
    size = lib.rs_mmoe_prepared_size(d, H, E, T, L, _ints(dims))
    assert size == expected_prepared_size(d, H, E, T, dims)
    prep = torch.empty(size, dtype=torch.float32, device=gpu)
    has_gb = "mmoe_layer/gate_bias0" in w
    _lib.call("rs_mmoe_prepare", d, H, E, T, p("mmoe_layer/expert_matrix"), p("mmoe_layer/expert_bias"),
              pa([f"mmoe_layer/gate_matrix{t}" for t in range(T)]),
              pa([f"mmoe_layer/gate_bias{t}" for t in range(T)]) if has_gb else None, L, _ints(dims),
              pa([n + "/kernel" for n in tnames]) if L else None, pa([n + "/bias" for n in tnames]) if L else None,
              _lib.ptr(prep), st)
    xb = torch.full((B, d + x_pad), float("nan"), device=gpu)
    xb[:, :d] = _dev(x, gpu)
    mixb = torch.full((B, T * H + mix_pad), -7.0, device=gpu) if with_mix else None
    y = torch.full((T, B, c.out), float("nan"), device=gpu) if L else None
    acts = [_lib.ACT[c.act]] * (L - 1) + [0]
    _lib.call("rs_mmoe_fwd", _lib.ptr(xb), xb.stride(0), d, H, E, T, L, _ints(dims), _ints(acts) if L else None,
              _lib.ptr(prep), _lib.ptr(mixb), mixb.stride(0) if with_mix else 0, _lib.ptr(y),
              y.stride(0) if L else 0, y.stride(1) if L else 0, B, st)
    torch.cuda.synchronize()
    if with_mix:
        assert bool((mixb[:, T * H:] == -7.0).all()), "mix: wrote past T * H columns"
        return mixb[:, :T * H].contiguous(), y
    return None, y


def check_case(gpu, c, x=None, ref=None, **kw):
    mix_ref, y_ref = ref if ref is not None else (c.mix, c.y)
    mix, y = abi_forward(gpu, c, x=x, **kw)
    assert bool(torch.isfinite(mix).all()) and bool(torch.isfinite(y).all())
    assert_scaled_close(mix, mix_ref, what="mix")
    for t in range(c.T):
        assert_scaled_close(y[t], y_ref[t], what=f"tower {t}")
    return mix, y


@gpu_test
def test_toy_configuration(gpu):
    """The reference's own configuration (model/mmoe.py:35-48): N1 = 39 is not
    a multiple of 16, expert and gate columns share a tile, E is not a power
    of two; on its own input and on random rows with negatives."""
    c = make_case(**TOY, B=7)
    check_case(gpu, c)
    check_case(gpu, c, x=TOY_X, ref=mmoe_ref(TOY_X, c.w, c.T, 2))


@gpu_test
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_batch_edges(gpu, B):
    check_case(gpu, make_case(**TOY, B=B), x_pad=5)


@gpu_test
@pytest.mark.parametrize("d", [1, 15, 16, 17, 221])
def test_input_width_edges(gpu, d):
    check_case(gpu, make_case(**{**TOY, "d": d}, B=19), x_pad=0 if d % 2 else 3)


@gpu_test
@pytest.mark.parametrize("H,E,T,towers", [
    (10, 3, 1, (20, 10)),   # N1 33: 3 tiles, K-split in stage 1; T 1: every tower layer K-split
    (9, 4, 3, (70,)),       # N1 48: 3 full tiles, the widest split shape; 3 x 5 tower tiles
    (12, 4, 3, (20,)),      # N1 60: padded up to 4 tiles
    (13, 4, 3, (8,)),       # N1 64: exactly 4 tiles, whole columns per wave; 3 tower tiles (split)
    (14, 4, 3, (40, 24)),   # N1 68: 5 tiles
    (64, 8, 2, (32, 16)),   # the timing shape: 33 tiles, more items than waves
])
def test_split_threshold_sides(gpu, H, E, T, towers):
    """N1 below and above 64 columns (MLP_SPLIT_T = 4 output tiles: K-split
    with the LDS reduction below, whole columns per wave from there on), and
    tower layers on both sides of it."""
    check_case(gpu, make_case(d=37, H=H, E=E, T=T, towers=towers, out=1, B=18))


@gpu_test
@pytest.mark.parametrize("over", [
    dict(E=1), dict(E=2), dict(E=16), dict(E=8, H=64, d=40), dict(T=1), dict(T=8),
    dict(eb=False), dict(gb=False), dict(eb=False, gb=False),
    dict(towers=()), dict(towers=(), out=3), dict(out=3), dict(act="sigmoid"), dict(act="sigmoid", out=3, T=2),
    dict(towers=(20, 10, 7), out=2),
], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_structure_edges(gpu, over):
    cfg = {**TOY, **over}
    c = make_case(**cfg, B=18)
    mix, _ = check_case(gpu, c)
    if c.E == 1:  # every gate is exactly 1: the mix is the relu expert output of every task
        assert torch.equal(mix[:, :c.H], mix[:, c.H:2 * c.H] if c.T > 1 else mix[:, :c.H])


@gpu_test
def test_softmax_stability_on_device(gpu):
    """Gate bias [90, 0, -90]: a softmax without max-subtraction is NaN in
    fp32 (exp(90) = inf).  Task 1 gets the reverse, task 2 a tie at the top."""
    c = make_case(**TOY, B=18)
    w = dict(c.w)
    w["mmoe_layer/gate_bias0"] = np.float32([90.0, 0.0, -90.0])
    w["mmoe_layer/gate_bias1"] = np.float32([-90.0, 0.0, 90.0])
    w["mmoe_layer/gate_bias2"] = np.float32([88.0, 88.0, -30.0])
    c2 = Case()
    c2.__dict__.update(c.__dict__)
    c2.w = w
    ref = mmoe_ref(c.x, w, c.T, 2)
    assert np.isfinite(ref[0]).all()
    check_case(gpu, c2, ref=ref)


@gpu_test
def test_contracts_bit_exact(gpu):
    c = make_case(**TOY, B=33)
    mix, y = abi_forward(gpu, c)
    # a row alone and as row 20 of 33
    mix1, y1 = abi_forward(gpu, c, x=c.x[20:21])
    assert torch.equal(mix1[0], mix[20]) and torch.equal(y1[:, 0], y[:, 20])
    # ... and as row 3 of another batch (another place in its tile)
    mix3, y3 = abi_forward(gpu, c, x=c.x[17:25])
    assert torch.equal(mix3, mix[17:25]) and torch.equal(y3, y[:, 17:25])
    # y with and without the mix output
    _, y_nomix = abi_forward(gpu, c, with_mix=False)
    assert torch.equal(y_nomix, y)
    # the layer-only launch
    mix_only, none = abi_forward(gpu, c, towers=False)
    assert none is None and torch.equal(mix_only, mix)
    # two runs
    mix_b, y_b = abi_forward(gpu, c)
    assert torch.equal(mix_b, mix) and torch.equal(y_b, y)
    # the same on a shape with whole-column stage 1 and more items than waves
    c = make_case(**TIMING, B=33)
    mix, y = check_case(gpu, c)
    mix1, y1 = abi_forward(gpu, c, x=c.x[20:21], with_mix=True)
    assert torch.equal(mix1[0], mix[20]) and torch.equal(y1[:, 0], y[:, 20])
    assert torch.equal(abi_forward(gpu, c, towers=False)[0], mix)
    assert torch.equal(abi_forward(gpu, c, with_mix=False)[1], y)


def _model(gpu, c, **kw):
    import recommender_system_amd as rs
    m = rs.MMOE(c.H, c.E, c.T, list(c.towers), c.out, activation=c.act,
                use_expert_bias="mmoe_layer/expert_bias" in c.w, use_gate_bias="mmoe_layer/gate_bias0" in c.w,
                device=gpu, seed=0, input_dim=c.d, **kw)
    m.set_keras_weights(c.w)
    return m


@gpu_test
def test_model_paths_agree(gpu):
    """forward_fused against forward_unfused and fp64, the layer alone, and a
    shape the one-launch form refuses through forward."""
    import recommender_system_amd as rs
    c = make_case(**TOY, B=33)
    m = _model(gpu, c)
    assert m.fused_ok() and m.mmoe_layer.fused_ok()
    fused, unfused, auto = m.forward_fused(c.x), m.forward_unfused(c.x), m(c.x)
    assert len(fused) == c.T and all(tuple(f.shape) == (c.B, c.out) for f in fused)
    for t in range(c.T):
        assert_scaled_close(fused[t], c.y[t], what=f"fused tower {t}")
        assert_scaled_close(unfused[t], c.y[t], what=f"unfused tower {t}")
        assert_scaled_close(fused[t], unfused[t].cpu().numpy(), rtol=2 * RTOL, what=f"fused vs unfused {t}")
        assert torch.equal(auto[t], fused[t])
    mixes = m.mmoe_layer(c.x)
    assert len(mixes) == c.T and all(tuple(v.shape) == (c.B, c.H) for v in mixes)
    assert mixes[0].data_ptr() + 4 * c.H == mixes[1].data_ptr()  # views of one [B, T H] buffer
    assert_scaled_close(torch.cat(mixes, 1), c.mix, what="layer mix")
    assert_scaled_close(m.mmoe_layer.forward_unfused(_dev(c.x, gpu)), c.mix, what="layer mix, unfused")
    mixbuf = torch.empty(c.B, c.T * c.H, device=gpu)
    again = m.forward_fused(c.x, mix=mixbuf)
    assert torch.equal(mixbuf, torch.cat(mixes, 1)) and all(torch.equal(a, f) for a, f in zip(again, fused))
    # refused shapes still give the right answer through forward: towers too wide for the tile ...
    c = make_case(d=9, H=10, E=3, T=8, towers=(160,), out=2, B=17)
    m = _model(gpu, c)
    assert not m.fused_ok() and m.mmoe_layer.fused_ok()
    for t, yt in enumerate(m(c.x)):
        assert_scaled_close(yt, c.y[t], what=f"refused shape, tower {t}")
    with pytest.raises(_lib.RSError):
        m.forward_fused(c.x)
    # ... and an activation the fused towers do not take
    c = make_case(**TOY, B=6)
    m = rs.MMOE(c.H, c.E, c.T, list(c.towers), c.out, activation="prelu", device=gpu, seed=0, input_dim=c.d)
    assert not m.fused_ok()
    m.set_keras_weights({**c.w, **{n: np.zeros(tuple(v.shape)) for n, v in m.keras_weights().items()
                                   if n.endswith("alpha")}})
    for t, yt in enumerate(m(c.x)):  # alpha 0: PReLU is relu
        assert_scaled_close(yt, c.y[t], what=f"prelu towers, tower {t}")


@gpu_test
def test_cache_invalidation_and_graph(gpu):
    c = make_case(**TOY, B=33)
    m = _model(gpu, c)
    x = _dev(c.x, gpu)
    before = [v.clone() for v in m(x)]
    # weights changed in place after a forward are picked up
    with torch.no_grad():
        m.mmoe_layer.gate_bias0.add_(0.5)
        m.tower_layer[1].output_layer.bias.add_(0.25)
    w2 = {n: v.detach().cpu().numpy() for n, v in m.keras_weights().items()}
    ref = mmoe_ref(c.x, w2, c.T, 2)[1]
    after = m(x)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
    for t in range(c.T):
        assert_scaled_close(after[t], ref[t], what=f"after the update, tower {t}")
    mix_after = torch.cat(m.mmoe_layer(x), 1)
    assert_scaled_close(mix_after, mmoe_ref(c.x, w2, c.T, 2)[0], what="layer mix after the update")
    # capture and replay
    eager = [v.clone() for v in m.forward_fused(x)]
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = m.forward_fused(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, eager))
    x2 = _dev(make_case(**TOY, B=33, seed=1).x, gpu)
    want = [v.clone() for v in m.forward_fused(x2)]
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, want)) and not torch.equal(out[0], eager[0])


@gpu_test
def test_empty_batch(gpu):
    c = make_case(**TOY, B=7)
    m = _model(gpu, c)
    out = m.forward_fused(torch.empty(0, c.d, device=gpu))
    assert len(out) == c.T and all(tuple(o.shape) == (0, c.out) for o in out)
    assert all(tuple(v.shape) == (0, c.H) for v in m.mmoe_layer(torch.empty(0, c.d, device=gpu)))
