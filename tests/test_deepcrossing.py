"""ResLayer (layer/interaction.py:261-278) and DeepCrossing
(model/deepCrossing.py:15-32) on the residual tower kernel (res_tower.hip).

The fp64 restatements (res_layer_ref, deepcrossing_ref) are composed from the
oracle's Dense / EmbedLayer and pinned by hand-computed cases.  CPU tests
cover the restatements, the Keras weight exchange, the support / size queries
and the argument checks (nothing is launched); the GPU tests compare the
kernels at the project's tolerance (tests.helpers.RTOL) and check the
bit-exactness contracts of the ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_rel_close, assert_scaled_close, criteo_columns, random_ids, tables_of

gpu_test = pytest.mark.gpu


def res_layer_ref(x, hidden, out, dt=np.float64):
    """ResLayer.call: Dense(relu) per (kernel, bias) of `hidden`, the linear
    Dense `out` back to the input width, relu(x + h)."""
    x = np.asarray(x, dt)
    h = x
    for kern, bias in hidden:
        h = O.dense(h, kern, bias, "relu", dt=dt)
    h = O.dense(h, out[0], out[1], None, dt=dt)
    return np.maximum(x + h, 0.0)


def res_stack_ref(x, units, dt=np.float64):
    for hidden, out in units:
        x = res_layer_ref(x, hidden, out, dt)
    return x


def deepcrossing_ref(dense, ids, tables, units, head, dt=np.float64):
    """DeepCrossing.call: (sigmoid(Dense1(x_L)), x_L) with x_0 = [dense | EmbedLayer(ids)]."""
    x = np.concatenate([np.asarray(dense, dt), O.embed_layer(ids, tables, dt)], axis=1)
    x = res_stack_ref(x, units, dt)
    return O.sigmoid(O.dense(x, head[0], head[1], None, dt=dt)), x


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def rand_units(rng, d, hidden, n_units):
    """Random weights in Keras shapes: glorot-sized kernels, small non-zero biases."""
    units = []
    for _ in range(n_units):
        dims = [d] + list(hidden) + [d]
        layers = []
        for kin, nout in zip(dims[:-1], dims[1:]):
            lim = np.sqrt(6.0 / (kin + nout))
            layers.append((rng.uniform(-lim, lim, (kin, nout)).astype(np.float32),
                           rng.normal(0, 0.05, nout).astype(np.float32)))
        units.append((layers[:-1], layers[-1]))
    return units


def unit_weights(unit):
    hidden, out = unit
    w = {}
    for i, (kern, bias) in enumerate(hidden):
        w[f"dense_{i}/kernel"], w[f"dense_{i}/bias"] = kern, bias
    w["dense_out/kernel"], w["dense_out/bias"] = out
    return w


def expected_prepared_size(d, hidden, n_units, head):
    up = lambda v: (v + 15) // 16 * 16
    dims = [d] + list(hidden) + [d]
    unit = sum(up(a) * up(b) + up(b) for a, b in zip(dims[:-1], dims[1:]))
    return n_units * unit + head * (up(d) + 16)


# ------------------------------------------------------------------ CPU
def test_restatement_known_answers():
    """d = 2, one hidden unit, by hand.  x = [1, -2]; hidden = relu(1*1 +
    (-2)*0.5 + 0.5) = 0.5; out = 0.5 * [2, -4] + [0, 0.5] = [1, -1.5];
    x + out = [2, -3.5] -> relu = [2, 0]: the second column's pre-skip sum is
    negative, so the result there is 0, not the skip value -2 (nor its relu)."""
    hidden = [(np.array([[1.0], [0.5]]), np.array([0.5]))]
    out = (np.array([[2.0, -4.0]]), np.array([0.0, 0.5]))
    np.testing.assert_allclose(res_layer_ref([[1.0, -2.0]], hidden, out), [[2.0, 0.0]], rtol=0, atol=0)
    # a positive skip under a negative branch: x = [3, 1] -> hidden 4, out [8, -15.5], sum [11, -14.5]
    np.testing.assert_allclose(res_layer_ref([[3.0, 1.0]], hidden, out), [[11.0, 0.0]], rtol=0, atol=0)
    # all-zero weights: every unit is relu(x)
    z = [([(np.zeros((3, 4)), np.zeros(4))], (np.zeros((4, 3)), np.zeros(3)))] * 3
    x = np.array([[1.0, -2.0, 0.5], [-1.0, 0.0, 4.0]])
    np.testing.assert_array_equal(res_stack_ref(x, z), np.maximum(x, 0))
    # the model: one field of two rows, no dense, head picks column 0
    prob, xl = deepcrossing_ref(np.zeros((2, 0)), [[1], [0]], [np.array([[1.0, -2.0], [3.0, 1.0]])],
                                [(hidden, out)], (np.array([[1.0], [0.0]]), np.array([-11.0])))
    np.testing.assert_array_equal(xl, [[11.0, 0.0], [2.0, 0.0]])
    np.testing.assert_allclose(prob, [[0.5], [1 / (1 + np.exp(9.0))]], rtol=1e-15)


def test_keras_names_and_round_trip_cpu():
    import recommender_system_amd as rs
    layer = rs.ResLayer([5, 7], device="cpu", seed=1)
    assert not layer.built
    layer.build(6)
    w = layer.keras_weights()
    assert {n: tuple(v.shape) for n, v in w.items()} == {
        "dense_0/kernel": (6, 5), "dense_0/bias": (5,), "dense_1/kernel": (5, 7), "dense_1/bias": (7,),
        "dense_out/kernel": (7, 6), "dense_out/bias": (6,)}
    lim = np.sqrt(6.0 / (6 + 5))
    assert float(w["dense_0/kernel"].abs().max()) <= lim and float(w["dense_0/kernel"].abs().max()) > 0.5 * lim
    assert all(float(w[n].abs().max()) == 0 for n in w if n.endswith("bias"))
    new = {n: np.full(tuple(v.shape), float(i)) for i, (n, v) in enumerate(w.items())}
    layer.set_keras_weights(new)
    assert all(float(v.mean()) == i for i, v in enumerate(layer.keras_weights().values()))
    with pytest.raises(KeyError):
        layer.set_keras_weights({k: v for k, v in new.items() if k != "dense_out/bias"})

    cols = criteo_columns([5, 3, 9], n_dense=2)
    m = rs.DeepCrossing(cols, 32, [4, 6], 2, device="cpu", seed=0)
    d = 2 + 3 * 8  # k = 32 is ignored: the embedding width is embed_dim = 8
    shapes = {n: tuple(v.shape) for n, v in m.keras_weights().items()}
    want = {f"embed_layer/embedding_{i}/embeddings": (v, 8) for i, v in enumerate([5, 3, 9])}
    for u in range(2):
        want.update({f"res_layer_{u}/dense_0/kernel": (d, 4), f"res_layer_{u}/dense_0/bias": (4,),
                     f"res_layer_{u}/dense_1/kernel": (4, 6), f"res_layer_{u}/dense_1/bias": (6,),
                     f"res_layer_{u}/dense_out/kernel": (6, d), f"res_layer_{u}/dense_out/bias": (d,)})
    want.update({"output_layer/kernel": (d, 1), "output_layer/bias": (1,)})
    assert shapes == want
    # the units have their own weights
    assert not torch.equal(m.res_layer[0].dense_layer[0].kernel, m.res_layer[1].dense_layer[0].kernel)
    new = {n: np.full(s, float(i)) for i, (n, s) in enumerate(want.items())}
    m.set_keras_weights(new)
    assert all(float(v.mean()) == i for i, v in enumerate(m.keras_weights().values()))
    with pytest.raises(KeyError):
        m.set_keras_weights({k: v for k, v in new.items() if k != "res_layer_1/dense_out/kernel"})
    with pytest.raises(KeyError):
        m.set_keras_weights({**new, "res_layer_2/dense_0/kernel": np.zeros((d, 4))})


def test_support_and_size_queries():
    lib = _lib.lib()
    ok = lambda d, hidden, n: lib.rs_res_tower_ok(d, len(hidden), _ints(hidden), n)
    assert ok(221, [256, 256], 4) == 1
    assert ok(429, [256, 256], 4) == 1
    assert ok(1024, [1024] * 4, 16) == 1
    assert ok(221, [], 4) == 0
    assert ok(221, [8] * 5, 4) == 0
    assert ok(221, [256, 256], 0) == 0
    assert ok(221, [256, 256], 17) == 0
    assert ok(1025, [256], 1) == 0
    assert ok(221, [256, 1025], 1) == 0
    assert ok(221, [0], 1) == 0
    size = lambda d, hidden, n, head: lib.rs_res_tower_prepared_size(d, len(hidden), _ints(hidden), n, head)
    assert size(221, [256, 256], 4, 1) == expected_prepared_size(221, [256, 256], 4, 1) \
        == 4 * (224 * 256 + 256 * 256 + 256 * 224 + 256 + 256 + 224) + 224 + 16
    assert size(33, [7, 50, 9], 3, 0) == expected_prepared_size(33, [7, 50, 9], 3, 0)
    assert size(221, [256, 256], 17, 0) == -1 and b"rs_res_tower_prepared_size" in lib.rs_last_error_string()
    assert size(221, [256, 256], 4, 2) == -1
    assert size(1025, [256], 1, 0) == -1


def test_argument_validation_without_device():
    lib = _lib.lib()
    p = C.c_void_p(16)
    h = _ints([8])
    err = lambda: lib.rs_last_error_string()
    # rs_res_tower_fwd: null pointers, a stride below the width, a bad shape, a bad head
    assert lib.rs_res_tower_fwd(None, 20, 20, 1, h, 1, p, 0, p, 20, 4, None) == -1
    assert b"rs_res_tower_fwd" in err() and b"null" in err()
    assert lib.rs_res_tower_fwd(p, 20, 20, 1, h, 1, None, 0, p, 20, 4, None) == -1 and b"null" in err()
    assert lib.rs_res_tower_fwd(p, 19, 20, 1, h, 1, p, 0, p, 20, 4, None) == -1
    assert b"rs_res_tower_fwd" in err() and b"stride" in err()
    assert lib.rs_res_tower_fwd(p, 20, 20, 1, h, 1, p, 0, p, 19, 4, None) == -1 and b"y_stride" in err()
    assert lib.rs_res_tower_fwd(p, 20, 20, 1, h, 17, p, 0, p, 20, 4, None) == -1 and b"rs_res_tower_fwd" in err()
    assert lib.rs_res_tower_fwd(p, 20, 20, 1, h, 1, p, 2, p, 20, 4, None) == -1 and b"rs_res_tower_fwd" in err()
    # rs_res_tower_prepare: no kernels, a missing kernel, a head bias without head weights
    assert lib.rs_res_tower_prepare(20, 1, h, 1, None, None, None, None, p, None) == -1
    assert b"rs_res_tower_prepare" in err() and b"null" in err()
    ws = (C.c_void_p * 2)(16, None)
    assert lib.rs_res_tower_prepare(20, 1, h, 1, ws, None, None, None, p, None) == -1
    assert b"rs_res_tower_prepare" in err() and b"layer 1" in err()
    ws = (C.c_void_p * 2)(16, 16)
    assert lib.rs_res_tower_prepare(20, 1, h, 1, ws, None, None, p, p, None) == -1 and b"head_b" in err()
    # rs_deepcrossing_fwd: d = 4 + 2 * 8 = 20
    dc = lambda ids=p, kind=0, ids_s=2, dense=p, dense_s=4, table=p, out=p, xl=None, xls=0: lib.rs_deepcrossing_fwd(
        ids, kind, ids_s, dense, dense_s, 4, table, p, p, 2, 8, 1, h, 1, p, out, xl, xls, 4, None, None)
    assert dc(ids=None) == -1 and b"rs_deepcrossing_fwd" in err() and b"null" in err()
    assert dc(out=None) == -1 and b"null" in err()
    assert dc(dense=None) == -1 and b"null" in err()
    assert dc(kind=3) == -1 and b"rs_deepcrossing_fwd" in err() and b"id_kind" in err()
    assert dc(kind=-1) == -1 and b"id_kind" in err()
    assert dc(ids_s=1) == -1 and b"rs_deepcrossing_fwd" in err() and b"stride" in err()
    assert dc(dense_s=3) == -1 and b"stride" in err()
    assert dc(xl=p, xls=19) == -1 and b"x_last_stride" in err()
    assert dc(table=C.c_void_p(20)) == -1 and b"16-B aligned" in err()
    # an empty batch launches nothing and needs no pointers
    assert lib.rs_res_tower_fwd(None, 0, 20, 1, h, 1, None, 0, None, 0, 0, None) == 0


def test_train_step_not_implemented():
    import recommender_system_amd as rs
    m = rs.DeepCrossing(criteo_columns([5, 3], n_dense=2), 8, [4], 1, device="cpu", seed=0)
    with pytest.raises(NotImplementedError, match="DeepCrossing"):
        m.train_step(np.zeros((2, 4)), np.zeros(2))


# ------------------------------------------------------------------ GPU
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def _flat(units):
    return [l for hidden, out in units for l in list(hidden) + [out]]


def run_res_tower(gpu, x, d, hidden, units, head=None, y=None, batch=None):
    """rs_res_tower_prepare + rs_res_tower_fwd on device x; returns y."""
    lib = _lib.lib()
    nh, nu = len(hidden), len(units)
    layers = [(_dev(k, gpu), _dev(b, gpu)) for k, b in _flat(units)]
    hw = None if head is None else (_dev(head[0].reshape(-1), gpu), _dev(head[1].reshape(-1), gpu))
    size = lib.rs_res_tower_prepared_size(d, nh, _ints(hidden), nu, 0 if head is None else 1)
    assert size > 0
    prep = torch.full((size,), float("nan"), dtype=torch.float32, device=gpu)
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    st = _lib.stream()
    _lib.call("rs_res_tower_prepare", d, nh, _ints(hidden), nu, arr([k for k, _ in layers]),
              arr([b for _, b in layers]), None if hw is None else hw[0].data_ptr(),
              None if hw is None else hw[1].data_ptr(), prep.data_ptr(), st)
    B = x.shape[0] if batch is None else batch
    if y is None:
        y = torch.empty(B, 1 if head is not None else d, dtype=torch.float32, device=gpu)
    _lib.call("rs_res_tower_fwd", x.data_ptr(), x.stride(0), d, nh, _ints(hidden), nu, prep.data_ptr(),
              0 if head is None else 1, y.data_ptr(), y.stride(0), B, st)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(prep).any()), "rs_res_tower_prepare left part of the image unwritten"
    return y


@gpu_test
@pytest.mark.parametrize("d,hidden,B", [(221, [256, 256], 37), (221, [256, 256], 1), (20, [24], 5), (16, [16], 16),
                                        (33, [7, 50, 9], 17), (429, [256, 256], 3)])
def test_res_layer_vs_reference(gpu, d, hidden, B):
    import recommender_system_amd as rs
    rng = np.random.default_rng(d * 1000 + B)
    unit = rand_units(rng, d, hidden, 1)[0]
    layer = rs.ResLayer(hidden, device=gpu, seed=0)
    layer.build(d)
    layer.set_keras_weights(unit_weights(unit))
    assert layer.tower_ok()
    x = rng.normal(0, 1, (B, d)).astype(np.float32)
    assert (x < 0).any()
    ref = res_layer_ref(x, *unit)
    assert (ref == 0).any() and (ref > 0).any()
    got = layer(_dev(x, gpu))
    assert_scaled_close(got, ref, RTOL, "ResLayer (rs_res_tower_fwd)")
    assert_scaled_close(layer.forward_layers(_dev(x, gpu)), ref, RTOL, "ResLayer (per layer)")
    # a strided view (rows further apart than d) takes the same launch
    wide = torch.full((B, d + 5), 9.0, dtype=torch.float32, device=gpu)
    wide[:, :d] = _dev(x, gpu)
    assert torch.equal(layer(wide[:, :d]), got)


TOWER_CASES = [(221, [256, 256], 4, 37), (20, [24], 5, 18), (100, [300], 2, 9), (221, [256, 256], 16, 4)]


@gpu_test
@pytest.mark.parametrize("d,hidden,n_units,B", TOWER_CASES)
def test_res_tower_units_and_head(gpu, d, hidden, n_units, B):
    rng = np.random.default_rng(d + 7 * n_units)
    units = rand_units(rng, d, hidden, n_units)
    head = (rng.normal(0, 0.05, (d, 1)).astype(np.float32), np.array([0.1], np.float32))
    x = rng.normal(0, 1, (B, d)).astype(np.float32)
    xl = res_stack_ref(x, units)
    prob = O.sigmoid(O.dense(xl, head[0], head[1]))
    xd = _dev(x, gpu)
    # head 0 into a wider, pre-filled buffer with rows past the batch
    y = torch.full((B + 2, d + 3), -7.0, dtype=torch.float32, device=gpu)
    run_res_tower(gpu, xd, d, hidden, units, None, y=y, batch=B)
    assert_scaled_close(y[:B, :d], xl, RTOL, "x_L")
    assert bool((y[:B, d:] == -7).all()) and bool((y[B:] == -7).all())
    lib = _lib.lib()
    # head 1: one probability per sample, y_stride 2
    p = torch.full((B + 2, 2), -7.0, dtype=torch.float32, device=gpu)
    run_res_tower(gpu, xd, d, hidden, units, head, y=p, batch=B)
    assert_rel_close(p[:B, :1], prob, RTOL, "sigmoid head")
    assert bool((p[:B, 1] == -7).all()) and bool((p[B:] == -7).all())
    assert lib.rs_res_tower_ok(d, len(hidden), _ints(hidden), n_units) == 1


@gpu_test
def test_res_tower_widest_input(gpu):
    """d = 1000: 63 output tiles in a unit's last layer, so every wave holds
    three or four skip tiles in registers, and the largest LDS tile (148 KB)."""
    d, hidden, n_units, B = 1000, [40], 2, 5
    rng = np.random.default_rng(2)
    units = rand_units(rng, d, hidden, n_units)
    x = rng.normal(0, 1, (B, d)).astype(np.float32)
    y = run_res_tower(gpu, _dev(x, gpu), d, hidden, units)
    assert_scaled_close(y, res_stack_ref(x, units), RTOL, "x_L at d = 1000")


@gpu_test
@pytest.mark.parametrize("head", [0, 1])
def test_batch_invariance(gpu, head):
    d, hidden, B = 221, [256, 256], 37
    rng = np.random.default_rng(5)
    units = rand_units(rng, d, hidden, 4)
    hd = (rng.normal(0, 0.05, (d, 1)).astype(np.float32), np.array([0.1], np.float32)) if head else None
    x = _dev(rng.normal(0, 1, (B, d)).astype(np.float32), gpu)
    full = run_res_tower(gpu, x, d, hidden, units, hd)
    for lo, hi in ((0, 5), (32, 37)):
        part = run_res_tower(gpu, x[lo:hi].contiguous(), d, hidden, units, hd)
        assert torch.equal(full[lo:hi], part), f"rows {lo}:{hi} depend on the batch"


def _model(gpu, vocabs, nd, hidden, n_units, embed_dim=8, seed=0):
    import recommender_system_amd as rs
    rng = np.random.default_rng(seed + 11)
    m = rs.DeepCrossing(criteo_columns(vocabs, n_dense=nd, embed_dim=embed_dim), 32, hidden, n_units,
                        embed_dim=embed_dim, device=gpu, seed=seed)
    units = rand_units(rng, m.d, hidden, n_units)
    head = (rng.normal(0, 0.05, (m.d, 1)).astype(np.float32), np.array([0.1], np.float32))
    w = {n: v.detach().cpu().numpy() for n, v in m.keras_weights().items() if n.startswith("embed_layer/")}
    for u, unit in enumerate(units):
        w.update({f"res_layer_{u}/{k}": v for k, v in unit_weights(unit).items()})
    w["output_layer/kernel"], w["output_layer/bias"] = head
    m.set_keras_weights(w)
    return m, units, head


VOCABS = [7, 300, 12, 2, 1000, 55, 31, 9, 4, 610, 77, 13, 5, 3, 200, 41, 8, 19, 6, 150, 23, 11, 90, 10, 17, 29]


@gpu_test
@pytest.mark.parametrize("k", [8, 16])
def test_ids_form_is_bit_exact(gpu, k):
    nd, B, hidden = 13, 37, [256, 256]
    m, units, head = _model(gpu, VOCABS, nd, hidden, 4, embed_dim=k)
    assert m.fused_ok()
    rng = np.random.default_rng(3)
    dense = _dev(rng.random((B, nd)).astype(np.float32) - 0.3, gpu)
    ids = random_ids(rng, B, VOCABS)
    nh = len(hidden)
    x = m.embed_layer.gather(_dev(ids, gpu), dense)
    assert x.shape == (B, nd + 26 * k)
    st = _lib.stream()
    prob_x = torch.empty(B, 1, dtype=torch.float32, device=gpu)
    xl_x = torch.empty(B, m.d, dtype=torch.float32, device=gpu)
    for hd, y in ((1, prob_x), (0, xl_x)):
        _lib.call("rs_res_tower_fwd", x.data_ptr(), x.stride(0), m.d, nh, _ints(hidden), 4, m.prepared().data_ptr(),
                  hd, y.data_ptr(), y.stride(0), B, st)
    ref, ref_xl = deepcrossing_ref(dense.cpu().numpy(), ids, tables_of(m.embed_layer), units, head)
    assert_rel_close(prob_x, ref, RTOL, "rs_res_tower_fwd head 1")
    assert_scaled_close(xl_x, ref_xl, RTOL, "rs_res_tower_fwd head 0")
    for dt in (np.int32, np.int64, np.float32):
        xl = torch.full((B, m.d + 1), -7.0, dtype=torch.float32, device=gpu)
        got = m.forward_fused((dense, _dev(ids.astype(dt), gpu)), x_last=xl)
        assert torch.equal(got, prob_x), f"ids form differs from the x form ({dt.__name__} ids)"
        assert torch.equal(xl[:, :m.d], xl_x) and bool((xl[:, m.d] == -7).all())
        assert torch.equal(m.forward_fused((dense, _dev(ids.astype(dt), gpu))), prob_x)
    # out-of-range ids: a zero row and the flag
    bad = ids.copy()
    bad[3, 1] = VOCABS[1]
    bad[36, 25] = -1
    for dt in (np.int32, np.int64, np.float32):
        got = m.forward_fused((dense, _dev(bad.astype(dt), gpu)), check_ids=False)
        assert int(m._err.t.item()) == _lib.FLAG_BAD_ID
        m._err.t.zero_()
        xz = x.clone()
        xz[3, nd + k:nd + 2 * k] = 0
        xz[36, nd + 25 * k:] = 0
        want = torch.empty(B, 1, dtype=torch.float32, device=gpu)
        _lib.call("rs_res_tower_fwd", xz.data_ptr(), xz.stride(0), m.d, nh, _ints(hidden), 4,
                  m.prepared().data_ptr(), 1, want.data_ptr(), 1, B, st)
        assert torch.equal(got, want)
    with pytest.raises(IndexError):
        m.forward_fused((dense, _dev(bad, gpu)))


@gpu_test
@pytest.mark.parametrize("B", [37, 1])
def test_deepcrossing_model(gpu, B):
    nd, hidden = 13, [256, 256]
    m, units, head = _model(gpu, VOCABS, nd, hidden, 4)
    assert m.fused_ok()
    rng = np.random.default_rng(B)
    dense = rng.random((B, nd))
    ids = random_ids(rng, B, VOCABS)
    X = np.concatenate([dense, ids], axis=1)  # float64, as create_criteo_dataset returns it
    ref, _ = deepcrossing_ref(dense.astype(np.float32), ids, tables_of(m.embed_layer), units, head)
    for name in ("forward", "forward_fused", "forward_unfused"):
        f = getattr(m, name)
        assert_rel_close(f(X), ref, RTOL, f"DeepCrossing.{name}(X)")
        assert_rel_close(f((dense, ids)), ref, RTOL, f"DeepCrossing.{name}((dense, ids))")
    assert torch.equal(m(X), m.forward_fused(X))
    # new weights: a stale packed image would keep the old answer
    rng2 = np.random.default_rng(99)
    units2 = rand_units(rng2, m.d, hidden, 4)
    w = {n: v.detach().cpu().numpy() for n, v in m.keras_weights().items()}
    for u, unit in enumerate(units2):
        w.update({f"res_layer_{u}/{k}": v for k, v in unit_weights(unit).items()})
    m.set_keras_weights(w)
    ref2, _ = deepcrossing_ref(dense.astype(np.float32), ids, tables_of(m.embed_layer), units2, head)
    assert float(np.max(np.abs(ref2 - ref))) > 1e-3
    assert_rel_close(m(X), ref2, RTOL, "DeepCrossing after set_keras_weights")
    assert_rel_close(m.forward_unfused(X), ref2, RTOL, "DeepCrossing.forward_unfused after set_keras_weights")


@gpu_test
def test_deepcrossing_fallback_shape(gpu):
    """A width the tower kernel refuses still answers through rs_dense_fwd."""
    nd, hidden, B = 2, [1100], 9
    vocabs = [5, 30, 7]
    m, units, head = _model(gpu, vocabs, nd, hidden, 2)
    assert not m.fused_ok() and not m.res_layer[0].tower_ok()
    rng = np.random.default_rng(1)
    dense = rng.random((B, nd)).astype(np.float32)
    ids = random_ids(rng, B, vocabs)
    ref, _ = deepcrossing_ref(dense, ids, tables_of(m.embed_layer), units, head)
    assert_rel_close(m((dense, ids)), ref, RTOL, "DeepCrossing fallback")


@gpu_test
def test_deepcrossing_graph_capture(gpu):
    nd, B = 13, 37
    m, units, head = _model(gpu, VOCABS, nd, [256, 256], 4)
    rng = np.random.default_rng(8)
    dense = _dev(rng.random((B, nd)).astype(np.float32), gpu)
    ids = _dev(random_ids(rng, B, VOCABS), gpu)
    eager = m((dense, ids))  # also packs the weights (an allocation: not inside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = m((dense, ids), check_ids=False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # new inputs in place, replayed
    ids2 = _dev(random_ids(rng, B, VOCABS), gpu)
    want = m((dense, ids2))
    ids.copy_(ids2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
