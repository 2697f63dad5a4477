"""Host-side building blocks of the training steps (models.py, sharded.py).

Plain functions over the librs_hip entry points, one per piece of plumbing
that every ``train_step`` needs: grow-only scratch buffers, the row-sparse
embedding update, the BCE head, one Dense layer's backward, the DNNLayer
forward with saved activations and its backward, DNNLayer's Dropout, training
BatchNormalization, the forward and backward of DIEN's two recurrences, and
the FM part of a DeepFM step.  A step keeps its own
launches in its own body, in order; only what repeated from step to step lives
here.  Nothing here chooses a kernel or changes what a step requests: each
caller passes the sizes and workspace it passed when the lines were its own
("Host side of the training steps").
"""
from __future__ import annotations

import torch

# layers imports scratch and _subseed from this module, and _split_criteo needs
# two of layers' helpers: this side takes the module object and looks the names
# up when it is called, so layers may still be half-imported here
from . import _lib
from . import layers as _layers
from ._lib import call, ptr


def _subseed(gen):
    return int(torch.randint(0, 2 ** 31, (1,), generator=gen))


def _split_criteo(inputs, nd, device):
    """(dense f32 [B,nd], ids [B,F]) from X[B,nd+F] or a (dense, ids) pair."""
    if isinstance(inputs, (tuple, list)):
        dense, ids = inputs
        return _layers._to_device_f32(dense, device), _layers._ids_tensor(ids, device)
    X = _layers._to_device_f32(inputs, device)  # Keras autocast (float64 -> float32)
    return X[:, :nd], X[:, nd:]


# ------------------------------------------------------------------ workspaces
def scratch(owner, name, nbytes):
    """The grow-only uint8 device buffer cached in owner.__dict__[name]: the
    cached one while it holds nbytes, a new one of nbytes otherwise."""
    ws = owner.__dict__.get(name)
    if ws is None or ws.numel() < nbytes:
        ws = owner.__dict__[name] = torch.empty(nbytes, dtype=torch.uint8, device=owner._dev)
    return ws


def gemm_need(shapes):
    """The largest rs_gemm_workspace_size over (M, N, K) triples."""
    size = _lib.lib().rs_gemm_workspace_size
    return max(size(m, n, k) for m, n, k in shapes)


def gemm_ws(owner, nbytes):
    """rs_gemm's (workspace, bytes) argument pair from the owner's grow-only
    ``_gemm_wsbuf``.  rs_gemm makes a single pass over K where the buffer is
    smaller than its split needs, and the buffer never shrinks — so a step asks
    for exactly what it always asked for."""
    ws = scratch(owner, "_gemm_wsbuf", max(nbytes, 1))
    return ptr(ws), ws.numel()


# ------------------------------------------------------------- embedding rows
def embedding_sgd(layer, ids, grad_ptr, ldg, lr, st, owner):
    """Row-sparse SGD of the rows of EmbedLayer ``layer`` that ids [rows, F]
    looked up, from dL/d(rows) at address grad_ptr with row stride ldg
    (rs_embedding_sgd: duplicates summed in lookup order).  The workspace is
    the owner's ``_emb_ws``."""
    rows = ids.shape[0]
    ws = scratch(owner, "_emb_ws", _lib.lib().rs_embedding_sgd_workspace_size(rows * layer.n_fields))
    call("rs_embedding_sgd", ptr(layer.table), layer.total_rows, layer.k, ptr(ids), _lib.id_kind(ids), ids.stride(0),
         ptr(layer.field_offsets), ptr(layer.field_vocab), layer.n_fields, rows, grad_ptr, ldg, float(lr), ptr(ws),
         None, st)


def embedding_sgd_strided(rows_ptr, n_rows, k, ids, offsets, vocab, grad, lr, st, owner, name="_emb_ws"):
    """rs_embedding_sgd_strided: every looked-up row (k wide, n_rows of them
    from address rows_ptr on; field c's code i is row offsets[c] + i) gets its
    SAMPLE's gradient row grad[b] (k wide), duplicates summed in lookup order.
    The workspace is owner.__dict__[name]."""
    B, F = ids.shape
    ws = scratch(owner, name, _lib.lib().rs_embedding_sgd_workspace_size(B * F))
    call("rs_embedding_sgd_strided", rows_ptr, n_rows, k, ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(offsets),
         ptr(vocab), F, B, ptr(grad), k, 0, float(lr), ptr(ws), None, st)


# ------------------------------------------------------------------- BCE head
def bce_head(z0, z1, labels, c0, c1, return_loss, st):
    """rs_head_grad on z = c0 z0 + c1 z1: (dL/dz0, dL/dz1, per-sample losses
    or None), each [B]."""
    B = labels.shape[0]
    g0, g1 = (torch.empty(B, dtype=torch.float32, device=labels.device) for _ in range(2))
    loss = torch.empty(B, dtype=torch.float32, device=labels.device) if return_loss else None
    call("rs_head_grad", ptr(z0), ptr(z1), ptr(labels), B, c0, c1, ptr(g0), ptr(g1), ptr(loss), st)
    return g0, g1, loss


def bce_head_logit(logit, labels, return_loss, st):
    """The head of a model with one logit: (dL/dlogit [B], losses or None)."""
    g, _, loss = bce_head(logit, logit, labels, 1.0, 0.0, return_loss, st)
    return g, loss


# ------------------------------------------------------------ Dense backward
def dense_backward(kernel, a_in, dz, gw, emp, st, out=None, mask=(None, 0), d_in=True, split_sum=False):
    """One Dense layer's backward from dz = dL/d(pre-activation) [m, N]:
    dW = a_in^T dz (split-K rs_gemm) and db = the column sums of dz, written
    into ``out`` = (dW, db) where given; with ``d_in`` also dL/d(a_in) =
    dz W^T, times [mask > 0] where ``mask`` = (address, row stride) names the
    ReLU output below (rs_gemm's mask epilogue).  ``split_sum``: the column
    sums by rs_col_sum_split on the gemm workspace instead of rs_col_sum.
    Returns (dW, db, dL/d(a_in) or None)."""
    K_in, N_out = kernel.shape
    m = dz.shape[0]
    dW, db = out if out is not None else (emp(K_in, N_out), emp(N_out))
    call("rs_gemm", 1, 0, K_in, N_out, m, 1.0, ptr(a_in), a_in.stride(0), ptr(dz), dz.stride(0), 0.0, ptr(dW), N_out,
         None, 0, *gw, st)
    if split_sum:
        call("rs_col_sum_split", ptr(dz), dz.stride(0), m, N_out, ptr(db), *gw, st)
    else:
        call("rs_col_sum", ptr(dz), dz.stride(0), m, N_out, ptr(db), st)
    if not d_in:
        return dW, db, None
    below = emp(m, K_in)
    call("rs_gemm", 0, 1, m, K_in, N_out, 1.0, ptr(dz), dz.stride(0), ptr(kernel), N_out, 0.0, ptr(below), K_in, *mask,
         *gw, st)
    return dW, db, below


# ------------------------------------------------------------------- Dropout
class _Dropout:
    """DNNLayer's Dropout(rate) in training steps (layer/interaction.py:35,44;
    active under compile_fit's model.fit, utils/compile_fit.py:14): inverted
    dropout with counter-based masks (rs_dropout_at: Philox4x32-10, key =
    seed, one counter per 4 elements).  Every draw of a step takes the next
    offset range relative to a counter in DEVICE memory, the backward
    regenerates a draw's mask from the same (seed, counter + rel) instead of
    storing it, and end_step() advances the counter on the stream by the
    step's total — so a captured hipGraph of a training step draws fresh
    masks on every replay.  TF's own draws cannot be reproduced;
    oracle.dropout_multiplier restates this generator."""

    def __init__(self, seed, device=None):
        self.seed = int(seed) & (2 ** 64 - 1)
        self.base = torch.zeros(1, dtype=torch.int64, device=device if device is not None else "cuda")
        self.rel = 0

    @property
    def offset(self):
        """The absolute offset the next draw takes (reads the device counter)."""
        return int(self.base.item()) + self.rel

    def draw(self, t, rate, st):
        """Apply a fresh mask to t [rows, cols] in place; returns its offset
        relative to the step's counter."""
        off = self.rel
        self.redraw(t, rate, off, st)
        self.rel += (t.shape[0] * t.shape[1] + 3) // 4 * 4
        return off

    def take(self, n):
        """Reserve the next n elements' range (a draw made elsewhere)."""
        off = self.rel
        self.rel += (int(n) + 3) // 4 * 4
        return off

    def redraw(self, t, rate, rel, st):
        call("rs_dropout_at", ptr(t), t.stride(0), t.shape[0], t.shape[1], float(rate), self.seed, ptr(self.base),
             int(rel), st)

    def end_step(self, st):
        """Advance the device counter past this step's draws."""
        if self.rel:
            call("rs_dropout_advance", ptr(self.base), int(self.rel), st)
            self.rel = 0


def _dropout_rate(dnn, dropout):
    """The rate a training step applies: DNNLayer's own (Keras' fit runs the
    Dropout layers in training mode) unless dropout=False turns it off, or a
    float overrides it."""
    if dropout is False:
        return 0.0
    if dropout is None or dropout is True:
        return float(getattr(dnn, "dropout", 0) or 0)
    return float(dropout)


def _dropout_rng(model):
    rng = model.__dict__.get("_drop_rng")
    if rng is None:
        rng = model.__dict__["_drop_rng"] = _Dropout(_subseed(model._gen) * 2654435761 + 97, model._dev)
    return rng


# ----------------------------------------------------------------- DNNLayer
def _check_train_tower(name, dnn):
    if any(l.activation not in (None, "linear", "relu") for l in dnn.hidden_layer):
        raise NotImplementedError(f"{name}.train_step: 'relu' or linear hidden layers only")


def _dnn_train_forward(model, dnn, x, rate, st, drop=None):
    """Hidden layers of DNNLayer in training: Dense + activation, then the
    dropout draw (rate > 0) from the model's generator.  ``drop`` = (_Dropout,
    rate, offsets) taken earlier (ShardedDeepFM._draws): the masks are applied
    at those offsets instead.  Returns (acts, drop) for _dnn_backward."""
    acts, taken = [x], drop is not None
    if not taken and rate > 0:
        drop = (_dropout_rng(model), rate, [])
    for i, layer in enumerate(dnn.hidden_layer):
        a = layer(acts[-1])
        if taken:
            drop[0].redraw(a, drop[1], drop[2][i], st)
        elif drop is not None:
            drop[2].append(drop[0].draw(a, drop[1], st))
        acts.append(a)
    return acts, drop


def _dnn_backward(layers, acts, delta, gw, emp, st, outs=None, drop=None):
    """Backward through Dense layers (relu or linear hidden activations):
    delta = dL/d(pre-activation) of the top layer; returns the (layer, dW, db)
    gradients and dL/d(acts[0]).  dW = a_in^T delta (split-K rs_gemm), db =
    column sums, delta_below = (delta W^T) [a_in > 0] (mask epilogue).
    outs: optional [(dW, db)] per layer to write into (contiguous views).
    drop: (_Dropout, rate, offsets) of the forward's hidden-layer dropout
    draws — delta_below is multiplied by the same keep / (1 - rate)."""
    grads = []
    for li in reversed(range(len(layers))):
        L, a_in = layers[li], acts[li]
        relu_below = li > 0 and layers[li - 1].activation == "relu"
        dW, db, prev = dense_backward(L.kernel, a_in, delta, gw, emp, st, out=outs[li] if outs is not None else None,
                                      mask=(ptr(a_in) if relu_below else None, a_in.stride(0)))
        grads.append((L, dW, db))
        if drop is not None and 0 < li <= len(drop[2]):  # acts[li] is dropped hidden output li-1
            rng, rate, offs = drop
            rng.redraw(prev, rate, offs[li - 1], st)
        delta = prev
    if drop is not None:
        drop[0].end_step(st)
    return grads, delta


def _dnn_updates(grads, l2=0.0):
    """[(w, grad, n, l2)] of Dense layers' kernels and biases (for
    _lib.sgd_update_multi)."""
    out = []
    for L, dW, db in grads:
        out.extend([(L.kernel, dW, dW.numel(), l2), (L.bias, db, db.numel(), l2)])
    return out


def _dnn_apply(grads, lr, st, l2=0.0):
    _lib.sgd_update_multi(_dnn_updates(grads, l2), lr, st)


# ------------------------------------------------------- BatchNormalization
def bn_train_fwd(bn, x, st):
    """BatchNormalization under fit on x [B, D]: the batch's own mean and
    biased variance (kept for the backward), the moving averages moved
    (momentum 0.99).  Returns ((mean, var), y)."""
    B, D = x.shape
    mean, var = (torch.empty(D, dtype=torch.float32, device=x.device) for _ in range(2))
    y = torch.empty(B, D, dtype=torch.float32, device=x.device)
    call("rs_bn_train_fwd", ptr(x), x.stride(0), B, D, ptr(bn.gamma), ptr(bn.beta), bn.epsilon, 0.99,
         ptr(bn.moving_mean), ptr(bn.moving_variance), ptr(mean), ptr(var), ptr(y), D, st)
    return (mean, var), y


def bn_train_bwd(bn, x, saved, dy, st):
    """(dL/dx [B, D], dgamma, dbeta) of bn_train_fwd from dy = dL/dy."""
    B, D = x.shape
    dx = torch.empty(B, D, dtype=torch.float32, device=x.device)
    dgamma, dbeta = (torch.empty(D, dtype=torch.float32, device=x.device) for _ in range(2))
    call("rs_bn_train_bwd", ptr(x), x.stride(0), B, D, ptr(saved[0]), ptr(saved[1]), ptr(bn.gamma), bn.epsilon,
         ptr(dy), dy.stride(0), ptr(dx), D, ptr(dgamma), ptr(dbeta), st)
    return dx, dgamma, dbeta


# ------------------------------------- Dense + activation blocks of DIEN's step
def dense_train_need(shapes):
    """Workspace bytes for DenseTrain over (K_in, N_out, rows) layer shapes:
    the split-K gemms in both orientations, the column sums, Dice."""
    lb = _lib.lib()
    need = [gemm_need(list(shapes) + [(m, kin, n) for kin, n, m in shapes])]
    need += [lb.rs_col_sum_workspace_size(m, n) for _, n, m in shapes]
    need += [lb.rs_dice_train_workspace_size(m, n) for _, n, m in shapes]
    return max(need)


class DenseTrain:
    """Dense layers with 'relu' / 'sigmoid' / 'dice' activations inside a
    training step (DNN's layers, LocalActivationUnit's, the auxiliary net's):
    rs_dense_fwd without activation, rs_dice_train_fwd/_bwd in training mode
    (the batch's statistics, moving averages moved with momentum 0.99),
    dense_backward.  relu, sigmoid and their backward (dy [y > 0], dy y (1 -
    y)) are torch elementwise ops.  ``updates`` collects (weight, gradient, l2)."""

    def __init__(self, gw, st, device):
        self.gw, self.st, self.updates = gw, st, []
        self.emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)

    def dense(self, xin, layer, m):
        n = layer.kernel.shape[1]
        z = self.emp(m, n)
        call("rs_dense_fwd", ptr(xin), xin.stride(0), ptr(layer.kernel), ptr(layer.bias), None, _lib.ACT[None], ptr(z),
             n, m, layer.kernel.shape[0], n, self.st)
        return z

    def act_fwd(self, layer, z, m):
        """(what the backward needs, the activation's output)."""
        if layer.activation == "dice":
            d, n = layer.dice, z.shape[1]
            mu, vr, y = self.emp(n), self.emp(n), self.emp(m, n)
            call("rs_dice_train_fwd", ptr(z), m, n, ptr(d.alphas), d.epsilon, 0.99, ptr(d.moving_mean),
                 ptr(d.moving_variance), ptr(mu), ptr(vr), ptr(y), *self.gw, self.st)
            return (mu, vr), y
        return None, (torch.relu(z) if layer.activation == "relu" else torch.sigmoid(z))

    def act_bwd(self, layer, z, y, saved, dy, m):
        if layer.activation == "dice":
            d, n = layer.dice, z.shape[1]
            dz, dal = self.emp(m, n), self.emp(n)
            call("rs_dice_train_bwd", ptr(z), m, n, ptr(d.alphas), ptr(saved[0]), ptr(saved[1]), d.epsilon, ptr(dy),
                 ptr(dz), ptr(dal), *self.gw, self.st)
            self.updates.append((d.alphas, dal, 0.0))
            return dz
        return dy * (y > 0) if layer.activation == "relu" else dy * y * (1 - y)

    def dense_bwd(self, layer, a_in, dz, l2=0.0):
        """dL/d(a_in); the kernel's and bias's gradients go to ``updates``."""
        dW, db, below = dense_backward(layer.kernel, a_in, dz.contiguous(), self.gw, self.emp, self.st, split_sum=True)
        self.updates.extend([(layer.kernel, dW, l2), (layer.bias, db, 0.0)])
        return below


# ------------------------------------------- DIEN's recurrences (dien_train.hip)
def _rnn_saved(size_fn, what, T, din, units, B, device):
    n = getattr(_lib.lib(), size_fn)(T, din, units, B)
    if n < 0:
        _lib.check(-1, what)
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)


def _rnn_ws(owner, M, din, U):
    """(workspace, bytes) for the weight-gradient gemms and column sums of a
    recurrence's backward at M = B T rows (the dx gemm takes none)."""
    need = gemm_need([(din, 3 * U, M), (U, 3 * U, M)])
    return gemm_ws(owner, max(need, _lib.lib().rs_col_sum_workspace_size(M, 3 * U)))


def gru_train_forward(gru, x, st):
    """GRU forward of a training step (rs_gru_train_fwd): (seq [B, T, units],
    saved) — seq is bit-identical to ``gru(x)``'s, saved is what gru_backward
    reads."""
    x = gru._input(x)
    B, T, din = x.shape
    if T < 1:
        raise ValueError("GRU: an empty sequence")
    saved = _rnn_saved("rs_gru_saved_size", "rs_gru_saved_size", T, din, gru.units, B, x.device)
    seq = torch.empty(B, T, gru.units, dtype=torch.float32, device=x.device)
    call("rs_gru_train_fwd", ptr(x), x.stride(0), x.stride(1), T, din, gru.units, ptr(gru.prepared()), ptr(seq), None,
         0, ptr(saved), B, st)
    return seq, saved


def gru_backward(gru, x, saved, dseq, dlast, st, d_in=True):
    """Backward of gru_train_forward from dseq = dL/dseq [B, T, units] and / or
    dlast = dL/d(last state) [B, units]: one rs_gru_bwd launch for the chain,
    then rs_gemm / rs_col_sum_split at M = B T.  Returns (dx [B, T, din] or
    None, dkernel, drecurrent_kernel, dbias [2, 3 units])."""
    B, T, din = x.shape
    U, M = gru.units, B * T
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
    x = x.contiguous()
    dseq = None if dseq is None else dseq.reshape(B, T, U).contiguous()
    dlast = None if dlast is None else dlast.reshape(B, U).contiguous()
    gx, gh, hp = emp(M, 3 * U), emp(M, 3 * U), emp(M, U)
    call("rs_gru_bwd", ptr(saved), ptr(dseq), ptr(dlast), U, T, U, ptr(gru.prepared_bwd()), ptr(gx), ptr(gh), ptr(hp),
         B, st)
    gw = _rnn_ws(gru, M, din, U)
    dW, dU, db = emp(din, 3 * U), emp(U, 3 * U), emp(2, 3 * U)
    call("rs_gemm", 1, 0, din, 3 * U, M, 1.0, ptr(x), din, ptr(gx), 3 * U, 0.0, ptr(dW), 3 * U, None, 0, *gw, st)
    call("rs_gemm", 1, 0, U, 3 * U, M, 1.0, ptr(hp), U, ptr(gh), 3 * U, 0.0, ptr(dU), 3 * U, None, 0, *gw, st)
    call("rs_col_sum_split", ptr(gx), 3 * U, M, 3 * U, ptr(db[0]), *gw, st)
    call("rs_col_sum_split", ptr(gh), 3 * U, M, 3 * U, ptr(db[1]), *gw, st)
    dx = None
    if d_in:
        dx = emp(B, T, din)
        # no workspace: always one pass over K = 3 U, so a sample's dx never depends on the batch
        call("rs_gemm", 0, 1, M, din, 3 * U, 1.0, ptr(gx), 3 * U, ptr(gru.kernel), 3 * U, 0.0, ptr(dx), din, None, 0,
             None, 0, st)
    return dx, dW, dU, db


def augru_train_forward(augru, x, scores, st):
    """AUGRU forward of a training step (rs_augru_train_fwd): (last [B, units],
    saved), last bit-identical to ``augru(x, scores)``'s."""
    c = augru.cell
    x = c._input(x)
    B, T, din = x.shape
    a = scores.reshape(B, T).to(torch.float32).contiguous()
    saved = _rnn_saved("rs_augru_saved_size", "rs_augru_saved_size", T, din, c.units, B, x.device)
    last = torch.empty(B, c.units, dtype=torch.float32, device=x.device)
    call("rs_augru_train_fwd", ptr(x), x.stride(0), x.stride(1), ptr(a), a.stride(0), T, din, c.units,
         _layers._DIEN_UPDATES[augru.augru_update], ptr(c.prepared()), ptr(last), last.stride(0), ptr(saved), B, st)
    return last, saved


def augru_backward(augru, x, scores, lengths, weight_norm, saved, dlast, st, want_da=False):
    """Backward of augru_train_forward from dlast = dL/d(last state): one
    rs_augru_bwd launch (the chain, da and the masked softmax's backward),
    then rs_gemm at M = B T.  ``scores`` are the forward's (masked, normalised
    when weight_norm), ``lengths`` [B] their mask.  Returns (dx [B, T, din],
    ds [B, T] = dL/d(unmasked scores), da or None, dkernel,
    drecurrent_kernel)."""
    c = augru.cell
    B, T, din = x.shape
    U, M = c.units, B * T
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
    x = x.contiguous()
    a = scores.reshape(B, T).to(torch.float32).contiguous()
    dlast = dlast.reshape(B, U).contiguous()
    gx, hrh, ds = emp(M, 3 * U), emp(M, 2 * U), emp(B, T)
    da = emp(B, T) if want_da else None
    call("rs_augru_bwd", ptr(saved), ptr(a), T, ptr(lengths), _lib.id_kind(lengths), 1 if weight_norm else 0,
         ptr(dlast), U, T, U, _layers._DIEN_UPDATES[augru.augru_update], ptr(c.prepared_bwd()), ptr(gx), ptr(hrh),
         ptr(ds), ptr(da), B, st)
    gw = _rnn_ws(c, M, din, U)
    dW, dU, dx = emp(din, 3 * U), emp(U, 3 * U), emp(B, T, din)
    call("rs_gemm", 1, 0, din, 3 * U, M, 1.0, ptr(x), din, ptr(gx), 3 * U, 0.0, ptr(dW), 3 * U, None, 0, *gw, st)
    # dU_zr = h_prev^T [da_z, da_r], dU_h = (r h_prev)^T dc: column blocks of hrh, gx and dU
    call("rs_gemm", 1, 0, U, 2 * U, M, 1.0, ptr(hrh), 2 * U, ptr(gx), 3 * U, 0.0, ptr(dU), 3 * U, None, 0, *gw, st)
    call("rs_gemm", 1, 0, U, U, M, 1.0, hrh.data_ptr() + 4 * U, 2 * U, gx.data_ptr() + 8 * U, 3 * U, 0.0,
         dU.data_ptr() + 8 * U, 3 * U, None, 0, *gw, st)
    # no workspace: always one pass over K = 3 U, so a sample's dx never depends on the batch
    call("rs_gemm", 0, 1, M, din, 3 * U, 1.0, ptr(gx), 3 * U, ptr(c.kernel), 3 * U, 0.0, ptr(dx), din, None, 0, None,
         0, st)
    return dx, ds, da, dW, dU


# ----------------------------------------------------- MMOE's step (mmoe_train.hip)
MMOE_L2 = 1e-4  # l2(1e-4) on every mmoe_layer weight (layer/interaction.py:441-477); the towers declare none


def mmoe_labels(labels, T, B, nout, device):
    """The labels [T, B, Nout] (float32, contiguous) from a list of T arrays
    [B] / [B, Nout] or one [T, B(, Nout)] tensor."""
    if isinstance(labels, (list, tuple)):
        if len(labels) != T:
            raise ValueError(f"MMOE: {T} tasks, got {len(labels)} label arrays")
        y = torch.stack([_layers._to_device_f32(l, device).reshape(B, nout) for l in labels])
    else:
        y = _layers._to_device_f32(labels, device).reshape(T, B, nout)
    return y.contiguous()


def mmoe_head(z, y, loss_weights, st):
    """rs_mmoe_head_grad on the towers' logits z [T, B, Nout] and labels y of
    the same shape: (G [B, T Nout] = dL/dz with the weights and the two means
    applied, the unweighted per-sample losses [T, B])."""
    T, B, nout = z.shape
    if loss_weights is not None and len(loss_weights) != T:
        raise ValueError(f"MMOE: {T} tasks, got {len(loss_weights)} loss_weights")
    lw = None if loss_weights is None else (_lib.C.c_float * T)(*[float(w) for w in loss_weights])
    G = torch.empty(B, T * nout, dtype=torch.float32, device=z.device)
    loss = torch.empty(T, B, dtype=torch.float32, device=z.device)
    call("rs_mmoe_head_grad", ptr(z), z.stride(0), z.stride(1), ptr(y), y.stride(0), y.stride(1), lw, nout, T, B,
         ptr(G), G.stride(0), ptr(loss), st)
    return G, loss


def mmoe_layer_grads(layer, x, dz1, gw, emp, st, d_in=False):
    """The mmoe_layer's weight gradients from dz1 [B, (H + T) E] (the
    forward's stage-1 column order): one x^T dz1 contraction and column sum
    for the experts and one per gate (dense_backward on column views), each
    into a contiguous buffer of the parameter's own shape.  Returns ({name:
    grad}, dL/dx or None — the T + 1 blocks' dz W^T summed in block order)."""
    d, H, E, T = layer.input_dim, layer.hidden_units, layer.num_experts, layer.num_tasks
    HE = H * E
    out, dx = {}, None
    dW, db, below = dense_backward(layer.expert_matrix.view(d, HE), x, dz1[:, :HE], gw, emp, st, d_in=d_in)
    out["expert_matrix"] = dW.view(d, H, E)
    if layer.use_expert_bias:
        out["expert_bias"] = db.view(H, E)
    dx = below
    for t, gm in enumerate(layer.gate_matrix):
        dW, db, below = dense_backward(gm, x, dz1[:, HE + t * E:HE + (t + 1) * E], gw, emp, st, d_in=d_in)
        out[f"gate_matrix{t}"] = dW
        if layer.use_gate_bias:
            out[f"gate_bias{t}"] = db
        if d_in:
            dx = dx + below
    return out, dx


# ------------------------------------------------ FM part of a DeepFM step
def fm_xv(x, v, gw, st, out=None):
    """s = x v [B, kfm] (rs_gemm), what rs_fm_x_grad / rs_fm_param_grads read."""
    (B, d), kfm = x.shape, v.shape[1]
    s = out if out is not None else torch.empty(B, kfm, dtype=torch.float32, device=x.device)
    call("rs_gemm", 0, 0, B, kfm, d, 1.0, ptr(x), d, ptr(v), kfm, 0.0, ptr(s), kfm, None, 0, *gw, st)
    return s


def fm_backward(x, s, w1, v, g_fm, dx, st, outs=None):
    """FMLayer's backward from g_fm = dL/d(FM logit) [B]: its dL/dx ADDED to
    dx [B, d] (rs_fm_x_grad), and (dw1 [d], dv [d, kfm], dw0 [1])
    (rs_fm_param_grads) written into ``outs`` where given."""
    (B, d), kfm = x.shape, v.shape[1]
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
    dw1, dv, dw0 = outs if outs is not None else (emp(d), emp(d, kfm), emp(1))
    call("rs_fm_x_grad", ptr(x), d, ptr(s), ptr(w1), ptr(v), B, d, kfm, ptr(g_fm), ptr(dx), d, st)
    call("rs_fm_param_grads", ptr(x), d, ptr(s), ptr(v), B, d, kfm, ptr(g_fm), ptr(dw1), ptr(dv), ptr(dw0), st)
    return dw1, dv, dw0
