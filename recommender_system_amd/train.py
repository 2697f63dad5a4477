"""compile_fit on the MI355X path.

Mirror of utils/compile_fit.py:9-15: ``tf.data.Dataset.from_tensor_slices((X,
y)).batch(batch_size)`` (no shuffle: the dataset order), SGD(sgd),
binary cross-entropy, ``epochs`` passes.  The data is the compact form of the
reference's X (dataset.criteo_compact / an RSCB file): dense [N, nd], label
codes [N, F], labels [N], per-field vocab.  Each batch is one
``model.train_step``: ``FM`` (rs_fm_train_step; the one-hot X of
model/fm.py), ``DeepFM`` (model/deepFM.py), ``DCN`` (model/dcn.py), ``NFM``
(model/nfm.py), ``FFM`` (model/ffm.py), ``AFM`` (model/afm.py) or
``DeepCrossing`` (model/deepCrossing.py) on dense + label-encoded X, ``WideDeep``
(model/wideDeep.py) on the compact form of its packed row
(``WideDeep.train_step_onehot``), and ``DIN`` (model/din.py:106) on the reference's input dict (pass it as
``dense``, ``ids=None``; every value is sliced along its first axis).

``predict`` and ``evaluate`` close the reference's workflow with the same data
conventions: the scripts' ``pre = model(X_test)`` followed by
``accuracy_score(y_test, [1 if x > 0.5 else 0 for x in pre])`` (model/fm.py:38,
deepFM.py:51, dcn.py:50, din.py:116, pnn.py:89, fnn.py:70-71) and the
``metrics=['accuracy']`` of utils/compile_fit.py:13, with the metrics computed
on the device (metrics.binary_metrics).
"""
from __future__ import annotations

import numpy as np
import torch

from . import metrics
from .layers import sigmoid_combine
from .models import AFM, DCN, DIEN, DIN, FFM, FM, FNN, MMOE, NFM, PNN, DeepCrossing, DeepFM, WideDeep


def compile_fit(model, dense, ids, labels, field_vocab=None, batch_size=32, epochs=10, sgd=0.01, device=None):
    """Train ``model`` (models.FM / DeepFM / DCN / NFM / FFM / AFM /
    DeepCrossing / WideDeep / DIN) in place;
    returns the per-epoch mean cross-entropy (before each step, without the l2
    terms).  ``field_vocab`` (feat_onehot_dim per field) is needed for FM's
    one-hot layout; the others read it from their layers (WideDeep's one-hot
    widths are ``field_vocab``, or its embedding layer's vocab when that is
    not given; the offsets are their cumulative sum).  PNN trains with its
    own loop in the reference (model/pnn.py:74-81): PNN.train_step."""
    if not isinstance(model, (FM, DeepFM, DCN, NFM, FFM, AFM, DeepCrossing, WideDeep, DIN, DIEN)):
        raise NotImplementedError("compile_fit: FM, DeepFM, DCN, NFM, FFM, AFM, DeepCrossing, WideDeep, DIN and DIEN "
                                  "(PNN: PNN.train_step)")
    dev = torch.device(device) if device is not None else model._dev
    labels = torch.as_tensor(np.asarray(labels, np.float32), device=dev)
    N = labels.shape[0]
    history = []
    if isinstance(model, (DIN, DIEN)):
        if ids is not None:
            raise ValueError(f"compile_fit({type(model).__name__}): pass the input dict as `dense` and ids=None")
        data = {key: torch.as_tensor(np.asarray(val), device=dev) for key, val in dense.items()}
        for _ in range(epochs):
            losses = [model.train_step({key: val[r0:r0 + batch_size] for key, val in data.items()},
                                       labels[r0:r0 + batch_size], lr=sgd, return_loss=True, check_ids=False)
                      for r0 in range(0, N, batch_size)]
            history.append(float(torch.cat(losses).mean().item()))
        return history
    dense = torch.as_tensor(np.asarray(dense, np.float32), device=dev)
    ids = torch.as_tensor(np.asarray(ids), device=dev)
    if isinstance(model, FM):
        if field_vocab is None:
            raise ValueError("compile_fit(FM): field_vocab is required (the one-hot layout)")
        vocab = np.asarray(field_vocab, np.int64)
        offs = np.concatenate([[0], np.cumsum(vocab)[:-1]])
        step = lambda d, i, t: model.train_step(d, i, t, offs, vocab, lr=sgd, return_loss=True, check_ids=False)
    elif isinstance(model, FFM):
        step = lambda d, i, t: model.train_step((d, i), t, lr=sgd, return_loss=True)
    elif isinstance(model, WideDeep):
        widths = np.asarray(field_vocab if field_vocab is not None else model.embed_layer.vocab_sizes, np.int64)
        woffs = np.concatenate([[0], np.cumsum(widths)[:-1]])
        step = lambda d, i, t: model.train_step_onehot(d, i, woffs, widths, t, lr=sgd, return_loss=True,
                                                       check_ids=False)
    else:
        step = lambda d, i, t: model.train_step((d, i), t, lr=sgd, return_loss=True, check_ids=False)
    for _ in range(epochs):
        losses = [step(dense[r0:r0 + batch_size], ids[r0:r0 + batch_size], labels[r0:r0 + batch_size])
                  for r0 in range(0, N, batch_size)]
        history.append(float(torch.cat(losses).mean().item()))
    return history


# Models whose forward ORs every id check into a device flag that lives as
# long as the model (layers._ErrFlag on the model or its embedding layer): a
# bad id seen with check_ids=False is still raised by the next checked call.
_DEFERRED_CHECK = (DeepFM, DCN, PNN, NFM, AFM, DeepCrossing, DIN)
_PREDICT_MODELS = _DEFERRED_CHECK + (FM, FFM, WideDeep, FNN, DIEN, MMOE)


def _on_device(x, dtype, dev):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype) if dtype is not None else x.to(dev)
    return torch.as_tensor(np.asarray(x, dtype) if dtype is not None else np.asarray(x), device=dev)


def predict(model, dense, ids, field_vocab=None, batch_size=4096, device=None):
    """``model``'s inference output on every sample, batch by batch, in one
    preallocated float32 device buffer: [N] probabilities (``model.forward``:
    Dropout off, BatchNormalization in inference), or [T, N] for MMOE — the
    sigmoid of each tower's logit, as ``MMOE.train_step`` reads them.

    The data conventions are compile_fit's: dense [N, nd] and label codes
    [N, F] (arrays or tensors); DIN and DIEN take the input dict as ``dense``
    with ``ids=None``; MMOE takes its input matrix as ``dense`` with
    ``ids=None``; FM and FNN need ``field_vocab`` and run ``forward_onehot``,
    as WideDeep does (its widths default to the embedding layer's vocab).

    For DeepFM, DCN, PNN, NFM, AFM, DeepCrossing and DIN the ids are checked
    once, on the last batch: the kernels OR their error bits into a flag that
    persists across calls, so that one check covers the pass (one host
    synchronisation instead of one per batch) and a bad id anywhere raises
    ``BadIdError`` at the end.  FM, WideDeep, FNN and DIEN make their flag per
    call and are checked every batch; FFM reads an out-of-range id as
    tf.one_hot's zero row and raises nothing.  PNN's output is its DNN's,
    without a sigmoid (model/pnn.py:53): the scripts threshold it at 0.5 all
    the same (model/pnn.py:88), and so do the metrics."""
    if not isinstance(model, _PREDICT_MODELS):
        raise NotImplementedError("predict: FM, DeepFM, DCN, PNN, NFM, AFM, FFM, DeepCrossing, WideDeep, FNN, DIN, "
                                  "DIEN and MMOE")
    dev = torch.device(device) if device is not None else model._dev
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("predict: batch_size must be >= 1")
    deferred = isinstance(model, _DEFERRED_CHECK)
    if isinstance(model, (DIN, DIEN)):
        if ids is not None:
            raise ValueError(f"predict({type(model).__name__}): pass the input dict as `dense` and ids=None")
        data = {key: _on_device(val, None, dev) for key, val in dense.items()}
        N = next(iter(data.values())).shape[0]
        run = lambda r0, r1, chk: model.forward({key: val[r0:r1] for key, val in data.items()}, check_ids=chk)
    elif isinstance(model, MMOE):
        if ids is not None:
            raise ValueError("predict(MMOE): pass the input matrix as `dense` and ids=None")
        x = _on_device(dense, np.float32, dev)
        N = x.shape[0]
        run = lambda r0, r1, chk: model.forward(x[r0:r1])
    else:
        dense = _on_device(dense, np.float32, dev)
        ids = _on_device(ids, None, dev)
        N = ids.shape[0]
        if isinstance(model, (FM, FNN, WideDeep)):
            if field_vocab is None and not isinstance(model, WideDeep):
                raise ValueError(f"predict({type(model).__name__}): field_vocab is required (the one-hot layout)")
            vocab = np.asarray(field_vocab if field_vocab is not None else model.embed_layer.vocab_sizes, np.int64)
            offs = np.concatenate([[0], np.cumsum(vocab)[:-1]])
            run = lambda r0, r1, chk: model.forward_onehot(dense[r0:r1], ids[r0:r1], offs, vocab, check_ids=chk)
        elif isinstance(model, FFM):
            run = lambda r0, r1, chk: model.forward((dense[r0:r1], ids[r0:r1]))
        else:
            run = lambda r0, r1, chk: model.forward((dense[r0:r1], ids[r0:r1]), check_ids=chk)
    T = model.mmoe_layer.num_tasks if isinstance(model, MMOE) else None
    out = torch.empty((N,) if T is None else (T, N), dtype=torch.float32, device=dev)
    for r0 in range(0, N, batch_size):
        r1 = min(r0 + batch_size, N)
        y = run(r0, r1, (not deferred) or r1 == N)
        if T is None:
            if y.numel() != r1 - r0:
                raise ValueError(f"predict: the model returns {tuple(y.shape)} for {r1 - r0} samples "
                                 "(one output per sample is needed)")
            out[r0:r1].copy_(y.reshape(-1))
        else:
            for t in range(T):
                if y[t].numel() != r1 - r0:
                    raise ValueError("predict(MMOE): output_dim must be 1")
                sigmoid_combine(y[t].reshape(-1).contiguous(), out=out[t, r0:r1])
    return out


def evaluate(model, dense, ids, labels, field_vocab=None, batch_size=4096, group_ids=None, device=None,
             n_groups=None):
    """``predict`` followed by ``metrics.binary_metrics`` on the whole buffer:
    ``{"loss", "accuracy", "auc", "n", "n_pos", ...}`` (with ``group_ids``
    [N], dense ids in [0, n_groups), also ``"gauc"``, ``"groups_used"`` and
    ``"impressions_used"``).  MMOE: ``labels`` is a list of T label vectors
    (or [T, N]) and the result a list of T dicts."""
    pred = predict(model, dense, ids, field_vocab, batch_size, device)
    dev = pred.device
    groups = None if group_ids is None else _on_device(group_ids, None, dev)
    if groups is not None and groups.dtype not in (torch.int32, torch.int64):
        groups = groups.to(torch.int64)
    if isinstance(model, MMOE):
        ys = [_on_device(y, np.float32, dev).reshape(-1) for y in labels]
        if len(ys) != pred.shape[0]:
            raise ValueError(f"evaluate(MMOE): {pred.shape[0]} tasks but {len(ys)} label vectors")
        return [metrics.binary_metrics(pred[t], ys[t], groups, n_groups) for t in range(pred.shape[0])]
    return metrics.binary_metrics(pred, _on_device(labels, np.float32, dev).reshape(-1), groups, n_groups)
