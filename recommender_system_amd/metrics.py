"""Evaluation metrics on the device: what the reference's scripts compute on
the host after training — ``accuracy_score(y_test, [1 if x > 0.5 else 0 ...])``
(model/fm.py:38, deepFM.py:51, dcn.py:50, din.py:116, pnn.py:89, fnn.py:70-71;
``metrics=['accuracy']`` in utils/compile_fit.py:13) — plus Keras' log-loss and
the ROC AUC two of those scripts name (deepFM.py:51, din.py:116), and the
impression-weighted group AUC (GAUC) of the DIN paper.

  binary_metrics(pred, labels, group_ids=None, n_groups=None) -> dict
  roc_auc(scores, labels) -> float
  auc_stats(scores, labels, group_ids=None, n_groups=None) -> dict
  group_auc(scores, labels, group_ids, n_groups=None) -> float
  BinaryMetrics(device): update(pred, labels) per batch, result() at the end

rs_binary_metrics and rs_auc (csrc/metrics.hip) do the work; the AUC is exact
(``sklearn.metrics.roc_auc_score`` to rounding: the numerator is an integer).
Device tensors only: a CPU tensor raises ``RSError``.  Every function makes
one host synchronisation, to read the result; a label that is neither 0 nor 1
or a NaN prediction raises ``ValueError`` there.  A single-class input gives
``auc = nan`` (no exception).

Group ids are dense: ``0 <= id < n_groups`` (int32 or int64).  Mapping
arbitrary ids (user ids, session hashes) to that range is the caller's job:
``ids = torch.unique(raw, return_inverse=True)[1]``.  ``n_groups=None`` takes
``group_ids.max() + 1``, which costs a second synchronisation.
"""
from __future__ import annotations

import struct

import torch

from . import _lib
from ._lib import call, ptr

_BM_WORDS, _AUC_WORDS = 8, 16  # result words of rs_binary_metrics / rs_auc


def _sized_ws(name, *args, device):
    n = getattr(_lib.lib(), name)(*args)
    if n < 0:
        _lib.check(-1, name)
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device)


def _flat(t, what):
    """[N] view of a [N] / [N, 1] float32 tensor and its element stride."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: a torch tensor on the HIP device is needed, got {type(t).__name__}")
    ptr(t)  # RSError for a CPU tensor
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise ValueError(f"{what}: shape [N] or [N, 1] needed, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.numel() > 1 and t.stride(0) < 1:
        t = t.contiguous()
    return t, max(int(t.stride(0)), 1)


def _labels(t, n):
    t, stride = _flat(t, "labels")
    if stride != 1:
        t = t.contiguous()
    if t.numel() != n:
        raise ValueError(f"{n} predictions but {t.numel()} labels")
    return t


def _groups(group_ids, n_groups, n):
    ptr(group_ids)
    g = group_ids.reshape(-1)
    if g.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"group_ids: int32 or int64 needed, got {g.dtype}")
    g = g.contiguous()
    if g.numel() != n:
        raise ValueError(f"{n} predictions but {g.numel()} group ids")
    if n_groups is None:
        n_groups = int(g.max().item()) + 1 if n else 1
    if n_groups < 1:
        raise ValueError("n_groups must be >= 1")
    return g, int(n_groups)


def _launch_bm(pred, stride, labels, accumulate, result):
    n = labels.numel()
    ws = _sized_ws("rs_binary_metrics_workspace_size", n, device=labels.device)
    call("rs_binary_metrics", ptr(pred), stride, ptr(labels), n, int(accumulate), ptr(result), ptr(ws),
         _lib.stream())  # (ws: freed in stream order by the caching allocator)


def _launch_auc(scores, stride, labels, groups, n_groups, result):
    n = labels.numel()
    ws = _sized_ws("rs_auc_workspace_size", n, n_groups if groups is not None else 0, device=labels.device)
    call("rs_auc", ptr(scores), stride, ptr(labels), ptr(groups), _lib.id_kind(groups) if groups is not None else 0,
         n_groups if groups is not None else 0, n, ptr(result), ptr(ws), _lib.stream())


def _f64(word):
    return struct.unpack("<d", struct.pack("<q", word))[0]


def _bm_dict(w):
    """rs_binary_metrics' 8 words (python ints) -> dict; raises on bad input."""
    n, n_pos, n_correct, loss_bits, n_bad, n_nan = w[:6]
    if n_bad:
        raise ValueError(f"{n_bad} label(s) are neither 0 nor 1")
    if n_nan:
        raise ValueError(f"{n_nan} prediction(s) are NaN")
    nan = float("nan")
    return {"loss": _f64(loss_bits) / n if n else nan, "accuracy": n_correct / n if n else nan,
            "n": n, "n_pos": n_pos, "n_correct": n_correct, "loss_sum": _f64(loss_bits)}


def _auc_dict(w, grouped):
    n, P, Q, U2, auc_bits, n_nan, flags, n_bad, gauc_bits, used, imp = w[:11]
    if n_bad:
        raise ValueError(f"{n_bad} label(s) are neither 0 nor 1")
    if n_nan:
        raise ValueError(f"{n_nan} score(s) are NaN")
    if flags & ~_lib.FLAG_BAD_ID:
        raise _lib.RSError(f"rs_auc: kernel error flag {flags:#x} ({_lib.flag_names(flags)})")
    if flags:
        raise _lib.BadIdError("group id out of range (group ids must be in [0, n_groups))")
    out = {"auc": _f64(auc_bits), "n": n, "n_pos": P, "n_neg": Q, "u2": U2}
    if grouped:
        out.update(gauc=_f64(gauc_bits), groups_used=used, impressions_used=imp)
    return out


def binary_metrics(pred, labels, group_ids=None, n_groups=None):
    """Log-loss, accuracy and exact ROC AUC of probabilities ``pred`` [N] (or
    [N, 1]) against 0/1 ``labels`` [N], computed on the device with one host
    synchronisation.  Returns ``{"loss", "accuracy", "auc", "n", "n_pos"}``
    (and the integer ``n_correct``, ``n_neg``, ``u2``, the fp64 ``loss_sum``);
    with ``group_ids`` [N] (dense ids in [0, n_groups), see the module
    docstring) also ``"gauc"``, ``"groups_used"`` and ``"impressions_used"``:
    the size-weighted mean of the per-group AUCs over the groups that hold
    both classes (NaN when there is none).  The loss is Keras'
    ``binary_crossentropy`` on probabilities (clip to [1e-7, 1 - 1e-7]) in
    fp64; accuracy counts ``(p > 0.5) == (y == 1)``."""
    pred, stride = _flat(pred, "pred")
    n = pred.numel()
    labels = _labels(labels, n)
    groups = None
    if group_ids is not None:
        groups, n_groups = _groups(group_ids, n_groups, n)
    res = torch.empty(_BM_WORDS + _AUC_WORDS, dtype=torch.int64, device=labels.device)
    _launch_bm(pred, stride, labels, 0, res[:_BM_WORDS])
    _launch_auc(pred, stride, labels, groups, n_groups, res[_BM_WORDS:])
    w = res.tolist()
    out = _bm_dict(w[:_BM_WORDS])
    out.update(_auc_dict(w[_BM_WORDS:], groups is not None))
    return out


def auc_stats(scores, labels, group_ids=None, n_groups=None):
    """rs_auc's result as a dict: ``auc`` and the integers behind it (``n``,
    ``n_pos`` = P, ``n_neg`` = Q, ``u2`` = U2 with auc = U2 / (2 P Q)); with
    ``group_ids`` also ``gauc``, ``groups_used`` and ``impressions_used``."""
    scores, stride = _flat(scores, "scores")
    n = scores.numel()
    labels = _labels(labels, n)
    groups = None
    if group_ids is not None:
        groups, n_groups = _groups(group_ids, n_groups, n)
    res = torch.empty(_AUC_WORDS, dtype=torch.int64, device=labels.device)
    _launch_auc(scores, stride, labels, groups, n_groups, res)
    w = res.tolist()
    return _auc_dict(w, groups is not None)


def roc_auc(scores, labels):
    """Exact tie-aware ROC AUC of any finite float32 ``scores`` [N]
    (probabilities or logits) against 0/1 ``labels``; NaN when one class is
    missing."""
    return auc_stats(scores, labels, None, None)["auc"]


def group_auc(scores, labels, group_ids, n_groups=None):
    """GAUC: sum_g size_g AUC_g / sum_g size_g over the groups with both
    classes (dense ``group_ids`` in [0, n_groups); NaN when no group
    qualifies)."""
    return auc_stats(scores, labels, group_ids, n_groups)["gauc"]


class BinaryMetrics:
    """Streaming form: ``update(pred, labels[, group_ids])`` per batch folds
    the batch into the device-side sums (rs_binary_metrics with accumulate)
    and keeps a copy of the batch for the AUC, with no host synchronisation;
    ``result()`` runs the AUC over everything seen and synchronises once.
    ``reset()`` starts over."""

    def __init__(self, device=None, n_groups=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.n_groups = n_groups
        self.reset()

    def reset(self):
        self._acc = torch.zeros(_BM_WORDS, dtype=torch.int64, device=self.device)
        self._pred, self._lab, self._grp = [], [], []

    def update(self, pred, labels, group_ids=None):
        pred, stride = _flat(pred, "pred")
        labels = _labels(labels, pred.numel())
        if (group_ids is None) != (not self._grp) and self._pred:
            raise ValueError("BinaryMetrics.update: group ids on every batch or on none")
        _launch_bm(pred, stride, labels, 1, self._acc)
        self._pred.append(pred.clone() if stride == 1 else pred.contiguous())
        self._lab.append(labels.clone())
        if group_ids is not None:
            ptr(group_ids)
            self._grp.append(group_ids.reshape(-1).clone())

    def result(self):
        if not self._pred:
            raise ValueError("BinaryMetrics.result: no batch seen")
        pred, labels = torch.cat(self._pred), torch.cat(self._lab)
        groups, n_groups = None, None
        if self._grp:
            groups, n_groups = _groups(torch.cat(self._grp), self.n_groups, pred.numel())
        res = torch.empty(_AUC_WORDS, dtype=torch.int64, device=labels.device)
        _launch_auc(pred, 1, labels, groups, n_groups, res)
        w = torch.cat([self._acc, res]).tolist()
        out = _bm_dict(w[:_BM_WORDS])
        out.update(_auc_dict(w[_BM_WORDS:], groups is not None))
        return out
