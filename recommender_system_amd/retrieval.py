"""Retrieval for the two-tower models: exact top-N by inner product.

``topn_inner_product(user, item, N)`` returns, for every row of ``user``
[U, E], the N rows of ``item`` [I, E] with the largest inner product, ordered
by the key (score descending, item position ascending): ``idx`` int32 [U, N]
(positions into ``item``) and ``score`` float32 [U, N].  A tie in score goes
to the lower position; where I < N the slots past I hold (-1, -inf).

  fused=True   rs_topn_inner_product (csrc/topn.hip): no [U, I] buffer; a
               shape rs_topn_inner_product_ok refuses raises.
  fused=False  the torch composition: ``matmul`` over (user, item) chunks small
               enough that no temporary exceeds 256 MB, ``topk`` of each chunk
               on the same 64-bit key (score, ~position) the kernel orders by,
               and a ``topk`` merge of the chunk results with the running best.
  fused=None   the kernel where rs_topn_inner_product_ok accepts the shape
               (it is the faster one at every measured shape class, DESIGN
               4.5e), the torch composition for a refused shape.

``DSSM.retrieve`` / ``DSSM.recall`` (dssm.py) are built on it.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, ptr
from ._train_ops import scratch

TEMP_BYTES = 256 << 20  # the torch composition's largest temporary
_EMPTY = -(1 << 63)     # the torch composition's "no item" key (below every real key)


class _Workspaces:
    """The grow-only workspace of every device (``_train_ops.scratch``)."""

    def __init__(self, dev):
        self._dev = dev


_ws_owner = {}


def _workspace(dev, nbytes):
    owner = _ws_owner.get(dev)
    if owner is None:
        owner = _ws_owner[dev] = _Workspaces(dev)
    return scratch(owner, "_topn_ws", max(int(nbytes), 8))


def topn_ok(E, N):
    """rs_topn_inner_product_ok: the kernel takes embedding width E and list length N."""
    return bool(_lib.lib().rs_topn_inner_product_ok(int(E), int(N)))


def _matrix(x, name):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    if t.dim() != 2:
        raise ValueError(f"topn_inner_product: {name} must be a matrix [rows, E], got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t


def _on_device(t):
    if not t.is_cuda:
        t = t.cuda()
    return t if t.stride(1) == 1 else t.contiguous()


def _keys(s, pos0):
    """int64 keys of the scores s [u, i] of item positions pos0 .. pos0 + i - 1:
    the score's bits made to order like the float (high word), ~position (low
    word) — a larger key is a better item, as in the kernel."""
    b = (s + 0.0).view(torch.int32)  # (-0 counts as +0)
    hi = torch.where(b < 0, b ^ 0x7FFFFFFF, b).to(torch.int64) << 32
    lo = 0xFFFFFFFF - torch.arange(pos0, pos0 + s.shape[1], device=s.device, dtype=torch.int64)
    return hi | lo.unsqueeze(0)


def _unkey(k):
    empty = k == _EMPTY
    idx = (0xFFFFFFFF - (k & 0xFFFFFFFF)).to(torch.int32)
    h = (k >> 32).to(torch.int32)
    score = torch.where(h < 0, h ^ 0x7FFFFFFF, h).view(torch.float32)
    return (torch.where(empty, torch.full_like(idx, -1), idx),
            torch.where(empty, torch.full_like(score, float("-inf")), score))


def _topn_torch(user, item, N):
    U, I = user.shape[0], item.shape[0]
    dev = user.device
    idx = torch.empty(U, N, dtype=torch.int32, device=dev)
    score = torch.empty(U, N, dtype=torch.float32, device=dev)
    uc = max(1, min(U, 4096))
    ic = max(1, min(I, TEMP_BYTES // 8 // uc))  # the int64 keys of a chunk are its largest temporary
    for u0 in range(0, U, uc):
        u = user[u0:u0 + uc]
        best = torch.full((u.shape[0], N), _EMPTY, dtype=torch.int64, device=dev)
        for i0 in range(0, I, ic):
            v = item[i0:i0 + ic]
            k = torch.topk(_keys(u @ v.t(), i0), min(N, v.shape[0]), dim=1).values
            best = torch.topk(torch.cat([best, k], 1), N, dim=1).values
        idx[u0:u0 + uc], score[u0:u0 + uc] = _unkey(best)
    return idx, score


def topn_inner_product(user, item, N, item_splits=0, fused=None):
    """(idx int32 [U, N], score float32 [U, N]): see the module docstring.
    ``item_splits``: the kernel's item split count (0 = chosen from the shape);
    the result does not depend on it."""
    user, item = _matrix(user, "user"), _matrix(item, "item")
    N, item_splits = int(N), int(item_splits)
    if user.shape[1] != item.shape[1]:
        raise ValueError(f"topn_inner_product: user rows hold {user.shape[1]} values, item rows {item.shape[1]}")
    if N < 1:
        raise ValueError("topn_inner_product: N must be at least 1")
    if item_splits < 0:
        raise ValueError("topn_inner_product: item_splits must be 0 (auto) or positive")
    U, E = user.shape
    I = item.shape[0]
    if E < 1:
        raise ValueError("topn_inner_product: empty rows")
    if I >= 1 << 31:
        raise ValueError("topn_inner_product: too many items")
    user, item = _on_device(user), _on_device(item)
    if user.device != item.device:
        raise ValueError("topn_inner_product: user and item are on different devices")
    if fused is None:
        fused = topn_ok(E, N)
    if not fused:
        return _topn_torch(user, item, N)
    dev = user.device
    idx = torch.empty(U, N, dtype=torch.int32, device=dev)
    score = torch.empty(U, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = _lib.lib().rs_topn_inner_product_workspace_size(U, I, N, item_splits)
        ws = _workspace(dev, need)
        call("rs_topn_inner_product", ptr(user), user.stride(0) if U > 1 else E, U, ptr(item),
             item.stride(0) if I > 1 else E, I, E, N, item_splits, ptr(idx), ptr(score), ptr(ws), ws.numel(), _lib.stream(dev))
    return idx, score
