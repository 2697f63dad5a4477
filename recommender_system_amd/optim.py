"""Optimizers of the training steps that do not use plain SGD.

``Adam`` is Keras optimizer_v2 Adam (the reference's ``optimizer="adam"``,
model/dssm.py:149): rs_adam_update_multi over every parameter, 32 tensors a
launch, with the step counter in device memory so that a captured step replays
correctly."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import call, ptr


class Adam:
    """Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7): at step
    t = 1, 2, ... with g = gradient + 2 l2 w,

        lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t)
        m = beta_1 m + (1 - beta_1) g;  v = beta_2 v + (1 - beta_2) g^2
        w -= lr_t m / (sqrt(v) + epsilon)

    ``m`` / ``v`` are created (zeros) the first time a weight is seen and kept
    per weight object (``state(weight)``); ``step`` is an int64 [1] device
    tensor that ``apply`` advances on the stream."""

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, device=None):
        self.lr, self.beta_1, self.beta_2, self.epsilon = float(lr), float(beta_1), float(beta_2), float(epsilon)
        self.step = torch.zeros(1, dtype=torch.int64, device=device if device is not None else "cuda")
        self._state = {}  # id(weight) -> (weight, m, v)

    def state(self, weight):
        """(m, v) of a weight, created on first sight."""
        s = self._state.get(id(weight))
        if s is None:
            s = self._state[id(weight)] = (weight, torch.zeros_like(weight), torch.zeros_like(weight))
        return s[1], s[2]

    def apply(self, updates, st, lr=None):
        """One Adam step over updates = [(weight, gradient, l2)] (float32
        device tensors, contiguous; l2 the Keras l2 factor): one
        rs_adam_update_multi, then rs_adam_advance."""
        if not updates:
            return
        n = len(updates)
        mv = [self.state(u[0]) for u in updates]
        for w, g, _ in updates:
            if not (w.is_contiguous() and g.is_contiguous() and g.numel() == w.numel()):
                raise ValueError("Adam.apply: weights and gradients must be contiguous and of one size")
        vp = lambda ts: (C.c_void_p * n)(*[ptr(t) for t in ts])
        call("rs_adam_update_multi", n, vp([u[0] for u in updates]), vp([u[1] for u in updates]),
             vp([s[0] for s in mv]), vp([s[1] for s in mv]), (C.c_int64 * n)(*[u[0].numel() for u in updates]),
             (C.c_float * n)(*[float(u[2]) for u in updates]), self.lr if lr is None else float(lr), self.beta_1,
             self.beta_2, self.epsilon, ptr(self.step), st)
        call("rs_adam_advance", ptr(self.step), st)


def adam_reference(w, g, m, v, t, l2=0.0, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """The same step in float64 numpy: returns (w, m, v) after step t (1-based)."""
    import numpy as np
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    g = g + 2.0 * l2 * w
    lr_t = lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m = beta_1 * m + (1.0 - beta_1) * g
    v = beta_2 * v + (1.0 - beta_2) * g * g
    return w - lr_t * m / (np.sqrt(v) + epsilon), m, v
