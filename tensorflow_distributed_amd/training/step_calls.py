"""Cut points of the ``--steps_per_call N`` driver mode (TF's ``iterations_per_loop``): how many optimizer
steps each host round trip takes. One pure function, no torch: the drivers and the tests share it.

A call is one ``runner.train_steps(k)`` -- ``k`` consecutive steps on the device with no host
synchronisation -- followed by one ``runner.read_step_log``. Everything the host does *between* steps
must therefore fall on the end of a call: the ``--eval_at_steps`` passes, the ``--check_consistency_every``
checksums, ``--fault_inject_step`` and, in ``mnist_single.py``, the ``--display_step`` minibatch-loss
forward, which needs the last batch. Those global steps are the cuts. Epoch boundaries are not cuts: the
per-epoch reshuffle happens inside ``train_steps``.
"""
from __future__ import annotations

from typing import Iterable, List


def call_lengths(step: int, n: int, train_steps: int, cuts: Iterable[int] = ()) -> List[int]:
    """Lengths of the calls that take global_step from ``step`` to ``train_steps``: each at most ``n``, and
    a call ends at every cut (a global step value) strictly between the two. Cuts outside that range are
    ignored (a cut at ``train_steps`` is the end of the last call anyway)."""
    if n < 1:
        raise ValueError("call_lengths: n must be >= 1, got %d" % n)
    todo = sorted({int(c) for c in cuts if step < int(c) < train_steps})
    out, i = [], 0
    while step < train_steps:
        end = min(step + n, train_steps)
        while i < len(todo) and todo[i] <= step:
            i += 1
        if i < len(todo) and todo[i] < end:
            end = todo[i]
        out.append(end - step)
        step = end
    return out


def multiples(every: int, start: int, stop: int, origin: int = 0) -> List[int]:
    """The values ``origin + k * every`` (k >= 1) in ``(start, stop]``; empty when ``every`` < 1."""
    if every < 1:
        return []
    k = max(1, (start - origin) // every + 1)
    return list(range(origin + k * every, stop + 1, every))
