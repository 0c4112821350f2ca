"""One pass over the clips of a ``DeviceFeatureStore``, as the result reports make it: every item once, in store order, ``batch_size``
clips per batch, the last batch kept even if short.  ``check`` holds the rules of a pass's arguments, ``batches`` walks it; what to
predict, which op to launch, the accumulators and the single read-back stay with each report (``protocols.evaluate_protocols``,
``detail_metrics.evaluate_detail``, ``dtw.evaluate_dtw``, ``baselines.evaluate_baselines``, ``hallucinate.evaluate_hallucinator``,
``forecast.evaluate_rollout``).
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch


def check(store, input_len: int, pred_len: int, batch_size: int, groups: Optional[Sequence[int]] = None, n_groups: int = 0,
          forecast_required: bool = True, max_pred_len: Optional[int] = None) -> Tuple[Optional[np.ndarray], int, int, int]:
    """The argument rules of a pass, before anything touches the head; only ``len(store)`` and ``store.feats.shape[1]`` are read.
    With ``groups`` (item i's group id): one id per item, ``n_groups >= 1``, every id in ``[0, n_groups)``.  The lengths: a required
    forecast needs ``input_len, pred_len >= 1`` (and ``pred_len <= max_pred_len``, an op's limit); an optional one ``pred_len >= 0``;
    one that is on must fit, ``input_len + pred_len <= seq_len``.  ``batch_size >= 1``.  ``ValueError`` otherwise.
    Returns (ids int64 or None, input_len, pred_len, seq_len)."""
    i_len, p_len = int(input_len), int(pred_len)
    seq_len = int(store.feats.shape[1])
    ids = None
    if groups is not None:
        if len(groups) != len(store):
            raise ValueError(f"groups has {len(groups)} ids for {len(store)} items")
        if n_groups < 1:
            raise ValueError("no groups")
        ids = np.asarray(groups, dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n_groups):
            raise ValueError(f"group ids must lie in [0, {n_groups})")
    if forecast_required:
        if i_len < 1 or p_len < 1 or (max_pred_len is not None and p_len > max_pred_len) or i_len + p_len > seq_len:
            cap = "" if max_pred_len is None else f", pred_len <= {max_pred_len}"
            raise ValueError(f"need input_len, pred_len >= 1{cap} and input_len + pred_len <= seq_len {seq_len} (got {i_len}, {p_len})")
    elif p_len < 0 or (p_len > 0 and (i_len < 1 or i_len + p_len > seq_len)):
        raise ValueError(f"need pred_len >= 0 and, with pred_len > 0, 1 <= input_len and input_len + pred_len <= seq_len {seq_len} "
                         f"(got {i_len}, {p_len})")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    return ids, i_len, p_len, seq_len


def spans(n: int, batch_size: int) -> Iterator[Tuple[int, int]]:
    """The batches' item ranges ``[s, e)`` over ``n`` items: store order, the short last batch kept."""
    for s in range(0, n, batch_size):
        yield s, min(s + batch_size, n)


def batches(head, store, batch_size: int, ids: Optional[np.ndarray] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]]:
    """Per batch of the pass: (the features, ``gt`` = the 3D joints as contiguous fp32 on the head's device, the batch's slice of the
    group ids as int32 on that device -- uploaded once -- or None without ``ids``)."""
    dev = head._device
    gdev = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
    for s, e in spans(len(store), batch_size):
        batch = store.get_batch(list(range(s, e)))
        yield batch[0], batch[1].to(device=dev, dtype=torch.float32).contiguous(), None if gdev is None else gdev[s:e]
