"""Forecast baselines: what a trivial predictor scores on the clips the rollout is scored on.

``results --pred-len P`` prints the rollout's MPJPE, P1 and P2 per horizon; a forecast error means something only beside these.  After
``I = input_len`` observed frames, for horizons ``h = 0 .. P-1`` (frame ``I + h``):

* ``const_pose``: the anchor pose, held: ``a1``;
* ``const_vel``: the anchor's last step, continued: ``a1 + (h + 1) (a1 - a0)``;
* ``nn``: the movie strip ``phi[I - 1]`` of the clip (``PHDFor3DJoints.observe``) is looked up among the strips of a database of
  training clips (squared L2, ``r50_op_nn_search``); the ``k`` nearest clips' futures, each relative to its own root at frame ``I - 1``,
  are averaged in list order and attached to the anchor's root: ``a1[root] + mean_i (J_i[I + h] - J_i[I - 1, root])``.

The anchor ``a1``, ``a0`` is the pose at frames ``I - 1`` and ``I - 2``: with ``anchor="pred"`` the head's own reconstruction from
``observe`` (the paper's form: the last prediction, held), with ``anchor="gt"`` the ground truth (the motion-forecasting literature's
form, a stronger opponent).  The paper does not say how a retrieved future is placed or which strip is the key: the L2 metric, the key
``phi[I - 1]`` and the root attachment are this project's choices.

The search never stores a distance matrix: one MFMA kernel walks the database once per 256 queries and keeps k candidates per query;
its order on (score, index) is strict and total, so the result is the same bits on every run and under every ``cu_cap``.  The three
forecasts are one gather launch (``r50_op_baseline_forecasts``); the scorers are ``forecast.add_horizon_metrics`` and
``protocols``' kernel, per baseline and for the model's own rollout in the same pass.  No CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, clip_pass, protocols
from .forecast import add_horizon_metrics, metrics_from_sums
from .protocols import ROOT_JOINT

BASELINES = ("const_pose", "const_vel", "nn")
ANCHORS = ("pred", "gt")
MAX_K = 8                                     # r50_op_nn_search's limit on k
MAX_D = 2048                                  # ... and on the row length


def _et(t: torch.Tensor) -> int:
    if t.dtype == torch.float16:
        return 1
    if t.dtype == torch.bfloat16:
        return 0
    raise ValueError(f"expected fp16 or bf16 rows, got {t.dtype}")


def row_norm2(x: torch.Tensor) -> torch.Tensor:
    """(N,) fp32 = ``|x_i|^2`` of the 16-bit rows x (N, D), D % 8 == 0: ``r50_op_row_norm2`` (fp64 sums in a fixed order, rounded once)."""
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 8 or x.shape[1] % 8:
        raise ValueError(f"x must be (N >= 1, D a positive multiple of 8), got {tuple(x.shape)}")
    et = _et(x)
    if not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be contiguous on the GPU: there is no CPU fallback")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load_library().r50_op_row_norm2(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), et, out.data_ptr(),
                                                  torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, None, "r50_op_row_norm2")
    return out


def nn_search(q: torch.Tensor, x: torch.Tensor, x_norm2: torch.Tensor, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k rows of x (N, D) nearest to each row of q (NQ, D) in squared L2: (idx (NQ, k) int32, dist2 (NQ, k) fp32), ascending by
    (score, index) with score = ``x_norm2[x] - 2 q.x`` (``r50_op_nn_search``).  q and x are 16-bit rows of one type, ``x_norm2`` (N,) fp32
    from ``row_norm2(x)``; 1 <= k <= 8, k <= N, D % 32 == 0, 32 <= D <= 2048."""
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1] or q.dtype != x.dtype:
        raise ValueError(f"q (NQ, D) and x (N, D) of one 16-bit type expected, got {tuple(q.shape)} {q.dtype}, {tuple(x.shape)} {x.dtype}")
    et = _et(x)
    nq, d = int(q.shape[0]), int(q.shape[1])
    n, k = int(x.shape[0]), int(k)
    if nq < 1 or not 1 <= k <= MAX_K or k > n or d % 32 or not 32 <= d <= MAX_D:
        raise ValueError(f"need NQ >= 1, 1 <= k <= {MAX_K}, k <= N, D % 32 == 0 and 32 <= D <= {MAX_D} (got NQ={nq}, N={n}, D={d}, k={k})")
    if x_norm2.dtype != torch.float32 or tuple(x_norm2.shape) != (n,):
        raise ValueError(f"x_norm2 must be ({n},) fp32, got {tuple(x_norm2.shape)} {x_norm2.dtype}")
    if not x.is_cuda or not (q.device == x.device == x_norm2.device):
        raise ValueError("q, x and x_norm2 must be on one GPU: there is no CPU fallback")
    if not (q.is_contiguous() and x.is_contiguous() and x_norm2.is_contiguous()):
        raise ValueError("q, x and x_norm2 must be contiguous")
    lib = _lib.load_library()
    idx = torch.empty((nq, k), dtype=torch.int32, device=x.device)
    dist2 = torch.empty((nq, k), dtype=torch.float32, device=x.device)
    ws_bytes = int(lib.r50_op_nn_search_workspace(nq, n, k))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.r50_op_nn_search(q.data_ptr(), nq, x.data_ptr(), n, d, et, x_norm2.data_ptr(), k, idx.data_ptr(), dist2.data_ptr(),
                                  ws.data_ptr(), ws_bytes, torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, None, "r50_op_nn_search")
    return idx, dist2


def _launch_forecasts(a1: torch.Tensor, a0: Optional[torch.Tensor], nn_row: Optional[torch.Tensor], dbj: Optional[torch.Tensor],
                      input_len: int, pred_len: int, which: Sequence[str], root: int) -> Dict[str, torch.Tensor]:
    """Shape, dtype and device checks, then one launch; the VALUES of ``nn_row`` are the caller's to have checked."""
    unknown = [w for w in which if w not in BASELINES]
    if unknown or not which:
        raise ValueError(f"which: expected some of {BASELINES}, got {tuple(which)}")
    if a1.dim() != 3 or a1.shape[2] != 3 or a1.dtype != torch.float32 or not a1.is_cuda or not a1.is_contiguous():
        raise ValueError(f"a1 must be (B, J, 3) contiguous fp32 on the GPU, got {tuple(a1.shape)} {a1.dtype}")
    b, j, _ = a1.shape
    i_len, p_len = int(input_len), int(pred_len)
    if b < 1 or not 1 <= j <= protocols.MAX_JOINTS or not 0 <= root < j or i_len < 1 or p_len < 1:
        raise ValueError(f"need B, input_len, pred_len >= 1, 1 <= J <= {protocols.MAX_JOINTS} and 0 <= root < J "
                         f"(got B={b}, J={j}, root={root}, input_len={i_len}, pred_len={p_len})")
    if "const_vel" in which:
        if i_len < 2:
            raise ValueError("const_vel needs input_len >= 2: it continues the last observed step")
        if a0 is None or tuple(a0.shape) != (b, j, 3) or a0.dtype != torch.float32 or a0.device != a1.device or not a0.is_contiguous():
            raise ValueError(f"const_vel needs a0 ({b}, {j}, 3) contiguous fp32 on a1's device")
    k = t_db = n_db = 0
    if "nn" in which:
        if nn_row is None or dbj is None:
            raise ValueError("nn needs nn_row (B, k) int32 and dbj (N, T, J, 3) fp32")
        if nn_row.dim() != 2 or nn_row.shape[0] != b or nn_row.dtype != torch.int32 or not 1 <= nn_row.shape[1] <= MAX_K:
            raise ValueError(f"nn_row must be ({b}, 1..{MAX_K}) int32, got {tuple(nn_row.shape)} {nn_row.dtype}")
        if dbj.dim() != 4 or tuple(dbj.shape[2:]) != (j, 3) or dbj.dtype != torch.float32 or dbj.shape[0] < 1:
            raise ValueError(f"dbj must be (N, T, {j}, 3) fp32, got {tuple(dbj.shape)} {dbj.dtype}")
        k, n_db, t_db = int(nn_row.shape[1]), int(dbj.shape[0]), int(dbj.shape[1])
        if i_len + p_len > t_db:
            raise ValueError(f"input_len + pred_len = {i_len + p_len} exceeds the database clips' {t_db} frames")
        if not (nn_row.device == dbj.device == a1.device) or not (nn_row.is_contiguous() and dbj.is_contiguous()):
            raise ValueError("nn_row and dbj must be contiguous on a1's device")
    out = {w: torch.empty((b, p_len, j, 3), dtype=torch.float32, device=a1.device) for w in which}
    ptr = lambda t: t.data_ptr() if t is not None else None                      # noqa: E731
    with torch.cuda.device(a1.device):
        rc = _lib.load_library().r50_op_baseline_forecasts(
            a1.data_ptr(), ptr(a0) if "const_vel" in which else None, ptr(nn_row) if "nn" in which else None,
            ptr(dbj) if "nn" in which else None, n_db, b, k, t_db, j, int(root), i_len, p_len, ptr(out.get("const_pose")),
            ptr(out.get("const_vel")), ptr(out.get("nn")), torch.cuda.current_stream(a1.device).cuda_stream)
    _lib.check(rc, None, "r50_op_baseline_forecasts")
    return out


def baseline_forecasts(a1: torch.Tensor, a0: Optional[torch.Tensor], nn_row: Optional[torch.Tensor], dbj: Optional[torch.Tensor],
                       input_len: int, pred_len: int, which: Sequence[str] = BASELINES, root: int = ROOT_JOINT) -> Dict[str, torch.Tensor]:
    """``{name: (B, P, J, 3) fp32}`` for the names in ``which``, one ``r50_op_baseline_forecasts`` launch.  a1, a0 (B, J, 3) fp32: the
    anchor poses (a0 only for ``const_vel``); nn_row (B, k) int32 rows of dbj (N, T, J, 3) fp32 (only for ``nn``), each in [0, N):
    checked on the host before the launch (one read)."""
    if "nn" in which and isinstance(nn_row, torch.Tensor) and isinstance(dbj, torch.Tensor) and nn_row.numel() > 0 \
            and nn_row.dtype == torch.int32:
        lo, hi = (int(v) for v in torch.stack([nn_row.min(), nn_row.max()]).cpu())
        if lo < 0 or hi >= dbj.shape[0]:
            raise ValueError(f"nn_row values must lie in [0, {dbj.shape[0]}), got [{lo}, {hi}]")
    return _launch_forecasts(a1, a0, nn_row, dbj, input_len, pred_len, tuple(which), int(root))


class StripDatabase:
    """The strips of a training ``DeviceFeatureStore`` to search in: ``keys`` (N, D) 16-bit = ``phi[:, I - 1]`` of every item in store
    order, ``norm2`` (N,) fp32 their squared norms, ``rows`` (N,) int32 the items' rows of ``joints`` = ``store.joints3d`` itself (a
    view: no copy of the joints is made)."""

    def __init__(self, keys: torch.Tensor, norm2: torch.Tensor, joints: torch.Tensor, rows: torch.Tensor, input_len: int):
        self.keys, self.norm2, self.joints, self.rows, self.input_len = keys, norm2, joints, rows, int(input_len)

    def __len__(self) -> int:
        return int(self.keys.shape[0])

    @classmethod
    @torch.no_grad()
    def build(cls, head, store, input_len: int, batch_size: int = 256) -> "StripDatabase":
        i_len = int(input_len)
        if not 1 <= i_len <= int(store.feats.shape[1]):
            raise ValueError(f"need 1 <= input_len <= the store's seq_len {int(store.feats.shape[1])}, got {i_len}")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if not 32 <= head.latent_dim <= MAX_D:
            raise ValueError(f"the search takes strips of 32 .. {MAX_D} values, this head has {head.latent_dim}")
        dev = head._device
        with torch.cuda.device(dev):
            keys = torch.empty((len(store), head.latent_dim), dtype=head._dtype, device=dev)
            for s, e in clip_pass.spans(len(store), batch_size):
                keys[s:e].copy_(head.observe(store.get_batch(list(range(s, e)))[0], i_len)[0][:, i_len - 1])
            joints = store.joints3d if store.joints3d.dtype == torch.float32 and store.joints3d.is_contiguous() \
                else store.joints3d.to(torch.float32).contiguous()
            return cls(keys, row_norm2(keys), joints, store._row.to(torch.int32), i_len)


@torch.no_grad()
def forecast_batch(head, db: Optional[StripDatabase], feats: torch.Tensor, gt: torch.Tensor, input_len: int, pred_len: int,
                   which: Sequence[str], nn_k: int = 1, anchor: str = "pred") -> Dict[str, torch.Tensor]:
    """The baselines' forecasts for one batch: ``{name: (B, P, J, 3) fp32}`` for the names in ``which`` and, with ``nn``, ``nn_index``
    (B, k) int32 (items of the database, store order) and ``nn_dist2`` (B, k) fp32.  gt (B, T, J, 3) fp32 is read only with
    ``anchor="gt"``."""
    i_len = int(input_len)
    if anchor not in ANCHORS:
        raise ValueError(f"anchor: expected one of {ANCHORS}, got {anchor!r}")
    phi, obs = head.observe(feats, i_len)
    src = obs if anchor == "pred" else gt
    a1 = src[:, i_len - 1].contiguous()
    a0 = src[:, i_len - 2].contiguous() if "const_vel" in which and i_len >= 2 else None
    out: Dict[str, torch.Tensor] = {}
    nn_row = None
    if "nn" in which:
        if db is None or db.input_len != i_len:
            raise ValueError("nn needs a StripDatabase built with the same input_len")
        idx, dist2 = nn_search(phi[:, i_len - 1].contiguous(), db.keys, db.norm2, nn_k)
        nn_row = db.rows.index_select(0, idx.reshape(-1).long()).view(idx.shape).contiguous()
        out.update(nn_index=idx, nn_dist2=dist2)
    out.update(_launch_forecasts(a1, a0, nn_row, db.joints if nn_row is not None else None, i_len, int(pred_len), tuple(which), ROOT_JOINT))
    return out


@torch.no_grad()
def evaluate_baselines(head, store, db: Optional[StripDatabase], groups: Sequence[int], group_names: Sequence[str], input_len: int,
                       pred_len: int, which: Sequence[str] = BASELINES, nn_k: int = 1, anchor: str = "pred",
                       batch_size: int = 256) -> Dict[str, object]:
    """The baselines ``which`` and the model's own rollout over every item of ``store`` (a ``DeviceFeatureStore``) once, in store order,
    ``batch_size`` clips per batch (the last kept even if short), all scored in the same pass by ``forecast.add_horizon_metrics`` and
    ``protocols``' kernel.  ``groups[i]`` in ``[0, len(group_names))`` is item i's group (``protocols.action_groups``); ``db`` a
    ``StripDatabase`` of training clips (needed for ``nn``).  Returns (metres, fp64)::

        names = ("model",) + which;  group_names [G];  clips (G,) int64;  anchor;  nn_k
        <name>: {"mpjpe" (P,), "p1" (P,), "p2" (P,), "per_action" (G, P, 2)}     for every name
        nn_dist2_mean: the mean squared strip distance to the retrieved clips (NaN without ``nn``)

    The ``model`` rows are ``evaluate_rollout``'s and ``evaluate_protocols``' numbers exactly.  The sums are read back once per pass."""
    which = tuple(which)
    unknown = [w for w in which if w not in BASELINES]
    if unknown or not which or len(set(which)) != len(which):
        raise ValueError(f"which: expected distinct names of {BASELINES}, got {which}")
    if anchor not in ANCHORS:
        raise ValueError(f"anchor: expected one of {ANCHORS}, got {anchor!r}")
    n_groups = len(group_names)
    ids, i_len, p_len, _ = clip_pass.check(store, input_len, pred_len, batch_size, groups, n_groups)
    if "const_vel" in which and i_len < 2:
        raise ValueError("const_vel needs input_len >= 2: it continues the last observed step")
    if "nn" in which and (db is None or not 1 <= int(nn_k) <= min(MAX_K, len(db))):
        raise ValueError(f"nn needs a StripDatabase and 1 <= nn_k <= min({MAX_K}, its clips)")
    names = ("model",) + which
    dev = head._device
    n_h, n_p = 2 * p_len + 1, 2 * n_groups * p_len + n_groups
    with torch.cuda.device(dev):
        acc_h = torch.zeros((len(names), n_h), dtype=torch.float64, device=dev)
        acc_p = torch.zeros((len(names), n_p), dtype=torch.float64, device=dev)
        dist = torch.zeros(1, dtype=torch.float64, device=dev)
        for feats, gt, group in clip_pass.batches(head, store, batch_size, ids):
            preds = forecast_batch(head, db, feats, gt, i_len, p_len, which, nn_k, anchor)
            preds["model"] = head.rollout(feats, i_len, p_len)[1]
            for r, name in enumerate(names):
                add_horizon_metrics(preds[name], gt, i_len, acc_h[r])
                protocols._launch(preds[name], gt, i_len, group, n_groups, acc_p[r], ROOT_JOINT)
            if "nn" in which:
                dist += preds["nn_dist2"].double().sum()
        sums = torch.cat([acc_h.reshape(-1), acc_p.reshape(-1), dist]).cpu().numpy()
    out: Dict[str, object] = {"names": names, "group_names": list(group_names), "anchor": anchor, "nn_k": int(nn_k)}
    for r, name in enumerate(names):
        hm = metrics_from_sums(sums[r * n_h:(r + 1) * n_h].tolist(), p_len, head.joints_num)
        per, all_, clips = protocols._values(sums[len(names) * n_h + r * n_p: len(names) * n_h + (r + 1) * n_p], n_groups, p_len)
        out[name] = {"mpjpe": np.asarray(hm["mpjpe"], dtype=np.float64), "p1": all_[:, 0].copy(), "p2": all_[:, 1].copy(), "per_action": per}
        out["clips"] = clips.round().astype(np.int64)
    out["nn_dist2_mean"] = float(sums[-1]) / (len(store) * int(nn_k)) if "nn" in which else float("nan")
    return out


def baseline_lines(res: Dict[str, object], input_len: int, pred_len: int) -> List[str]:
    """The printed lines of ``--baselines`` from an ``evaluate_baselines`` result: the ``Baselines`` header, then one indented line per
    predictor, ``model`` first: MPJPE, P1 and P2 in mm at horizons 1, 5, 10 and P and their mean over the horizons, and for each
    baseline the model's skill ``1 - model / baseline`` on the P1 mean (positive: the model beats it)."""
    hs = sorted({h for h in (1, 5, 10, pred_len) if h <= pred_len})
    head = (f"Baselines | input {input_len} | pred {pred_len} | clips {int(np.sum(res['clips']))} | anchor {res['anchor']} | predictors "
            f"{len(res['names'])}")
    if "nn" in res["names"]:
        head += f" | nn k {int(res['nn_k'])} | nn strip dist2 mean {res['nn_dist2_mean']:.6g}"
    lines = [head]
    model_p1 = float(np.mean(res["model"]["p1"]))
    for name in res["names"]:
        row = res[name]
        parts = [f"{key} (mm) " + " | ".join(f"@{h}: {row[key][h - 1] * 1000.0:.2f}" for h in hs) + f" | mean: {np.mean(row[key]) * 1000.0:.2f}"
                 for key in ("mpjpe", "p1", "p2")]
        line = f"  {name} | " + " | ".join(parts)
        if name != "model":
            base_p1 = float(np.mean(row["p1"]))
            line += f" | model skill on p1: {(1.0 - model_p1 / base_p1) if base_p1 > 0 else float('nan'):+.4f}"
        lines.append(line)
    return lines


def baseline_arrays(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--baselines``: ``baseline_names`` (Nb,) str, ``model`` first; fp32 ``baseline_mpjpe``, ``baseline_p1``,
    ``baseline_p2`` (Nb, P) in metres; ``baseline_actions`` (G,) str; ``baseline_per_action`` (Nb, G, P, 2) fp32 [p1, p2];
    ``baseline_anchor`` str.  (``main`` adds ``nn_index``, ``nn_dist2`` and ``nn_future3djoints`` of the dumped clips.)"""
    names = list(res["names"])
    out = {"baseline_names": np.array(names, dtype=str), "baseline_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "baseline_anchor": np.array(str(res["anchor"])),
           "baseline_per_action": np.stack([np.asarray(res[n]["per_action"], dtype=np.float32) for n in names])}
    for key in ("mpjpe", "p1", "p2"):
        out["baseline_" + key] = np.stack([np.asarray(res[n][key], dtype=np.float32) for n in names])
    return out
