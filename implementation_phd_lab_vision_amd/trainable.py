"""What the head trainers share (train.py phase 1, train_ar.py phase 2 and rollout, train_joint.py joint): a lifting head whose
trainable parameters live in flat fp32 master / 16-bit / gradient buffers, the launches of its backward pass, and the tail of a step.

A subclass of ``FlatTrainableHead`` says WHICH parameters train and in what order (``_flat_items``: the order decides where a
parameter sits in the buffer RCCL reduces), which 16-bit weights need no transpose or a one-time one, where its dropout sits and what
its clips must look like; it keeps its own ``forward_backward`` and loss.  Everything else is here, once: ``_upload``, the
reference-layout round trip (``flat_to_reference`` / ``flat_from_reference``), the GEMM / weight-gradient / GroupNorm-backward launch
helpers, the residual blocks' saved forward and per-block backward, the regressor's backward, the arena's overflow sweep and ``_finish_step``
(all-reduce, finite check -- or, with clipping on, the global gradient norm that contains it --, AdamW, scale update), and ``WeightEMA``,
the averaged weights the optimizer's launch keeps next to the raw ones.  PyTorch is used for device memory, the stream, the dropout masks' random bits and
torch.distributed.  No CPU fallback.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .model import _GN_EPS, _GROUPS, _REG_HIDDEN, _REG_ITERS, PHDFor3DJoints, _round_up, expected_keys

DROPOUT_P = 0.5        # ResidualBlock(dropout=0.5), JointRegressor(dropout=0.5): src/model.py:39,87

# ---- the item table: (flat name, reference key, kind) in flat-buffer order ------------------------------------------------------
# kinds: "plain"    the reference tensor as it is;
#        "conv"     Conv1d weight (d, d, 3) <-> GEMM layout (d, 3d): column k*d + c multiplies x(t-2+k)[c];
#        "pad_cols" columns padded with zeros to a multiple of 64 (mlp0.w: K of the regressor's first Linear, ``_dp``);
#        "pad_rows" rows padded with zeros to a multiple of 64 (mlp5.w / mlp5.b: the last Linear's cout, ``_op``).
FlatItem = Tuple[str, str, str]


def block_items(prefix: str, order: Sequence[str] = ("gn1", "conv1", "gn2", "conv2")) -> List[FlatItem]:
    """One ResidualBlock's eight entries, its modules in ``order`` (phase 1 keeps gn1, gn2, conv1, conv2)."""
    items: List[FlatItem] = []
    for m in order:
        if m.startswith("gn"):
            items += [(f"{prefix}.{m}.g", f"{prefix}.{m}.weight", "plain"), (f"{prefix}.{m}.b", f"{prefix}.{m}.bias", "plain")]
        else:
            items += [(f"{prefix}.{m}.w", f"{prefix}.{m}.conv.weight", "conv"), (f"{prefix}.{m}.b", f"{prefix}.{m}.conv.bias", "plain")]
    return items


def regressor_items() -> List[FlatItem]:
    return [("mlp0.w", "f_3D.mlp.0.weight", "pad_cols"), ("mlp0.b", "f_3D.mlp.0.bias", "plain"),
            ("mlp3.w", "f_3D.mlp.3.weight", "plain"), ("mlp3.b", "f_3D.mlp.3.bias", "plain"),
            ("mlp5.w", "f_3D.mlp.5.weight", "pad_rows"), ("mlp5.b", "f_3D.mlp.5.bias", "pad_rows")]


def input_proj_items() -> List[FlatItem]:
    return [("input_proj.w", "input_proj.weight", "plain"), ("input_proj.b", "input_proj.bias", "plain")]


def _flat_shape(kind: str, ref: Tuple[int, ...]) -> Tuple[int, ...]:
    if kind == "conv":
        return (ref[0], 3 * ref[1])
    if kind == "pad_cols":
        return (ref[0], _round_up(ref[1], 64))
    if kind == "pad_rows":
        return (_round_up(ref[0], 64),) + tuple(ref[1:])
    return tuple(ref)


def _ref_view(kind: str, entry: torch.Tensor, ref: Tuple[int, ...]) -> torch.Tensor:
    """The part of a flat entry (in its flat shape) that holds the reference tensor, viewed in the reference's layout."""
    if kind == "conv":
        return entry.view(ref[0], 3, ref[1]).permute(0, 2, 1)
    if kind == "pad_cols":
        return entry[:, : ref[1]]
    if kind == "pad_rows":
        return entry[: ref[0]]
    return entry


def flat_layout(items: Sequence[FlatItem], ref_shapes: Dict[str, Tuple[int, ...]]) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(flat name, offset, flat shape) of every item, packed in order."""
    layout, off = [], 0
    for name, key, kind in items:
        shape = _flat_shape(kind, ref_shapes[key])
        n = int(torch.Size(shape).numel())
        assert n % 64 == 0
        layout.append((name, off, shape))
        off += n
    return layout


def _entries(items, ref_shapes, flat):
    for (name, key, kind), (_, off, shape) in zip(items, flat_layout(items, ref_shapes)):
        yield key, _ref_view(kind, flat[off: off + int(torch.Size(shape).numel())].view(shape), ref_shapes[key])


def unpack_flat(items: Sequence[FlatItem], ref_shapes: Dict[str, Tuple[int, ...]], flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    """A flat buffer under the reference's keys and layouts: new fp32 CPU tensors, the GEMM padding dropped."""
    return {key: torch.empty(ref_shapes[key], dtype=torch.float32).copy_(view) for key, view in _entries(items, ref_shapes, flat)}


def pack_flat(items: Sequence[FlatItem], ref_shapes: Dict[str, Tuple[int, ...]], named: Dict[str, torch.Tensor],
              flat: torch.Tensor) -> torch.Tensor:
    """Inverse of ``unpack_flat`` into ``flat`` (zeros on entry: the GEMM padding stays zero).  Returns ``flat``."""
    for key, view in _entries(items, ref_shapes, flat):
        t = named[key].detach().to(torch.float32)
        if tuple(t.shape) != tuple(view.shape):
            raise ValueError(f"{key}: shape {tuple(t.shape)}, expected {tuple(view.shape)}")
        view.copy_(t)
    return flat


def all_reduce_gradients(flat_grad: torch.Tensor, group=None) -> None:
    """Average the flat gradient buffer over the ranks: one all-reduce per step (RCCL over xGMI on GPUs; gloo in the CPU tests)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    world = dist.get_world_size(group)
    if world == 1:
        return
    dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=group)
    flat_grad.mul_(1.0 / world)


def sync_overflow_flag(found: torch.Tensor, group=None) -> None:
    """Make the skip decision of a data-parallel step GLOBAL: MAX-reduce the found-overflow flag over the ranks, so every
    replica skips (and backs its loss scale off) or steps together.  Needed because an fp16 overflow on ONE rank is a
    saturated 65504 -- finite -- so after the gradient all-reduce the averaged buffer is finite everywhere and only the
    overflowing rank's own arena check fires.  The reference's ``nn.DataParallel`` has one scaler and one optimizer
    (src/train.py:382-393) and cannot disagree with itself; this is the one-process-per-GPU equivalent."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    dist.all_reduce(found, op=dist.ReduceOp.MAX, group=group)


GRAD_NORM_MAX_PARTS = 2048        # r50_op_grad_norm never launches more workgroups than this (include/r50.h)


class WeightEMA:
    """Exponential moving average of a head's trainable parameters, in the flat layout: what
    ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay))`` keeps, ``ema += w * (p - ema)`` after every
    APPLIED optimizer step, computed inside the optimizer's launch (``r50_op_adamw_clip_ema``).  ``warmup``: the effective decay of
    update ``u`` (0-based) is min(decay, (1 + u) / (10 + u)), so early averages are not dominated by the initial weights.
    ``flat``: the averaged parameters (a clone of ``head.flat_master`` at construction); ``updates``: applied updates so far."""

    def __init__(self, head: "FlatTrainableHead", decay: float, warmup: bool = True):
        if not 0.0 < float(decay) < 1.0:
            raise ValueError(f"decay must lie in (0, 1), got {decay!r}")
        if head.flat_master is None:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') on the head first")
        self.head, self.decay, self.warmup = head, float(decay), bool(warmup)
        self.flat = head.flat_master.clone()
        self.updates = 0

    def weight(self) -> float:
        """The lerp weight of the next update, 1 - (effective decay): the host scalar handed to the kernel."""
        if not self.warmup:
            return 1.0 - self.decay
        return 1.0 - min(self.decay, (1.0 + self.updates) / (10.0 + self.updates))

    def state_dict(self) -> dict:
        """{"decay", "warmup", "updates", "model"}: ``model`` is ``head.state_dict()`` with the trainable entries from ``flat``."""
        model = {k: v.clone() for k, v in self.head._sd.items()}
        model.update(self.head.flat_to_reference(self.flat))
        return {"decay": self.decay, "warmup": self.warmup, "updates": self.updates, "model": model}

    def load_state_dict(self, state: dict) -> None:
        self.decay, self.warmup, self.updates = float(state["decay"]), bool(state["warmup"]), int(state["updates"])
        self.flat.copy_(self.head.flat_from_reference({n: state["model"][n] for n in self.head.trainable_parameter_names()}))


class _Arena:
    """Bump allocator for the backward pass's GEMM outputs: one 16-bit buffer, so ONE overflow check covers every gradient the matrix
    cores produced in a step (and nothing is allocated per step once the first step has sized it)."""

    def __init__(self, device, dtype):
        self.device, self.dtype = device, dtype
        self.chunks: List[torch.Tensor] = []
        self.used: List[int] = []

    def reset(self) -> None:
        total = sum(self.used)
        if len(self.chunks) != 1 or self.chunks[0].numel() < total:
            self.chunks = [torch.empty(max(total, 1 << 20), dtype=self.dtype, device=self.device)]
        self.used = [0]

    def take(self, rows: int, cols: int) -> torch.Tensor:
        n = _round_up(rows * cols, 64)
        if self.used[-1] + n > self.chunks[-1].numel():
            self.chunks.append(torch.empty(max(n, 1 << 22), dtype=self.dtype, device=self.device))
            self.used.append(0)
        o = self.used[-1]
        self.used[-1] = o + n
        return self.chunks[-1][o: o + rows * cols].view(rows, cols)


class FlatTrainableHead(PHDFor3DJoints):
    """``PHDFor3DJoints`` with the parameters of ``_flat_items()`` in flat fp32 master / 16-bit / gradient buffers (GEMM layout), and
    the launches of a lifting-head backward pass over them."""

    _no_transpose: frozenset = frozenset()         # trainable 16-bit weights no dX product reads
    _frozen_transposes: Tuple[str, ...] = ()       # frozen weights a dX product reads: transposed once at upload
    _clip_rule: Optional[Tuple[int, str]] = None   # (minimum clip length, the stage's wording in the error); None: any (B, T)

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 hallucinator: bool = False):
        super().__init__(latent_dim, joints_num, number_blocks, precision, hallucinator)
        self.flat_master: Optional[torch.Tensor] = None
        self._layout: List[Tuple[str, int, Tuple[int, ...]]] = []
        self.last_losses: Dict[str, float] = {}
        self._ref_shapes = expected_keys(self.latent_dim, self.joints_num, self.number_blocks, self.hallucinator)

    # ---- what a subclass says ---------------------------------------------------------------------
    def _flat_items(self) -> List[FlatItem]:
        raise NotImplementedError

    def trainable_parameter_names(self) -> List[str]:
        """The names of the optimizer's parameters, in its numbering."""
        raise NotImplementedError

    def _dropout_sites(self) -> List[Tuple[str, int]]:
        """(mask name, columns) of the dropout sites of one step, in draw order."""
        raise NotImplementedError

    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    # ---- flat parameter buffers (GEMM layout) -------------------------------------------------
    def _upload(self) -> None:
        super()._upload()                      # y0, the frozen weights and everything eval() needs; trainable entries are re-pointed below
        dev, d = self._device, self.latent_dim
        items = self._flat_items()
        self._layout = flat_layout(items, self._ref_shapes)
        total = self._layout[-1][1] + int(torch.Size(self._layout[-1][2]).numel())
        self.flat_master = pack_flat(items, self._ref_shapes, self._sd, torch.zeros(total, dtype=torch.float32)).to(dev)
        self.flat_w16 = self.flat_master.to(self._dtype)
        self.flat_grad = torch.zeros_like(self.flat_master)
        self._off = {name: (o_, shape) for name, o_, shape in self._layout}
        for name, o_, shape in self._layout:       # weights: the 16-bit copy; biases and GroupNorm parameters: the fp32 master itself
            n = int(torch.Size(shape).numel())
            src = self.flat_w16 if name.endswith(".w") else self.flat_master
            self._dev[name] = src[o_: o_ + n].view(shape)
        self._wt: Dict[str, torch.Tensor] = {}     # transposed 16-bit weights for the dX products
        self._transpose_weights(self._frozen_transposes)
        self._transposed = [name for name, _, _ in self._layout if name.endswith(".w") and name not in self._no_transpose]
        self._refresh_transposes()
        self._zero_bias = torch.zeros(max(3 * d, 2048, self._dp, _REG_HIDDEN), dtype=torch.float32, device=dev)
        self._found = torch.zeros(1, dtype=torch.int32, device=dev)
        self._arena = _Arena(dev, self._dtype)
        # r50_op_grad_norm's buffers (section S; read only when clipping is on): per-workgroup partial sums, {coef, norm}, the statistics
        self._norm_part = torch.zeros(GRAD_NORM_MAX_PARTS, dtype=torch.float64, device=dev)
        self._clip2 = torch.ones(2, dtype=torch.float32, device=dev)
        self._stats4 = torch.zeros(4, dtype=torch.float64, device=dev)

    def _transpose_weights(self, names: Sequence[str]) -> None:
        lib = _lib.load_library()
        for name in names:
            n, k = self._dev[name].shape
            if name not in self._wt:                   # (k, n) with row stride n: the transpose writes every element
                self._wt[name] = torch.empty((k, n), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_transpose16(self._dev[name].data_ptr(), n, k, self._wt[name].data_ptr(), n, self._stream()), None,
                       "r50_op_transpose16")

    def _refresh_transposes(self) -> None:
        """The transposes of the trainable weights, after an optimizer step changed them."""
        self._transpose_weights(self._transposed)

    def refresh_weights16(self) -> None:
        """The 16-bit weights and their transposes from ``flat_master`` (after its values were replaced from outside)."""
        self.flat_w16.copy_(self.flat_master.to(self._dtype))
        self._refresh_transposes()

    @contextlib.contextmanager
    def swapped_weights(self, flat: torch.Tensor):
        """Run the body on the weights of ``flat`` (a buffer in the flat parameter layout, e.g. ``WeightEMA.flat``): the contents of
        ``flat_master`` and ``flat`` are exchanged and the 16-bit weights and transposes refreshed; on exit they are exchanged back and
        refreshed again.  The exchanges are exact copies, so the raw master returns bit for bit."""
        if flat.shape != self.flat_master.shape or flat.dtype != torch.float32 or flat.device != self.flat_master.device:
            raise ValueError("swapped_weights: expected an fp32 buffer in the flat parameter layout on the head's device")

        def exchange():
            keep = self.flat_master.clone()
            self.flat_master.copy_(flat)
            flat.copy_(keep)
            self.refresh_weights16()
        exchange()
        try:
            yield self
        finally:
            exchange()

    def clip_stats(self, reset: bool = True) -> Dict[str, float]:
        """What ``r50_op_grad_norm`` counted over the applied steps since the last reset (one host read; call it once per epoch):
        ``grad_norm_mean`` and ``grad_norm_max`` of the unclipped global norm, ``clipped_frac`` = the share of steps with coef < 1,
        ``steps``.  Skipped steps are not counted."""
        steps, clipped, norm_sum, norm_max = self._stats4.tolist()
        if reset:
            self._stats4.zero_()
        return {"grad_norm_mean": norm_sum / max(steps, 1.0), "grad_norm_max": norm_max, "clipped_frac": clipped / max(steps, 1.0),
                "steps": int(steps)}

    def flat_to_reference(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """A buffer in the flat parameter layout (master, gradient, AdamW moments) under the reference's names and layouts of the
        trainable parameters (fp32, CPU), in ``trainable_parameter_names()`` order; the GEMM padding is dropped."""
        out = unpack_flat(self._flat_items(), self._ref_shapes, flat)
        return {n: out[n] for n in self.trainable_parameter_names()}

    def flat_from_reference(self, named: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Inverse of ``flat_to_reference``: a new device buffer in the flat layout, zero in the GEMM padding."""
        return pack_flat(self._flat_items(), self._ref_shapes, named, torch.zeros_like(self.flat_master))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's keys and layouts (fp32, CPU): the trainable entries from the flat master buffer, the others as loaded."""
        out = {k: v.clone() for k, v in self._sd.items()}
        out.update(self.flat_to_reference(self.flat_master))
        return out

    def named_gradients(self) -> Dict[str, torch.Tensor]:
        """flat_grad under the reference's parameter names and layouts (fp32, CPU): what ``p.grad`` holds after ``backward()``."""
        return self.flat_to_reference(self.flat_grad)

    def grad_view(self, name: str) -> torch.Tensor:
        o_, shape = self._off[name]
        return self.flat_grad[o_: o_ + int(torch.Size(shape).numel())].view(shape)

    def make_dropout_masks(self, b: int, t: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """Byte keep-masks (1 = keep, probability 1 - p), (B*T, columns), for the sites of ``_dropout_sites()``, drawn in its order."""
        return {name: (torch.rand(b * t, cols, device=self._device, generator=generator) >= DROPOUT_P).to(torch.uint8)
                for name, cols in self._dropout_sites()}

    def _check_batch(self, feats: torch.Tensor, joints3d: torch.Tensor) -> Tuple[int, int]:
        if self.flat_master is None:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') first")
        if feats.dim() != 3 or feats.shape[-1] != 2048 or feats.device != self._device:
            raise ValueError("feats: expected (B,T,2048) on the head's device")
        b, t, _ = feats.shape
        if tuple(joints3d.shape) != (b, t, self.joints_num, 3) or joints3d.device != self._device:
            raise ValueError("joints3d: expected (B,T,J,3) on the head's device")
        if self._clip_rule is not None and (b < 1 or t < self._clip_rule[0]):
            raise ValueError(f"{self._clip_rule[1]} needs clips of at least {self._clip_rule[0]} frames (frame 0 has no prediction)")
        return b, t

    # ---- launch helpers -----------------------------------------------------------------------
    def _mm(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """x (R, K) @ w (N, K)^T -> (R, N), 16-bit out, fp32 accumulation, no bias: one igemm launch."""
        rows, k = x.shape
        n = w.shape[0]
        assert w.shape[1] == k and x.is_contiguous() and w.is_contiguous() and k % 64 == 0 and n % 64 == 0
        y = self._arena.take(rows, n)
        lib = _lib.load_library()
        fn = lib.r50_op_conv2d_f16 if self._et else lib.r50_op_conv2d
        _lib.check(fn(x.data_ptr(), rows, 1, 1, k, w.data_ptr(), self._zero_bias.data_ptr(), None, y.data_ptr(), n, 1, 1, 0, 0, 0,
                      self._stream()), None, "r50_op_conv2d (lifting head backward)")
        return y

    def _t(self, x: torch.Tensor) -> torch.Tensor:
        """(R, C) -> (C, Rp) transposed, Rp = R rounded up to 64 with zero padding (the K of a dW product)."""
        rows, cols = x.shape
        rp = _round_up(rows, 64)
        out = torch.zeros((cols, rp), dtype=self._dtype, device=self._device) if rp != rows else \
            torch.empty((cols, rp), dtype=self._dtype, device=self._device)
        _lib.check(_lib.load_library().r50_op_transpose16(x.data_ptr(), rows, cols, out.data_ptr(), rp, self._stream()), None,
                   "r50_op_transpose16")
        return out

    def _wgrad(self, name: str, dy: torch.Tensor, x: torch.Tensor, inv_scale: float, accumulate: bool, bias: Optional[str] = None) -> None:
        """flat_grad[name] (N, K) [+]= inv_scale * dy (R, N)^T x (R, K); flat_grad[bias] (N) [+]= inv_scale * column sums of dy."""
        dw = self._mm(self._t(dy), self._t(x))                    # (N, Rp) @ (K, Rp)^T -> (N, K)
        gv = self.grad_view(name)
        assert tuple(dw.shape) == tuple(gv.shape)
        _lib.check(_lib.load_library().r50_op_grad_accum(dw.data_ptr(), inv_scale, gv.data_ptr(), dw.numel(), int(accumulate), self._et,
                                                          self._stream()), None, "r50_op_grad_accum")
        if bias is not None:
            self._bias_grad(dy, self.grad_view(bias), inv_scale, accumulate)

    def _bias_grad(self, dy: torch.Tensor, gb: torch.Tensor, inv_scale: float, accumulate: bool) -> None:
        _lib.check(_lib.load_library().r50_op_colsum(dy.data_ptr(), dy.shape[0], dy.shape[1], dy.shape[1], inv_scale, gb.data_ptr(),
                                                      int(accumulate), self._et, self._stream()), None, "r50_op_colsum")

    def _mask_scale(self, x: torch.Tensor, mask: torch.Tensor, scale: float) -> None:
        assert mask.dtype == torch.uint8 and mask.numel() == x.numel() and mask.is_contiguous()
        _lib.check(_lib.load_library().r50_op_mask_scale(x.data_ptr(), mask.data_ptr(), scale, x.numel(), self._et, self._stream()), None,
                   "r50_op_mask_scale")

    def _relu_bwd(self, dy: torch.Tensor, act: torch.Tensor, scale: float) -> None:
        _lib.check(_lib.load_library().r50_op_relu_bwd(dy.data_ptr(), act.data_ptr(), scale, dy.numel(), self._et, self._stream()), None,
                   "r50_op_relu_bwd")

    def _gn_bwd(self, dr: torch.Tensor, x: torch.Tensor, b: int, t: int, prefix: str, add: Optional[torch.Tensor], inv_scale: float,
                t0: Optional[int] = None, accumulate: bool = False) -> torch.Tensor:
        """GroupNorm + ReLU + causal-rows backward: dx (b*t, D); the GroupNorm parameter gradients [+]= into flat_grad.  ``t0`` None:
        batch-major rows (``r50_op_gn_relu_causal3_bwd``); else time-major rows of which ``dr`` holds frames t0 .. t-1
        (``r50_op_gn_relu_causal3_tm_bwd``)."""
        d = self.latent_dim
        lib = _lib.load_library()
        dx = torch.empty((b * t, d), dtype=self._dtype, device=self._device)
        part = torch.empty((2, b, d), dtype=torch.float32, device=self._device)
        g, beta, add_p = self._dev[prefix + ".g"].data_ptr(), self._dev[prefix + ".b"].data_ptr(), add.data_ptr() if add is not None else None
        if t0 is None:
            _lib.check(lib.r50_op_gn_relu_causal3_bwd(dr.data_ptr(), x.data_ptr(), b, t, d, _GROUPS, g, beta, _GN_EPS, add_p, dx.data_ptr(),
                                                      part[0].data_ptr(), part[1].data_ptr(), self._et, self._stream()), None,
                       "r50_op_gn_relu_causal3_bwd")
        else:
            _lib.check(lib.r50_op_gn_relu_causal3_tm_bwd(dr.data_ptr(), x.data_ptr(), b, t, t0, d, _GROUPS, g, beta, _GN_EPS, add_p,
                                                         dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), self._et, self._stream()),
                       None, "r50_op_gn_relu_causal3_tm_bwd")
        for j, suffix in ((0, ".g"), (1, ".b")):
            _lib.check(lib.r50_op_colsum_f32(part[j].data_ptr(), b, d, inv_scale, self.grad_view(prefix + suffix).data_ptr(),
                                             int(accumulate), self._stream()), None, "r50_op_colsum_f32")
        return dx

    def _check_arena(self) -> None:
        """Raise ``_found`` if any 16-bit gradient the GEMMs (and the latent kernels) wrote into the arena overflowed."""
        lib = _lib.load_library()
        for chunk, used in zip(self._arena.chunks, self._arena.used):
            if used:
                _lib.check(lib.r50_op_check_overflow16(chunk.data_ptr(), used, self._found.data_ptr(), self._et, self._stream()), None,
                           "r50_op_check_overflow16")

    # ---- the batch-major pieces of a step ---------------------------------------------------------
    def _blocks_forward_saved(self, net: str, nb: int, x: torch.Tensor, b: int, t: int, masks: Optional[Dict[str, torch.Tensor]],
                              keep_scale: float, out_last: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[tuple]]:
        """``nb`` residual blocks of ``net`` over x (B*T, D), dropout after conv1 where ``masks`` has the block; the last block's conv2
        stores into ``out_last`` if given.  Returns (output, per block (input, gn1 rows, conv1 output, gn2 rows, mask))."""
        saved = []
        for i in range(nb):
            p = f"{net}.blocks.{i}"
            r1 = self._gn_relu_rows(x, b, t, p + ".gn1")
            h = self._gemm(r1, p + ".conv1", relu=False)
            m = masks[p] if masks is not None else None
            if m is not None:
                self._mask_scale(h, m, keep_scale)
            r2 = self._gn_relu_rows(h, b, t, p + ".gn2")
            xo = self._gemm(r2, p + ".conv2", relu=False, residual=x, out=out_last if i == nb - 1 else None)
            saved.append((x, r1, h, r2, m))
            x = xo
        return x, saved

    def _block_backward(self, p: str, saved: tuple, dx: torch.Tensor, b: int, t: int, inv: float, keep_scale: float) -> torch.Tensor:
        """The backward of one block of ``_blocks_forward_saved`` (``saved``: its tuple), weight gradients into flat_grad.  Returns
        d/d(the block's input).  The walk over the blocks, last first, stays a loop at the call site: a callee that walked them would
        pin the incoming ``dx`` through its caller's reference for the whole walk, B*T*D 16-bit elements more at the step's peak."""
        xin, r1, h, r2, m = saved
        self._wgrad(p + ".conv2.w", dx, r2, inv, False, bias=p + ".conv2.b")
        dr2 = self._mm(dx, self._wt[p + ".conv2.w"])                   # (rows, 3D)
        dh = self._gn_bwd(dr2, h, b, t, p + ".gn2", None, inv)
        if m is not None:
            self._mask_scale(dh, m, keep_scale)
        self._wgrad(p + ".conv1.w", dh, r1, inv, False, bias=p + ".conv1.b")
        dr1 = self._mm(dh, self._wt[p + ".conv1.w"])
        return self._gn_bwd(dr1, xin, b, t, p + ".gn1", dx, inv)       # + the skip connection's gradient

    def _regressor_backward(self, reg: List[tuple], dyacc: torch.Tensor, rows: int, inv: float, relu1_scale: float,
                            weights: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """The regressor's backward, last iteration first, from ``dyacc`` (rows, J*3) fp32 = the loss gradient (it accumulates each
        iteration's d/dy on the way).  ``reg``: per iteration (input, first hidden, second hidden) of the forward (the input is read
        for the weight gradients only).  ``relu1_scale``: the dropout's keep scale behind the first ReLU, or 1.  ``weights``: also
        the three Linears' gradients into flat_grad.  Returns d/d(strips) (rows, D) fp32, summed over the iterations, and the 16-bit
        buffer the iterations cast ``dyacc`` into: the caller holds it to the end of its step, so the step's memory is as it always was."""
        lib = _lib.load_library()
        d, o = self.latent_dim, self.out_dim
        dphi = torch.zeros((rows, d), dtype=torch.float32, device=self._device)
        g5 = torch.empty((rows, self._op), dtype=self._dtype, device=self._device)
        for i in reversed(range(_REG_ITERS)):
            inp, h1, h2 = reg[i]
            acc = i < _REG_ITERS - 1
            _lib.check(lib.r50_op_cast_rows(dyacc.data_ptr(), rows, o, g5.data_ptr(), self._op, self._et, self._stream()), None, "r50_op_cast_rows")
            if weights:
                self._wgrad("mlp5.w", g5, h2, inv, acc, bias="mlp5.b")
            dh2 = self._mm(g5, self._wt["mlp5.w"])                         # (rows, H)
            self._relu_bwd(dh2, h2, 1.0)
            if weights:
                self._wgrad("mlp3.w", dh2, h1, inv, acc, bias="mlp3.b")
            dh1 = self._mm(dh2, self._wt["mlp3.w"])
            self._relu_bwd(dh1, h1, relu1_scale)
            if weights:
                self._wgrad("mlp0.w", dh1, inp, inv, acc, bias="mlp0.b")
            dinp = self._mm(dh1, self._wt["mlp0.w"])                       # (rows, Dp) = [dstrip | dy | 0]
            _lib.check(lib.r50_op_add_rows(dphi.data_ptr(), d, dinp.data_ptr(), self._dp, rows, self._et, self._stream()), None, "r50_op_add_rows")
            if i > 0:                                                      # after iteration 0 nothing reads dyacc again
                _lib.check(lib.r50_op_add_rows(dyacc.data_ptr(), o, dinp.data_ptr() + 2 * d, self._dp, rows, self._et, self._stream()), None,
                           "r50_op_add_rows")
        return dphi, g5

    # ---- the tail of a step -----------------------------------------------------------------------
    def _finish_step(self, optim, scaler, group) -> bool:
        """From the gradient all-reduce to the scale update: average ``flat_grad`` over the ranks, raise the flag on a non-finite
        entry, agree on it over the ranks, read it (the reference's scaler.step() synchronises on the same flag), apply AdamW and
        refresh the transposes unless it is raised, update the loss scale.  Returns the flag: True = the step was skipped.
        With ``optim.max_grad_norm`` set, one ``r50_op_grad_norm`` call takes the finite check's place: the same read of ``flat_grad``
        also gives the global L2 norm and the clip coefficient ``optim.step`` applies (after the all-reduce, so every rank computes the
        same bits).  ``flat_grad`` keeps the UNCLIPPED gradient."""
        with torch.cuda.device(self._device):
            all_reduce_gradients(self.flat_grad, group)
            max_norm = getattr(optim, "max_grad_norm", None)
            if max_norm is None:
                _lib.check(_lib.load_library().r50_op_check_finite(self.flat_grad.data_ptr(), self.flat_grad.numel(), self._found.data_ptr(),
                                                                    self._stream()), None, "r50_op_check_finite")
            else:
                _lib.check(_lib.load_library().r50_op_grad_norm(self.flat_grad.data_ptr(), self.flat_grad.numel(), float(max_norm),
                                                                 self._norm_part.data_ptr(), self._norm_part.numel(), self._found.data_ptr(),
                                                                 self._clip2.data_ptr(), self._stats4.data_ptr(), self._stream()), None,
                           "r50_op_grad_norm")
            sync_overflow_flag(self._found, group)        # any rank overflowed -> every rank skips this step
            found = bool(self._found.item())
            if not found:
                optim.step(self._found)
                self._refresh_transposes()
            if scaler is not None:
                scaler.update(found)
        return found
