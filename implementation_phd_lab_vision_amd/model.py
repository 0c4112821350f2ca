"""Host-side mirror of the reference's lifting head for the MI355X path, forward / inference only.

The reference builds and calls it as (src/train.py:370, src/model.py:127-178)::

    model = PHD(latent_dim=1024, joints_num=17, number_blocks=2)
    phi, phi_hat, joints_phi, joints_hat = model(feats, predict_future=True)        # feats (B,T,2048)

``PHDFor3DJoints`` keeps that surface (constructor arguments, ``load_state_dict`` with the reference's keys, ``.to(device)``,
``.eval()``, ``__call__`` returning the same 4-tuple of fp32 tensors) and routes the arithmetic to libr50hip.so:

* every ``nn.Linear`` (input_proj :143, the regressor's MLP :95-102) and every ``CausalConv1d`` (:20-35) is one launch of the
  implicit-GEMM MFMA kernel (``r50_op_conv2d_f16`` / ``r50_op_conv2d``) as a 1x1 convolution over the B*T rows.  A causal
  conv1d with kernel 3 and replicate left padding is a GEMM with K = 3*C against the row [x(t-2) | x(t-1) | x(t)], indices
  clamped at 0; its weight (C_out, C_in, 3) is repacked once to (C_out, 3*C_in) in that order.  Bias, ReLU and the residual
  add (:57) are the kernel's fused epilogue;
* GroupNorm(32) + ReLU (:47-55) and the construction of those rows are one kernel (``r50_op_gn_relu_causal3``);
* ``torch.cat([phi, y])`` (:113) and ``y = y + dy`` (:114-115) are ``r50_op_concat_pad`` / ``r50_op_add_rows`` (y stays fp32).

Element type: IEEE half by default -- the reference runs the head under ``torch.autocast(dtype=torch.float16)`` on the GPU
(src/train.py:154); ``precision="bf16"`` selects bf16.  Accumulation is fp32.  Dropout is identity (eval mode); there is no
backward pass here, so ``.train()`` raises.  PyTorch is used for device memory, the stream and the phi_hat shift (a copy).
No fallback: without the shared library or a gfx950 GPU the calls raise.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

_GROUPS = 32           # ResidualBlock(groups=32), src/model.py:39
_GN_EPS = 1e-5         # nn.GroupNorm default
_AR_BLOCKS = 3         # CausalTemporalNet(latent_dim) default num_blocks, src/model.py:69,141
_REG_ITERS = 3         # JointRegressor(iters=3), src/model.py:87
_REG_HIDDEN = 1024


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


HAL_KEYS = ("f_hal.fc1.weight", "f_hal.fc1.bias", "f_hal.fc2.weight", "f_hal.fc2.bias")      # Hallucinator's parameters, in registration order


def has_hallucinator(state_keys) -> bool:
    """Whether a state dict (or any collection of its keys) carries the hallucinator f_hal."""
    return HAL_KEYS[0] in state_keys


def expected_keys(latent_dim: int, joints_num: int, number_blocks: int, hallucinator: bool = False) -> Dict[str, Tuple[int, ...]]:
    """state-dict keys and shapes of the reference module (src/model.py:127-143); with ``hallucinator`` also f_hal's four
    (section V: ``model.f_hal = Hallucinator(latent_dim)``, registered after the reference's modules)."""
    d, o = latent_dim, joints_num * 3
    keys: Dict[str, Tuple[int, ...]] = {"input_proj.weight": (d, 2048), "input_proj.bias": (d,)}
    for net, nb in (("f_movie", number_blocks), ("f_AR", _AR_BLOCKS)):
        for i in range(nb):
            p = f"{net}.blocks.{i}"
            for gn in ("gn1", "gn2"):
                keys[f"{p}.{gn}.weight"] = (d,)
                keys[f"{p}.{gn}.bias"] = (d,)
            for cv in ("conv1", "conv2"):
                keys[f"{p}.{cv}.conv.weight"] = (d, d, 3)
                keys[f"{p}.{cv}.conv.bias"] = (d,)
    keys["f_3D.y0"] = (o,)
    keys["f_3D.mlp.0.weight"] = (_REG_HIDDEN, d + o)
    keys["f_3D.mlp.0.bias"] = (_REG_HIDDEN,)
    keys["f_3D.mlp.3.weight"] = (_REG_HIDDEN, _REG_HIDDEN)
    keys["f_3D.mlp.3.bias"] = (_REG_HIDDEN,)
    keys["f_3D.mlp.5.weight"] = (o, _REG_HIDDEN)
    keys["f_3D.mlp.5.bias"] = (o,)
    if hallucinator:
        for fc in ("fc1", "fc2"):
            keys[f"f_hal.{fc}.weight"] = (d, d)
            keys[f"f_hal.{fc}.bias"] = (d,)
    return keys


def checked_window_starts(starts, src_rows: int, t: int) -> np.ndarray:
    """``starts`` (a host sequence or a 1-D integer tensor, read back if it lives on the device) as a contiguous int32 host array, after
    the check ``r50_op_gather_window_rows`` leaves to its caller: at least one start, ``1 <= t <= src_rows`` and every start in
    ``[0, src_rows - t]``.  Raises ValueError otherwise; touches neither the library nor the GPU when ``starts`` is on the host."""
    host = starts.detach().cpu().numpy() if isinstance(starts, torch.Tensor) else np.asarray(starts)
    if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
        raise ValueError(f"starts must be a non-empty 1-D integer sequence, got {host.dtype} {host.shape}")
    if not 1 <= int(t) <= int(src_rows):
        raise ValueError(f"need 1 <= t <= src_rows (got t={t}, src_rows={src_rows})")
    lo, hi = int(host.min()), int(host.max())
    if lo < 0 or hi > int(src_rows) - int(t):
        raise ValueError(f"every start must lie in [0, {int(src_rows) - int(t)}] (windows of {t} rows in {src_rows}), got [{lo}, {hi}]")
    return np.ascontiguousarray(host, dtype=np.int32)


def gather_window_rows(src: torch.Tensor, starts, t: int, dtype: torch.dtype = torch.float16,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``r50_op_gather_window_rows`` launch: ``src`` (N, C) fp32 on an MI355X, ``starts`` B window starts (host sequence or int32
    device tensor) -> (B*t, C) ``dtype`` (fp16 or bf16), row ``w*t + i`` = the cast of ``src[starts[w] + i]``: the bits of
    ``r50_op_cast_rows`` on ``src[idx]`` without that fp32 intermediate.  The starts are checked on the host before anything else
    (the kernel trusts them): a device tensor of starts is read back for that, one blocking device-to-host copy per call, so pass a host
    sequence where the starts are known on the host.  ``out``: an optional contiguous (B*t, C) destination.  There is no CPU fallback."""
    if src.dim() != 2 or src.dtype != torch.float32:
        raise ValueError(f"src must be (N, C) fp32, got {tuple(src.shape)} {src.dtype}")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    n, c = int(src.shape[0]), int(src.shape[1])
    if c < 8 or c % 8:
        raise ValueError(f"C must be a positive multiple of 8, got {c}")
    host = checked_window_starts(starts, n, t)
    b, t = int(host.size), int(t)
    if not src.is_cuda or not src.is_contiguous():
        raise ValueError("src must be contiguous on the GPU: there is no CPU fallback")
    dev_starts = starts if isinstance(starts, torch.Tensor) and starts.device == src.device and starts.dtype == torch.int32 \
        and starts.is_contiguous() else torch.from_numpy(host).to(src.device)
    if out is None:
        out = torch.empty((b * t, c), dtype=dtype, device=src.device)
    elif tuple(out.shape) != (b * t, c) or out.dtype != dtype or out.device != src.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({b * t}, {c}) {dtype} tensor on {src.device}")
    with torch.cuda.device(src.device):
        rc = _lib.load_library().r50_op_gather_window_rows(src.data_ptr(), n, c, dev_starts.data_ptr(), b, t, out.data_ptr(),
                                                           1 if dtype == torch.float16 else 0,
                                                           torch.cuda.current_stream(src.device).cuda_stream)
    _lib.check(rc, None, "r50_op_gather_window_rows")
    return out


class PHDFor3DJoints:
    """``PHDFor3DJoints(latent_dim, joints_num, number_blocks)`` of src/model.py in eval mode on one MI355X."""

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 hallucinator: bool = False):
        if latent_dim % 64 or latent_dim % _GROUPS:
            raise ValueError("latent_dim must be a multiple of 64 (GEMM granularity) and of 32 (GroupNorm groups)")
        if precision not in ("fp16", "bf16"):
            raise ValueError("precision must be 'fp16' or 'bf16'")
        self.latent_dim = int(latent_dim)
        self.joints_num = int(joints_num)
        self.number_blocks = int(number_blocks)
        self.out_dim = self.joints_num * 3
        self.hallucinator = bool(hallucinator)                 # f_hal (section V): four more keys, ``hallucinate`` / ``hallucinated_rollout``
        self._et = 1 if precision == "fp16" else 0
        self._dtype = torch.float16 if precision == "fp16" else torch.bfloat16
        self._sd: Optional[Dict[str, torch.Tensor]] = None
        self._dev: Dict[str, torch.Tensor] = {}
        self._device: Optional[torch.device] = None
        self.training = False

    # ---- nn.Module-like surface -------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        want = expected_keys(self.latent_dim, self.joints_num, self.number_blocks, self.hallucinator)
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in want]
        if missing or (strict and unexpected):
            raise KeyError(f"load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                           f"unexpected {unexpected[:4]}{'...' if len(unexpected) > 4 else ''}")
        for k, shape in want.items():
            if tuple(state_dict[k].shape) != shape:
                raise ValueError(f"load_state_dict: {k} has shape {tuple(state_dict[k].shape)}, expected {shape}")
        self._sd = {k: state_dict[k].detach().to("cpu", torch.float32).contiguous() for k in want}
        if self._device is not None:
            self._upload()
        return self

    def to(self, device) -> "PHDFor3DJoints":
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.R50Error(f"PHDFor3DJoints runs on an MI355X only (got device '{device}'); "
                                "there is no CPU fallback in the product path")
        _lib.load_library()
        index = device.index if device.index is not None else torch.cuda.current_device()
        self._device = torch.device("cuda", index)
        if self._sd is not None:
            self._upload()
        return self

    def eval(self) -> "PHDFor3DJoints":
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise _lib.R50Error("PHDFor3DJoints here is the forward pass only (eval mode); training is not implemented")
        return self

    # ---- weights: repacked once, GEMM-ready --------------------------------------------------
    def _upload(self) -> None:
        sd, dev, dt = self._sd, self._device, self._dtype
        d, o = self.latent_dim, self.out_dim
        w: Dict[str, torch.Tensor] = {}

        def elem(t):
            return t.to(dt).contiguous().to(dev)

        def f32(t):
            return t.to(torch.float32).contiguous().to(dev)

        w["input_proj.w"] = elem(sd["input_proj.weight"])                        # (D, 2048) = (cout, 1, 1, cin)
        w["input_proj.b"] = f32(sd["input_proj.bias"])
        for net, nb in (("f_movie", self.number_blocks), ("f_AR", _AR_BLOCKS)):
            for i in range(nb):
                p = f"{net}.blocks.{i}"
                for gn in ("gn1", "gn2"):
                    w[f"{p}.{gn}.g"] = f32(sd[f"{p}.{gn}.weight"])
                    w[f"{p}.{gn}.b"] = f32(sd[f"{p}.{gn}.bias"])
                for cv in ("conv1", "conv2"):
                    # (cout, cin, k) -> (cout, k, cin): column k*D + c multiplies x(t-2+k)[c]
                    w[f"{p}.{cv}.w"] = elem(sd[f"{p}.{cv}.conv.weight"].permute(0, 2, 1).reshape(d, 3 * d))
                    w[f"{p}.{cv}.b"] = f32(sd[f"{p}.{cv}.conv.bias"])
        self._dp = _round_up(d + o, 64)                                          # K of the regressor's first Linear
        self._op = _round_up(o, 64)                                              # its last Linear's cout
        w0 = torch.zeros(_REG_HIDDEN, self._dp)
        w0[:, : d + o] = sd["f_3D.mlp.0.weight"]
        w5 = torch.zeros(self._op, _REG_HIDDEN)
        w5[:o] = sd["f_3D.mlp.5.weight"]
        b5 = torch.zeros(self._op)
        b5[:o] = sd["f_3D.mlp.5.bias"]
        w["mlp0.w"], w["mlp0.b"] = elem(w0), f32(sd["f_3D.mlp.0.bias"])
        w["mlp3.w"], w["mlp3.b"] = elem(sd["f_3D.mlp.3.weight"]), f32(sd["f_3D.mlp.3.bias"])
        w["mlp5.w"], w["mlp5.b"] = elem(w5), f32(b5)
        w["y0"] = f32(sd["f_3D.y0"])
        if self.hallucinator:                                                    # (D, D) = (cout, 1, 1, cin), as input_proj
            for fc in ("fc1", "fc2"):
                w[f"f_hal.{fc}.w"] = elem(sd[f"f_hal.{fc}.weight"])
                w[f"f_hal.{fc}.b"] = f32(sd[f"f_hal.{fc}.bias"])
        self._dev = w

    # ---- launches ---------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self._device).cuda_stream

    def _gemm(self, x: torch.Tensor, wname: str, relu: bool, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """rows (R, K) element @ W (cout, K)^T + bias [+ residual] [ReLU] -> (R, cout) element: a 1x1 convolution over R pixels.
        ``out``: a contiguous (R, cout) view to store into (the rollout's append), else a new tensor."""
        wt, b = self._dev[wname + ".w"], self._dev[wname + ".b"]
        rows, k = x.shape
        cout = wt.shape[0]
        assert wt.shape[1] == k and x.is_contiguous()
        if out is None:
            y = torch.empty((rows, cout), dtype=self._dtype, device=self._device)
        else:
            assert out.is_contiguous() and tuple(out.shape) == (rows, cout) and out.dtype == self._dtype
            y = out
        lib = _lib.load_library()
        fn = lib.r50_op_conv2d_f16 if self._et else lib.r50_op_conv2d
        rc = fn(x.data_ptr(), rows, 1, 1, k, wt.data_ptr(), b.data_ptr(), residual.data_ptr() if residual is not None else None,
                y.data_ptr(), cout, 1, 1, 0, int(relu), 0, self._stream())
        _lib.check(rc, None, "r50_op_conv2d (lifting head)")
        return y

    def _gn_relu_rows(self, x: torch.Tensor, b: int, t: int, prefix: str) -> torch.Tensor:
        d = self.latent_dim
        out = torch.empty((b * t, 3 * d), dtype=self._dtype, device=self._device)
        rc = _lib.load_library().r50_op_gn_relu_causal3(x.data_ptr(), b, t, d, _GROUPS, self._dev[prefix + ".g"].data_ptr(),
                                                        self._dev[prefix + ".b"].data_ptr(), _GN_EPS, out.data_ptr(), self._et,
                                                        self._stream())
        _lib.check(rc, None, "r50_op_gn_relu_causal3")
        return out

    def _gn_relu_rows_tm(self, x: torch.Tensor, b: int, t: int, t0: int, prefix: str) -> torch.Tensor:
        """``_gn_relu_rows`` on a time-major x (t*b, D), emitting the rows of frames t0 .. t-1 only: ((t-t0)*b, 3D), time-major."""
        d = self.latent_dim
        out = torch.empty(((t - t0) * b, 3 * d), dtype=self._dtype, device=self._device)
        rc = _lib.load_library().r50_op_gn_relu_causal3_tm(x.data_ptr(), b, t, t0, d, _GROUPS, self._dev[prefix + ".g"].data_ptr(),
                                                           self._dev[prefix + ".b"].data_ptr(), _GN_EPS, out.data_ptr(), self._et,
                                                           self._stream())
        _lib.check(rc, None, "r50_op_gn_relu_causal3_tm")
        return out

    def _temporal_net(self, x: torch.Tensor, b: int, t: int, net: str, nb: int) -> torch.Tensor:   # CausalTemporalNet, :69-78
        for i in range(nb):
            p = f"{net}.blocks.{i}"
            h = self._gemm(self._gn_relu_rows(x, b, t, p + ".gn1"), p + ".conv1", relu=False)
            x = self._gemm(self._gn_relu_rows(h, b, t, p + ".gn2"), p + ".conv2", relu=False, residual=x)
        return x

    def _regressor(self, phi: torch.Tensor, b: int, t: int) -> torch.Tensor:                       # JointRegressor.forward, :104-126
        rows, d, o = b * t, self.latent_dim, self.out_dim
        lib = _lib.load_library()
        y = self._dev["y0"].view(1, o).expand(rows, o).contiguous()
        inp = torch.empty((rows, self._dp), dtype=self._dtype, device=self._device)
        for _ in range(_REG_ITERS):
            _lib.check(lib.r50_op_concat_pad(phi.data_ptr(), d, y.data_ptr(), o, rows, inp.data_ptr(), self._dp, self._et,
                                             self._stream()), None, "r50_op_concat_pad")
            h = self._gemm(inp, "mlp0", relu=True)
            h = self._gemm(h, "mlp3", relu=True)
            dy = self._gemm(h, "mlp5", relu=False)
            _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows, self._et, self._stream()), None,
                       "r50_op_add_rows")
        return y.view(b, t, self.joints_num, 3)

    def __call__(self, feats: torch.Tensor, predict_future: bool = False):
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats.dim() != 3 or feats.shape[-1] != 2048:
            raise ValueError(f"expected (B,T,2048) features, got {tuple(feats.shape)}")
        if feats.device != self._device:
            raise ValueError(f"features are on {feats.device}, head on {self._device}")
        b, t, _ = feats.shape
        if b * t == 0:
            raise ValueError("empty batch")
        d = self.latent_dim
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((b * t, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * t, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None,
                       "r50_op_cast_rows")
            x = self._gemm(x0, "input_proj", relu=False)                                     # :155
            phi = self._temporal_net(x, b, t, "f_movie", self.number_blocks)                 # :156
            ar = self._temporal_net(phi, b, t, "f_AR", _AR_BLOCKS)                           # :158
            phi_hat = torch.zeros_like(ar).view(b, t, d)                                     # :159-160 (a shifted copy)
            phi_hat[:, 1:, :] = ar.view(b, t, d)[:, :-1, :]
            joints_phi = self._regressor(phi, b, t)                                          # :162
            joints_hat = self._regressor(phi_hat.view(b * t, d), b, t) if predict_future else None   # :164-166
        return phi.view(b, t, d).float(), phi_hat.float(), joints_phi, joints_hat

    forward = __call__

    def joints(self, feats: torch.Tensor) -> torch.Tensor:
        """``self(feats)[2]`` (joints_phi, (B,T,J,3) fp32) without f_AR: the evaluation pass (src/train.py:247) uses only joints_phi,
        and f_AR's output feeds phi_hat alone.  The same launches in the same order as ``__call__`` on this path, so the result is
        bit-equal."""
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats.dim() != 3 or feats.shape[-1] != 2048:
            raise ValueError(f"expected (B,T,2048) features, got {tuple(feats.shape)}")
        if feats.device != self._device:
            raise ValueError(f"features are on {feats.device}, head on {self._device}")
        b, t, _ = feats.shape
        if b * t == 0:
            raise ValueError("empty batch")
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((b * t, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * t, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None,
                       "r50_op_cast_rows")
            x = self._gemm(x0, "input_proj", relu=False)
            phi = self._temporal_net(x, b, t, "f_movie", self.number_blocks)
            return self._regressor(phi, b, t)

    def joints_windows(self, feats_nd: torch.Tensor, starts, t: int) -> torch.Tensor:
        """``joints`` over B windows of ONE feature matrix: ``feats_nd`` (N, 2048) fp32 on the head's device,
        ``starts`` B window starts (an int32 device tensor or a host sequence, each in ``[0, N - t]``, checked on the host) -> (B, t, J, 3)
        fp32.  One ``r50_op_gather_window_rows`` launch takes the place of ``feats_nd[idx]`` (a (B, t, 2048) fp32 copy) and the
        ``r50_op_cast_rows`` launch on it; the launches after it are those of ``joints``, so the result is bit-equal to
        ``joints(feats_nd[idx])`` with ``idx[w, i] = starts[w] + i``.  The host check of a DEVICE tensor of starts reads it back first (one
        blocking device-to-host copy per call); a host sequence costs no synchronisation."""
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats_nd.dim() != 2 or feats_nd.shape[-1] != 2048 or feats_nd.dtype != torch.float32:
            raise ValueError(f"expected (N,2048) fp32 features, got {tuple(feats_nd.shape)} {feats_nd.dtype}")
        if feats_nd.device != self._device:
            raise ValueError(f"features are on {feats_nd.device}, head on {self._device}")
        t = int(t)
        with torch.cuda.device(self._device):
            x0 = gather_window_rows(feats_nd.contiguous(), starts, t, self._dtype)
            b = x0.shape[0] // t
            x = self._gemm(x0, "input_proj", relu=False)
            phi = self._temporal_net(x, b, t, "f_movie", self.number_blocks)
            return self._regressor(phi, b, t)

    @torch.no_grad()
    def observe(self, feats: torch.Tensor, input_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """What the head knows after ``input_len`` observed frames: ``input_proj`` + ``f_movie`` + ``f_3D`` over
        ``feats[:, :input_len]`` ONLY -- GroupNorm's statistics span time, so a slice of a full-length pass is not the same thing.  The
        launches are those ``rollout`` makes for the observed part and those of ``joints(feats[:, :input_len])``.  Returns (phi
        (B, I, D) 16-bit: the strips ``rollout`` puts in front of its sequence buffer; joints (B, I, J, 3) fp32, bit-equal to
        ``joints(feats[:, :input_len])``)."""
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats.dim() != 3 or feats.shape[-1] != 2048:
            raise ValueError(f"expected (B,T,2048) features, got {tuple(feats.shape)}")
        if feats.device != self._device:
            raise ValueError(f"features are on {feats.device}, head on {self._device}")
        b, t, _ = feats.shape
        i_len = int(input_len)
        if b < 1 or not 1 <= i_len <= t:
            raise ValueError(f"observe needs B >= 1 and 1 <= input_len <= T (got B={b}, input_len={i_len}, T={t})")
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats[:, :i_len].to(torch.float32).contiguous()
            x0 = torch.empty((b * i_len, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * i_len, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None,
                       "r50_op_cast_rows")
            phi = self._temporal_net(self._gemm(x0, "input_proj", relu=False), b, i_len, "f_movie", self.number_blocks)
            return phi.view(b, i_len, self.latent_dim), self._regressor(phi, b, i_len)

    @torch.no_grad()
    def rollout(self, feats: torch.Tensor, input_len: int = 15, pred_len: int = 25) -> Tuple[torch.Tensor, torch.Tensor]:
        """Autoregressive forecast: f_movie over the first ``input_len`` frames only, then ``pred_len``
        times the next strip ``f_AR(seq)[:, -1]`` appended to ``seq``, then f_3D on the appended strips.  Returns (future_phi
        (B, P, D) fp32, future_joints (B, P, J, 3) fp32).  Only ``feats[:, :input_len]`` is read.  Eval-mode arithmetic (dropout
        is the identity) with the current weights; the mode and the weights are left as they are.

        The sequence lives in ONE time-major 16-bit buffer of (I+P)*B rows: frame t of sample b is row t*B + b, so the L frames
        seen at step k = L - I are its first L*B rows.  f_AR is recomputed over all of them (GroupNorm's statistics change with
        every frame, so no per-layer cache is exact), except the last block's conv2, which only the new frame needs: its
        GroupNorm emits that frame's rows alone (t0 = L-1) and its GEMM over B rows stores straight into rows L*B .. (L+1)*B-1,
        which is the append.  12 launches per step, no copies."""
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats.dim() != 3 or feats.shape[-1] != 2048:
            raise ValueError(f"expected (B,T,2048) features, got {tuple(feats.shape)}")
        if feats.device != self._device:
            raise ValueError(f"features are on {feats.device}, head on {self._device}")
        b, t, _ = feats.shape
        i_len, p_len = int(input_len), int(pred_len)
        if b < 1 or not 1 <= i_len <= t:
            raise ValueError(f"rollout needs B >= 1 and 1 <= input_len <= T (got B={b}, input_len={i_len}, T={t})")
        if p_len < 1:
            raise ValueError(f"rollout needs pred_len >= 1 (got {p_len})")
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats[:, :i_len].to(torch.float32).contiguous()
            x0 = torch.empty((b * i_len, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * i_len, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None,
                       "r50_op_cast_rows")
            phi = self._temporal_net(self._gemm(x0, "input_proj", relu=False), b, i_len, "f_movie", self.number_blocks)
            return self._rollout_from(phi, b, i_len, p_len)

    def _rollout_from(self, phi_rows: torch.Tensor, b: int, i_len: int, p_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``rollout`` after its observed strips: ``phi_rows`` (b*i_len, D) 16-bit, batch-major -> (future_phi (B, P, D) fp32,
        future_joints (B, P, J, 3) fp32).  The caller has selected the head's device."""
        d = self.latent_dim
        seq = torch.empty(((i_len + p_len) * b, d), dtype=self._dtype, device=self._device)
        seq[: i_len * b].view(i_len, b, d).copy_(phi_rows.view(b, i_len, d).transpose(0, 1))       # batch-major -> time-major
        last = _AR_BLOCKS - 1
        for k in range(p_len):
            n = i_len + k
            x = seq[: n * b]
            for i in range(_AR_BLOCKS):
                p = f"f_AR.blocks.{i}"
                h = self._gemm(self._gn_relu_rows_tm(x, b, n, 0, p + ".gn1"), p + ".conv1", relu=False)
                if i < last:
                    x = self._gemm(self._gn_relu_rows_tm(h, b, n, 0, p + ".gn2"), p + ".conv2", relu=False, residual=x)
                else:
                    self._gemm(self._gn_relu_rows_tm(h, b, n, n - 1, p + ".gn2"), p + ".conv2", relu=False,
                               residual=x[(n - 1) * b:], out=seq[n * b: (n + 1) * b])
        future = seq[i_len * b:]                                                      # (P*B, D) time-major
        joints = self._regressor(future, p_len, b)                                    # (P, B, J, 3)
        return future.view(p_len, b, d).transpose(0, 1).float(), joints.transpose(0, 1).contiguous()

    # ---- the hallucinator f_hal ----------------------------------------
    def _check_hal(self, feats: torch.Tensor, what: str) -> None:
        if not self.hallucinator:
            raise _lib.R50Error(f"{what} needs a head built with hallucinator=True (a checkpoint of train_hal carries f_hal.*)")
        if self._device is None or not self._dev:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') before running the head")
        if feats.dim() != 3 or feats.shape[-1] != 2048:
            raise ValueError(f"expected (B,T,2048) features, got {tuple(feats.shape)}")
        if feats.device != self._device:
            raise ValueError(f"features are on {feats.device}, head on {self._device}")

    def _hal_rows(self, x0: torch.Tensor) -> torch.Tensor:
        """``x + fc2(relu(fc1(x)))`` with ``x = input_proj(x0)``, row by row: three GEMM launches, (R, 2048) -> (R, D) 16-bit."""
        x = self._gemm(x0, "input_proj", relu=False)
        h1 = self._gemm(x, "f_hal.fc1", relu=True)
        return self._gemm(h1, "f_hal.fc2", relu=False, residual=x)

    @torch.no_grad()
    def hallucinate(self, feats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The movie strip and the 3D pose of every frame from that frame ALONE: ``phi_tilde = f_hal(input_proj(feats))`` and
        ``f_3D(phi_tilde)``.  Returns (phi_tilde (B, T, D) fp32, joints (B, T, J, 3) fp32).  The launches: cast, input_proj, f_hal's two
        GEMMs (ReLU, then the skip connection as the residual epilogue), the regressor.  No GroupNorm and no launch that sees more than
        a row, so the result of a frame does not depend on the frames around it."""
        self._check_hal(feats, "hallucinate")
        b, t, _ = feats.shape
        if b * t == 0:
            raise ValueError("empty batch")
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((b * t, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * t, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None,
                       "r50_op_cast_rows")
            phi_tilde = self._hal_rows(x0)
            return phi_tilde.view(b, t, self.latent_dim).float(), self._regressor(phi_tilde, b, t)

    @torch.no_grad()
    def hallucinated_rollout(self, feats: torch.Tensor, frame: int, pred_len: int = 25) -> Tuple[torch.Tensor, torch.Tensor]:
        """The forecast from ONE frame: ``rollout`` with input_len = 1 whose only observed strip is f_hal's for ``feats[:, frame]``
        instead of f_movie's.  Returns (future_phi (B, P, D) fp32, future_joints (B, P, J, 3) fp32): the ``pred_len`` strips after
        ``frame`` and f_3D on them.  Only ``feats[:, frame]`` is read: one ``r50_op_gather_window_rows`` launch (t = 1) picks and casts
        it, then input_proj and f_hal over B rows and ``rollout``'s launches on its time-major buffer."""
        self._check_hal(feats, "hallucinated_rollout")
        b, t, _ = feats.shape
        fr, p_len = int(frame), int(pred_len)
        if b < 1 or not 0 <= fr < t:
            raise ValueError(f"hallucinated_rollout needs B >= 1 and 0 <= frame < T (got B={b}, frame={fr}, T={t})")
        if p_len < 1:
            raise ValueError(f"hallucinated_rollout needs pred_len >= 1 (got {p_len})")
        with torch.cuda.device(self._device):
            src = feats.to(torch.float32).contiguous().view(b * t, 2048)
            x0 = gather_window_rows(src, [w * t + fr for w in range(b)], 1, self._dtype)
            return self._rollout_from(self._hal_rows(x0), b, 1, p_len)


PHD = PHDFor3DJoints       # the name src/train.py imports it under
