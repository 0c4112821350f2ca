"""Looking at a prediction: pose overlays and a 3D view drawn on the MI355X, written as PNG / APNG.

The reference looks at the ``.npz`` of ``src/results.py`` with matplotlib ``FuncAnimation`` on the host (``src/visualize_2d.py``: the
frame with the GT 2D joints, the frame with the projected 3D joints, a 3D axes).  Here the three panels are drawn on the device by one
HIP op, ``r50_op_draw_skeletons_u8`` (anti-aliased bones and joints of several layers blended over uint8 frames, gather form, no
atomics), and written with ``zlib`` and ``struct`` alone: no matplotlib, no image library.

* ``draw_skeletons``   the ctypes wrapper of the op.  No CPU fallback.
* ``view_points`` / ``project``   the 3D panel's orthographic map and the pinhole projection of ``project_with_K_torch``
  (src/train.py:84-110): a handful of torch ops on N*T*17 points, not the hot path.
* ``render_panels``    (N,T,S,3S,3) uint8 on the device from three launches: frame + GT 2D | frame + projected GT and prediction | 3D view.
* ``write_png`` / ``write_apng`` / ``contact_sheet``   the files.
* ``python -m implementation_phd_lab_vision_amd.render --npz FILE --outdir DIR``   renders a dump written earlier by ``results``.

Coordinates: x first, pixel (row i, col j) has its centre at (x = j, y = i) -- the convention under which matplotlib overlays
``scatter`` on ``imshow``, so the 2D joints of the shards (pixels of the 224x224 person crop) land where the reference draws them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

# The 16 bones of the 17-joint H3.6M skeleton as src/visualize_2d.py:11-17 lists them (and src/train.py:29-36): pairs of joint indices.
H36M_EDGES: List[Tuple[int, int]] = [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10),
                                     (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16)]

MAX_JOINTS, MAX_LAYERS, MAX_EDGES = 64, 8, 128            # the op's limits (include/r50.h)
PANEL_BG_RGB = 0x18181C                                    # the 3D panel's dark background, and the frames' stand-in when there is no crop
GT_RGB, PRED_RGB, FUTURE_RGB = (64, 224, 96), (255, 80, 64), (80, 160, 255)


def _rgb_int(rgb) -> int:
    if isinstance(rgb, int):
        return rgb
    r, g, b = (int(v) for v in rgb)
    return (r << 16) | (g << 8) | b


def _rgb_tuple(rgb) -> Tuple[int, int, int]:
    if isinstance(rgb, int):
        return (rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255
    return tuple(int(v) for v in rgb)


# ---- the op ---------------------------------------------------------------------------------------------------------------------
def draw_skeletons(bg: Optional[torch.Tensor], pts: torch.Tensor, style: torch.Tensor, edges: Sequence[Sequence[int]],
                   half_width: float, joint_radius: float, out: Optional[torch.Tensor] = None, *, bg_rgb=0,
                   hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """``r50_op_draw_skeletons_u8``: ``bg`` (F,H,W,3) uint8 on an MI355X or None (then the uniform colour ``bg_rgb``, 0xRRGGBB or an
    (r,g,b) triple, on a canvas of ``hw`` = (H,W) or of ``out``'s size), ``pts`` (F,L,J,2) fp32 pixel coordinates (x first), ``style``
    (F,L,4) uint8 R,G,B,A, ``edges`` (E,2) joint-index pairs on the host -> (F,H,W,3) uint8 on the device, later layers on top.  The
    pixel rule is in include/r50.h.  ``out`` may not overlap ``bg``.  One launch on the current stream.  There is no CPU fallback."""
    if not pts.is_cuda or pts.dtype != torch.float32 or pts.dim() != 4 or pts.shape[-1] != 2 or not pts.is_contiguous():
        raise ValueError("draw_skeletons: pts must be a contiguous (F,L,J,2) fp32 tensor on the GPU")
    f, layers, joints, _ = pts.shape
    if style.dtype != torch.uint8 or tuple(style.shape) != (f, layers, 4) or style.device != pts.device or not style.is_contiguous():
        raise ValueError("draw_skeletons: style must be a contiguous (F,L,4) uint8 tensor on the points' device")
    if bg is not None:
        if bg.dtype != torch.uint8 or bg.dim() != 4 or bg.shape[0] != f or bg.shape[-1] != 3 or bg.device != pts.device or not bg.is_contiguous():
            raise ValueError("draw_skeletons: bg must be a contiguous (F,H,W,3) uint8 tensor on the points' device")
        h, w = int(bg.shape[1]), int(bg.shape[2])
    elif out is not None:
        h, w = int(out.shape[1]), int(out.shape[2])
    elif hw is not None:
        h, w = int(hw[0]), int(hw[1])
    else:
        raise ValueError("draw_skeletons: without bg, give hw=(H,W) or out")
    if out is None:
        out = torch.empty((f, h, w, 3), dtype=torch.uint8, device=pts.device)
    elif tuple(out.shape) != (f, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != pts.device:
        raise ValueError("draw_skeletons: `out` must be a contiguous (F,H,W,3) uint8 tensor on the points' device")
    flat = [int(v) for e in edges for v in e]
    if len(flat) % 2:
        raise ValueError("draw_skeletons: edges must be pairs of joint indices")
    arr = (C.c_int * max(len(flat), 1))(*flat)
    lib = _lib.load_library()
    with torch.cuda.device(pts.device):
        rc = lib.r50_op_draw_skeletons_u8(bg.data_ptr() if bg is not None else None, _rgb_int(bg_rgb), pts.data_ptr(), style.data_ptr(),
                                          arr, len(flat) // 2, f, h, w, layers, joints, float(half_width), float(joint_radius),
                                          out.data_ptr(), torch.cuda.current_stream(pts.device).cuda_stream)
    _lib.check(rc, None, "r50_op_draw_skeletons_u8")
    return out


# ---- the two maps (torch ops; any device) -----------------------------------------------------------------------------------------
def view_points(j3d: torch.Tensor, centre: torch.Tensor, azim_deg: float = 30.0, elev_deg: float = 15.0, size: int = 224,
                half_extent_m: float = 1.0) -> torch.Tensor:
    """The 3D panel's orthographic map: ``j3d`` (...,J,3) camera-space points (y down, as on the screen), ``centre`` (...,3) (the GT root
    joint of that frame, for GT and prediction alike, so a root offset of the prediction shows) -> (...,J,2) pixels:
    ``q = Rx(elev) . Ry(azim) . (P - centre)``, ``u = size/2 + s q.x``, ``v = size/2 + s q.y``, ``s = (size/2) / half_extent_m``.
    ``Ry(a)`` takes +z towards +x (x' = x cos a + z sin a), ``Rx(e)`` takes +z towards -y, i.e. up the screen (y' = y cos e - z sin e):
    azim = elev = 0 is the camera's own view, and at azim 90 the depth axis runs to the right."""
    a, e = math.radians(azim_deg), math.radians(elev_deg)
    ca, sa, ce, se = math.cos(a), math.sin(a), math.cos(e), math.sin(e)
    p = j3d - centre.unsqueeze(-2)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    x1 = x * ca + z * sa
    z1 = z * ca - x * sa
    y2 = y * ce - z1 * se
    s = (size / 2.0) / float(half_extent_m)
    return torch.stack([size / 2.0 + s * x1, size / 2.0 + s * y2], dim=-1)


def project(j3d: torch.Tensor, K: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """Pinhole projection, the formula of ``project_with_K_torch`` (src/train.py:84-110): ``j3d`` (N,T,J,3) or (...,3) with ``K`` (3,3),
    (N,3,3) or (N,T,3,3) -> (...,2) = ``(K P)[:2] / (K P)[2]``.  Where the reference clamps the depth at ``eps``, a joint with
    ``(K P)[2] <= eps`` (at or behind the camera plane) becomes NaN here, so the drawing op drops it along with its bones."""
    k = K.to(j3d.dtype)
    if k.dim() == 2:
        while k.dim() < j3d.dim() + 1:
            k = k.unsqueeze(0)
    elif k.dim() == 3:
        k = k[:, None, None, :, :]
    elif k.dim() == 4:
        k = k[:, :, None, :, :]
    else:
        raise ValueError(f"project: unexpected K shape {tuple(K.shape)}")
    ph = torch.matmul(k, j3d.unsqueeze(-1)).squeeze(-1)
    z = ph[..., 2:3]
    uv = ph[..., 0:2] / z
    return torch.where(z > eps, uv, torch.full_like(uv, float("nan")))


# ---- the panels ---------------------------------------------------------------------------------------------------------------------
def _styles(n: int, t: int, layers: Sequence[Tuple[Tuple[int, int, int], torch.Tensor]], device) -> torch.Tensor:
    """(N*T, L, 4) uint8 from per-layer (rgb (T,3) or (3,), alpha (T,)) rows."""
    st = torch.zeros((n, t, len(layers), 4), dtype=torch.uint8)
    for l, (rgb, alpha) in enumerate(layers):
        st[:, :, l, :3] = torch.as_tensor(rgb, dtype=torch.uint8)
        st[:, :, l, 3] = torch.as_tensor(alpha, dtype=torch.uint8)
    return st.reshape(n * t, len(layers), 4).to(device)


def render_panels(frames_u8: Optional[torch.Tensor], joints2d: Optional[torch.Tensor], K: Optional[torch.Tensor],
                  gt3d: Optional[torch.Tensor], pred3d: torch.Tensor,
                  future3d: Optional[torch.Tensor] = None, input_len: int = 0, *, size: Optional[int] = None,
                  edges: Sequence[Sequence[int]] = H36M_EDGES, root: int = 0, gt_rgb=GT_RGB, pred_rgb=PRED_RGB, future_rgb=FUTURE_RGB,
                  gt_alpha: int = 255, ref_alpha: int = 153, pred_alpha: int = 255, bg_rgb=PANEL_BG_RGB, half_width: float = 1.0,
                  joint_radius: float = 2.0, azim_deg: float = 30.0, elev_deg: float = 15.0, half_extent_m: float = 1.0,
                  eps: float = 1e-6) -> torch.Tensor:
    """(N,T,S,3S,3) uint8 on the device, three ``draw_skeletons`` launches over the N*T frames:

    * panel 0: the frame + the GT 2D joints (``joints2d`` (N,T,J,2), pixels of the frame);
    * panel 1: the frame + the projected GT (``project(gt3d, K)``, at ``ref_alpha``: the op has one width per launch, so the reference
      layer is told apart by its lower alpha) + the projected prediction on top;
    * panel 2: ``bg_rgb`` + GT and prediction in the 3D view (``view_points``, both centred on the GT root joint).

    ``frames_u8`` (N,T,S,S,3) uint8 on the device, or None: then panels 0 and 1 get ``bg_rgb`` too (``size`` gives S, default 224).
    With ``future3d`` (N,P,J,3) the prediction layer of the frames ``t >= input_len`` carries the rollout's poses in ``future_rgb``, and
    the frames ``t >= input_len + P`` have it switched off.  gt3d / pred3d (N,T,J,3), K (N,3,3) or, a camera per frame (``predict
    --track``), (N,T,3,3), all on the device.

    A prediction without annotations (``predict``): ``joints2d``, ``K`` and ``gt3d`` may each be None.  A layer whose input is missing is
    left out (panel 0 without ``joints2d`` is the bare frame, and so is panel 1 without ``K``: nothing can be projected), and without
    ``gt3d`` the 3D view is centred on the prediction's own root joint.  With all three given nothing changes."""
    shape_of = gt3d if gt3d is not None else pred3d
    n, t, j = int(shape_of.shape[0]), int(shape_of.shape[1]), int(shape_of.shape[2])
    dev = shape_of.device
    if frames_u8 is not None:
        if frames_u8.dim() != 5 or frames_u8.shape[:2] != (n, t) or frames_u8.shape[2] != frames_u8.shape[3] or frames_u8.shape[4] != 3:
            raise ValueError(f"render_panels: frames_u8 must be (N,T,S,S,3), got {tuple(frames_u8.shape)}")
        s = int(frames_u8.shape[2])
        bg = frames_u8.reshape(n * t, s, s, 3).contiguous()
    else:
        s, bg = int(size or 224), None
    pred3d = pred3d.float()
    gt3d = gt3d.float() if gt3d is not None else None
    joints2d = joints2d.float() if joints2d is not None else None
    pred_col = torch.tensor(_rgb_tuple(pred_rgb), dtype=torch.uint8).repeat(t, 1)
    pred_a = torch.full((t,), int(pred_alpha), dtype=torch.uint8)
    if future3d is not None:
        p = int(future3d.shape[1])
        lo, hi = min(int(input_len), t), min(int(input_len) + p, t)
        pred3d = pred3d.clone()
        pred3d[:, lo:hi] = future3d[:, :hi - lo].float()
        pred_col[lo:] = torch.tensor(_rgb_tuple(future_rgb), dtype=torch.uint8)
        pred_a[hi:] = 0
    gt_a, ref_a = torch.full((t,), int(gt_alpha), dtype=torch.uint8), torch.full((t,), int(ref_alpha), dtype=torch.uint8)
    gt_c = _rgb_tuple(gt_rgb)

    def layers(*pts):
        return torch.stack([q.reshape(n * t, j, 2) for q in pts], dim=1).to(torch.float32).contiguous()

    kw = dict(bg_rgb=bg_rgb, hw=(s, s))

    def panel(back, *drawn):
        """One launch over ``back`` with the (points, rgb, alpha) layers whose points are there; with none, ``back`` as it is."""
        drawn = [d for d in drawn if d[0] is not None]
        if not drawn:
            if back is not None:
                return back.clone()
            return torch.tensor(_rgb_tuple(bg_rgb), dtype=torch.uint8, device=dev).expand(n * t, s, s, 3).contiguous()
        return draw_skeletons(back, layers(*[d[0] for d in drawn]), _styles(n, t, [d[1:] for d in drawn], dev), edges, half_width,
                              joint_radius, **kw)

    p0 = panel(bg, (joints2d, gt_c, gt_a))
    p1 = panel(bg, (project(gt3d, K, eps) if gt3d is not None and K is not None else None, gt_c, ref_a),
               (project(pred3d, K, eps) if K is not None else None, pred_col, pred_a))
    centre = (gt3d if gt3d is not None else pred3d)[:, :, root]
    view = dict(azim_deg=azim_deg, elev_deg=elev_deg, size=s, half_extent_m=half_extent_m)
    p2 = panel(None, (view_points(gt3d, centre, **view) if gt3d is not None else None, gt_c, gt_a),
               (view_points(pred3d, centre, **view), pred_col, pred_a))
    return torch.cat([p0, p1, p2], dim=2).reshape(n, t, s, 3 * s, 3)


# ---- files: PNG and APNG with zlib and struct alone ---------------------------------------------------------------------------------
_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _hwc(img) -> np.ndarray:
    a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != 3 or a.shape[-2] < 1 or a.shape[-3] < 1:
        raise ValueError(f"expected uint8 (...,H,W,3) with H, W >= 1, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _scanlines(hwc: np.ndarray, level: int) -> bytes:
    """The zlib stream of one image: every row behind filter type 0 (None), so the inflated bytes are the pixels themselves."""
    h, w, _ = hwc.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    rows[:, 1:] = hwc.reshape(h, 3 * w)
    return zlib.compress(rows.tobytes(), level)


def _ihdr(h: int, w: int) -> bytes:
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))          # 8-bit RGB, no interlace


def write_png(path, hwc_u8, level: int = 6) -> None:
    """One (H,W,3) uint8 image (numpy or torch) as an 8-bit RGB PNG."""
    a = _hwc(hwc_u8)
    if a.ndim != 3:
        raise ValueError(f"write_png: expected (H,W,3), got {a.shape}")
    with open(path, "wb") as fh:
        fh.write(_PNG_SIG + _ihdr(a.shape[0], a.shape[1]) + _chunk(b"IDAT", _scanlines(a, level)) + _chunk(b"IEND", b""))


def apng_delay(fps: float) -> Tuple[int, int]:
    """(delay_num, delay_den) of an fcTL chunk: 1/fps seconds in milliseconds, at least 1 ms."""
    return max(1, min(65535, int(round(1000.0 / float(fps))))), 1000


def write_apng(path, thwc_u8, fps: float = 10.0, level: int = 6) -> None:
    """(T,H,W,3) uint8 frames as an animated PNG that loops for ever: ``acTL``, then per frame an ``fcTL`` and its data (``IDAT`` for
    frame 0, ``fdAT`` after it).  Frame 0 is the default image, so a viewer that knows only PNG shows it."""
    a = _hwc(thwc_u8)
    if a.ndim != 4 or a.shape[0] < 1:
        raise ValueError(f"write_apng: expected (T,H,W,3) with T >= 1, got {a.shape}")
    if not float(fps) > 0:
        raise ValueError(f"write_apng: fps must be > 0, got {fps}")
    t, h, w, _ = a.shape
    num, den = apng_delay(fps)
    seq = 0
    with open(path, "wb") as fh:
        fh.write(_PNG_SIG + _ihdr(h, w) + _chunk(b"acTL", struct.pack(">II", t, 0)))
        for i in range(t):
            fh.write(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
            seq += 1
            data = _scanlines(a[i], level)
            if i == 0:
                fh.write(_chunk(b"IDAT", data))
            else:
                fh.write(_chunk(b"fdAT", struct.pack(">I", seq) + data))
                seq += 1
        fh.write(_chunk(b"IEND", b""))


def contact_sheet(thwc_u8, every: int = 5):
    """One image holding every ``every``-th frame (0, every, 2 every, ...) of (T,H,W,3), stacked top to bottom: (ceil(T/every) H, W, 3).
    numpy in, numpy out; torch in, torch out."""
    if int(every) < 1:
        raise ValueError(f"contact_sheet: every must be >= 1, got {every}")
    if len(thwc_u8.shape) != 4 or thwc_u8.shape[0] < 1:
        raise ValueError(f"contact_sheet: expected (T,H,W,3) with T >= 1, got {tuple(thwc_u8.shape)}")
    picked = thwc_u8[::int(every)]
    return picked.reshape(picked.shape[0] * picked.shape[1], picked.shape[2], picked.shape[3])


# ---- clips to files -------------------------------------------------------------------------------------------------------------------
def _safe(text) -> str:
    return "".join(ch if ch.isalnum() or ch in "-_" else "_" for ch in str(text))


def clip_stem(i: int, meta) -> str:
    """``clip_<i>_S<subject>_<action>`` (without the meta: ``clip_<i>``)."""
    if isinstance(meta, dict) and "subject" in meta and "action" in meta:
        return f"clip_{i}_S{int(meta['subject'])}_{_safe(meta['action'])}"
    return f"clip_{i}"


def render_clips(outdir, frames_u8: Optional[torch.Tensor], joints2d, K, gt3d, pred3d, future3d=None, input_len: int = 0,
                 metas: Optional[Sequence] = None, fps: float = 10.0, sheet_every: int = 5, **panel_kw) -> List[str]:
    """``render_panels`` over n clips, then per clip ``<stem>.png`` (an APNG of the T frames) and ``clip_<i>_sheet.png`` (the contact
    sheet) under ``outdir``.  ``joints2d``, ``K`` and ``gt3d`` may be None, as in ``render_panels``.  Returns the written paths."""
    os.makedirs(outdir, exist_ok=True)
    panels = render_panels(frames_u8, joints2d, K, gt3d, pred3d, future3d, input_len, **panel_kw).cpu().numpy()
    written = []
    for i in range(panels.shape[0]):
        anim = os.path.join(outdir, clip_stem(i, metas[i] if metas is not None else None) + ".png")
        sheet = os.path.join(outdir, f"clip_{i}_sheet.png")
        write_apng(anim, panels[i], fps)
        write_png(sheet, contact_sheet(panels[i], sheet_every))
        written += [anim, sheet]
    return written


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("Render the .npz dump of the results pass: pose overlays and a 3D view per clip, as APNG + contact sheet")
    p.add_argument("--npz", type=str, required=True, help="a dump written by python -m implementation_phd_lab_vision_amd.results")
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--n", type=int, default=4, help="how many of the dumped clips to render")
    p.add_argument("--fps", type=float, default=10.0)
    p.add_argument("--sheet-every", type=int, default=5)
    p.add_argument("--device", type=str, default="cuda")
    return p


def main(argv: Optional[List[str]] = None) -> List[str]:
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.R50Error("rendering runs on an MI355X only; there is no CPU fallback")
    z = np.load(args.npz, allow_pickle=True)
    n = max(1, min(int(args.n), int(z["joints3d"].shape[0])))
    dev = lambda key: torch.from_numpy(np.ascontiguousarray(z[key][:n])).to(device)         # noqa: E731
    frames = None
    if "video_crop" in z.files:
        n = min(n, int(z["video_crop"].shape[0]))
        frames = dev("video_crop")
    else:
        print("render: the dump holds no video_crop (written by results --render): its `video` is the whole uncropped frame, which the "
              "2D joints and K do not refer to, so the panels get the plain background")
    future, input_len = None, 0
    if "predicted_future3djoints" in z.files and "rollout_lens" in z.files:
        future, input_len = dev("predicted_future3djoints"), int(z["rollout_lens"][0])
    metas = list(z["meta"][:n]) if "meta" in z.files else None
    written = render_clips(args.outdir, frames, dev("joints2d"), dev("K"), dev("joints3d"), dev("predicted3djoints"), future, input_len,
                           metas, args.fps, args.sheet_every)
    print(f"[OK] Rendered {n} clips to: {args.outdir}")
    return written


if __name__ == "__main__":
    main()
