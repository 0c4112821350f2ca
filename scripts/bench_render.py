"""The skeleton drawing op on one MI355X, at the size the results pass renders: F = 16 x 40 frames of
224 x 224, L = 2 layers of the 17-joint skeleton (96 MB in, 96 MB out per launch).  In one process, on the same inputs:

* ``r50_op_draw_skeletons_u8`` per launch, and ``render.render_panels`` per call (three launches plus the projection, the 3D view and
  the side-by-side copy in torch);
* the same pixel rule written in torch ops on the device (fp32, one pass of elementwise kernels per bone and joint);
* a plain device copy of the frames (``out.copy_(bg)``): the rate a kernel that reads and writes every byte once can reach;
* the fp64 numpy oracle of tests/render_reference.py on the host over --oracle-frames frames, scaled to F, for scale.

Each device figure is the median of --runs runs timed with device events after --warmup warm-up runs, the variants alternating
inside every run.  Also reports how far the op's bytes are from the torch composition's and from the oracle's.  Prints one JSON line.
    python scripts/bench_render.py [--runs 20] [--warmup 3] [--oracle-frames 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, T, S, LAYERS, JOINTS = 16, 40, 224, 2, 17
HALF_WIDTH, JOINT_RADIUS = 1.0, 2.0


def torch_draw(bg, pts, style, edges, half_width, joint_radius):
    """The pixel rule of r50_op_draw_skeletons_u8 in torch ops (fp32 throughout), the whole batch at once."""
    f, h, w, _ = bg.shape
    dev = bg.device
    c = bg.float()
    ys = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1)
    xs = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w)
    inf = torch.tensor(float("inf"), device=dev)
    for l in range(pts.shape[1]):
        p = pts[:, l]
        fin = torch.isfinite(p).all(dim=-1)
        de2 = torch.full((f, h, w), float("inf"), device=dev)
        for a_i, b_i in edges:
            a, d = p[:, a_i], p[:, b_i] - p[:, a_i]
            ok = (fin[:, a_i] & fin[:, b_i]).view(f, 1, 1)
            rx, ry = xs - a[:, 0].view(f, 1, 1), ys - a[:, 1].view(f, 1, 1)
            dx, dy = d[:, 0].view(f, 1, 1), d[:, 1].view(f, 1, 1)
            len2 = dx * dx + dy * dy
            inv = torch.where(len2 > 0, 1.0 / len2, torch.zeros_like(len2))
            t = ((rx * dx + ry * dy) * inv).clamp(0.0, 1.0)
            qx, qy = rx - t * dx, ry - t * dy
            de2 = torch.minimum(de2, torch.where(ok, qx * qx + qy * qy, inf))
        dj2 = torch.full((f, h, w), float("inf"), device=dev)
        for j in range(p.shape[1]):
            rx, ry = xs - p[:, j, 0].view(f, 1, 1), ys - p[:, j, 1].view(f, 1, 1)
            dj2 = torch.minimum(dj2, torch.where(fin[:, j].view(f, 1, 1), rx * rx + ry * ry, inf))
        cov = torch.maximum((half_width + 0.5 - de2.sqrt()).clamp(0.0, 1.0), (joint_radius + 0.5 - dj2.sqrt()).clamp(0.0, 1.0))
        a = (cov * (style[:, l, 3].float() / 255.0).view(f, 1, 1)).unsqueeze(-1)
        c = c * (1.0 - a) + style[:, l, :3].float().view(f, 1, 1, 3) * a
    return (c + 0.5).floor().clamp(0.0, 255.0).to(torch.uint8)


def inputs(dev):
    """Frames of noise and, per frame, a person-sized skeleton (bones of a few tens of pixels around a root that wanders) twice."""
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, generator=g)
    gt3d = torch.randn(N, T, JOINTS, 3, generator=g) * 0.25 + torch.tensor([0.0, 0.0, 4.5])
    pred3d = gt3d + 0.04 * torch.randn(N, T, JOINTS, 3, generator=g)
    k = torch.eye(3).repeat(N, 1, 1)
    k[:, 0, 0] = k[:, 1, 1] = 560.0
    k[:, 0, 2] = k[:, 1, 2] = S / 2.0
    return frames.to(dev), k.to(dev), gt3d.to(dev), pred3d.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-frames", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: needs an MI355X; a CPU run measures nothing")
    from implementation_phd_lab_vision_amd import render
    from tests import render_reference as rr
    dev = "cuda:0"
    frames, k, gt3d, pred3d = inputs(dev)
    f = N * T
    bg = frames.reshape(f, S, S, 3)
    pts = torch.stack([render.project(gt3d, k).reshape(f, JOINTS, 2), render.project(pred3d, k).reshape(f, JOINTS, 2)], dim=1).contiguous()
    style = torch.tensor([[*render.GT_RGB, 153], [*render.PRED_RGB, 255]], dtype=torch.uint8, device=dev).repeat(f, 1, 1).contiguous()
    joints2d = pts[:, 0].reshape(N, T, JOINTS, 2).contiguous()
    edges = render.H36M_EDGES
    out = torch.empty_like(bg)
    copy_out = torch.empty_like(bg)
    variants = {"draw_op": lambda: render.draw_skeletons(bg, pts, style, edges, HALF_WIDTH, JOINT_RADIUS, out=out),
                "device_copy": lambda: copy_out.copy_(bg),
                "render_panels": lambda: render.render_panels(frames, joints2d, k, gt3d, pred3d),
                "torch_ops": lambda: torch_draw(bg, pts, style, edges, HALF_WIDTH, JOINT_RADIUS)}
    ms = {name: [] for name in variants}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(max(a.runs, 1)):                                        # alternate, so drift hits all alike
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = {name: statistics.median(v) for name, v in ms.items()}
    got = variants["draw_op"]().cpu().numpy()
    via_torch = variants["torch_ops"]().cpu().numpy()
    d_torch = np.abs(got.astype(np.int16) - via_torch.astype(np.int16))
    nf = max(1, min(a.oracle_frames, f))
    pick = np.linspace(0, f - 1, nf).astype(int)
    t0 = time.perf_counter()
    ref = rr.draw_reference(bg[pick].cpu().numpy(), 0, pts[pick].cpu().numpy(), style[pick].cpu().numpy(), edges, HALF_WIDTH, JOINT_RADIUS)
    oracle_s = time.perf_counter() - t0
    mx, bad, near = rr.check_against(got[pick], ref, rr.margin(LAYERS))
    bytes_moved = 2 * bg.numel()
    res = {"device": torch.cuda.get_device_name(0), "frames": f, "size": S, "layers": LAYERS, "joints": JOINTS, "edges": len(edges),
           "half_width": HALF_WIDTH, "joint_radius": JOINT_RADIUS, "runs": len(ms["draw_op"]), "warmup": a.warmup,
           "bytes_in_plus_out": bytes_moved,
           "draw_op_ms": round(med["draw_op"], 4), "draw_op_ms_min": round(min(ms["draw_op"]), 4),
           "draw_op_gb_per_s": round(bytes_moved / med["draw_op"] / 1e6, 1),
           "device_copy_ms": round(med["device_copy"], 4), "device_copy_gb_per_s": round(bytes_moved / med["device_copy"] / 1e6, 1),
           "render_panels_ms": round(med["render_panels"], 4), "torch_ops_ms": round(med["torch_ops"], 3),
           "numpy_oracle_ms_scaled_to_all_frames": round(oracle_s * 1e3 * f / nf, 1), "numpy_oracle_frames_timed": nf,
           "torch_over_op": round(med["torch_ops"] / med["draw_op"], 1), "op_over_copy": round(med["draw_op"] / med["device_copy"], 2),
           "oracle_over_op": round(oracle_s * 1e3 * f / nf / med["draw_op"], 0),
           "blended_pixel_share": round(float(ref[2].mean()), 4),
           "bytes_differing_from_torch_ops": int((d_torch > 0).sum()), "max_diff_from_torch_ops": int(d_torch.max()),
           "oracle_max_diff": mx, "oracle_bytes_outside_margin": bad, "oracle_bytes_within_margin": near}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
