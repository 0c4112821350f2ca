"""``predict --track`` (INTEGRATION.md section AA) on one MI355X.  Every timing runs in a fresh child process of a tree:

* ``ops``: ``r50_op_crop_resize_boxes_u8`` beside the frame producer ``r50_op_crop_resize_u8`` on the same 256 frames of 500 x 500
  -> 224: (1) a constant table against one launch of the producer; (2) one launch with ``out_flip`` against the producer's two launches
  (plain and ``hflip``); (3) one launch over 256 different boxes against 256 single-frame launches of the producer; (4) a device copy of
  the frames' bytes, for scale.  The forms alternate in rounds of --iters launches, each round under a host clock that ends in a
  synchronise; per form the best round and all rounds (the spread) are reported.  The outputs are compared bit for bit first.
* ``pass``: one ``VideoPredictor.predict`` pass over --frames synthetic 1002 x 1000 frames (as scripts/bench_predict.py), a subject of
  about 250 pixels walking across: with ``track`` (a box per frame, about 400 pixels) and without (the centred square), and, with
  ``--parent-tree DIR`` (a built checkout of the parent commit), without it there: this tree and the parent alternate, --passes children
  each.  That last pair is the proof that the default path did not move.
Prints one JSON line.
    python scripts/bench_track.py [--iters 50] [--rounds 5] [--frames 1000] [--passes 2] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STRIDE, H, W = 40, 5, 1002, 1000
DEV = "cuda:0"


def _rounds(forms, iters, rounds, warmup):
    us = {name: [] for name in forms}
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):                                                              # alternate, so drift hits all alike
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / iters)
    return {name: {"best_us": round(min(v), 2), "rounds_us": [round(x, 2) for x in v]} for name, v in us.items()}


def child_ops(a):
    from implementation_phd_lab_vision_amd import frames as F
    from implementation_phd_lab_vision_amd import track
    t, h, w, out = 256, 500, 500, 224
    frames = torch.randint(0, 256, (t, h, w, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
    flat = frames.view(-1)
    offsets = np.arange(t, dtype=np.int64) * 3 * h * w
    whole = [0, 0, h, w]
    const = track.BoxTable(offsets, [h, w], [whole] * t, flat.numel(), out, F.RESIZE_FLOAT, device=DEV)
    rng = np.random.default_rng(1)
    side = rng.integers(150, 400, t)
    moving = np.stack([rng.integers(0, h - side + 1), rng.integers(0, w - side + 1), side, side], axis=1).astype(np.int64)
    ragged = track.BoxTable(offsets, [h, w], moving, flat.numel(), out, F.RESIZE_FLOAT, device=DEV)
    o1, o2, o3, o4 = (torch.empty((t, 3, out, out), dtype=torch.uint8, device=DEV) for _ in range(4))
    copy_dst = torch.empty_like(flat)

    def per_frame():
        for i in range(t):
            F.crop_and_resize_video_uint8(frames[i:i + 1], moving[i].tolist(), out, out=o3[i:i + 1])
    forms = {
        "producer_one_box": lambda: F.crop_and_resize_video_uint8(frames, whole, out, out=o1),
        "boxes_constant_table": lambda: track.crop_resize_boxes_u8(flat, const, out=o2),
        "producer_two_launches_flip": lambda: (F.crop_and_resize_video_uint8(frames, whole, out, out=o1),
                                               F.crop_and_resize_video_uint8(frames, whole, out, hflip=True, out=o3)),
        "boxes_one_launch_flip": lambda: track.crop_resize_boxes_u8(flat, const, out=o2, out_flip=o4),
        "boxes_256_boxes_one_launch": lambda: track.crop_resize_boxes_u8(flat, ragged, out=o2),
        "producer_256_single_frame_launches": per_frame,
        "device_copy_of_the_frames": lambda: copy_dst.copy_(flat),
    }
    forms["producer_two_launches_flip"]()
    forms["boxes_one_launch_flip"]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(o1, o2)) and bool(torch.equal(o3, o4))
    forms["boxes_256_boxes_one_launch"]()
    per_frame()
    torch.cuda.synchronize()
    equal = equal and bool(torch.equal(o2, o3))
    res = _rounds(forms, a.iters, a.rounds, a.warmup)
    res.update({"frames": t, "height": h, "width": w, "out": out, "frames_bytes": int(flat.numel()), "bit_equal": equal})
    return res


def synthetic_video(n):
    """n frames (H, W, 3) uint8: one random frame, shifted by a few pixels per frame (scripts/bench_predict.py's)."""
    base = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = np.empty((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        frames[i] = np.roll(base, (3 * i, 5 * i), axis=(0, 1))
    return frames


def walking_joints(n):
    """(n, 17, 2) fp32: a body of about 100 x 250 pixels that walks from x = 150 to x = 850."""
    rng = np.random.default_rng(2)
    body = rng.uniform(-1.0, 1.0, (17, 2)) * [50.0, 125.0]
    cx = np.linspace(150.0, 850.0, n)
    return (body[None] + np.stack([cx, np.full(n, H / 2)], axis=-1)[:, None] + rng.normal(0.0, 2.0, (n, 17, 2))).astype(np.float32)


def child_pass(a):
    from implementation_phd_lab_vision_amd import predict, train
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
    head = PHDFor3DJoints(1024, 17, 2, precision="fp16")
    head.load_state_dict(train.default_state_dict(1024, 17, 2, seed=0))
    head.to(DEV).eval()
    backbone = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=256).to(DEV).eval()
    frames = synthetic_video(a.frames)
    box = predict.centred_square(H, W).tolist()
    kw = {}
    if a.track:
        from implementation_phd_lab_vision_amd.track import TrackSettings
        kw = {"joints2d": walking_joints(a.frames), "track": TrackSettings(T)}
    p = predict.VideoPredictor(backbone, head, seq_len=T, stride=STRIDE, flip_tta=bool(a.flip))
    warm = {k: (v[:2 * T] if k == "joints2d" else v) for k, v in kw.items()}
    p.predict(frames[:2 * T], box=box, **warm)
    secs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = p.predict(frames, box=box, **kw)
        torch.cuda.synchronize()
        secs.append(round(time.perf_counter() - t0, 3))
    backbone.close()
    out = {"seconds": secs, "stats": res["stats"]}
    if a.track:
        out["mean_box_side"] = round(float(res["boxes"][:, 2].mean()), 1)
    return out


def spawn(tree, *args):
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, *args]
    done = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
    if done.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({done.returncode}):\n{done.stdout}\n{done.stderr}")
    print(f"{tree}: {' '.join(args)}: done", file=sys.stderr, flush=True)
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--flip", type=int, default=0)
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--tree", type=str, default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--child", choices=("ops", "pass"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--track", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.tree)
        print(json.dumps(child_ops(a) if a.child == "ops" else child_pass(a)))
        return
    common = ["--frames", str(a.frames), "--flip", str(a.flip)]
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "ops": spawn(HERE, "--child", "ops", "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)),
           "pass": {"frames": a.frames, "height": H, "width": W, "flip_tta": bool(a.flip), "track": [], "no_track": [], "parent_no_track": []}}
    for _ in range(a.passes):
        out["pass"]["track"].append(spawn(HERE, "--child", "pass", "--track", "1", *common))
        out["pass"]["no_track"].append(spawn(HERE, "--child", "pass", *common))
        if a.parent_tree:
            out["pass"]["parent_no_track"].append(spawn(os.path.abspath(a.parent_tree), "--child", "pass", *common))
    if not a.parent_tree:
        out["pass"]["parent_no_track"] = "not measured (no --parent-tree)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
