"""``predict`` on one MI355X.  In one process:

* ``r50_op_gather_window_rows`` beside the two steps it replaces, ``feats[idx]`` (torch's fp32 gather) + ``r50_op_cast_rows``, on the
  same (1000, 2048) feature matrix and the same windows, at W x T = 193 x 40 (a 1000-frame video at stride 5) and 8 x 40.  The two
  alternate in rounds of --iters launches, each round under a warmed host clock that ends in a synchronise; the figure is the best
  round of each.  The outputs are compared bit for bit first;
* one ``VideoPredictor.predict`` pass over --frames synthetic 1002 x 1000 frames (host memory in, poses out; PHD(1024, 17, 2) fp16,
  bf16 backbone with seeded weights) beside the window-by-window form -- the frames already on the device, then per window
  ``features_from_video`` + ``head.joints``, one stitch -- with and without flip test-time augmentation, in video frames per second
  (host clock, synchronised, best of --passes after a warm-up).
Prints one JSON line.
    python scripts/bench_predict.py [--iters 200] [--rounds 5] [--frames 1000] [--passes 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, STRIDE, H, W = 40, 5, 1002, 1000
DEV = "cuda:0"


def time_gather(n_windows, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import _lib, model, predict
    lib = _lib.load_library()
    feats = torch.randn(1000, 2048, generator=torch.Generator().manual_seed(0)).to(DEV)
    starts = predict.window_starts(1000, T, STRIDE)[:n_windows]
    rows = len(starts) * T
    dev_starts = torch.from_numpy(starts).to(DEV)
    idx = (dev_starts.long()[:, None] + torch.arange(T, device=DEV)[None]).reshape(-1)
    one, two = (torch.empty((rows, 2048), dtype=torch.float16, device=DEV) for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream

    def gather():
        rc = lib.r50_op_gather_window_rows(feats.data_ptr(), 1000, 2048, dev_starts.data_ptr(), len(starts), T, one.data_ptr(), 1, stream)
        assert rc == 0

    def two_step():
        f = feats[idx]
        assert lib.r50_op_cast_rows(f.data_ptr(), rows, 2048, two.data_ptr(), 2048, 1, stream) == 0

    launch = {"gather": gather, "index_then_cast": two_step}
    model.gather_window_rows(feats, starts, T, torch.float16, out=one)                   # the checked path once: the starts are legal
    two_step()
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    us = {name: [] for name in launch}
    for fn in launch.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):                                                              # alternate, so drift hits both alike
        for name, fn in launch.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / iters)
    best = {name: min(v) for name, v in us.items()}
    return {"windows": len(starts), "t": T, "rows": rows, "gather_op_us": round(best["gather"], 2),
            "index_then_cast_us": round(best["index_then_cast"], 2), "two_step_over_gather": round(best["index_then_cast"] / best["gather"], 3),
            "gather_op_us_rounds": [round(v, 2) for v in us["gather"]], "index_then_cast_us_rounds": [round(v, 2) for v in us["index_then_cast"]],
            "fp32_intermediate_bytes_removed": rows * 2048 * 4, "bit_equal": True}


def synthetic_video(n):
    """n frames (H, W, 3) uint8: one random frame, shifted by a few pixels per frame."""
    base = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = np.empty((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        frames[i] = np.roll(base, (3 * i, 5 * i), axis=(0, 1))
    return frames


def window_by_window(backbone, head, frames, box, flip):
    from implementation_phd_lab_vision_amd import frames as F
    from implementation_phd_lab_vision_amd import predict
    from implementation_phd_lab_vision_amd.sequences import SequenceTable, stitch_poses
    n = frames.shape[0]
    dev_frames = torch.from_numpy(frames).to(DEV)
    starts = predict.window_starts(n, T, STRIDE)
    perm = predict.MirrorPerm(predict.flip_perm(17), DEV)
    pred = torch.empty((len(starts), T, 17, 3), dtype=torch.float32, device=DEV)
    for w, s in enumerate(starts):
        clip = dev_frames[s:s + T]
        p = head.joints(backbone.features_from_video(clip, box, F.RESIZE_FLOAT)[None])[0]
        if flip:
            q = head.joints(backbone.features_u8(F.crop_and_resize_video_uint8(clip, box, 224, F.RESIZE_FLOAT, hflip=True))[None])[0]
            predict.merge_mirrored_poses(p, q, perm, out=p)
        pred[w] = p
    table = SequenceTable.from_clips(predict.window_clips(starts, T), T)
    return stitch_poses(pred, pred, (table.offsets, table.src), "context", 1 + 4 * head.number_blocks)[0]


def time_passes(n, passes):
    from implementation_phd_lab_vision_amd import predict, train
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(DEV).eval()
    backbone = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=256).to(DEV).eval()
    frames = synthetic_video(n)
    box = predict.centred_square(H, W).tolist()
    out = {"frames": n, "height": H, "width": W, "box": box, "windows": int(len(predict.window_starts(n, T, STRIDE))), "latent_dim": d,
           "head_precision": "fp16", "backbone_precision": "bf16"}
    for flip in (False, True):
        p = predict.VideoPredictor(backbone, head, seq_len=T, stride=STRIDE, flip_tta=flip)
        forms = {"predict": lambda: torch.from_numpy(p.predict(frames, box=box)["joints3d"]).to(DEV),
                 "window_by_window": lambda: window_by_window(backbone, head, frames, box, flip)}
        p.predict(frames[:2 * T], box=box)                                                  # warm-up: every kernel of both forms once
        window_by_window(backbone, head, frames[:T + STRIDE], box, flip)
        secs = {name: [] for name in forms}
        res = {}
        for _ in range(passes):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = fn()
                torch.cuda.synchronize()
                secs[name].append(time.perf_counter() - t0)
        key = "flip_tta" if flip else "plain"
        out[key] = {"predict_s": [round(v, 3) for v in secs["predict"]], "window_by_window_s": [round(v, 3) for v in secs["window_by_window"]],
                    "predict_frames_per_s": round(n / min(secs["predict"]), 1),
                    "window_by_window_frames_per_s": round(n / min(secs["window_by_window"]), 1),
                    "speedup": round(min(secs["window_by_window"]) / min(secs["predict"]), 2), "stats": dict(p.stats),
                    "bit_equal": bool(torch.equal(res["predict"], res["window_by_window"]))}
    backbone.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "gather": [time_gather(w, a.iters, a.rounds, a.warmup) for w in (193, 8)], "pass": time_passes(a.frames, a.passes)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
