"""The results CLI on the MI355X (src/results.py): the whole-frame resize kernel against torch's CPU ``F.interpolate`` path,
``evaluate`` over a given batch order, and end-to-end runs of ``python -m implementation_phd_lab_vision_amd.results`` on a small S9
cache with a fake video reader.  CLI runs are fresh child processes under a time limit."""
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import results_data as rd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
BS = 4


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("results")
    return rd.make_results_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


def _torch_resize_f32(frames_nhwc_u8: torch.Tensor, size: int) -> torch.Tensor:
    """``_resize_video_hw`` (src/results.py:81-93) restated with torch ops on the CPU, up to (not including) the ``.byte()``: the fp32
    value in [0, 255] that is then truncated, (n, size, size, 3)."""
    v = frames_nhwc_u8.permute(0, 3, 1, 2).float() / 255.0
    v = F.interpolate(v, size=(size, size), mode="bilinear", align_corners=False)
    return (v.clamp(0, 1) * 255.0).permute(0, 2, 3, 1).contiguous()


def _torch_resize(frames_nhwc_u8: torch.Tensor, size: int) -> torch.Tensor:
    return _torch_resize_f32(frames_nhwc_u8, size).byte()


# ------------------------------------------------------------------ kernel ----------------------------------------------------
@pytest.mark.parametrize("h,w,n,size", [(1000, 1002, 3, 224), (1002, 1000, 3, 224), (100, 100, 4, 224), (37, 53, 5, 112),
                                        (480, 640, 2, 97), (64, 48, 3, 1), (224, 224, 3, 224)])
def test_resize_kernel_matches_torch_cpu(lib, h, w, n, size):
    from implementation_phd_lab_vision_amd.frames import resize_frames_uint8
    g = torch.Generator().manual_seed(h * 7 + w + size)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    if h == w == size:
        frames.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)          # every byte value through the identity
    idx = [n - 1, 0, 0, 1, n - 1, n - 1] + list(range(n))                      # repeats, padding, any order
    got = resize_frames_uint8(frames.to(DEV), torch.tensor(idx, dtype=torch.int32), size).cpu()
    want = _torch_resize(frames[idx], size)
    assert got.shape == (len(idx), size, size, 3) and got.dtype == torch.uint8
    diff = (got.int() - want.int()).abs()
    bad = int((diff > 0).sum())
    print(f"resize {n}x{h}x{w} -> {size}: {bad} of {diff.numel()} bytes differ from torch's CPU path (max {int(diff.max())})")
    if h == w == size:
        assert bad == 0
    else:
        assert int(diff.max()) <= 1 and bad <= 1e-4 * diff.numel()


# Distance of torch's own fp32 value (before ``.byte()`` truncates it) from an integer below which the kernel may land on the other side.
# The kernel evaluates the same expression as torch's CPU loop with its own contraction: at most three roundings of values in [0, 1]
# (half an ulp each, 2^-25), scaled by 255 (3 * 255 * 2^-25 < 2^-15.4), plus the rounding of the product with 255 (half an ulp below
# 256, 2^-17): below 2^-15 in all.  2^-14 is twice that.
INTEGER_BAND = 2.0 ** -14


@pytest.mark.parametrize("h,w,n,size", [(2, 3, 2, 224), (1, 1, 2, 8), (7, 1, 2, 12), (1, 7, 2, 12), (500, 131, 2, 344), (40, 8, 2, 448)])
def test_resize_kernel_differs_from_torch_only_next_to_an_integer(lib, h, w, n, size):
    """Up-scaling from a tiny source, one-pixel rows and columns, a non-square source: values that sit exactly on an integer before the
    truncation are common there (the source bytes themselves come back), so a share of the bytes says nothing.  Instead: at most 1,
    and only where torch's own value before the truncation lies within ``INTEGER_BAND`` of an integer."""
    from implementation_phd_lab_vision_amd.frames import resize_frames_uint8
    g = torch.Generator().manual_seed(h * 7 + w + size)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    idx = [n - 1, 0] + list(range(n))
    got = resize_frames_uint8(frames.to(DEV), torch.tensor(idx, dtype=torch.int32), size).cpu()
    before = _torch_resize_f32(frames[idx], size)
    want = before.byte()
    assert got.shape == want.shape == (len(idx), size, size, 3) and got.dtype == torch.uint8
    diff = (got.int() - want.int()).abs()
    dist = (before.double() - before.double().round()).abs()[diff > 0]
    worst = float(dist.max()) if dist.numel() else 0.0
    print(f"resize {n}x{h}x{w} -> {size}: {int((diff > 0).sum())} of {diff.numel()} bytes differ from torch's CPU path (max {int(diff.max())}), "
          f"largest distance of torch's value from an integer there {worst:.3g}")
    assert int(diff.max()) <= 1
    assert worst <= INTEGER_BAND


def test_resize_kernel_writes_only_its_slice(lib):
    from implementation_phd_lab_vision_amd.frames import resize_frames_uint8
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (6, 50, 70, 3), dtype=torch.uint8, generator=g)
    buf = torch.full((3, 5, 33, 33, 3), 0xAB, dtype=torch.uint8, device=DEV)
    idx = torch.tensor([5, 2, 2, 0, 4], dtype=torch.int32, device=DEV)
    out = resize_frames_uint8(frames.to(DEV), idx, 33, out=buf[1])
    assert out.data_ptr() == buf[1].data_ptr()
    host = buf.cpu()
    assert torch.all(host[0] == 0xAB) and torch.all(host[2] == 0xAB)
    assert torch.equal(host[1], resize_frames_uint8(frames.to(DEV), [5, 2, 2, 0, 4], 33).cpu())


def test_resize_kernel_refuses_bad_arguments(lib):
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.frames import resize_frames_uint8
    frames = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device=DEV)
    for idx in ([0, 4], [-1], [1, 2, 3, 100]):
        with pytest.raises(_lib.R50Error, match="outside"):
            resize_frames_uint8(frames, idx, 16)
    out = torch.empty(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for args in ((frames.data_ptr(), 4, 8, 8, idx.data_ptr(), 2, out.data_ptr(), 0, stream),      # out_size 0
                 (frames.data_ptr(), 0, 8, 8, idx.data_ptr(), 2, out.data_ptr(), 16, stream),     # no frames
                 (frames.data_ptr(), 4, 8, 8, idx.data_ptr(), 0, out.data_ptr(), 16, stream),     # empty map
                 (frames.data_ptr(), 4, 8, 8, None, 2, out.data_ptr(), 16, stream),
                 (frames.data_ptr(), 4, 8, 30000, idx.data_ptr(), 2, out.data_ptr(), 16, stream)):  # rows too wide for LDS
        assert lib.r50_op_resize_frames_u8(*args) != 0
        assert b"r50_op_resize_frames_u8" in lib.r50_last_error(None)
    with pytest.raises(ValueError):
        resize_frames_uint8(frames, [0], 0)
    with pytest.raises(ValueError):
        resize_frames_uint8(frames.cpu(), [0], 16)                             # no CPU fallback
    with pytest.raises(ValueError):
        resize_frames_uint8(frames, [0, 1], 16, out=torch.empty(2, 16, 16, 3, dtype=torch.uint8, device=DEV)[:, :8])
    assert torch.equal(frames, torch.zeros_like(frames))


# ------------------------------------------------------------------ evaluate --------------------------------------------------
def test_evaluate_over_given_batches(lib, trees):
    from implementation_phd_lab_vision_amd import results, train
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    store = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    assert len(store) == rd.N_S9
    sd = lo.synthetic_head_state_dict(1024, 2, 4)
    head = results.build_head(sd, DEV)
    default = train.evaluate(head, store, BS, test_set=True)
    assert train.evaluate(head, store, BS, test_set=True, batches=None) == default
    assert train.evaluate(head, store, 999, batches=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]) == default
    order, _ = results.loader_batch_order(len(store), BS, 0)
    loss, mpjpe, l3d, l2d = train.evaluate(head, store, BS, test_set=True, batches=order)
    assert loss == l3d and l2d == 0.0
    ls, ms = [], []
    for idx in order:                                          # the reference's evaluate(), per batch, on the host
        feats, j3d = store.get_batch(idx)[:2]
        pred = lo.forward_reference(sd, feats.cpu())[2]
        ls.append(float((pred - j3d.cpu()).pow(2).mean()))
        ms.append(float(torch.norm(pred - j3d.cpu(), dim=-1).mean()))
    want_l, want_m = sum(ls) / len(order), sum(ms) / len(order)
    assert abs(mpjpe - want_m) <= 5e-3 * want_m, (mpjpe, want_m)
    assert abs(loss - want_l) <= 1e-2 * want_l, (loss, want_l)
    assert (loss, mpjpe) != default[:2]                        # a different order over fewer clips: different numbers


# ------------------------------------------------------------------ CLI -------------------------------------------------------
def _cli(*argv, timeout=600, ok=True):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def _same_meta(a: dict, b: dict) -> bool:
    if set(a) != set(b):
        return False
    return all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)


def _expected_video(meta, videos_root, skip, size, reader=rd.read_video):
    """The reference's clip video: ``frames[::skip][start:end]``, pad / trim, then (size > 0) the kernel on those frames."""
    from implementation_phd_lab_vision_amd.frames import resize_frames_uint8
    from implementation_phd_lab_vision_amd.results import find_video_path
    frames = reader(find_video_path(str(videos_root), meta))[::skip][int(meta["start"]):int(meta["end"])]
    if frames.shape[0] < rd.SEQ_LEN:
        frames = torch.cat([frames, frames[-1:].expand(rd.SEQ_LEN - frames.shape[0], *frames.shape[1:])])
    frames = frames[:rd.SEQ_LEN].contiguous()
    if size == 0:
        return frames.numpy()
    return resize_frames_uint8(frames.to(DEV), list(range(rd.SEQ_LEN)), size).cpu().numpy()


@pytest.mark.parametrize("case", ["train_ckpt_reference_frames", "plain_2048_aligned", "no_resize"])
def test_cli_end_to_end(lib, trees, tmp_path, case):
    from implementation_phd_lab_vision_amd import results, train
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    features, videos = trees
    dims, aligned, size, save_n, seed = {"train_ckpt_reference_frames": ((1024, 2), False, 224, 3, 0),
                                         "plain_2048_aligned": ((2048, 3), True, 56, 16, 5),
                                         "no_resize": ((1024, 2), False, 0, 4, 1)}[case]
    sd = lo.synthetic_head_state_dict(*dims, seed=2)
    ckpt = tmp_path / "model.pt"
    if case == "plain_2048_aligned":
        torch.save(sd, ckpt)                                   # a plain state dict, as the reference's results.py expects
    else:                                                      # a training checkpoint of this project's driver
        th = train.TrainableHead(dims[0], 17, dims[1])
        th.load_state_dict(sd)
        th.to(DEV)
        train.save_checkpoint(str(ckpt), th, train.AdamW(th), 0, 1.0, {"lr": 1e-4})
    out = tmp_path / "sub" / "batch.npz"
    argv = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--out", str(out),
            "--seq-len", str(rd.SEQ_LEN), "--batch-size", str(BS), "--save-n", str(save_n), "--video-size", str(size),
            "--seed", str(seed), "--video-reader", "tests.results_data:" + ("read_video_same_size" if size == 0 else "read_video")]
    t0 = time.time()
    r = _cli(*argv, *(["--aligned-video"] if aligned else []))
    wall = time.time() - t0
    assert "Test metrics | loss: " in r.stdout and "[OK] Saved batch to: " in r.stdout
    print(f"{case}: CLI wall {wall:.1f}s;", [l for l in r.stdout.splitlines() if l.startswith("Results time")])

    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(sd, DEV)
    assert (head.latent_dim, head.number_blocks) == dims
    order, dump_idx = results.loader_batch_order(len(store), BS, seed)
    metrics = train.evaluate(head, store, BS, test_set=True, batches=order)
    feats, j3d, j2d, k, metas = store.get_batch(dump_idx)
    n = min(BS, save_n)

    z = np.load(out, allow_pickle=True)
    assert set(z.files) == {"video", "joints3d", "predicted3djoints", "joints2d", "K", "meta", "test_metrics"}
    hw = size if size else None
    assert z["video"].dtype == np.uint8 and z["video"].shape[:2] == (n, rd.SEQ_LEN) and z["video"].shape[-1] == 3
    if hw:
        assert z["video"].shape[2:4] == (hw, hw)
    assert z["test_metrics"].dtype == np.float32 and np.array_equal(z["test_metrics"], np.array(metrics, dtype=np.float32))
    pred = head.joints(feats)[:n].cpu()
    assert z["predicted3djoints"].shape == (n, rd.SEQ_LEN, 17, 3)
    assert np.array_equal(z["predicted3djoints"], pred.numpy())
    ref = lo.forward_reference(sd, feats.cpu())[2][:n]
    m_dev = float(torch.norm(pred - j3d[:n].cpu(), dim=-1).mean())
    m_ref = float(torch.norm(ref - j3d[:n].cpu(), dim=-1).mean())
    assert abs(m_dev - m_ref) <= 5e-3 * m_ref, (m_dev, m_ref)
    assert np.array_equal(z["joints3d"], j3d[:n].cpu().numpy()) and np.array_equal(z["joints2d"], j2d[:n].cpu().numpy())
    assert z["K"].dtype == np.float32 and np.array_equal(z["K"], k[:n].cpu().numpy())
    assert z["meta"].dtype == object and len(z["meta"]) == n and all(_same_meta(a, b) for a, b in zip(z["meta"], metas[:n]))

    skip = rd.FRAME_SKIP if aligned else 1                     # shard metas carry no frame_skip: the reference slices with 1
    for b in range(n):
        reader = rd.read_video_same_size if size == 0 else rd.read_video
        assert np.array_equal(z["video"][b], _expected_video(metas[b], videos, skip, size, reader)), b
    if size == 224:                                            # the dump against torch's CPU resize, within the kernel's tolerance
        for b in range(n):
            want = _expected_video(metas[b], videos, skip, 0)
            diff = np.abs(z["video"][b].astype(int) - _torch_resize(torch.from_numpy(want), 224).numpy().astype(int))
            assert diff.max() <= 1 and (diff > 0).sum() <= 1e-4 * diff.size


def test_cli_refusals_leave_no_file(lib, trees, tmp_path):
    from oracle import lifting_oracle as lo
    features, videos = trees
    ckpt = tmp_path / "model.pt"
    torch.save(lo.synthetic_head_state_dict(1024, 2, seed=0), ckpt)
    out = tmp_path / "never.npz"
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--out", str(out),
            "--seq-len", str(rd.SEQ_LEN)]
    r = _cli(*base, "--batch-size", str(BS), "--video-reader", "no_such_reader_module:read", ok=False)
    assert r.returncode not in (0, 124, 137) and "video-reader" in r.stderr and not out.exists()
    r = _cli(*base, "--batch-size", str(rd.N_S9 + 1), "--video-reader", "tests.results_data:read_video", ok=False)
    assert r.returncode not in (0, 124, 137) and "fewer than one batch" in r.stderr and not out.exists()
