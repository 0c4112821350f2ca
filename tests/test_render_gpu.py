"""``r50_op_draw_skeletons_u8`` and the render path on the MI355X, against the fp64 oracle of tests/render_reference.py: a device byte
may differ from the oracle's by one, and only where the oracle's value lies within the derived margin of a rounding boundary."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import png_reader
from tests import render_reference as rr
from tests import results_data as rd
from tests.kernel_cases import _assert_matches  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
EDGES = rr.H36M_EDGES


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _draw(bg, pts, style, edges, half_width, joint_radius, **kw):
    from implementation_phd_lab_vision_amd.render import draw_skeletons
    out = draw_skeletons(None if bg is None else torch.from_numpy(bg).to(DEV), torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(DEV),
                         torch.from_numpy(style).to(DEV), edges, half_width, joint_radius, **kw)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def parity_refs():
    """The oracle of each parity case, computed once and shared."""
    out = {}
    for name in rr.PARITY_CASES:
        bg, pts, style = rr.parity_inputs(name)
        out[name] = (bg, pts, style, rr.draw_reference(bg, 0, pts, style, EDGES, rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS))
    return out


# ------------------------------------------------------------------ oracle parity ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.PARITY_CASES))
def test_oracle_parity(lib, parity_refs, name):
    """byte_37x53: the per-byte path (w % 4 != 0); vec_32x64, vec_224: the 12-byte path into a freshly allocated tensor."""
    layers = rr.PARITY_CASES[name][3]
    bg, pts, style, ref = parity_refs[name]
    share = rr.near_fraction(ref, rr.margin(layers))
    assert share <= rr.MAX_NEAR_SHARE, share
    got = _draw(bg, pts, style, EDGES, rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS)
    _assert_matches(got, ref, layers, f"{name} ({share:.3%} of the blended pixels within the margin)")


def test_both_paths_give_the_same_bytes(lib, parity_refs):
    """A w % 4 == 0 canvas through the per-byte path (bg and out one byte off alignment) equals the vector path's result."""
    from implementation_phd_lab_vision_amd.render import draw_skeletons
    bg, pts, style, ref = parity_refs["vec_32x64"]
    want = _draw(bg, pts, style, EDGES, rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS)
    n = bg.size
    raw_bg, raw_out = torch.zeros(n + 4, dtype=torch.uint8, device=DEV), torch.full((n + 4,), 0xCD, dtype=torch.uint8, device=DEV)
    raw_bg[1:n + 1] = torch.from_numpy(bg).to(DEV).reshape(-1)
    out = raw_out[1:n + 1].view(bg.shape)
    assert out.data_ptr() % 4 == 1
    draw_skeletons(raw_bg[1:n + 1].view(bg.shape), torch.from_numpy(pts).to(DEV), torch.from_numpy(style).to(DEV), EDGES,
                   rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    host = raw_out.cpu()
    assert host[0] == 0xCD and torch.all(host[n + 1:] == 0xCD)                  # nothing outside its slice


# ------------------------------------------------------------------ exact cases ------------------------------------------------------
def test_exact_cases(lib):
    rng = np.random.default_rng(5)
    h, w = 40, 52
    bg = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    pts = np.zeros((2, 2, 3, 2), dtype=np.float32)
    pts[:, 0] = [[6.0, 8.0], [40.0, 8.0], [40.0, 30.0]]                        # layer 0: an L of two thick bones
    pts[:, 1] = [[10.0, 35.0], [30.0, 20.0], [45.0, 36.0]]                     # layer 1: switched off
    style = np.array([[[250, 3, 128, 255], [9, 9, 9, 0]]] * 2, dtype=np.uint8)
    edges = [(0, 1), (1, 2)]
    got = _draw(bg, pts, style, edges, 3.0, 1.0)
    ref = rr.draw_reference(bg, 0, pts, style, edges, 3.0, 1.0)
    _assert_matches(got, ref, 2, "exact cases")
    untouched = ~ref[2]
    assert untouched.sum() > 0.5 * untouched.size and np.array_equal(got[untouched], bg[untouched])     # the background, bit for bit
    deep = np.zeros((h, w), dtype=bool)
    deep[6:11, 8:39] = True                                                    # |y - 8| <= 2 <= half_width - 0.5 along the first bone
    deep[10:29, 38:43] = True                                                  # and along the second
    assert (got[:, deep] == np.array([250, 3, 128], dtype=np.uint8)).all()     # A = 255 deep inside a bone: the colour exactly
    only1 = style.copy()
    only1[:, 0, 3] = 0                                                         # both layers off: no trace
    assert np.array_equal(_draw(bg, pts, only1, edges, 3.0, 1.0), bg)
    # bg = NULL: the uniform colour, on both paths (w = 52: vector; w = 51: per byte)
    for ww in (52, 51):
        flat = _draw(None, pts, only1, edges, 3.0, 1.0, bg_rgb=0x0A80FE, hw=(h, ww))
        assert flat.shape == (2, h, ww, 3) and (flat == np.array([0x0A, 0x80, 0xFE], dtype=np.uint8)).all()
        got = _draw(None, pts, style, edges, 3.0, 1.0, bg_rgb=(10, 128, 254), hw=(h, ww))
        _assert_matches(got, rr.draw_reference(None, 0x0A80FE, pts, style, edges, 3.0, 1.0, hw=(h, ww)), 2, f"bg NULL, w {ww}")


# ------------------------------------------------------------------ edge cases -------------------------------------------------------
def test_edge_cases(lib):
    rng = np.random.default_rng(6)
    h, w = 37, 53
    bg = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    style = np.array([[[255, 255, 0, 255], [0, 200, 255, 153]]], dtype=np.uint8)
    pts = rng.uniform([2, 2], [w - 3, h - 3], (1, 2, 5, 2)).astype(np.float32)
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]

    def both(name, p, e, st=style, hw_=1.0, jr=2.0):
        got = _draw(bg, p, st, e, hw_, jr)
        ref = rr.draw_reference(bg, 0, p, st, e, hw_, jr)
        _assert_matches(got, ref, p.shape[1], name)
        return got, ref

    _, ref = both("E = 0 (joints only)", pts, [])
    assert ref[2].sum() > 0
    both("J = 2, E = 1", pts[:, :, :2].copy(), [(0, 1)])
    both("widths 0", pts, edges, hw_=0.0, jr=0.0)
    same = pts.copy()
    same[:, :, 1] = same[:, :, 0]                                              # coincident end points: a point, no NaN
    same[:, :, 3] = same[:, :, 4]
    got, _ = both("coincident end points", same, edges + [(2, 2)])
    bad = pts.copy()
    bad[0, 0, 1, 0] = np.nan                                                   # dropped along with the edges at them
    bad[0, 0, 3, 1] = np.inf
    bad[0, 1, 0] = [-np.inf, np.nan]
    got, ref = both("a NaN joint and an inf joint", bad, edges)
    kept = rr.draw_reference(bg, 0, pts, style, edges, 1.0, 2.0)
    assert (ref[0] != kept[0]).any()
    gone = pts.copy()
    gone[0, 0] = np.nan                                                        # a whole layer non-finite: only layer 1 shows
    got, _ = both("a whole layer non-finite", gone, edges)
    off = style.copy()
    off[0, 0, 3] = 0
    assert np.array_equal(got, _draw(bg, pts, off, edges, 1.0, 2.0))
    far = pts.copy()
    far[0, 0] += 1.0e4                                                         # all points far outside
    far[0, 1] = -far[0, 1] - 500.0
    assert np.array_equal(_draw(bg, far, style, edges, 1.0, 2.0), bg)
    far[0, 1, :, 0] = 3.0e38                                                   # and at the end of fp32's range
    assert np.array_equal(_draw(bg, far, style, edges, 1.0, 2.0), bg)


def test_limits_j64_l8_e128(lib):
    rng = np.random.default_rng(7)
    h, w = 33, 36
    bg = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    pts = rng.uniform([-4, -4], [w + 4, h + 4], (1, 8, 64, 2)).astype(np.float32)
    style = rng.integers(0, 256, (1, 8, 4), dtype=np.uint8)
    style[0, :, 3] = [40, 0, 255, 153, 80, 0, 30, 60]
    edges = [(int(a), int(b)) for a, b in rng.integers(0, 64, (128, 2))]
    got = _draw(bg, pts, style, edges, 0.5, 1.0)
    _assert_matches(got, rr.draw_reference(bg, 0, pts, style, edges, 0.5, 1.0), 8, "J 64, L 8, E 128")


# ------------------------------------------------------------------ layer order, seams, determinism ----------------------------------------
def test_layer_order(lib):
    h, w = 24, 28
    bg = np.full((1, h, w, 3), 40, dtype=np.uint8)
    pts = np.array([[[[3.0, 4.0], [24.0, 20.0]], [[24.0, 3.0], [4.0, 21.0]]]], dtype=np.float32)      # an X
    style = np.array([[[255, 0, 0, 255], [0, 0, 255, 153]]], dtype=np.uint8)
    ab = _draw(bg, pts, style, [(0, 1)], 2.0, 1.0)
    ba = _draw(bg, pts[:, ::-1].copy(), style[:, ::-1].copy(), [(0, 1)], 2.0, 1.0)
    _assert_matches(ab, rr.draw_reference(bg, 0, pts, style, [(0, 1)], 2.0, 1.0), 2, "layer order a, b")
    _assert_matches(ba, rr.draw_reference(bg, 0, pts[:, ::-1], style[:, ::-1], [(0, 1)], 2.0, 1.0), 2, "layer order b, a")
    differ = (ab != ba).any(axis=-1)[0]
    assert differ.any() and differ[8:16, 10:18].any() and not differ[:4].any()     # the overlap changes, the arms do not
    centre = (int(round(12.0)), 14)
    assert tuple(ba[0, centre[0], centre[1]]) == (255, 0, 0)                       # the opaque layer on top hides the other


@pytest.mark.parametrize("h,w", [(70, 130), (72, 132)])
def test_tile_seams(lib, h, w):
    """Bones across every boundary of the 32 x 32 tiles (diagonals through all of them, lines along a seam and just beside one): a
    tile that culled a bone it should draw would leave a gap the oracle does not have.  (70, 130): per-byte path; (72, 132): vector."""
    rng = np.random.default_rng(h)
    bg = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    pts = np.zeros((2, 2, 8, 2), dtype=np.float32)
    pts[:, 0] = [[-5.0, -3.0], [w + 5.0, h + 3.0], [-4.0, h + 2.0], [w + 3.0, -6.0], [0.0, 31.5], [w - 1.0, 31.5], [63.5, 0.0], [63.5, h - 1.0]]
    pts[:, 1] = [[2.0, 33.6], [w - 2.0, 30.2], [33.7, 1.0], [30.4, h - 2.0], [95.5, 2.0], [97.1, h - 3.0], [5.0, 63.9], [w - 6.0, 64.2]]
    pts[1] += rng.uniform(-0.5, 0.5, (2, 8, 2)).astype(np.float32)
    style = np.array([[[255, 255, 255, 255], [255, 32, 0, 153]]] * 2, dtype=np.uint8)
    edges = [(0, 1), (2, 3), (4, 5), (6, 7)]
    for half_width, joint_radius in ((1.0, 2.0), (0.0, 4.0), (2.5, 0.0)):
        got = _draw(bg, pts, style, edges, half_width, joint_radius)
        ref = rr.draw_reference(bg, 0, pts, style, edges, half_width, joint_radius)
        _assert_matches(got, ref, 2, f"seams {h}x{w}, widths {half_width} / {joint_radius}")
        seam = np.zeros((h, w), dtype=bool)
        seam[[31, 32, 63, 64], :] = True
        seam[:, [31, 32, 63, 64, 95, 96, 127, 128]] = True
        assert (ref[2] & seam).sum() > 40                                          # the seams are drawn on


def test_determinism(lib, parity_refs):
    bg, pts, style, _ = parity_refs["vec_224"]
    a = _draw(bg, pts, style, EDGES, 1.0, 2.0)
    b = _draw(bg, pts, style, EDGES, 1.0, 2.0)
    assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))


# ------------------------------------------------------------------ validation -------------------------------------------------------
def test_refusals_launch_nothing(lib):
    f, h, w, layers, joints = 2, 8, 12, 2, 3
    bg = torch.zeros((f, h, w, 3), dtype=torch.uint8, device=DEV)
    pts = torch.full((f, layers, joints, 2), 4.0, device=DEV)
    style = torch.full((f, layers, 4), 255, dtype=torch.uint8, device=DEV)
    out = torch.full((f, h, w, 3), 0xCD, dtype=torch.uint8, device=DEV)
    edges = (C.c_int * 4)(0, 1, 1, 2)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(bg=bg.data_ptr(), rgb=0, pts=pts.data_ptr(), style=style.data_ptr(), edges=edges, e=2, f=f, h=h, w=w, l=layers, j=joints,
                hw=1.0, jr=1.0, out=out.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.r50_op_draw_skeletons_u8(a["bg"], a["rgb"], a["pts"], a["style"], a["edges"], a["e"], a["f"], a["h"], a["w"], a["l"], a["j"],
                                            a["hw"], a["jr"], a["out"], stream)

    cases = {"null pts": dict(pts=None), "null style": dict(style=None), "null out": dict(out=None), "null edges": dict(edges=None),
             "f < 1": dict(f=0), "J > 64": dict(j=65), "L > 8": dict(l=9), "E > 128": dict(e=129), "h < 1": dict(h=0),
             "edge index >= J": dict(edges=(C.c_int * 4)(0, 1, 1, 3)), "edge index < 0": dict(edges=(C.c_int * 4)(0, -1, 1, 2)),
             "negative width": dict(hw=-0.5), "negative radius": dict(jr=-1.0), "NaN width": dict(hw=float("nan")),
             "out is bg": dict(bg=out.data_ptr()), "out overlaps bg": dict(bg=out.data_ptr() + 3 * w)}
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc != 0, name
        assert b"r50_op_draw_skeletons_u8" in lib.r50_last_error(None), name
    torch.cuda.synchronize()
    assert torch.all(out == 0xCD) and torch.all(bg == 0)                           # nothing was launched
    assert call() == 0                                                         # and a valid call afterwards works
    torch.cuda.synchronize()
    assert not torch.all(out == 0xCD) and tuple(out[0, 4, 4].tolist()) == (255, 255, 255)
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.render import draw_skeletons
    with pytest.raises(_lib.R50Error, match="outside"):
        draw_skeletons(bg, pts, style, [(0, 3)], 1.0, 1.0)
    with pytest.raises(ValueError):
        draw_skeletons(bg, pts.cpu(), style, [(0, 1)], 1.0, 1.0)                   # no CPU fallback
    with pytest.raises(ValueError):
        draw_skeletons(bg, pts, style, [(0, 1)], 1.0, 1.0, out=out[:, :, :6])


# ------------------------------------------------------------------ render_panels ------------------------------------------------------
def _panel_inputs(n=2, t=3, s=32, seed=8):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (n, t, s, s, 3), dtype=torch.uint8, generator=g)
    j2d = torch.rand(n, t, 17, 2, generator=g) * (s + 8) - 4.0
    gt = torch.randn(n, t, 17, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 4.0])
    pred = gt + 0.05 * torch.randn(n, t, 17, 3, generator=g)
    k = torch.eye(3).repeat(n, 1, 1)
    k[:, 0, 0] = k[:, 1, 1] = 40.0
    k[:, 0, 2] = k[:, 1, 2] = s / 2.0
    gt[0, 1, 5, 2] = -1.0                                                       # a joint behind the camera: dropped from panel 1
    return frames, j2d, k, gt, pred


def _expected_panels(frames, j2d, k, gt, pred_used, pred_rgb, pred_alpha, render):
    """Three oracle draws pasted side by side, fed the fp32 points the same torch ops give on the device."""
    n, t, s = frames.shape[:3]
    bg = frames.reshape(n * t, s, s, 3).numpy()
    dev = lambda x: x.to(DEV)                                                      # noqa: E731
    host = lambda *q: torch.stack([x.reshape(n * t, 17, 2) for x in q], dim=1).float().cpu().numpy()   # noqa: E731
    gt_d, pr_d, k_d = dev(gt), dev(pred_used), dev(k)
    centre = gt_d[:, :, 0]
    st1 = np.zeros((n * t, 1, 4), dtype=np.uint8)
    st1[:, 0] = [*render.GT_RGB, 255]
    st2 = np.zeros((n, t, 2, 4), dtype=np.uint8)
    st2[:, :, 0] = [*render.GT_RGB, 153]
    st2[:, :, 1, :3] = pred_rgb
    st2[:, :, 1, 3] = pred_alpha
    st3 = st2.copy()
    st3[:, :, 0, 3] = 255
    st2, st3 = st2.reshape(n * t, 2, 4), st3.reshape(n * t, 2, 4)
    refs = [rr.draw_reference(bg, 0, host(dev(j2d)), st1, EDGES, 1.0, 2.0),
            rr.draw_reference(bg, 0, host(render.project(gt_d, k_d), render.project(pr_d, k_d)), st2, EDGES, 1.0, 2.0),
            rr.draw_reference(None, render.PANEL_BG_RGB, host(render.view_points(gt_d, centre, size=s), render.view_points(pr_d, centre, size=s)),
                              st3, EDGES, 1.0, 2.0, hw=(s, s))]
    return tuple(np.concatenate([r[i] for r in refs], axis=2) for i in range(3))


def test_render_panels_layout(lib):
    from implementation_phd_lab_vision_amd import render
    frames, j2d, k, gt, pred = _panel_inputs()
    n, t, s = frames.shape[:3]
    dev = lambda x: x.to(DEV)                                                      # noqa: E731
    got = render.render_panels(dev(frames), dev(j2d), dev(k), dev(gt), dev(pred))
    assert tuple(got.shape) == (n, t, s, 3 * s, 3) and got.dtype == torch.uint8 and got.is_cuda
    first = got.cpu().numpy()
    rgb = np.broadcast_to(np.array(render.PRED_RGB, dtype=np.uint8), (n, t, 3))
    ref = _expected_panels(frames, j2d, k, gt, pred, rgb, np.full((n, t), 255, dtype=np.uint8), render)
    _assert_matches(got.cpu().numpy().reshape(n * t, s, 3 * s, 3), ref, 2, "render_panels")
    # with a rollout: input_len 1, P 1 -> frame 0 the reconstruction, frame 1 the forecast in the third colour, frame 2 nothing
    g = torch.Generator().manual_seed(9)
    future = gt[:, 1:2] + 0.05 * torch.randn(n, 1, 17, 3, generator=g)
    got = render.render_panels(dev(frames), dev(j2d), dev(k), dev(gt), dev(pred), dev(future), 1).cpu().numpy()
    used = pred.clone()
    used[:, 1:2] = future
    rgb = np.stack([np.array(c, dtype=np.uint8) for c in (render.PRED_RGB, render.FUTURE_RGB, render.FUTURE_RGB)])[None].repeat(n, axis=0)
    alpha = np.array([255, 255, 0], dtype=np.uint8)[None].repeat(n, axis=0)
    ref = _expected_panels(frames, j2d, k, gt, used, rgb, alpha, render)
    _assert_matches(got.reshape(n * t, s, 3 * s, 3), ref, 2, "render_panels with a rollout")
    has = lambda fr, colour: bool((got[:, fr, :, 2 * s:] == np.array(colour, dtype=np.uint8)).all(axis=-1).any())   # noqa: E731  (3D panel)
    assert has(0, render.PRED_RGB) and not has(0, render.FUTURE_RGB)
    assert has(1, render.FUTURE_RGB) and not has(1, render.PRED_RGB)
    assert not has(2, render.FUTURE_RGB) and not has(2, render.PRED_RGB) and has(2, render.GT_RGB)
    # no frames: the plain background in panels 0 and 1 as well
    plain = render.render_panels(None, dev(j2d), dev(k), dev(gt), dev(pred), size=s).cpu().numpy()
    corner = np.array(render._rgb_tuple(render.PANEL_BG_RGB), dtype=np.uint8)
    assert plain.shape == first.shape and np.array_equal(plain[:, :, :, 2 * s:], first[:, :, :, 2 * s:])      # the 3D panel as before
    twice = np.concatenate([frames.numpy(), frames.numpy()], axis=3)               # panels 0 and 1 of the run with frames
    untouched = (first[:, :, :, :2 * s] == twice).all(axis=-1)
    assert untouched.mean() > 0.3 and (plain[:, :, :, :2 * s][untouched] == corner).all(axis=-1).mean() > 0.99


# ------------------------------------------------------------------ results --render, end to end -------------------------------------------
def _fitted_box(c: int):
    h, w, _ = rd.VIDEOS[list(rd.VIDEOS)[c % len(rd.VIDEOS)]]
    side = min(h, w) - 3
    return torch.tensor([1, 2, side, side])


def _make_cache(root, boxed: bool, n_s9: int = 6, seed: int = 0):
    """The S9 cache of tests/results_data.py (its clip metas, videos and packer settings) with 2D joints and intrinsics in the pixels of
    the 224 x 224 crop, 3D joints in metres, and each clip's box either fitted inside its video's frames or None."""
    from implementation_phd_lab_vision_amd.shards import ShardPacker
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=1, shard_size=4, shuffle_pool=5, shuffle_seed=seed)
    for c in range(n_s9):
        meta = dict(rd.clip_meta(c), box=_fitted_box(c) if boxed else None)
        k = torch.eye(3)
        k[0, 0] = k[1, 1] = 250.0
        k[0, 2] = k[1, 2] = 112.0
        packer.add_group([{"feat": torch.randn(rd.SEQ_LEN, 2048, generator=g).abs(),
                           "joints3d": torch.randn(rd.SEQ_LEN, 17, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 4.0]),
                           "joints2d": torch.rand(rd.SEQ_LEN, 17, 2, generator=g) * 224.0, "K": k, "meta": meta}])
    packer.finish()
    packer.write_index(seq_len=rd.SEQ_LEN, frame_skip=rd.FRAME_SKIP, save_fp16=False, augment=False)
    return Path(root)


def _results(*argv, timeout=600):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


OLD_KEYS = {"video", "joints3d", "predicted3djoints", "joints2d", "K", "meta", "test_metrics"}
ROLLOUT_KEYS = {"predicted_future3djoints", "future_mpjpe", "rollout_lens"}


@pytest.mark.parametrize("boxed", [True, False], ids=["boxed", "box_none"])
def test_results_render_end_to_end(lib, tmp_path, boxed):
    from implementation_phd_lab_vision_amd import render, results
    from implementation_phd_lab_vision_amd.frames import crop_and_resize_video_uint8
    from oracle import lifting_oracle as lo
    features, videos = _make_cache(tmp_path / "features", boxed), rd.make_preprocessed_tree(tmp_path / "videos")
    ckpt = tmp_path / "model.pt"
    torch.save(lo.synthetic_head_state_dict(1024, 2, seed=2), ckpt)
    t, bs, n_render = rd.SEQ_LEN, 4, 3
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--seq-len", str(t),
            "--batch-size", str(bs), "--video-size", "56", "--video-reader", "tests.results_data:read_video"]
    if boxed:
        base += ["--pred-len", "3", "--input-len", "4"]
    outdir = tmp_path / "pictures"
    r = _results(*base, "--out", str(tmp_path / "with.npz"), "--render", str(outdir), "--render-n", str(n_render), "--render-fps", "8",
                 "--render-sheet-every", "3")
    assert f"Rendered {n_render} clips" in r.stdout
    assert r.stdout.count("has no crop box") == (0 if boxed else n_render)
    z = np.load(tmp_path / "with.npz", allow_pickle=True)
    keys = OLD_KEYS | (ROLLOUT_KEYS if boxed else set())
    assert set(z.files) == keys | {"video_crop"}
    crop = z["video_crop"]
    assert crop.shape == (n_render, t, 224, 224, 3) and crop.dtype == np.uint8
    future = torch.from_numpy(z["predicted_future3djoints"][:n_render]).to(DEV) if boxed else None
    dev = lambda key: torch.from_numpy(z[key][:n_render]).to(DEV)                   # noqa: E731
    want = render.render_panels(dev("video_crop"), dev("joints2d"), dev("K"), dev("joints3d"), dev("predicted3djoints"), future,
                                4 if boxed else 0).cpu().numpy()
    names = sorted(p.name for p in outdir.iterdir())
    assert len(names) == 2 * n_render
    for i in range(n_render):
        meta = z["meta"][i]
        anim = outdir / f"clip_{i}_S9_{meta['action']}.png"
        sheet = outdir / f"clip_{i}_sheet.png"
        assert anim.exists() and sheet.exists(), names
        frames, info = png_reader.decode(anim)
        assert info["animated"] and info["num_frames"] == t and frames.shape == (t, 224, 672, 3) and info["delays"][0] == (125, 1000)
        assert np.array_equal(frames, want[i])
        picked, _ = png_reader.decode(sheet)
        assert picked.shape == (1, 3 * 224, 672, 3) and np.array_equal(picked[0], np.concatenate([want[i][0], want[i][3], want[i][6]]))
        if boxed:                                                                # the crop: the clip's own selected frames through frames.py
            full = rd.read_video(results.find_video_path(str(videos), meta))[int(meta["start"]):int(meta["end"])]
            if full.shape[0] < t:
                full = torch.cat([full, full[-1:].expand(t - full.shape[0], *full.shape[1:])])
            ref = crop_and_resize_video_uint8(full[:t].contiguous().to(DEV), meta["box"], 224).permute(0, 2, 3, 1).cpu().numpy()
            assert np.array_equal(crop[i], ref)
            assert (frames[:, :, :224] != crop[i]).any() and (frames[:, :, :224] == crop[i]).mean() > 0.5   # drawn over, mostly kept
        else:
            assert (crop[i] == np.array(render._rgb_tuple(render.PANEL_BG_RGB), dtype=np.uint8)).all()
    # the same run without --render, alongside: exactly the old key set, the same arrays
    r0 = _results(*base, "--out", str(tmp_path / "without.npz"))
    assert "Rendered" not in r0.stdout and "render:" not in r0.stdout
    z0 = np.load(tmp_path / "without.npz", allow_pickle=True)
    assert set(z0.files) == keys
    for key in keys - {"meta"}:
        assert np.array_equal(z0[key], z[key]), key
    drop = lambda out: [l for l in out.splitlines() if not l.startswith(("Rendered", "render:", "Results time", "[OK] Saved"))]   # noqa: E731
    assert drop(r0.stdout) == drop(r.stdout)
    # python -m ...render on the dumps: the same files from the one with video_crop, a notice and plain panels from the other
    again = render.main(["--npz", str(tmp_path / "with.npz"), "--outdir", str(tmp_path / "again"), "--n", str(n_render), "--fps", "8",
                         "--sheet-every", "3"])
    assert sorted(Path(p).name for p in again) == names
    for name in names:
        assert (tmp_path / "again" / name).read_bytes() == (outdir / name).read_bytes(), name
    render.main(["--npz", str(tmp_path / "without.npz"), "--outdir", str(tmp_path / "plain"), "--n", "1"])
    frames, _ = png_reader.decode(next(p for p in (tmp_path / "plain").iterdir() if "sheet" not in p.name))
    assert frames.shape == (t, 224, 672, 3)
