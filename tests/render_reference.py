"""fp64 numpy restatement of the pixel rule of ``r50_op_draw_skeletons_u8`` (include/r50.h), the oracle
of tests/test_render_gpu.py, and the margin within which the device's fp32 blend may round a byte the other way.

The rule, per frame and pixel p = (x = column, y = row), layers l = 0 .. L-1 in order:

    d_e = min over the edges with two finite end points of the distance from p to the segment (zero length: a point)
    d_j = min over the finite joints of |p - joint|
    a   = max(clamp(half_width + 0.5 - d_e, 0, 1), clamp(joint_radius + 0.5 - d_j, 0, 1)) * A / 255
    c   = c * (1 - a) + rgb * a          per channel, from the background byte
    out = clamp(floor(c + 0.5), 0, 255)

``draw_reference`` returns the bytes, the value ``c`` before the rounding, and which pixels some layer blended (a > 0).

The margin.  The device forms d^2 in fp64 and everything from the square root on in fp32; u = 2^-24 is fp32's unit roundoff.
For point coordinates in [-64, 512] and pixels in [0, 512) every difference is below R = 576 sqrt(2) < 815 px, and with radii
half_width, joint_radius <= 16 only distances up to rho = 16.5 px matter (beyond, both sides clamp to 0):

 1. d^2 in fp64: the differences (p - a), (b - a), the projection t and the residual q = r - t d each round at 2^-53 relative to
    magnitudes <= R, so the distance is off by less than 14 * 815 * 2^-53 < 2e-12 px: a few fp64 ulp of the differences, nothing
    next to what follows.  (In fp32 the same term would be 14 * 815 * u = 7e-4 px, i.e. 0.17 grey levels per layer: that is why
    the distances are fp64.)
 2. one conversion to fp32 (relative u on d^2, u / 2 on d) and one fp32 square root (allowed 1 ulp = 2 u): |delta d| <= 2.5 u rho.
 3. the coverage clamp(fl(radius + 0.5) - d): the constant rounds by <= u rho, the subtraction, where its result lies in [0, 1], by
    <= u:  |delta cov| <= 3.5 u rho + u.
 4. a = max(cov_e, cov_j) * fl(A / 255): the quotient is good to 2 u, the product to u, both factors <= 1:
    |delta a| <= 3.5 u rho + 4 u <= 62 u.
 5. the blend c' = fl(fl(c fl(1 - a)) + fl(rgb a)) with c, rgb <= 255: the error of a moves it by |rgb - c| |delta a| <= 255 * 62 u,
    and its four roundings by <= 255 u each; an error already in c is carried with weight (1 - a) <= 1.  Per layer: <= 66 * 255 u.
 6. fl(c + 0.5) rounds by <= 256 u; the floor is exact.

So after L layers the device's c + 0.5 is within  margin(L) = (66 * 255 * L + 256) u + 1e-9  grey levels of the exact one: 1.0e-3 for
one layer, 3.0e-3 for three, 8.0e-3 for eight.  The device byte must equal the oracle's wherever the oracle's c + 0.5 is farther than
that from an integer, and may differ by one where it is nearer.  The figure is derived from the formats alone; it was not tuned on
the kernel's output.
"""
import numpy as np

U32 = 2.0 ** -24
MAX_LAYERS = 8


def margin(layers: int = MAX_LAYERS) -> float:
    """The derived margin in grey levels after ``layers`` blends (module docstring)."""
    return (66.0 * 255.0 * layers + 256.0) * U32 + 1e-9


def draw_reference(bg, bg_rgb, pts, style, edges, half_width, joint_radius, hw=None):
    """bg (F,H,W,3) uint8 or None (then 0xRRGGBB ``bg_rgb`` on ``hw`` = (H,W)), pts (F,L,J,2) fp32, style (F,L,4) uint8, edges (E,2).
    Returns (out uint8 (F,H,W,3), c float64 (F,H,W,3) before the rounding, blended bool (F,H,W))."""
    pts = np.asarray(pts, dtype=np.float32).astype(np.float64)
    style = np.asarray(style, dtype=np.uint8)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    f, layers, _, _ = pts.shape
    if bg is not None:
        c = np.asarray(bg, dtype=np.uint8).astype(np.float64)
        h, w = c.shape[1:3]
    else:
        h, w = hw
        c = np.empty((f, h, w, 3), dtype=np.float64)
        c[...] = [(bg_rgb >> 16) & 255, (bg_rgb >> 8) & 255, bg_rgb & 255]
    re = float(np.float32(half_width)) + 0.5
    rj = float(np.float32(joint_radius)) + 0.5
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    blended = np.zeros((f, h, w), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(f):
            for l in range(layers):
                p = pts[i, l]
                fin = np.isfinite(p).all(axis=1)
                d_e = np.full((h, w), np.inf)
                for a_i, b_i in edges:
                    if not (fin[a_i] and fin[b_i]):
                        continue
                    a, d = p[a_i], p[b_i] - p[a_i]
                    rx, ry = px - a[0], py - a[1]
                    len2 = d[0] * d[0] + d[1] * d[1]
                    t = np.clip((rx * d[0] + ry * d[1]) / len2, 0.0, 1.0) if len2 > 0.0 else 0.0
                    d_e = np.minimum(d_e, np.hypot(rx - t * d[0], ry - t * d[1]))
                d_j = np.full((h, w), np.inf)
                for j in np.nonzero(fin)[0]:
                    d_j = np.minimum(d_j, np.hypot(px - p[j, 0], py - p[j, 1]))
                a = np.maximum(np.clip(re - d_e, 0.0, 1.0), np.clip(rj - d_j, 0.0, 1.0)) * (float(style[i, l, 3]) / 255.0)
                blended[i] |= a > 0.0
                c[i] = c[i] * (1.0 - a)[..., None] + style[i, l, :3].astype(np.float64) * a[..., None]
    out = np.clip(np.floor(c + 0.5), 0.0, 255.0).astype(np.uint8)
    return out, c, blended


def near_boundary(c, delta):
    """bool (F,H,W,3): the oracle's c + 0.5 lies within ``delta`` of an integer, so an fp32 blend may round that byte either way."""
    t = c + 0.5
    return np.abs(t - np.round(t)) <= delta


def check_against(got, ref, delta):
    """(max |got - out|, bytes that differ where they must not, near-boundary bytes) of device bytes ``got`` against
    ``ref = draw_reference(...)``."""
    out, c, _ = ref
    diff = np.abs(np.asarray(got).astype(np.int64) - out.astype(np.int64))
    near = near_boundary(c, delta)
    return int(diff.max()), int(((diff > 0) & ~near).sum()), int(near.sum())


def near_fraction(ref, delta):
    """Share of the blended pixels with a byte the margin leaves open."""
    _, c, blended = ref
    n = int(blended.sum())
    return (int((near_boundary(c, delta).any(axis=-1) & blended).sum()) / n) if n else 0.0


# ---- the seeded inputs of the oracle-parity tests (tests/test_render_gpu.py; their margin condition is checked in
# tests/test_render_cpu.py from the oracle alone) ----
H36M_EDGES = [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14),
              (14, 15), (15, 16)]
#               name: (F, H, W, L, seed)
PARITY_CASES = {"byte_37x53": (3, 37, 53, 3, 11), "vec_32x64": (2, 32, 64, 3, 12), "vec_224": (2, 224, 224, 3, 13)}
PARITY_HALF_WIDTH, PARITY_JOINT_RADIUS = 1.0, 2.0
MAX_NEAR_SHARE = 0.02


def parity_inputs(name):
    """(bg (F,H,W,3) uint8, pts (F,L,17,2) fp32, style (F,L,4) uint8) of a parity case: random skeletons whose joints lie inside the
    canvas, exactly on its border (x or y equal to 0 or to the last pixel centre) and up to a quarter canvas outside it; alphas 255 and 153."""
    f, h, w, layers, seed = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    pts = rng.uniform([-0.25 * w, -0.25 * h], [1.25 * w, 1.25 * h], (f, layers, 17, 2))
    pts[:, :, 3, 0] = 0.0                       # on the left border
    pts[:, :, 6, 1] = h - 1.0                   # on the bottom border
    pts[:, :, 10, 0] = w - 1.0                  # on the right border
    pts[:, :, 13] = [0.0, 0.0]                  # the top-left pixel's centre
    pts[:, :, 16] = [w + 7.5, -3.25]            # outside
    style = rng.integers(0, 256, (f, layers, 4), dtype=np.uint8)
    style[..., 3] = np.array([255, 153, 255, 153, 153, 255, 153, 255])[:layers]
    return bg, pts.astype(np.float32), style
