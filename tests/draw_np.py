"""Numpy restatement of the overlay rasteriser ("Drawing on the device"): the yardstick the HIP kernels are compared to.

Pure integer: one unit is 1/8 pixel, a coordinate x becomes rint(8 x) after clamping to [-8192, 16384] px, pixel (x, y) has its centre
at (x, y) and carries 16 samples at 8x + {-3,-1,1,3}, 8y + {-3,-1,1,3}.  A shape's coverage n is the number of samples inside it and
the shape is composited as c <- (c (16 - n) + colour n + 8) >> 4, shape after shape in painter's order: per image the boxes in index
order, then per pose the limbs in table order and the joints in index order (disc, then white ring).  Written shape by shape on the
pixels of each shape's bounding box -- nothing of the kernel's tiling, culling or record lists is shared with it.

Also the float64 restatement of the heatmap overlay's colour index (max, bilinear resize, normalise, floor) and its integer blend.
"""
import numpy as np

OFFS = np.array([-3, -1, 1, 3], dtype=np.int64)


def quant(v):
    """float32 coordinate -> units, or None when it is not finite."""
    v = np.float32(v)
    if not np.isfinite(v):
        return None
    return int(np.rint(np.float32(8.0) * np.clip(v, np.float32(-8192.0), np.float32(16384.0))))


def _window(H, W, x0, y0, x1, y1):
    """Pixels whose samples can fall inside the unit bounding box [x0, x1] x [y0, y1] (generous by one pixel), clipped to the image.
    -> (ys, xs, SX, SY): pixel ranges and the (h, w, 4, 4) sample coordinates, or None if empty."""
    px0, px1 = max(0, x0 // 8 - 1), min(W - 1, -(-x1 // 8) + 1)
    py0, py1 = max(0, y0 // 8 - 1), min(H - 1, -(-y1 // 8) + 1)
    if px0 > px1 or py0 > py1:
        return None
    xs, ys = np.arange(px0, px1 + 1, dtype=np.int64), np.arange(py0, py1 + 1, dtype=np.int64)
    SX = np.broadcast_to((8 * xs)[None, :, None, None] + OFFS[None, None, None, :], (len(ys), len(xs), 4, 4))
    SY = np.broadcast_to((8 * ys)[:, None, None, None] + OFFS[None, None, :, None], (len(ys), len(xs), 4, 4))
    return (py0, py1 + 1), (px0, px1 + 1), SX, SY


def _composite(img, ys, xs, inside, colour):
    n = inside.sum(axis=(2, 3)).astype(np.int64)[..., None]
    c = img[ys[0]:ys[1], xs[0]:xs[1]].astype(np.int64)
    img[ys[0]:ys[1], xs[0]:xs[1]] = ((c * (16 - n) + np.asarray(colour, np.int64)[None, None, :] * n + 8) >> 4).astype(np.uint8)


def draw_joint(img, cx, cy, r, colour):
    """Disc of radius r in `colour`, then the white ring r < d <= r + 1.  cx, cy in units."""
    H, W = img.shape[:2]
    R0, R1 = 8 * r, 8 * (r + 1)
    win = _window(H, W, cx - R1, cy - R1, cx + R1, cy + R1)
    if win is None:
        return
    ys, xs, SX, SY = win
    d2 = (SX - cx) ** 2 + (SY - cy) ** 2
    _composite(img, ys, xs, d2 <= R0 * R0, colour)
    _composite(img, ys, xs, (d2 > R0 * R0) & (d2 <= R1 * R1), (255, 255, 255))


def limb_inside(SX, SY, ax, ay, bx, by, h):
    """Samples inside the capsule from A to B with half-width h (units), all in integers."""
    ex, ey = bx - ax, by - ay
    lq = ex * ex + ey * ey                                  # Python ints: < 2^38
    wx, wy = SX - ax, SY - ay
    s = wx * ex + wy * ey
    near_a = (wx * wx + wy * wy) <= h * h
    if lq == 0:
        return near_a
    near_b = ((SX - bx) ** 2 + (SY - by) ** 2) <= h * h
    cr = np.abs(wx * ey - wy * ex)
    small = cr < (1 << 32)                                  # else certainly outside: h^2 Lq < 2^64
    cu = np.where(small, cr, 0).astype(np.uint64)
    side = small & (cu * cu <= np.uint64(h * h * lq))
    return np.where(s <= 0, near_a, np.where(s >= lq, near_b, side))


def draw_limb(img, ax, ay, bx, by, thickness, colour):
    H, W = img.shape[:2]
    h = 4 * thickness
    win = _window(H, W, min(ax, bx) - h, min(ay, by) - h, max(ax, bx) + h, max(ay, by) + h)
    if win is None:
        return
    ys, xs, SX, SY = win
    _composite(img, ys, xs, limb_inside(SX, SY, ax, ay, bx, by, h), colour)


def draw_box(img, x1, y1, x2, y2, thickness, colour):
    H, W = img.shape[:2]
    t = 4 * thickness
    win = _window(H, W, x1 - t, y1 - t, x2 + t, y2 + t)
    if win is None:
        return
    ys, xs, SX, SY = win
    outer = (SX >= x1 - t) & (SX <= x2 + t) & (SY >= y1 - t) & (SY <= y2 + t)
    inner = (SX > x1 + t) & (SX < x2 - t) & (SY > y1 + t) & (SY < y2 - t)
    _composite(img, ys, xs, outer & ~inner, colour)


def joint_units(kp, sc, k, thr):
    """Joint k of one pose in units, or None when it is not drawn (score below the float32 threshold, or anything not finite)."""
    s = np.float32(sc[k])
    if not np.isfinite(s) or not (s >= np.float32(thr)):
        return None
    x, y = quant(kp[k, 0]), quant(kp[k, 1])
    return None if x is None or y is None else (x, y)


def draw_pose(img, kp, sc, skeleton, colors, thr, r, thickness):
    K = kp.shape[0]
    for a, b in skeleton:
        if not (0 <= a < K and 0 <= b < K):
            continue
        A, B = joint_units(kp, sc, a, thr), joint_units(kp, sc, b, thr)
        if A is not None and B is not None:
            draw_limb(img, A[0], A[1], B[0], B[1], thickness, colors[a % len(colors)])
    for k in range(K):
        J = joint_units(kp, sc, k, thr)
        if J is not None:
            draw_joint(img, J[0], J[1], r, colors[k % len(colors)])


def draw_batch(images, keypoints=None, scores=None, image_index=None, boxes=None, box_image_index=None, skeleton=(), colors=((0, 0, 0),),
               score_threshold=0.3, point_radius=4, line_thickness=2, box_color=(0, 255, 0), box_thickness=2):
    """(N,H,W,3) uint8 -> new batch; the whole painter's order of pk_draw_shapes."""
    out = np.array(images, dtype=np.uint8, copy=True)
    for n in range(out.shape[0]):
        if boxes is not None:
            for q in range(len(boxes)):
                if int(box_image_index[q]) == n:
                    c = [quant(v) for v in boxes[q]]
                    if all(v is not None for v in c):
                        draw_box(out[n], c[0], c[1], c[2], c[3], box_thickness, box_color)
        if keypoints is not None:
            for p in range(len(keypoints)):
                if int(image_index[p]) == n:
                    draw_pose(out[n], np.asarray(keypoints[p], np.float32), np.asarray(scores[p], np.float32), skeleton, colors, score_threshold,
                              point_radius, line_thickness)
    return out


def expanded_mask(shape_hw, keypoints, boxes, point_radius, line_thickness, box_thickness, skeleton):
    """Pixels that may change: the union of every drawable shape's bounding box expanded by its width plus one pixel of sample reach.
    Limb boxes are taken over the finite joints of the pose regardless of score: a superset is all the test needs."""
    H, W = shape_hw
    m = np.zeros((H, W), bool)

    def mark(x0, y0, x1, y1, pad):
        if not all(np.isfinite([x0, y0, x1, y1])):
            return
        a, b = int(np.clip(np.floor(min(x0, x1) - pad - 1), 0, W)), int(np.clip(np.ceil(max(x0, x1) + pad + 2), 0, W))
        c, d = int(np.clip(np.floor(min(y0, y1) - pad - 1), 0, H)), int(np.clip(np.ceil(max(y0, y1) + pad + 2), 0, H))
        m[c:d, a:b] = True
    for kp in ([] if keypoints is None else keypoints):
        K = len(kp)
        for k in range(K):
            mark(kp[k][0], kp[k][1], kp[k][0], kp[k][1], point_radius + 1)
        for a, b in skeleton:
            if a < K and b < K:
                mark(kp[a][0], kp[a][1], kp[b][0], kp[b][1], line_thickness / 2)
    for bx in ([] if boxes is None else boxes):
        mark(bx[0], bx[1], bx[2], bx[3], box_thickness / 2)
    return m


# ---------------------------------------------------------------------------------------------------- heatmap overlay
def jet_lut():
    """The overlay's 256 x 3 BGR colour ramp from its closed form (r, g, b = clip(1.5 - |4t - 3|, |4t - 2|, |4t - 1|))."""
    t = np.arange(256) / 255.0
    ch = lambda c: np.rint(255.0 * np.clip(1.5 - np.abs(4.0 * t - c), 0.0, 1.0)).astype(np.uint8)     # noqa: E731
    return np.stack([ch(1.0), ch(2.0), ch(3.0)], 1)


def _taps(n_out, n_in):
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def overlay_value_f64(heatmaps, H, W):
    """(K,h,w) -> 255 v in float64: max over K, half-pixel bilinear resize to (H,W), (m - min) / (max - min + 1e-8)."""
    m = np.asarray(heatmaps, np.float64).max(axis=0)
    y0, y1, fy = _taps(H, m.shape[0])
    x0, x1, fx = _taps(W, m.shape[1])
    top = m[y0][:, x0] * (1 - fx) + m[y0][:, x1] * fx
    bot = m[y1][:, x0] * (1 - fx) + m[y1][:, x1] * fx
    r = top * (1 - fy)[:, None] + bot * fy[:, None]
    return 255.0 * (r - r.min()) / (r.max() - r.min() + 1e-8)


def overlay_blend(img, index, lut, alpha):
    """The integer blend from a colour-index plane: (img (256 - a) + lut[idx] a + 128) >> 8, a = clamp(rint(256 alpha), 0, 256)."""
    a = int(min(256, max(0, np.rint(256.0 * np.float32(alpha)))))
    return ((img.astype(np.int64) * (256 - a) + lut[index].astype(np.int64) * a + 128) >> 8).astype(np.uint8)
