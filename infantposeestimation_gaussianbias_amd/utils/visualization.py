"""Pose overlays drawn on the device: skeletons, heatmaps, boxes (the counterpart of the reference's utils/visualization.py).

Same function names, parameter names, defaults and draw order as the reference; the pixels follow this project's own rasterisation
rule ("Drawing on the device"), not OpenCV's: sub-pixel placement with 16-sample integer coverage instead of truncated
integer coordinates.  Every drawing function launches HIP kernels (hipops.draw_shapes / hipops.heatmap_overlay); there is no CPU
drawing path, so without the library or without a device they raise like every other op of the package.

Types: a numpy (H, W, 3) uint8 image returns numpy, a device uint8 tensor returns a device tensor; the input is never modified.
Images are BGR like the reference's (cv2.imread), and so are the palette and the heatmap LUT.
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib, hipops
from ..datasets.transforms import get_affine_matrix

_JOINTS = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
           "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")
_LIMB_NAMES = (
    # drawn from the feet up, so the short face limbs end on top of the long ones
    ("left_ankle", "left_knee"), ("left_knee", "left_hip"), ("right_ankle", "right_knee"), ("right_knee", "right_hip"),
    ("left_hip", "right_hip"), ("left_hip", "left_shoulder"), ("right_hip", "right_shoulder"), ("left_shoulder", "right_shoulder"),
    ("left_shoulder", "left_elbow"), ("left_elbow", "left_wrist"), ("right_shoulder", "right_elbow"), ("right_elbow", "right_wrist"),
    ("left_ear", "left_eye"), ("left_eye", "nose"), ("right_ear", "right_eye"), ("right_eye", "nose"),
)
# the 16 limbs of the COCO 17-keypoint person as (joint, joint) index pairs
COCO_SKELETON = [(_JOINTS.index(a), _JOINTS.index(b)) for a, b in _LIMB_NAMES]


def _hue_sweep(n: int) -> List[Tuple[int, int, int]]:
    """n fully saturated colours evenly spaced around the hue circle, from red, as BGR tuples."""
    out = []
    for i in range(n):
        t = 6.0 * i / n                                       # position on the six-segment hue circle
        ramp = lambda o: min(1.0, max(0.0, abs((t - o) % 6.0 - 3.0) - 1.0))     # noqa: E731
        r, g, b = ramp(0.0), ramp(2.0), ramp(4.0)
        out.append((int(round(255 * b)), int(round(255 * g)), int(round(255 * r))))
    return out


# one colour per COCO joint (BGR); other keypoint sets wrap around it
COCO_COLORS = _hue_sweep(17)


def heatmap_lut() -> np.ndarray:
    """(256, 3) uint8 BGR colour ramp of the heatmap overlay, blue -> cyan -> green -> yellow -> red, from the closed form
    r = clip(1.5 - |4t - 3|), g = clip(1.5 - |4t - 2|), b = clip(1.5 - |4t - 1|), t = i / 255."""
    t = np.arange(256, dtype=np.float64) / 255.0
    chan = lambda c: np.rint(255.0 * np.clip(1.5 - np.abs(4.0 * t - c), 0.0, 1.0)).astype(np.uint8)     # noqa: E731
    return np.stack([chan(1.0), chan(2.0), chan(3.0)], axis=1)


_RAMP_ANCHORS = {
    # RGB colours at evenly spaced t in [0, 1], joined by straight lines
    'sequential': ((68, 1, 84), (59, 82, 139), (33, 145, 140), (94, 201, 98), (253, 231, 37)),
    'diverging': ((59, 76, 192), (221, 221, 221), (180, 4, 38)),
}


def colour_ramp(name: str) -> np.ndarray:
    """(256, 3) uint8 BGR colour ramp of the feature sheets, entry i at t = i / 255, interpolated in float64 and rounded with rint.
    'hot': r = clip(t / 0.365079), g = clip((t - 0.365079) / 0.380953), b = clip((t - 0.746032) / 0.253968) (black, red, yellow, white);
    'sequential': dark violet to yellow through (68,1,84), (59,82,139), (33,145,140), (94,201,98), (253,231,37) at t = 0, 1/4, 1/2, 3/4, 1;
    'diverging': blue to red through (59,76,192), (221,221,221), (180,4,38) at t = 0, 1/2, 1; 'jet': `heatmap_lut()`."""
    t = np.arange(256, dtype=np.float64) / 255.0
    if name == 'jet':
        return heatmap_lut()
    if name == 'hot':
        rgb = 255.0 * np.clip(np.stack([t / 0.365079, (t - 0.365079) / 0.380953, (t - 0.746032) / 0.253968], axis=1), 0.0, 1.0)
    elif name in _RAMP_ANCHORS:
        anchors = np.asarray(_RAMP_ANCHORS[name], np.float64)
        rgb = np.stack([np.interp(t, np.linspace(0.0, 1.0, len(anchors)), anchors[:, c]) for c in range(3)], axis=1)
    else:
        raise ValueError(f"colour_ramp: no ramp named {name!r}; the ramps are 'hot', 'sequential', 'diverging', 'jet'")
    return np.ascontiguousarray(np.rint(rgb).astype(np.uint8)[:, ::-1])


_TABLES = {}


def _device():
    if not torch.cuda.is_available():
        raise _lib.PoseKernelError("drawing: expected a CUDA(HIP) device; the overlays are HIP kernels and have no CPU implementation")
    return torch.device("cuda", torch.cuda.current_device())


def _table(kind, values, dtype, device):
    """Small constant tables (limbs, palette, LUT) cached on the device by value."""
    arr = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    key = (kind, str(device), arr.shape, arr.tobytes())
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(arr).to(device)
    return _TABLES[key]


def _dev(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype])).to(device)


def _images_in(img):
    """-> (fresh contiguous device batch (N,H,W,3), restore(batch) -> same kind and rank as `img`).  Always a copy: the input stays."""
    if isinstance(img, torch.Tensor):
        if not img.is_cuda:
            raise _lib.PoseKernelError("image: expected a CUDA(HIP) tensor or a numpy array; drawing has no CPU implementation")
        if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
            raise _lib.PoseKernelError(f"image: expected uint8 (H, W, 3) or (N, H, W, 3), got {img.dtype} {tuple(img.shape)}")
        single = img.dim() == 3
        batch = (img[None] if single else img).contiguous().clone()
        return batch, (lambda b: b[0] if single else b)
    dev = _device()
    arr = np.asarray(img)
    if arr.dtype != np.uint8 or arr.ndim not in (3, 4) or arr.shape[-1] != 3:
        raise ValueError(f"image: expected uint8 (H, W, 3) or (N, H, W, 3), got {arr.dtype} {arr.shape}")
    single = arr.ndim == 3
    batch = torch.from_numpy(np.ascontiguousarray(arr[None] if single else arr)).to(dev)
    return batch, (lambda b: b[0].cpu().numpy() if single else b.cpu().numpy())


def _check_sizes(point_radius=0, line_thickness=1, thickness=1):
    if not (0 <= int(point_radius) <= 64 and 1 <= int(line_thickness) <= 64 and 1 <= int(thickness) <= 64):
        raise ValueError("point_radius must be 0..64, line and box thickness 1..64")


def draw_poses(images, keypoints, scores, image_index, boxes=None, box_image_index=None, heatmaps=None, score_threshold: float = 0.3,
               skeleton: Sequence[Tuple[int, int]] = COCO_SKELETON, colors: Sequence[Tuple[int, int, int]] = COCO_COLORS,
               point_radius: int = 4, line_thickness: int = 2, box_color: Tuple[int, int, int] = (0, 255, 0), box_thickness: int = 2,
               alpha: float = 0.5, heatmap_centers=None, heatmap_scales=None, heatmap_rotations=None, heatmap_image_index=None):
    """Batched overlays for served / video use: (N, H, W, 3) uint8 frames of one size -> a new batch with everything drawn.

    keypoints (P, K, 2) image pixels, scores (P, K) or None (all drawn), image_index (P,) non-decreasing frame of each pose: several
    poses per frame are allowed.  boxes (Q, 4) x1 y1 x2 y2 with box_image_index (Q,) non-decreasing; heatmaps (N, K', h, w), one
    stack per frame.  One overlay launch (if heatmaps are given) and one shape launch for the whole batch; per frame the heatmap goes
    underneath, then boxes in index order, then the poses in index order (limbs in table order, then joints: disc and white ring).
    Limbs naming a joint >= K are skipped and the palette wraps, so K = 13 works with the COCO tables.

    With `heatmap_centers` and `heatmap_scales` (P', 2) the heatmaps are per person instead: (P', K', h, w), each laid where its crop
    (center, scale, `heatmap_rotations` degrees, default 0) lies in frame `heatmap_image_index` (default: the poses' `image_index`), as
    `draw_person_heatmaps` does; still underneath boxes and poses.
    """
    batch, restore = _images_in(images)
    patches = None
    if heatmap_centers is not None or heatmap_scales is not None:
        if heatmaps is None or heatmap_centers is None or heatmap_scales is None:
            raise ValueError("draw_poses: per-person heatmaps need heatmaps, heatmap_centers and heatmap_scales together")
        if heatmap_image_index is None and keypoints is not None:
            heatmap_image_index = image_index                 # one stack per pose, in the order of the poses
        patches = (heatmap_centers, heatmap_scales, heatmap_rotations, heatmap_image_index)
    _draw_into(batch, keypoints, scores, image_index, boxes, box_image_index, heatmaps, score_threshold, skeleton, colors, point_radius,
               line_thickness, box_color, box_thickness, alpha, patches)
    return restore(batch)


def _draw_into(batch, keypoints, scores, image_index, boxes=None, box_image_index=None, heatmaps=None, score_threshold=0.3,
               skeleton=COCO_SKELETON, colors=COCO_COLORS, point_radius=4, line_thickness=2, box_color=(0, 255, 0), box_thickness=2, alpha=0.5,
               patches=None):
    """draw_poses on a batch this module owns (a fresh copy of the caller's images), in place."""
    _check_sizes(point_radius, line_thickness, box_thickness)
    dev = batch.device
    if patches is not None:
        _patches_into(batch, heatmaps, alpha, *patches)
    elif heatmaps is not None:
        hm = _dev(heatmaps, torch.float32, dev)
        hipops.heatmap_overlay(batch, hm[None] if hm.dim() == 3 else hm, alpha, _table("lut", heatmap_lut(), np.uint8, dev))
    kp = sc = idx = bx = bidx = None
    if keypoints is not None:
        kp = _dev(keypoints, torch.float32, dev)
        kp = kp[None] if kp.dim() == 2 else kp
        sc = torch.ones(kp.shape[:2], dtype=torch.float32, device=dev) if scores is None else _dev(scores, torch.float32, dev).reshape(kp.shape[:2])
        idx = _dev(image_index, torch.int32, dev).reshape(-1)
    if boxes is not None:
        bx = _dev(boxes, torch.float32, dev).reshape(-1, 4)
        bidx = _dev(box_image_index, torch.int32, dev).reshape(-1)
    if (kp is not None and kp.shape[0]) or (bx is not None and bx.shape[0]):
        hipops.draw_shapes(batch, kp, sc, idx, _table("limbs", np.asarray(list(skeleton)).reshape(-1, 2), np.int32, dev),
                           _table("colors", np.asarray(list(colors)).reshape(-1, 3), np.uint8, dev), bx, bidx, box_color, box_thickness,
                           score_threshold, point_radius, line_thickness)


def draw_skeleton(img, keypoints, scores=None, score_threshold: float = 0.3, skeleton: Sequence[Tuple[int, int]] = COCO_SKELETON,
                  colors: Sequence[Tuple[int, int, int]] = COCO_COLORS, point_radius: int = 4, line_thickness: int = 2):
    """One pose (K, 2) with scores (K,) on one (H, W, 3) BGR image: limbs between joints whose scores both reach the threshold, in the
    colour of the limb's first joint, then a disc and a white ring per joint.  Returns a new image."""
    batch, restore = _images_in(img)
    if batch.shape[0] != 1:
        raise ValueError("draw_skeleton draws one image; use draw_poses for a batch")
    _draw_into(batch, keypoints, scores, [0], score_threshold=score_threshold, skeleton=skeleton, colors=colors, point_radius=point_radius,
               line_thickness=line_thickness)
    return restore(batch)


def draw_heatmaps(img, heatmaps, alpha: float = 0.5):
    """Overlay the maximum over the (K, h, w) heatmaps, resized to the image, normalised to its own range and coloured blue -> red,
    blended with weight `alpha`.  A batch (N, H, W, 3) takes (N, K, h, w).  (hipops.heatmap_overlay also hands out the colour-index
    plane.)"""
    batch, restore = _images_in(img)
    dev = batch.device
    hm = _dev(heatmaps, torch.float32, dev)
    hm = hm[None] if hm.dim() == 3 else hm
    hipops.heatmap_overlay(batch, hm, alpha, _table("lut", heatmap_lut(), np.uint8, dev))
    return restore(batch)


def crop_heatmap_matrices(centers, scales, heatmap_size, rotations=None) -> np.ndarray:
    """(P, 2, 3) float64 maps from image pixels to heat-map pixels of the crops (center, scale, rotation in degrees): the crop matrix
    with the heat-map size (w, h) as its output size.  Heat pixel x is input pixel x w_in / w -- the decode's convention, not the
    half-pixel one -- so this equals diag(w / w_in, h / h_in) times the crop matrix the network's input was cut with."""
    c, s = np.asarray(centers, np.float64).reshape(-1, 2), np.asarray(scales, np.float64).reshape(-1, 2)
    r = np.zeros(len(c)) if rotations is None else np.asarray(rotations, np.float64).reshape(-1)
    if not (len(c) == len(s) == len(r)):
        raise ValueError(f"crop_heatmap_matrices: {len(c)} centers, {len(s)} scales, {len(r)} rotations")
    return np.stack([get_affine_matrix(c[i], s[i], heatmap_size, r[i]) for i in range(len(c))]) if len(c) else np.zeros((0, 2, 3))


def _patches_into(batch, heatmaps, alpha, centers=None, scales=None, rotations=None, image_index=None, matrices=None):
    """Per-person heatmaps blended into a batch this module owns, in place (hipops.heatmap_overlay_patches)."""
    dev = batch.device
    hm = _dev(heatmaps, torch.float32, dev)
    hm = hm[None] if hm.dim() == 3 else hm
    if hm.dim() != 4:
        raise ValueError(f"heatmaps: expected (P, K, h, w), or (K, h, w) for one person, got {tuple(hm.shape)}")
    P = int(hm.shape[0])
    if matrices is None:
        if centers is None or scales is None:
            raise ValueError("per-person heatmaps need centers and scales, or matrices")
        matrices = crop_heatmap_matrices(centers, scales, (int(hm.shape[3]), int(hm.shape[2])), rotations)
    elif centers is not None or scales is not None or rotations is not None:
        raise ValueError("per-person heatmaps take centers / scales / rotations or matrices, not both")
    if image_index is None:
        if batch.shape[0] != 1:
            raise ValueError("per-person heatmaps on a batch of frames need image_index")
        image_index = np.zeros(P, np.int32)
    hipops.heatmap_overlay_patches(batch, hm, image_index, matrices, alpha, _table("lut", heatmap_lut(), np.uint8, dev))


def draw_person_heatmaps(img, heatmaps, centers=None, scales=None, rotations=None, image_index=None, matrices=None, alpha: float = 0.5):
    """Overlay each person's heatmaps where that person's crop lies in the frame (top-down use; rule: DESIGN.md, "Heatmaps where the crop
    lies").  heatmaps (P, K, h, w), or (K, h, w) for one person; the crops as `centers` / `scales` (P, 2) with optional `rotations` (P,)
    in degrees -- what the network's input was cut with -- or directly as `matrices` (P, 2, 3), image pixels -> heat-map pixels.  A
    batch (N, H, W, 3) needs `image_index` (P,), the non-decreasing frame of each person.  Each stack is reduced to its maximum over K
    and normalised to its own range; where persons overlap the larger value wins, whatever their order; pixels outside every crop keep
    their bytes.  Returns a new image.  (`draw_heatmaps` keeps the reference's signature and stretches one stack over the frame.)"""
    batch, restore = _images_in(img)
    _patches_into(batch, heatmaps, alpha, centers, scales, rotations, image_index, matrices)
    return restore(batch)


def draw_bbox(img, bbox, color: Tuple[int, int, int] = (0, 255, 0), thickness: int = 2):
    """A box outline (x1, y1, x2, y2) of the given thickness centred on the box edges.  Returns a new image."""
    batch, restore = _images_in(img)
    if batch.shape[0] != 1:
        raise ValueError("draw_bbox draws one image; use draw_poses for a batch")
    _draw_into(batch, None, None, None, boxes=bbox, box_image_index=[0], box_color=color, box_thickness=thickness)
    return restore(batch)


def create_grid_image(images, ncols: int = 4, padding: int = 2, bg_color: Tuple[int, int, int] = (255, 255, 255)):
    """Tile same-sized images into a grid, `ncols` per row with `padding` pixels of `bg_color` around each.  Plumbing: numpy on the host
    for numpy images, torch slicing on the device for device tensors; no kernel.  Unlike the reference, which resizes images that differ
    from the first one, a differing size raises ValueError.  The empty list gives the reference's 100 x 100 black image."""
    if len(images) == 0:
        return np.zeros((100, 100, 3), dtype=np.uint8)
    h, w = images[0].shape[:2]
    for im in images:
        if tuple(im.shape) != (h, w, 3):
            raise ValueError(f"create_grid_image: every image must be ({h}, {w}, 3) like the first, got {tuple(im.shape)} (no resizing here)")
    nrows = (len(images) + ncols - 1) // ncols
    gh, gw = nrows * h + (nrows + 1) * padding, ncols * w + (ncols + 1) * padding
    if isinstance(images[0], torch.Tensor):
        grid = torch.empty(gh, gw, 3, dtype=torch.uint8, device=images[0].device)
        grid[:] = torch.tensor([int(c) for c in bg_color], dtype=torch.uint8, device=grid.device)
    else:
        grid = np.full((gh, gw, 3), bg_color, dtype=np.uint8)
    for i, im in enumerate(images):
        y, x = padding + (i // ncols) * (h + padding), padding + (i % ncols) * (w + padding)
        grid[y:y + h, x:x + w] = im
    return grid


def write_image(img, output_path: str) -> None:
    """Write a BGR uint8 image (numpy or device tensor) with Pillow, converting to RGB; the format follows the file name."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("saving an overlay needs Pillow (PIL), which is not installed") from e
    arr = img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    Image.fromarray(np.ascontiguousarray(arr[:, :, ::-1])).save(output_path)


def save_visualization(img, output_path: str, keypoints=None, scores=None, heatmaps=None, bbox=None):
    """Draw in the reference's order -- box, heatmaps at alpha 0.3, skeleton -- and write the file (Pillow, BGR -> RGB)."""
    result = _images_in(img)[0][0]                        # on the device once; the three steps below each return a new tensor
    if bbox is not None:
        result = draw_bbox(result, bbox)
    if heatmaps is not None:
        result = draw_heatmaps(result, heatmaps, alpha=0.3)
    if keypoints is not None:
        result = draw_skeleton(result, keypoints, scores)
    write_image(result, output_path)


def save_person_visualization(img, output_path: str, keypoints=None, scores=None, heatmaps=None, bbox=None, center=None, scale=None):
    """`save_visualization` for a person whose box is not the whole image: the heatmaps go where the crop (center, scale) lies."""
    result = _images_in(img)[0][0]
    if bbox is not None:
        result = draw_bbox(result, bbox)
    if heatmaps is not None:
        result = draw_person_heatmaps(result, heatmaps, centers=center, scales=scale, alpha=0.3)
    if keypoints is not None:
        result = draw_skeleton(result, keypoints, scores)
    write_image(result, output_path)
