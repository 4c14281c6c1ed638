"""Configuration surface (drop-in for the reference's configs/config.py:15-130).

Same dataclass fields and defaults, so `cfg.data.input_size`, `cfg.model.backbone`, `cfg.train.lr` ... read
identically.  Extension over the reference: `get_config(path_or_name)` also accepts
  * a preset name ("hrformer_small", "hrformer_base", "hrnet_w32", "hrnet_w48", "hrnet_w18", "preemie"), or
  * a legacy-format yaml (reference configs/*.yaml, written by root config.py:135-224): `MODEL.NUM_JOINTS`,
    `MODEL.IMAGE_SIZE`, `MODEL.HEATMAP_SIZE`, `MODEL.SIGMA`, `TRAIN.*` are mapped onto the dataclass fields, and
    `DATA.COLOR_JITTER.{BRIGHTNESS,CONTRAST,SATURATION}` onto `cfg.train.color_jitter` (a yaml that names it trains with it; a
    missing sub-key reads as 0, and a block that is empty or all zero leaves jitter off), this project's own `DATA.BLUR {PROB, SIGMA}` /
    `DATA.NOISE {PROB, SIGMA}` / `DATA.OCCLUSION {PROB, MAX_RECTS, AREA, ASPECT, FILL}` onto `cfg.train.blur` / `sensor_noise` /
    `occlusion` (`check_augment`; an empty block or `PROB: 0` leaves the stage off), and `ADVANCED.MULTI_SCALE_TEST` /
    `ADVANCED.SCALE_LIST` onto `cfg.test_scales` (multi-scale test; off unless MULTI_SCALE_TEST is true), `EVAL.{METRICS, PCK_THRESHOLD,
    MIN_KEYPOINT_VISIBILITY}` onto `cfg.eval_metrics` / `pck_threshold` / `min_keypoint_visibility`, `TEMPORAL.*` onto `cfg.temporal` and
    `CLINICAL.*` onto `cfg.clinical` (movement analysis: utils/metrics.py, `validate.py --pck`, `inference.py --sequence`), and
    `TEST.{COCO_BBOX_FILE, IMAGE_THRE, OKS_THRE, IN_VIS_THRE, SOFT_NMS}` onto `cfg.bbox_file` / `det_score_thr` / `oks_nms_thr` /
    `in_vis_thr` / `soft_nms` (validation on detector boxes; `TEST.USE_GT_BBOX: false` without a box file changes nothing and says so),
    and `TEST.DECODE: 'shift' | 'unbiased'` / `TEST.MODULATE_KERNEL` onto `cfg.decode` / `cfg.modulate_kernel` (the heatmap decode of the
    heatmap-head models; a bad value raises and names the key).  `TEST.POST_PROCESS` and `TEST.SHIFT_HEATMAP` are deliberately NOT mapped:
    both shipped yamls set them true, and mapping them would change what those configurations do today.  `CLINICAL.FREQUENCY_BAND:
    [lo, hi]` (Hz; this project's own key) maps onto `cfg.frequency_band`, the band of the movement spectrum; a bad value names the key.
    `CLINICAL.JOINT_ANGLES: {name: [a, b, c]}` and `CLINICAL.KINEMATICS: {MAX_LAG, ENTROPY_M, ENTROPY_R}` (this project's own keys) map onto
    `cfg.joint_angles` / `cfg.kinematics`, the angle table and settings of the limb kinematics; `cfg.clinical` keeps its four entries.
    `LOSS.USE_OHKM` / `LOSS.TOPK` (HRNet's keys; TOPK defaults to 8) / `LOSS.OHKM_WEIGHT` map onto `cfg.model.ohkm_topk` /
    `cfg.model.ohkm_weight` (online hard keypoint mining; off unless USE_OHKM is true).
"""
import logging
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

_COCO_NAMES = ("nose left_eye right_eye left_ear right_ear left_shoulder right_shoulder left_elbow right_elbow "
               "left_wrist right_wrist left_hip right_hip left_knee right_knee left_ankle right_ankle").split()


@dataclass
class DataConfig:
    data_root: str = 'data/coco/'
    train_ann: str = 'annotations/person_keypoints_train2017.json'
    val_ann: str = 'annotations/person_keypoints_val2017.json'
    train_img_prefix: str = 'train2017/'
    val_img_prefix: str = 'val2017/'
    input_size: Tuple[int, int] = (192, 256)     # (width, height)
    heatmap_size: Tuple[int, int] = (48, 64)     # (width, height)
    num_keypoints: int = 17
    sigma: float = 2.0
    keypoint_names: List[str] = field(default_factory=lambda: list(_COCO_NAMES))
    flip_pairs: List[Tuple[int, int]] = field(default_factory=lambda: [(i, i + 1) for i in range(1, 17, 2)])


@dataclass
class ModelConfig:
    backbone: str = 'hrformer_base'
    pretrained: bool = True
    in_channels: int = 3
    base_channels: int = 78
    head_type: str = 'fusion'
    head_in_channels: int = 78
    num_keypoints: int = 17
    hidden_dim: int = 256
    use_target_weight: bool = True
    use_fusion_loss: bool = True
    heatmap_loss_weight: float = 1.0
    offset_loss_weight: float = 1.0
    peak_loss_weight: float = 0.5
    variance_loss_weight: float = 0.1
    overlap_loss_weight: float = 0.05
    shape_loss_weight: float = 0.05
    target_sigma: float = 2.0
    # Online hard keypoint mining (legacy yaml LOSS.USE_OHKM / LOSS.TOPK / LOSS.OHKM_WEIGHT, `train.py --ohkm TOPK --ohkm_weight W`): 0 (off)
    # or the number of worst-fitted joints per sample that count in the heatmap loss, and the weight of that term in the fusion loss.  Plain
    # class attributes like TrainConfig.color_jitter: the field set stays the reference's.
    ohkm_topk = 0
    ohkm_weight = 1.0


@dataclass
class TrainConfig:
    max_epochs: int = 210
    val_interval: int = 10
    batch_size: int = 32
    num_workers: int = 4
    optimizer: str = 'AdamW'
    lr: float = 5e-4
    weight_decay: float = 0.01
    betas: Tuple[float, float] = (0.9, 0.999)
    warmup_epochs: int = 5
    warmup_lr: float = 5e-7
    lr_milestones: List[int] = field(default_factory=lambda: [170, 200])
    lr_gamma: float = 0.1
    flip_prob: float = 0.5
    half_body_prob: float = 0.3
    rotation_factor: float = 40.0
    scale_factor: Tuple[float, float] = (0.5, 1.5)
    save_best: str = 'AP'
    checkpoint_dir: str = 'checkpoints/'
    device: str = 'cuda'
    fp16: bool = True        # "mixed precision on": bf16 on MI355X (no GradScaler needed)
    # Colour jitter of the training crops (legacy yaml DATA.COLOR_JITTER, `train.py --color_jitter`): None or the (brightness, contrast,
    # saturation) ranges.  Plain class attributes, NOT dataclass fields: the field set stays the reference's (asdict, __init__, ==).
    color_jitter = None
    color_jitter_prob = 0.5
    # Weight EMA (`train.py --ema DECAY`): None (off) or the decay of the average the optimiser kernel keeps.  A plain class attribute too;
    # no yaml key (the reference's configs have none).
    ema_decay = None
    # Occlusion, blur and sensor noise of the training crops (this project's own legacy-yaml keys DATA.BLUR / DATA.NOISE / DATA.OCCLUSION,
    # `train.py --blur / --noise / --occlusion`), plain class attributes as well: None (off) or what `check_augment` returns --
    # {'prob', 'sigma': (lo, hi)} for blur and sensor_noise, {'prob', 'max_rects', 'area': (lo, hi), 'aspect': (lo, hi), 'fill'} for occlusion.
    blur = None
    sensor_noise = None
    occlusion = None


@dataclass
class Config:
    data: DataConfig = field(default_factory=DataConfig)
    model: ModelConfig = field(default_factory=ModelConfig)
    train: TrainConfig = field(default_factory=TrainConfig)
    exp_name: str = 'hrformer_base_coco_256x192'
    seed: int = 42
    # Multi-scale test (legacy yaml ADVANCED.MULTI_SCALE_TEST + SCALE_LIST, `--scales`): None (one crop per person) or the box-scale factors
    # of the crops whose heatmaps are merged, exactly one of them 1.0.  A plain class attribute like `color_jitter`: same field set.
    test_scales = None
    # Evaluation and movement analysis (legacy yaml EVAL / TEMPORAL / CLINICAL blocks), plain class attributes as well.  eval_metrics: the
    # metrics validate.py's command line reports ('PCK' adds PCK at pck_threshold); min_keypoint_visibility: the confidence below which a
    # frame of a joint does not count in the movement statistics; temporal: None or (window, method) for temporal_smoothing; clinical: None
    # or {'min_movement', 'max_movement', 'alert_low', 'alert_asymmetry'} (amplitude thresholds in pixels and which flags to raise).
    eval_metrics = ('AP',)
    pck_threshold = 0.2
    min_keypoint_visibility = 0.3
    temporal = None
    clinical = None
    # Validation on detector boxes (legacy yaml TEST block, `validate.py --bbox_file / --oks_nms`), plain class attributes as well.
    # bbox_file: None (crops from the ground-truth boxes) or a COCO-style person-detection file, relative to data_root; det_score_thr: boxes
    # scored below it are dropped; oks_nms_thr: None (every pose is evaluated) or the OKS threshold of the per-image pose NMS, which then
    # also rescores every pose as box score x mean keypoint score above in_vis_thr; soft_nms: the soft variant.
    bbox_file = None
    det_score_thr = 0.0
    oks_nms_thr = None
    in_vis_thr = 0.2
    soft_nms = False
    # Heatmap decode of the heatmap-head models (legacy yaml TEST.DECODE / TEST.MODULATE_KERNEL, `--decode / --modulate_kernel`), plain class
    # attributes as well.  decode: None or 'shift' (argmax + quarter-pixel shift) or 'unbiased' (distribution-aware: one Newton step on the
    # log of the map smoothed with `modulate_kernel` Gaussian taps, an odd size from 3 to 31).
    decode = None
    modulate_kernel = 11
    # Movement spectrum (this project's own legacy-yaml key CLINICAL.FREQUENCY_BAND, `inference.py --freq_band`), a plain class attribute as
    # well.  frequency_band: None or (f_min, f_max) in Hz, the band whose dominant frequency and power `movement_report` adds per joint.
    frequency_band = None
    # Limb kinematics (this project's own legacy-yaml keys CLINICAL.JOINT_ANGLES and CLINICAL.KINEMATICS, `inference.py --kinematics`), plain
    # class attributes as well.  joint_angles: None (COCO_ANGLES of utils/kinematics.py for 17 joints) or {name: (a, b, c)}, the angle at joint
    # b between the rays to a and c; kinematics: None or {'max_lag': frames or None, 'entropy': (m, r)}, the lags searched by the
    # cross-correlation and the template length and tolerance of the sample entropy.
    joint_angles = None
    kinematics = None


_PRESETS = {
    # name: (backbone, head_type, channels, (W_in,H_in), (W_hm,H_hm), K, sigma)
    'hrformer_base': ('hrformer_base', 'fusion', 78, (192, 256), (48, 64), 17, 2.0),
    'hrformer_small': ('hrformer_small', 'fusion', 32, (192, 256), (48, 64), 17, 2.0),
    'hrnet_w32': ('hrnet_w32', 'heatmap', 32, (288, 384), (72, 96), 17, 2.0),      # root config.py:135-164
    'hrnet_w48': ('hrnet_w48', 'heatmap', 48, (288, 384), (72, 96), 17, 2.0),
    'hrnet_w18': ('hrnet_w18', 'heatmap', 18, (96, 128), (24, 32), 17, 2.0),       # BASELINE config 1
    'preemie': ('hrformer_base', 'fusion', 78, (288, 384), (72, 96), 13, 1.5),     # BASELINE config 5 (K=13, sigma 1.5)
}


def check_test_scales(scales) -> Tuple[float, ...]:
    """The scale list of a multi-scale test as a tuple of floats: 1 to 8 finite, positive, distinct entries, exactly one of them 1.0
    (the base crop, in whose frame the passes are merged).  ValueError otherwise."""
    try:
        sc = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise ValueError(f"test scales must be a list of numbers, got {scales!r}") from None
    if not 1 <= len(sc) <= 8:
        raise ValueError(f"test scales: {len(sc)} entries (1 to 8)")
    if not all(math.isfinite(s) and s > 0 for s in sc):
        raise ValueError(f"test scales must be finite and > 0, got {sc}")
    if len(set(sc)) != len(sc):
        raise ValueError(f"test scales must be distinct, got {sc}")
    if sc.count(1.0) != 1:
        raise ValueError(f"test scales need exactly one 1.0 (the base crop), got {sc}")
    return sc


def check_decode(decode, modulate_kernel=11, what=("decode", "modulate_kernel")):
    """The decode choice and its smoothing size as (None | 'shift' | 'unbiased', int): ValueError naming `what` (the key or flag the value
    came from) for any other choice, or a size that is not an odd integer from 3 to 31."""
    if decode is not None and decode not in ("shift", "unbiased"):
        raise ValueError(f"{what[0]} must be 'shift' or 'unbiased', got {decode!r}")
    try:
        k = int(modulate_kernel)
        ok = not isinstance(modulate_kernel, bool) and k == modulate_kernel and 3 <= k <= 31 and k % 2 == 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what[1]} must be an odd integer from 3 to 31, got {modulate_kernel!r}")
    return decode, k


def check_frequency_band(band, what="frequency_band") -> Tuple[float, float]:
    """A movement-frequency band as (f_min, f_max) in Hz: two finite numbers with 0 <= f_min < f_max.  ValueError naming `what` (the key or
    flag the value came from) otherwise."""
    try:
        lo, hi = band
        ok = not isinstance(lo, (bool, str)) and not isinstance(hi, (bool, str))
        lo, hi = float(lo), float(hi)
        ok = ok and math.isfinite(lo) and math.isfinite(hi) and 0 <= lo < hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be [f_min, f_max] in Hz with 0 <= f_min < f_max, got {band!r}")
    return lo, hi


def check_joint_angles(table, what="joint_angles", num_joints=None):
    """A table of joint angles as an ordered {name: (a, b, c)}: a non-empty mapping (at most 64 entries) of names onto three integer joints,
    a != b and b != c, each in 0 .. num_joints - 1 where the layout is known.  ValueError naming `what` (the key or argument the value
    came from) otherwise."""
    if not isinstance(table, dict) or not 1 <= len(table) <= 64:
        raise ValueError(f"{what} must map 1 to 64 names onto joints [a, b, c], got {table!r}")
    out = {}
    for name, triple in table.items():
        try:
            ok = len(triple) == 3 and all(not isinstance(v, bool) and int(v) == v for v in triple)
            a, b, c = (int(v) for v in triple) if ok else (0, 0, 0)
            ok = ok and min(a, b, c) >= 0 and a != b and b != c and (num_joints is None or max(a, b, c) < num_joints)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            top = "" if num_joints is None else f" of 0 to {int(num_joints) - 1}"
            raise ValueError(f"{what}[{name!r}] must be three joints [a, b, c]{top} with a != b and b != c, got {triple!r}")
        out[str(name)] = (a, b, c)
    return out


def check_kinematics(max_lag=None, entropy=None, what=("max_lag", "entropy m", "entropy r")):
    """The settings of the limb kinematics as {'max_lag': None or an integer from 0 to 4096 (frames), 'entropy': None or (m, r) with m an
    integer from 1 to 4 and r finite and >= 0}.  ValueError naming the entry of `what` (key, flag or argument) the bad value came from."""
    out = {"max_lag": None, "entropy": None}
    if max_lag is not None:
        try:
            ok = not isinstance(max_lag, bool) and int(max_lag) == max_lag and 0 <= int(max_lag) <= 4096
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what[0]} must be an integer from 0 to 4096 frames, got {max_lag!r}")
        out["max_lag"] = int(max_lag)
    if entropy is not None:
        try:
            m, r = entropy
        except (TypeError, ValueError):
            raise ValueError(f"{what[1]} and {what[2]}: expected (m, r), got {entropy!r}") from None
        try:
            ok = not isinstance(m, bool) and int(m) == m and 1 <= int(m) <= 4
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what[1]} must be an integer from 1 to 4, got {m!r}")
        try:
            ok = not isinstance(r, (bool, str)) and math.isfinite(float(r)) and float(r) >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what[2]} must be a finite number >= 0 (a share of the standard deviation), got {r!r}")
        out["entropy"] = (int(m), float(r))
    return out


def check_ohkm(topk, weight=1.0, num_keypoints=None, allow_off=True, what=("ohkm_topk", "ohkm_weight")):
    """The settings of online hard keypoint mining as (int topk, float weight): `topk` an integer from 1 to `num_keypoints` (to the
    kernels' 256 where the number of joints is not known yet), or 0 = off where `allow_off`; `weight` finite and >= 0.  ValueError naming
    `what` (the argument, key or flag the value came from) otherwise."""
    hi = 256 if num_keypoints is None else int(num_keypoints)
    try:
        k = int(topk)
        ok = not isinstance(topk, bool) and k == topk and ((allow_off and k == 0) or 1 <= k <= hi)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what[0]} must be an integer from 1 to {hi}" + (" (or 0 = off)" if allow_off else "") + f", got {topk!r}")
    try:
        w = float(weight)
        ok = not isinstance(weight, (bool, str)) and math.isfinite(w) and w >= 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what[1]} must be finite and >= 0, got {weight!r}")
    return k, w


AUGMENT_DEFAULTS = {
    'blur': {'prob': 0.3, 'sigma': (0.3, 2.0)},
    'noise': {'prob': 0.3, 'sigma': (2.0, 10.0)},
    'occlusion': {'prob': 0.5, 'max_rects': 2, 'area': (0.02, 0.2), 'aspect': (0.3, 3.3), 'fill': 'random'},
}
_AUGMENT_SIGMA_MAX = {'blur': 2.5, 'noise': 73.0}      # blur: radius 7 holds 3 sigma up to 2.33 and the table no more; noise: amp <= 255


def _check_range(value, what, hi=None):
    """(lo, hi) with 0 < lo <= hi (<= `hi`), as floats."""
    try:
        lo, up = value
        ok = not isinstance(lo, (bool, str)) and not isinstance(up, (bool, str))
        lo, up = float(lo), float(up)
        ok = ok and math.isfinite(lo) and math.isfinite(up) and 0 < lo <= up and (hi is None or up <= hi)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be [lo, hi] with 0 < lo <= hi" + (f" <= {hi:g}" if hi is not None else "") + f", got {value!r}")
    return lo, up


def _check_prob(value, what):
    try:
        p = float(value)
        ok = not isinstance(value, (bool, str)) and 0 <= p <= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be a probability in [0, 1], got {value!r}")
    return p


def check_fill(fill, what="fill"):
    """The fill of the erased rectangles: 'random', 'mean' or an (r, g, b) triple of bytes (returned as a tuple of ints)."""
    if isinstance(fill, str):
        if fill in ("random", "mean"):
            return fill
        raise ValueError(f"{what} must be 'random', 'mean' or three bytes R,G,B, got {fill!r}")
    try:
        rgb = tuple(fill)
        ok = len(rgb) == 3 and all(not isinstance(v, (bool, str)) and int(v) == v and 0 <= int(v) <= 255 for v in rgb)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be 'random', 'mean' or three bytes R,G,B, got {fill!r}")
    return tuple(int(v) for v in rgb)


def check_augment(kind, setting, what=None):
    """One of the three augmentation settings ('blur', 'noise', 'occlusion') as the dict `get_train_transforms` takes, or None when it is
    off (`setting` None or empty, or prob 0); missing entries take AUGMENT_DEFAULTS.  ValueError naming `what` (the yaml block or flag the
    value came from) and the entry: prob outside [0, 1]; a sigma range that is not 0 < lo <= hi <= 2.5 (blur: the table holds radius 7)
    or <= 73 (noise: the amplitude 2 sqrt(3) sigma must stay <= 255); max_rects outside 1 .. 4; an area range outside 0 < lo <= hi <= 1;
    an aspect range that is not 0 < lo <= hi; an unknown fill."""
    what = what or kind
    if kind not in AUGMENT_DEFAULTS:
        raise ValueError(f"unknown augmentation {kind!r}")
    if not setting:
        return None
    if not isinstance(setting, dict) or set(setting) - set(AUGMENT_DEFAULTS[kind]):
        raise ValueError(f"{what} must be a mapping with keys from {sorted(AUGMENT_DEFAULTS[kind])}, got {setting!r}")
    s = {**AUGMENT_DEFAULTS[kind], **setting}
    out = {'prob': _check_prob(s['prob'], f"{what}.prob")}
    if kind in ('blur', 'noise'):
        out['sigma'] = _check_range(s['sigma'], f"{what}.sigma", _AUGMENT_SIGMA_MAX[kind])
    else:
        try:
            n = int(s['max_rects'])
            ok = not isinstance(s['max_rects'], bool) and n == s['max_rects'] and 1 <= n <= 4
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what}.max_rects must be an integer from 1 to 4, got {s['max_rects']!r}")
        out['max_rects'] = n
        out['area'] = _check_range(s['area'], f"{what}.area", 1.0)
        out['aspect'] = _check_range(s['aspect'], f"{what}.aspect")
        out['fill'] = check_fill(s['fill'], f"{what}.fill")
    return out if out['prob'] > 0 else None


def _apply_preset(cfg: Config, name: str) -> Config:
    bb, head, ch, insz, hmsz, K, sigma = _PRESETS[name]
    cfg.model.backbone, cfg.model.head_type = bb, head
    cfg.model.base_channels = cfg.model.head_in_channels = ch
    cfg.data.input_size, cfg.data.heatmap_size = insz, hmsz
    cfg.data.num_keypoints = cfg.model.num_keypoints = K
    cfg.data.sigma = cfg.model.target_sigma = sigma
    if K != 17:
        cfg.data.keypoint_names = [f'kpt_{i}' for i in range(K)]
        cfg.data.flip_pairs = []
    cfg.exp_name = f'{name}_{insz[1]}x{insz[0]}'
    return cfg


def _apply_legacy_yaml(cfg: Config, path: str) -> Config:
    import yaml
    with open(path) as f:
        y = yaml.safe_load(f) or {}
    m, t = y.get('MODEL', {}) or {}, y.get('TRAIN', {}) or {}
    if 'NUM_JOINTS' in m:
        K = int(m['NUM_JOINTS'])
        cfg.data.num_keypoints = cfg.model.num_keypoints = K
        if K != 17:
            cfg.data.keypoint_names = [f'kpt_{i}' for i in range(K)]
            cfg.data.flip_pairs = []
    if 'IMAGE_SIZE' in m:      # legacy order is [W, H] as written by root config.py (IMAGE_SIZE = [288, 384])
        cfg.data.input_size = (int(m['IMAGE_SIZE'][0]), int(m['IMAGE_SIZE'][1]))
    if 'HEATMAP_SIZE' in m:
        cfg.data.heatmap_size = (int(m['HEATMAP_SIZE'][0]), int(m['HEATMAP_SIZE'][1]))
    if 'SIGMA' in m:
        cfg.data.sigma = cfg.model.target_sigma = float(m['SIGMA'])
    name = str(m.get('NAME', ''))
    if 'w48' in name:
        cfg.model.backbone, cfg.model.head_type, cfg.model.base_channels = 'hrnet_w48', 'heatmap', 48
    elif 'w32' in name:
        cfg.model.backbone, cfg.model.head_type, cfg.model.base_channels = 'hrnet_w32', 'heatmap', 32
    if m.get('FUSED_HEAD'):
        cfg.model.head_type = 'fusion'
    cfg.model.head_in_channels = cfg.model.base_channels
    for src, dst, cast in (('BATCH_SIZE', 'batch_size', int), ('EPOCHS', 'max_epochs', int), ('LR', 'lr', float),
                           ('WEIGHT_DECAY', 'weight_decay', float), ('NUM_WORKERS', 'num_workers', int),
                           ('VAL_INTERVAL', 'val_interval', int)):
        if src in t:
            setattr(cfg.train, dst, cast(t[src]))
    cj = (y.get('DATA', {}) or {}).get('COLOR_JITTER')
    if cj is not None:
        # an empty or all-zero block stays off: ranges (0, 0, 0) would still send half the samples through factors (1, 1, 1), which is
        # not the identity (u / 255 * 255 truncates)
        rng = tuple(float((cj or {}).get(k, 0) or 0) for k in ('BRIGHTNESS', 'CONTRAST', 'SATURATION'))
        cfg.train.color_jitter = rng if any(rng) else None
    # DATA.BLUR / DATA.NOISE / DATA.OCCLUSION are this project's own keys (the reference's yamls have none); an empty block or PROB: 0 is off
    for key, kind, attr in (('BLUR', 'blur', 'blur'), ('NOISE', 'noise', 'sensor_noise'), ('OCCLUSION', 'occlusion', 'occlusion')):
        blk = (y.get('DATA', {}) or {}).get(key)
        if blk is not None:
            if not isinstance(blk, dict):
                raise ValueError(f"DATA.{key} must be a mapping, got {blk!r}")
            setattr(cfg.train, attr, check_augment(kind, {str(k).lower(): v for k, v in blk.items()}, f"DATA.{key}"))
    # LOSS.USE_OHKM / LOSS.TOPK are HRNet's own keys (TOPK defaults to its 8); LOSS.OHKM_WEIGHT weighs the term in the fusion loss.  A yaml
    # without USE_OHKM: true keeps mining off whatever else the block holds
    ls = y.get('LOSS', {}) or {}
    if ls.get('USE_OHKM'):
        cfg.model.ohkm_topk, cfg.model.ohkm_weight = check_ohkm(ls.get('TOPK', 8), ls.get('OHKM_WEIGHT', ModelConfig.ohkm_weight),
                                                                cfg.model.num_keypoints, False, ('LOSS.TOPK', 'LOSS.OHKM_WEIGHT'))
    adv = y.get('ADVANCED', {}) or {}
    if adv.get('MULTI_SCALE_TEST'):
        sl = adv.get('SCALE_LIST')
        cfg.test_scales = check_test_scales(sl) if sl is not None else (1.0,)
    ev = y.get('EVAL', {}) or {}
    if ev.get('METRICS') is not None:
        cfg.eval_metrics = tuple(str(v) for v in ev['METRICS'])
    if 'PCK_THRESHOLD' in ev:
        cfg.pck_threshold = float(ev['PCK_THRESHOLD'])
    if 'MIN_KEYPOINT_VISIBILITY' in ev:
        cfg.min_keypoint_visibility = float(ev['MIN_KEYPOINT_VISIBILITY'])
    # TEST block: detector boxes.  (EVAL.OKS_THRESHOLD is the match threshold of an AP, not an NMS threshold: not mapped.)
    te = y.get('TEST', {}) or {}
    if te.get('COCO_BBOX_FILE'):
        cfg.bbox_file = str(te['COCO_BBOX_FILE'])
    for src, dst in (('IMAGE_THRE', 'det_score_thr'), ('OKS_THRE', 'oks_nms_thr'), ('IN_VIS_THRE', 'in_vis_thr')):
        if te.get(src) is not None:
            setattr(cfg, dst, float(te[src]))
    if 'SOFT_NMS' in te:
        cfg.soft_nms = bool(te['SOFT_NMS'])
    # TEST.DECODE / TEST.MODULATE_KERNEL choose the heatmap decode.  TEST.POST_PROCESS and TEST.SHIFT_HEATMAP are NOT mapped: both shipped
    # yamls set them true, so mapping them would change what those configurations compute today.
    if te.get('DECODE') is not None or te.get('MODULATE_KERNEL') is not None:
        cfg.decode, cfg.modulate_kernel = check_decode(te.get('DECODE'), te.get('MODULATE_KERNEL', Config.modulate_kernel),
                                                       ('TEST.DECODE', 'TEST.MODULATE_KERNEL'))
    if te.get('USE_GT_BBOX') is False and cfg.bbox_file is None:
        logging.getLogger(__name__).warning(f"{path}: TEST.USE_GT_BBOX is false but no TEST.COCO_BBOX_FILE is given: validation keeps "
                                            "cropping from the ground-truth boxes")
    tp = y.get('TEMPORAL', {}) or {}
    if tp.get('ENABLED'):
        window = int(tp.get('WINDOW_SIZE', 5))
        if window < 1 or window % 2 == 0:
            raise ValueError(f"TEMPORAL.WINDOW_SIZE must be odd and positive (temporal_smoothing has no even window), got {window}")
        cfg.temporal = (window, str(tp.get('SMOOTHING_METHOD', 'gaussian')))
    cl = y.get('CLINICAL', {}) or {}
    if cl.get('ENABLE_MOVEMENT_TRACKING'):
        cfg.clinical = {'min_movement': float(cl.get('MIN_MOVEMENT_THRESHOLD', 5.0)), 'max_movement': float(cl.get('MAX_MOVEMENT_THRESHOLD', 200.0)),
                        'alert_low': bool(cl.get('ALERT_ON_LOW_MOVEMENT', False)), 'alert_asymmetry': bool(cl.get('ALERT_ON_ASYMMETRY', False))}
    # CLINICAL.FREQUENCY_BAND: [lo, hi] in Hz is this project's own key (the reference's yamls have none): the band of the movement spectrum
    if cl.get('FREQUENCY_BAND') is not None:
        cfg.frequency_band = check_frequency_band(cl['FREQUENCY_BAND'], 'CLINICAL.FREQUENCY_BAND')
    # CLINICAL.JOINT_ANGLES: {name: [a, b, c]} and CLINICAL.KINEMATICS: {MAX_LAG, ENTROPY_M, ENTROPY_R} are this project's own keys as well:
    # the angle table and the settings of `kinematics_report`.  They land on attributes of their own; `cfg.clinical` keeps its four entries.
    if cl.get('JOINT_ANGLES') is not None:
        cfg.joint_angles = check_joint_angles(cl['JOINT_ANGLES'], 'CLINICAL.JOINT_ANGLES')
    if cl.get('KINEMATICS') is not None:
        kin = cl['KINEMATICS']
        if not isinstance(kin, dict) or set(kin) - {'MAX_LAG', 'ENTROPY_M', 'ENTROPY_R'}:
            raise ValueError(f"CLINICAL.KINEMATICS must be a mapping with the keys MAX_LAG, ENTROPY_M, ENTROPY_R, got {kin!r}")
        cfg.kinematics = check_kinematics(kin.get('MAX_LAG'), (kin.get('ENTROPY_M', 2), kin.get('ENTROPY_R', 0.2)),
                                          ('CLINICAL.KINEMATICS.MAX_LAG', 'CLINICAL.KINEMATICS.ENTROPY_M', 'CLINICAL.KINEMATICS.ENTROPY_R'))
    cfg.exp_name = os.path.splitext(os.path.basename(path))[0]
    return cfg


def get_config(source: Optional[str] = None) -> Config:
    """`get_config()` == the reference default. `get_config('hrformer_small')` / `get_config('x.yaml')` extend it."""
    cfg = Config()
    if source is None:
        return cfg
    if source in _PRESETS:
        return _apply_preset(cfg, source)
    if os.path.isfile(source):
        return _apply_legacy_yaml(cfg, source)
    raise ValueError(f"Unknown config source: {source}")
