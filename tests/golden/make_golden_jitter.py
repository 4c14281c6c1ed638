#!/usr/bin/env python3
"""Golden vectors of the reference's CustomColorJitter (data/examples.py:367-401), captured from the reference's own class (build
container only: the reference tree cannot travel).

    POSE_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_jitter.py      # writes tests/golden/color_jitter.npz

data/examples.py imports cv2 and other packages this image lacks, so the module is not imported: its source is parsed and ONLY the
`CustomColorJitter` class definition is compiled, with numpy as its one global.  Each case seeds numpy's global RandomState, which the
class draws from, and records the input crop, the seed, the factors those draws produce (re-derived here with the same calls) and the
class's uint8 output.  prob = 1.0, so every case is jittered; the ranges are configs/preemie_optimized.yaml's (0.3, 0.3, 0.2), wider for
the saturating case.

Before writing, the numpy model of the device arithmetic (tests/jitter_np.py) is held against every case: it may differ from the
reference by at most 1 on at most 0.1 % of the bytes (float32 pairwise mean() against the exact sum).  A case that misses that for the
model alone is not a fixture: pick another seed.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import jitter_np  # noqa: E402

CAP_SHARE, CAP_DIFF = 1e-3, 1


def reference_class():
    root = os.environ.get("POSE_REFERENCE_ROOT")
    if not root:
        sys.exit("set POSE_REFERENCE_ROOT to the reference checkout")
    path = os.path.join(root, "data", "examples.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CustomColorJitter")
    ns = {"np": np}
    exec(compile(ast.Module([node], []), path, "exec"), ns)
    return ns["CustomColorJitter"]


def cases():
    rng = np.random.default_rng(20251017)
    smooth = np.clip(np.add.outer(np.linspace(20, 200, 64), np.linspace(0, 50, 48))[..., None] + rng.integers(-12, 13, (64, 48, 3)), 0, 255)
    return [  # name, crop, seed, (brightness, contrast, saturation) ranges
        ("rand16x12", rng.integers(0, 256, (16, 12, 3), dtype=np.uint8), 101, (0.3, 0.3, 0.2)),
        ("rand64x48", rng.integers(0, 256, (64, 48, 3), dtype=np.uint8), 102, (0.3, 0.3, 0.2)),
        ("smooth64x48", smooth.astype(np.uint8), 103, (0.3, 0.3, 0.2)),
        ("constant", np.full((16, 12, 3), 137, np.uint8), 104, (0.3, 0.3, 0.2)),
        ("saturating", rng.integers(150, 256, (16, 12, 3), dtype=np.uint8), brightening_seed(105, 0.6, 1.4), (0.6, 0.6, 0.6)),
    ]


def brightening_seed(first, brightness, at_least):
    """First seed from `first` on whose draws give a brightness factor >= at_least (the saturating case has to be brightened)."""
    seed = first
    while True:
        np.random.seed(seed)
        np.random.rand()
        if 1 + np.random.uniform(-brightness, brightness) >= at_least:
            return seed
        seed += 1


def main():
    cls = reference_class()
    out, names = {}, []
    for name, img, seed, (rb, rc, rs) in cases():
        np.random.seed(seed)
        want = cls(brightness=rb, contrast=rc, saturation=rs, prob=1.0)({"img": img.copy()})["img"]
        after = np.random.get_state()[1].copy()
        np.random.seed(seed)
        np.random.rand()
        factors = np.array([1 + np.random.uniform(-r, r) for r in (rb, rc, rs)], np.float64)
        assert np.array_equal(np.random.get_state()[1], after), "the class drew something else than rand() + 3 x uniform()"
        assert want.dtype == np.uint8 and want.shape == img.shape
        got = jitter_np.jitter_u8(img, *factors)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        share = float((diff > 0).mean())
        print(f"{name:12s} seed {seed} factors {factors.round(4)} changed bytes {float((want != img).mean()):.3f} "
              f"model != reference on {share:.2e} of the bytes, max {int(diff.max())}")
        assert diff.max() <= CAP_DIFF and share <= CAP_SHARE, f"{name}: the model alone misses the cap, pick another seed"
        if name == "saturating":
            assert (want == 255).mean() > 0.05, "the saturating case must clip"
        names.append(name)
        out[f"{name}.img"], out[f"{name}.seed"], out[f"{name}.ranges"] = img, np.int64(seed), np.array([rb, rc, rs], np.float64)
        out[f"{name}.factors"], out[f"{name}.out"] = factors, want
    out["names"] = np.array(names)
    path = os.path.join(HERE, "color_jitter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
