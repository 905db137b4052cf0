"""Inputs of the float64 pins of the depth filters, the sampler, the crop window, the pose update and arg-max, built
without a GPU and shared by tests/test_pose_rules_ref_cpu.py (oracle) and tests/test_pose_rules_gpu.py (device)."""
import dataclasses
import functools
from fractions import Fraction as Fr

import numpy as np

from foundationpose_cpp_amd import synthetic as syn
from geometry_cases import random_case

RATIOS = (1.2, 1.1)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Frame:
    name: str
    K: np.ndarray
    rgb: np.ndarray
    depth: np.ndarray
    mask: np.ndarray
    hw: tuple


def _ragged_mask(rng, hw, value):
    """a third of the frame each way, 40 % of it set to `value`"""
    H, W = hw
    m = np.zeros(hw, np.uint8)
    y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
    m[y0:y0 + H // 3, x0:x0 + W // 3] = (rng.uniform(size=(H // 3, W // 3)) < 0.4) * value
    return m


MASK_VALUES = (1, 128, 255)
RULE_FRAME_SIZES = {"f160x120": (160, 120), "f333x257": (333, 257), "f641x479": (641, 479)}   # H W: a multiple of 256, a tail of 77, odd both ways


@functools.lru_cache(maxsize=None)
def frame(name):
    """`rnd<seed>`: the frame of geometry_cases.random_case(seed) | `scene`: syn.make_scene | `f<W>x<H>`: a wavy surface with steps of
    0.6 ... 1.4 mm between neighbouring columns (the erode rule's 1 mm), 2 mm of noise, holes, a noise corner and a border of valid
    depth 2 mm rough all round (the filters' frame-edge rule meets valid taps there, and most of them are bad).  Masks take the values 1, 128 and 255 in turn."""
    if name.startswith("rnd"):
        seed = int(name[3:])
        _, K, rgb, depth, _, hw = random_case(seed)
        rng = np.random.default_rng(2000 + seed)
        return Frame(name, K, rgb, depth, _ragged_mask(rng, hw, MASK_VALUES[seed % 3]), hw)
    if name == "scene":
        mesh = syn.make_mesh()
        sc = syn.make_scene(mesh)
        return Frame(name, sc.K, sc.rgb, sc.depth, sc.mask, sc.depth.shape)
    W, H = RULE_FRAME_SIZES[name]
    rng = np.random.default_rng(W * 1000 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = 0.7 + 0.2 * np.sin(xx / W * 5.0) * np.cos(yy / H * 3.0) + 0.001 * (xx % 7) * rng.uniform(0.6, 1.4, (H, W)) + rng.normal(0, 0.002, (H, W))
    depth[rng.uniform(size=(H, W)) < 0.1] = 0.0
    depth[H // 2:H // 2 + H // 8, :W // 8] = rng.uniform(0.0005, 6.0, (H // 8, W // 8))
    border = np.ones((H, W), bool)
    border[2:H - 2, 2:W - 2] = False
    depth[border] = 0.65 + rng.normal(0, 0.002, int(border.sum()))
    K = np.array([[0.9 * W, 0, 0.47 * W], [0, 1.05 * W, 0.55 * H], [0, 0, 1]], np.float32)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = _ragged_mask(rng, (H, W), MASK_VALUES[(W + H) % 3])
    return Frame(name, K, rgb, depth.astype(np.float32), mask, (H, W))


CPU_FRAMES = [f"rnd{s}" for s in range(12)] + ["scene"] + list(RULE_FRAME_SIZES)
GPU_FRAMES = list(RULE_FRAME_SIZES) + ["rnd0", "rnd1", "rnd2"]


# ---- crop windows ---------------------------------------------------------------------------------------------------------------------
def sweep_poses(seed, n=200):
    """n seeded poses of random_case(seed)'s camera: z from 0.12 to 3 m, centres up to 10 % outside the frame -> (mesh, K, poses, hw)"""
    mesh, K, _, _, _, hw = random_case(seed)
    rng = np.random.default_rng(7000 + seed)
    H, W = hw
    poses = []
    for i in range(n):
        z = float(np.exp(rng.uniform(np.log(0.12), np.log(3.0))))
        u, w = rng.uniform(-0.1, 1.1) * W, rng.uniform(-0.1, 1.1) * H
        t = (z * (u - K[0, 2]) / K[0, 0], z * (w - K[1, 2]) / K[1, 1], z)
        poses.append(syn.pose_matrix(syn.random_rotation(31 * seed + i), t))
    return mesh, K, np.stack(poses).astype(np.float32), hw


# Hand-made ties, every f32 operation exact: fx = fy = 256, cx = 300.5, cy = 200.5, diameter 0.25, ratio 1.5 -> r = 0.1875 m, 48 px at
# z = 1.  With t = ((a - 300.5) / 256, (b - 200.5) / 256, 1) the centre is (a, b) and the edges are a -+ 48, b -+ 48 before rounding.
HAND_K = np.array([[256, 0, 300.5], [0, 256, 200.5], [0, 0, 1]], np.float32)
HAND_DIAMETER, HAND_RATIO, HAND_RADIUS = 0.25, 1.5, 48
HAND_HW = (480, 640)
# (centre a, centre b) as fractions -> the expected (left, right, top, bottom), rounded half away from zero BY HAND
HAND_WINDOWS = [
    ((Fr(3, 2), Fr(5, 2)), (-47, 50, -46, 51)),          # tx = -299/256: left = round(-46.5) = -47 (half-even and floor(x + 1/2): -46); top -45.5 -> -46
    ((Fr(101, 2), Fr(103, 2)), (3, 99, 4, 100)),         # positive ties of both parities: 2.5 -> 3, 98.5 -> 99, 3.5 -> 4, 99.5 -> 100
    ((Fr(-201, 2), Fr(-203, 2)), (-149, -53, -150, -54)),   # wholly left of and above the frame: -148.5, -52.5, -149.5, -53.5
    ((Fr(100), Fr(60)), (52, 148, 12, 108)),             # no tie at all
    ((Fr(193, 4), Fr(1, 4)), (0, 96, -48, 48)),          # x.25: 0.25 -> 0, 96.25 -> 96, -47.75 -> -48, 48.25 -> 48
]


def hand_poses():
    out = []
    for (a, b), _ in HAND_WINDOWS:
        t = (float((a - Fr(601, 2)) / 256), float((b - Fr(401, 2)) / 256), 1.0)
        assert all(np.float32(x) == x for x in t)
        out.append(syn.pose_matrix(np.eye(3), t))
    return np.stack(out).astype(np.float32)


def hand_mesh():
    """any small mesh; only its DECLARED diameter (0.25) enters the window"""
    s, faces = syn._icosphere(1)
    v = (s * 0.05).astype(np.float32)
    return syn.Mesh("hand", v, s.astype(np.float32), np.zeros((len(s), 2), np.float32), faces, np.full((2, 2, 3), 100, np.uint8),
                    diameter=HAND_DIAMETER, center=np.zeros(3, np.float32))


# ---- pose updates -----------------------------------------------------------------------------------------------------------------------
def pose_updates(n=2000, seed=5):
    """poses [n, 4, 4], trans [n, 3], rot [n, 3]: rot of every 7th row scaled by 1e-4, of every 11th by 20, of every 13th exactly zero; row 0
    has a zero update altogether"""
    rng = np.random.default_rng(seed)
    poses = np.stack([syn.pose_matrix(syn.random_rotation(900 + i), rng.normal(size=3) * (0.3, 0.3, 1.0)) for i in range(n)]).astype(np.float32)
    trans = rng.normal(size=(n, 3)).astype(np.float32)
    rot = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
    rot[::7] *= np.float32(1e-4)
    rot[::11] *= np.float32(20)
    rot[::13] = 0
    rot[0] = 0
    trans[0] = 0
    return poses, trans, rot


# ---- sampler patterns (values, mask) for the raw hook, K = identity: the centre's z is the median's bits --------------------------------
@dataclasses.dataclass
class Pattern:
    name: str
    vals: np.ndarray       # [H, W] f32
    mask: np.ndarray       # [H, W] u8
    min_depth: float = 0.001


def _bits(x):
    return np.array(x, np.uint32).view(np.float32)


def _scatter(rng, hw, values, mask_value=1, background=7.0):
    """the values at random pixels under the mask; everything else holds `background` (and a few NaNs) outside the mask"""
    H, W = hw
    vals = np.full(H * W, background, np.float32)
    vals[::17] = np.nan
    mask = np.zeros(H * W, np.uint8)
    idx = rng.permutation(H * W)[:len(values)]
    vals[idx] = np.asarray(values, np.float32)
    mask[idx] = mask_value
    return vals.reshape(H, W), mask.reshape(H, W)


SMALL, TAIL = (48, 64), (257, 333)       # H, W: 12 workgroups of the scan | 334 workgroups + a tail of 77 pixels


@functools.lru_cache(maxsize=None)
def sampler_patterns():
    rng = np.random.default_rng(77)
    out = []

    def add(name, hw, values, mask_value=1, min_depth=0.001):
        v, m = _scatter(rng, hw, values, mask_value)
        out.append(Pattern(name, v, m, min_depth))

    for n in (1, 2, 3, 1023, 1024, 1025):
        add(f"n={n}", SMALL, rng.uniform(0.3, 1.2, n))
    add("n=20001", TAIL, rng.uniform(0.3, 1.2, 20001))
    add("n=20000 quantised", TAIL, rng.integers(600, 640, 20000) / 1000.0)
    add("all equal", SMALL, np.full(500, 0.731))
    add("clusters 0.4 / 0.6, even", SMALL, [0.4] * 300 + [0.6] * 300)          # the two middle values in top-digit buckets 0x3E / 0x3F
    add("clusters 0.4 / 0.6, spread", SMALL, np.concatenate([rng.uniform(0.39, 0.41, 513), rng.uniform(0.59, 0.61, 513)]))
    add("lowest byte only", SMALL, _bits(0x3F000000 + rng.integers(0, 256, 700)))
    add("byte 1 only", SMALL, _bits(0x3F000000 + (rng.integers(0, 256, 701) << 8)))
    add("byte 1 only, even", SMALL, _bits(0x3F000000 + (rng.integers(0, 256, 1400) << 8)))
    # k = n / 2 exactly on a bucket boundary of pass 3, 2, 1, 0 (digit = bits 24-31, 16-23, 8-15, 0-7): A below B in that digit alone
    for p, (a, b) in zip((3, 2, 1, 0), ((0x3E800000, 0x3F800000), (0x3F010000, 0x3F020000), (0x3F000100, 0x3F000200), (0x3F000001, 0x3F000002))):
        for ka, kb in ((37, 38), (38, 37), (37, 37), (1024, 1025), (1025, 1024), (1024, 1024)):
            add(f"pass {p} boundary {ka}+{kb}", SMALL, _bits([a] * ka + [b] * kb))
        # ... with values in other buckets on both sides
        add(f"pass {p} boundary flanked", SMALL, np.concatenate([_bits([a] * 40 + [b] * 41), np.full(25, 0.1, np.float32), np.full(24, 3.0, np.float32)]))
    add("0.49999997 / 0.5", SMALL, [np.float32(0.49999997)] * 50 + [0.5] * 50)
    add("0.49999997 / 0.5 odd", SMALL, [np.float32(0.49999997)] * 50 + [0.5] * 51)
    md = np.float32(0.001)
    add("at min_depth and just below", SMALL, [md] * 3 + [np.nextafter(md, np.float32(0))] * 5 + [0.5] * 2)     # valid: md md md .5 .5
    add("at min_depth, even", SMALL, [md] * 2 + [np.nextafter(md, np.float32(0))] * 7 + [0.5] * 2)           # valid: md md .5 .5
    add("min_depth 0.25", SMALL, [0.25] * 4 + [np.nextafter(np.float32(0.25), np.float32(0))] * 9 + [0.75] * 3, min_depth=0.25)
    add("+inf and NaN under the mask", SMALL, [0.3, 0.5, np.inf, np.nan, np.nan])
    add("+inf in the middle pair", SMALL, [0.3, 0.5, np.inf, np.inf, np.nan])
    add("zeros and negatives under the mask", SMALL, [0.0, -0.0, -1.0, 0.4, 0.45, 0.5, 0.0005])
    # masks
    for name, hw, pix, mv in (("one pixel at index 0", SMALL, [(0, 0)], 1), ("one pixel at the last index of a tail wave", TAIL, [(256, 332)], 255),
                              ("corners in different workgroups", TAIL, [(0, 0), (256, 332)], 128), ("last pixel of a full frame", SMALL, [(47, 63)], 1)):
        v = rng.uniform(0.3, 1.2, hw).astype(np.float32)
        m = np.zeros(hw, np.uint8)
        for y, x in pix:
            m[y, x] = mv
        out.append(Pattern(name, v, m))
    v = rng.uniform(0.3, 1.2, SMALL).astype(np.float32)
    m = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), SMALL)
    out.append(Pattern("mask values 1, 128, 255", v, m))
    out.append(Pattern("full-frame mask, tail", rng.uniform(0.3, 1.2, TAIL).astype(np.float32), np.full(TAIL, 1, np.uint8)))
    return out


def sampler_sequence():
    """valid -> empty mask -> valid -> no valid depth -> valid, on one frame size"""
    rng = np.random.default_rng(78)
    va, ma = _scatter(rng, SMALL, rng.uniform(0.3, 1.2, 333))
    vb, mb = _scatter(rng, SMALL, rng.uniform(0.3, 1.2, 1000), 255)
    vc, mc = _scatter(rng, SMALL, rng.uniform(0.3, 1.2, 64), 128)
    return [Pattern("valid a", va, ma), Pattern("empty mask", va, np.zeros(SMALL, np.uint8)), Pattern("valid b", vb, mb),
            Pattern("no valid depth", np.where(mc > 0, np.float32(0.0005), vc).astype(np.float32), mc), Pattern("valid c", vc, mc)]


# ---- arg-max -----------------------------------------------------------------------------------------------------------------------------
ARGMAX_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1008)


@functools.lru_cache(maxsize=None)
def argmax_cases():
    """(name, scores); a NaN case has to be an error"""
    rng = np.random.default_rng(79)
    out = []
    for n in ARGMAX_SIZES:
        s = rng.normal(size=n).astype(np.float32)
        out.append((f"random n={n}", s))
        last = s.copy()
        last[-1] = 9.0
        out.append((f"maximum at the last index n={n}", last))
        out.append((f"all equal n={n}", np.full(n, 0.25, np.float32)))
        out.append((f"all -inf n={n}", np.full(n, -np.inf, np.float32)))
        z = np.full(n, -0.0, np.float32)
        z[n // 2:] = 0.0
        out.append((f"-0.0 then +0.0 n={n}", z))
        z = np.full(n, 0.0, np.float32)
        z[n // 2:] = -0.0
        out.append((f"+0.0 then -0.0 n={n}", z))
        if n > 256:                       # a tie inside one thread's stride: i and i + 256
            t = s.copy()
            t[[n - 257, n - 1]] = 8.0
            out.append((f"tie at i and i + 256 n={n}", t))
        if n >= 255:                      # ties across threads, the later one in a lower thread
            t = s.copy()
            t[[200, 3, 77]] = 8.0
            out.append((f"tie across threads n={n}", t))
            if n > 300:
                t = s.copy()
                t[[258, 5 + 256, 200]] = 8.0    # thread 2 (second element), thread 5 (second element), thread 200 (first): the first is 200
                out.append((f"tie across strides n={n}", t))
        inf = s.copy()
        inf[n // 3] = np.inf
        out.append((f"+inf n={n}", inf))
    return out


def argmax_nan_cases():
    rng = np.random.default_rng(80)
    out = []
    for n, where in ((1, 0), (2, 1), (256, 255), (257, 256), (513, 300), (1008, 0), (1008, 1007)):
        s = rng.normal(size=n).astype(np.float32)
        s[where] = np.nan
        out.append((f"NaN at {where} of {n}", s))
    return out
