"""Seeded cases under a GENERAL camera, shared by tests/test_camera_cases_cpu.py and tests/test_camera_sweep_gpu.py
and built without a GPU: fx != fy by at least 10 %, a principal point off the centre and off every integer and half pixel, landscape,
portrait and odd frames, one axis an exact multiple of the 32 px tile and the other ragged.  Nobody hand-picked the numbers: every case
is drawn from its seed under the conditions stated in `camera_case`, and the module asserts that the mistakes the sweep is for (fx for
fy, cx for cy, a truncated principal point) move the image of the frame's corner by more than 2 px.  References are computed once and
shared; callers must not modify them."""
import functools

import numpy as np

import frame_render_ref as FR
from vsd_ref import is_convex
from foundationpose_cpp_amd import synthetic as syn

f32 = np.float32
SEEDS = (0, 1, 2, 3, 4, 5)
SIZES = ((160, 120), (120, 160), (131, 97), (97, 131), (224, 96), (96, 224))          # (W, H), taken in turn by the seeds
POSES = ("inside", "vertical_edge", "horizontal_edge", "near")
TILE = 32
MIN_MODEL_PIXELS = 500
MIN_Z = 0.05                 # every vertex of every truth pose and estimate is at least this far in front of the camera plane
NEAR_Z = 0.15
BROKEN = ("swap_fx_fy", "swap_cx_cy", "principal_point_truncated", "fy_is_fx")          # the camera controls of the CPU tests
ICP_ITERATIONS = 8

# ---- measured on the CPU by tests/test_camera_cases_cpu.py, which holds the references to them -------------------
# (d) the "inside" pose of every case, estimate -> 8 iterations at gate 0.2 x diameter on the case's depth: how far icp32 (the
# iteration on the f32 restatement's sums) ends from icp64 (degrees, millimetres), and how far they end from the truth pose
ICP_AB = {0: (0.0359, 0.0074), 1: (0.0, 0.0056), 2: (0.0262, 0.0097), 3: (0.0867, 0.0465), 4: (0.0, 0.0204), 5: (0.0, 0.0022)}
ICP_GT = {0: (0.0431, 0.0155), 1: (0.0, 0.0073), 2: (0.0219, 0.0194), 3: (0.0813, 0.0432), 4: (0.0083, 0.0169), 5: (0.0, 0.0054)}          # the farther of the two
# what a recorded value may differ by on another numpy / BLAS, degrees and millimetres.  The angle between two poses held in f32 has a floor:
# the entries of a rotation carry 6e-8, the trace 1e-7 or so, and arccos turns that into sqrt(2e-7) rad = 0.03 deg, which is why the
# angles above are 0 or a few hundredths
ICP_SLACK = (0.05, 2e-3)
# the device is held to twice the worst of each, the margin of section 4.12: both iterations sit in a small cycle around the fixed point
AB_BOUND_DEG, AB_BOUND_M = 2 * max(v[0] for v in ICP_AB.values()), 2 * max(v[1] for v in ICP_AB.values()) * 1e-3
GT_BOUND_DEG, GT_BOUND_M = 2 * max(v[0] for v in ICP_GT.values()), 2 * max(v[1] for v in ICP_GT.values()) * 1e-3
# fp_register_depth's scene (`register_scene`): search_ref.register_ref with icp64, top_k 16, tol 5 mm, 15 iterations -> MSSD in millimetres.
# Seed 2, not 0: on seed 0 the float64 reference itself ends on a mirrored pose of the nearly symmetric body, 57 mm from the truth
# (seeds 1 to 5: 0.12 to 0.19 mm)
REGISTER_SEED = 2
REF_MSSD_MM = 0.171
REF_SLACK_MM = 0.01
REGISTER_BOUND_M = 2 * REF_MSSD_MM * 1e-3


def broken(K, how):
    """K with one mistake of a kernel or of the host's staging made on purpose"""
    K = np.array(K, f32).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if how == "swap_fx_fy":
        K[0, 0], K[1, 1] = fy, fx
    elif how == "swap_cx_cy":
        K[0, 2], K[1, 2] = cy, cx
    elif how == "principal_point_truncated":
        K[0, 2], K[1, 2] = np.floor(cx), np.floor(cy)
    elif how == "fy_is_fx":
        K[1, 1] = fx
    else:
        raise KeyError(how)
    return K


def _away_from_the_grid(x):
    """not within 0.2 px of an integer or a half, and on the far side of the half: truncating it moves the image by 0.7 px at least (a
    fraction of 0.2 to 0.3 moved two of the 24 pose pairs by too little for the ICP and the search references to notice)"""
    return 0.7 <= x % 1.0 <= 0.8


def _camera(rng, W, H, tall):
    """tall: fy > fx (r in [1.1, 1.4]), else r in [0.7, 0.9]"""
    while True:
        fx = rng.uniform(0.6, 1.4) * W
        r = rng.uniform(1.1, 1.4) if tall else rng.uniform(0.7, 0.9)
        cx, cy = rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H
        K = np.array([[fx, 0, cx], [0, fx * r, cy], [0, 0, 1]], f32)
        if _away_from_the_grid(float(K[0, 2])) and _away_from_the_grid(float(K[1, 2])) and abs(float(K[0, 2]) - float(K[1, 2])) > 3.0:
            return K


def corner_shift(K, how, W, H):
    """how far (px) the image of the point behind the frame's corner farthest from the principal point moves under broken(K, how)"""
    K = np.asarray(K, np.float64)
    B = np.asarray(broken(K, how), np.float64)
    u = 0.0 if K[0, 2] > (W - 1) / 2 else W - 1.0
    v = 0.0 if K[1, 2] > (H - 1) / 2 else H - 1.0
    X, Y = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    return float(np.hypot(B[0, 0] * X + B[0, 2] - u, B[1, 1] * Y + B[1, 2] - v))


def _meshes(rng, seed):
    """the dented, off-centre icosphere of geometry_cases.random_case (1 or 2 subdivisions: 80 or 320 faces, semi-axes small enough for
    the near pose) and, for the float64 VSD reference, a convex one: the undented ellipsoid with its own axes, off-centre too"""
    s, faces = syn._icosphere(1 + seed % 2)
    tex = np.full((2, 2, 3), 100, np.uint8)
    uv = np.zeros((len(s), 2), f32)
    out = []
    for name, dent in ((f"cam{seed}", 0.25), (f"cvx{seed}", 0.0)):
        ax = rng.uniform(0.025, 0.06, 3)
        v = s * ax * (1.0 + dent * rng.uniform(-1, 1, (len(s), 1))) + rng.uniform(-0.05, 0.05, 3)
        n = s / ax
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        out.append(syn.Mesh(name, v.astype(f32), n.astype(f32), uv, faces, tex).finalize())
    return out


def model_depth(mesh, P, K, H, W):
    """fp_render_pose's model_depth of the mesh under P: [H,W] f32, 0 where no model"""
    v = FR.centred(mesh)
    cam, snap, near, far = FR.project(v, np.asarray(P, f32), K)
    assert not near.any() and not far.any()
    keys = FR.rasterize(cam, snap, FR.stored_faces(v, mesh.faces), H, W)
    return np.where(keys != FR.EMPTY, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)


def _min_z(mesh, P):
    v = FR.centred(mesh).astype(np.float64)
    P = np.asarray(P, np.float64)
    return float((v @ P[2, :3] + P[2, 3]).min())


def _truths(rng, seed, mesh, K, W, H):
    """four poses: inside the frame, across a vertical edge of it, across a horizontal edge, and near (about 0.15 m, many tiles)"""
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    radius = float(np.linalg.norm(FR.centred(mesh).astype(np.float64), axis=1).mean())
    z_floor = float(np.linalg.norm(FR.centred(mesh).astype(np.float64), axis=1).max()) + MIN_Z + 0.005
    z_mid = min(fx, fy) * radius / (0.2 * min(W, H))           # a silhouette about 0.4 of the shorter side across
    out = []
    for i, kind in enumerate(POSES):
        R = syn.random_rotation(100 * seed + i)
        for _ in range(100):
            if kind == "inside":
                z, u, w = z_mid * rng.uniform(0.9, 1.1), rng.uniform(0.4, 0.6) * W, rng.uniform(0.4, 0.6) * H
            elif kind == "vertical_edge":
                z, u, w = z_mid * rng.uniform(0.7, 0.9), float(rng.choice([0.0, W - 1.0])) + rng.uniform(-4, 4), rng.uniform(0.35, 0.65) * H
            elif kind == "horizontal_edge":
                z, u, w = z_mid * rng.uniform(0.7, 0.9), rng.uniform(0.35, 0.65) * W, float(rng.choice([0.0, H - 1.0])) + rng.uniform(-4, 4)
            else:
                z, u, w = NEAR_Z * rng.uniform(0.95, 1.1), rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H
            z = max(z, z_floor)
            G = syn.pose_matrix(R, (z * (u - cx) / fx, z * (w - cy) / fy, z))
            E = syn.perturb_pose(G, deg=3.0, trans=0.03 * mesh.diameter, seed=10 * seed + i)
            if _min_z(mesh, G) >= MIN_Z and _min_z(mesh, E) >= MIN_Z and (model_depth(mesh, G, K, H, W) != 0).sum() >= MIN_MODEL_PIXELS:
                break
        else:
            raise AssertionError(f"seed {seed}: no {kind} pose under the conditions")
        out.append((G, E))
    return np.stack([g for g, _ in out]).astype(f32), np.stack([e for _, e in out]).astype(f32)


def _background(rng, W, H):
    """random_case's wavy surface, behind the objects: 2 mm of noise, 10 % of it missing"""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (rng.uniform(0.9, 2.0) + 0.5 * np.sin(xx / W * rng.uniform(2, 9) + rng.uniform(0, 6)) * np.cos(yy / H * rng.uniform(2, 9)) * rng.uniform(0.1, 0.5)
             + rng.normal(0, 0.002, (H, W))).astype(f32)
    return depth, rng.uniform(size=(H, W)) < 0.1


def _laid_over(background, missing, z, holes=True):
    """the rendering z laid over the background; 10 % of the pixels missing; on the object a block each of NaN, +inf, 0 and a value
    under FP_MIN_DEPTH (0.001 m)"""
    D = np.where(z != 0, z, background).astype(f32)
    D[missing] = 0.0
    if holes:
        rows, cols = np.nonzero(z != 0)
        r0, r1, c0, c1 = rows.min(), rows.max(), cols.min(), cols.max()
        h, w = max((r1 - r0) // 6, 2), max((c1 - c0) // 6, 2)
        rc, cc = (r0 + r1) // 2, (c0 + c1) // 2
        for (dr, dc), value in zip(((-h, -w), (-h, 0), (0, -w), (0, 0)), (np.nan, np.inf, 0.0, 0.0005)):
            D[rc + dr:rc + dr + h, cc + dc:cc + dc + w] = value
    return D


class Case:
    """seed, W, H, K [3,3] f32, mesh (dented), convex, G [4,4,4] f32 truth poses and E their estimates (in the order of POSES), rgb,
    depths [4]: depths[i] is the rendering of the dented mesh under G[i] laid over the case's surface; depth = depths[0] is THE frame"""


@functools.lru_cache(maxsize=None)
def camera_case(seed):
    rng = np.random.default_rng(7000 + seed)
    c = Case()
    c.seed = seed
    c.W, c.H = SIZES[seed % len(SIZES)]
    c.K = _camera(rng, c.W, c.H, tall=seed % 3 != 1)          # seeds 1 and 4: fy < fx
    for how in ("swap_fx_fy", "swap_cx_cy", "fy_is_fx"):
        assert corner_shift(c.K, how, c.W, c.H) > 2.0, (seed, how)
    assert corner_shift(c.K, "principal_point_truncated", c.W, c.H) > 0.98          # 0.7 px on both axes
    c.mesh, c.convex = _meshes(rng, seed)
    assert is_convex(c.convex) and not is_convex(c.mesh)
    c.G, c.E = _truths(rng, seed, c.mesh, c.K, c.W, c.H)
    c.rgb = rng.integers(0, 256, (c.H, c.W, 3), dtype=np.uint8)
    background, missing = _background(rng, c.W, c.H)
    c.depths = [_laid_over(background, missing, model_depth(c.mesh, G, c.K, c.H, c.W)) for G in c.G]
    c.depth = c.depths[0]
    c.gate = 0.2 * c.mesh.diameter
    return c


def tiles_of(z):
    """the 32 px tiles with a model pixel: {(tx, ty)}"""
    return {(int(x) // TILE, int(y) // TILE) for y, x in zip(*np.nonzero(z != 0))}


def symmetries(mesh):
    """two mesh-frame "symmetries" about the OFF-CENTRE mesh centre (half turns about its x and z axes): the dented mesh has none, so
    they only have to be applied right, conjugation with the centre included"""
    c = np.asarray(mesh.center, np.float64)
    out = []
    for d in ((1, -1, -1), (-1, -1, 1)):
        S = np.eye(4)
        S[:3, :3] = np.diag(d)
        S[:3, 3] = c - S[:3, :3] @ c
        out.append(S)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def register_scene(seed=REGISTER_SEED):
    """fp_register_depth's scene: the "inside" truth's rendering with 1 mm of noise over the case's surface (no holes), the mask from the
    model pixels -> (rgb, depth, mask, truth pose)"""
    c = camera_case(seed)
    rng = np.random.default_rng(7100 + seed)
    background, missing = _background(rng, c.W, c.H)
    z = model_depth(c.mesh, c.G[0], c.K, c.H, c.W)
    noisy = np.where(z != 0, z + rng.normal(0, 0.001, z.shape).astype(f32), 0).astype(f32)
    D = _laid_over(background, missing & (z == 0), noisy, holes=False)
    return c.rgb, D, np.where(z != 0, 255, 0).astype(np.uint8), c.G[0]


def mssd(mesh, P, G):
    v = FR.centred(mesh).astype(np.float64)
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    return float(np.linalg.norm((v @ P[:3, :3].T + P[:3, 3]) - (v @ G[:3, :3].T + G[:3, 3]), axis=1).max())
