"""The meshes, frames and poses tests/test_color_ref_cpu.py and the GPU tests of fp_pose_color / fp_resolve_symmetry share, built without a
GPU, and the hand answers.  The 200 x 150 frame, the intrinsics and the icospheres are those of tests/icp_cases.py, the scenes those of
tests/search_cases.py with the textured mesh (its depth is identical).  References are computed once and shared; callers must not
modify them."""
import dataclasses
import functools

import numpy as np

import color_ref as CR
import frame_render_ref as FR
import icp_cases as IC
import search_cases as SC
from foundationpose_cpp_amd import synthetic as syn

f32 = np.float32
W, H, K = IC.W, IC.H, IC.K
TOL = 0.005
SCENE_SEEDS, GPU_SEEDS = SC.SCENE_SEEDS, SC.GPU_SEEDS


def seeded_texture(th, tw, seed):
    return np.random.default_rng(seed).integers(0, 256, (th, tw, 3)).astype(np.uint8)


def with_texture(mesh, tex, name):
    return dataclasses.replace(mesh, name=name, texture=np.ascontiguousarray(tex, np.uint8))


def noise_rgb(seed, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mesh3():
    """the textured twin of search_cases.mesh(): 642 vertices, the synthetic 512 x 512 texture"""
    return syn.make_mesh(3, textured=True, name="ico3t")


@functools.lru_cache(maxsize=None)
def mesh2_tex8():
    """the mesh of the comparison of the two restatements: an 8 x 8 seeded texture (texels of several pixels, so that the 1/16 px snap
    moves few pixels over a texel boundary) on the 320-face ellipsoid.  Under the scenes' poses the 1 280 faces of mesh3() are about half a
    pixel each, and the snap alone then gives 2.2 to 3.4 % of the pixels to the triangle across an edge (measured on the four scenes:
    above the 2 % cap on all of them, with 0 to 4 pixels that differ in coverage or visibility); with 320 faces it is 1.3 to 1.9 %.  The
    scenes -- pose, picture and depth -- are the same: they are the analytic ellipsoid's."""
    return with_texture(syn.make_mesh(2, textured=True, name="ico2t8"), seeded_texture(8, 8, 8), "ico2t8")


@functools.lru_cache(maxsize=None)
def ico2(kind):
    m = syn.make_mesh(2, textured=True, name=f"ico2_{kind}")
    return m if kind == "512" else with_texture(m, seeded_texture(1, 47, 47), m.name)          # "47x1": 47 texels wide, 1 high


@functools.lru_cache(maxsize=None)
def quad():
    """a 12 cm square whose texture coordinates span several wraps and go negative, under a 4 x 3 texture"""
    h = 0.06
    v = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], f32)
    n = np.tile(np.array([[0, 0, 1]], f32), (4, 1))
    uv = np.array([[-0.6, -0.4], [1.7, -0.4], [1.7, 1.3], [-0.6, 1.3]], f32)
    return syn.Mesh("quad", v, n, uv, np.array([[0, 1, 2], [0, 2, 3]], np.int32), seeded_texture(3, 4, 5)).finalize()


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


QUAD_P = IC.pose(_rot_y(55.0), (0.0, 0.0, 0.25))          # strongly foreshortened: depths from 0.20 to 0.30 m


@functools.lru_cache(maxsize=None)
def scene(seed):
    return syn.make_scene(mesh3(), W=W, H=H, t=SC.SCENE_T, rot_seed=seed, noise_seed=seed + 1, drop_seed=seed + 2, bg_seed=seed + 3)


def mesh_frame_symmetries(mesh):
    """search_cases.SYMMETRIES (about the ellipsoid's centre, centred frame) as matrices of the MESH frame: x' = R (x - c) + c"""
    c = np.asarray(mesh.center, np.float64)
    out = []
    for S in SC.SYMMETRIES:
        M = np.array(S, np.float64)
        M[:3, 3] = c - M[:3, :3] @ c
        out.append(M.astype(f32))
    return np.stack(out)


def scene_equivalents(seed, pose=None):
    """the four equivalents of the scene's true pose (or of `pose`), the given one first"""
    m = mesh3()
    return CR.equivalents(scene(seed).gt_pose if pose is None else pose, mesh_frame_symmetries(m), m.center)


def frame_for(mesh, pose, k, D, seed, **kw):
    """a frame that shows the mesh under `pose`: its own values, dimmed (0.7 m + 20), over seeded noise"""
    bg = noise_rgb(seed, *D.shape)
    r = CR.sums_of_mesh(mesh, pose, k, bg, D, TOL, maps=True, **kw)
    at = r["texel"] >= 0
    out = bg.copy()
    out[at] = (r["values"][at] * 7 // 10 + 20).astype(np.uint8)
    return out


# ---- the ragged 96 x 80 window of tests/test_stage_scratch_gpu.py -----------------------------------------------------------------------
RW, RH = 96, 80
RX0, RY0 = (IC.W - RW) // 2, 35
RK = np.array(IC.K, f32)
RK[0, 2] -= RX0
RK[1, 2] -= RY0


def vertex_colors(mesh, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (len(mesh.vertices), 3)).astype(np.uint8)


BEHIND = IC.moved(IC.ICO_G, (0, 0, -0.5))                        # behind the camera: refused, near
BEYOND = IC.pose(t=(20000.0, 0.0, 0.2))                          # 1e7 px to the right, every vertex beyond the near constant: refused, range


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(mesh, poses [N,4,4], K, rgb, D, colors or None): the device records must equal color_ref.sums on each"""
    G = np.asarray(IC.ICO_G, f32)
    D2 = IC.rendering(IC.ico(2), G)
    c = dict(K=K, colors=None)
    if name in ("batch_47x1", "batch_512"):                       # 7 poses: near, far off, one over the frame's edge, one wholly outside
        m = ico2(name[6:])
        c.update(mesh=m, poses=IC.batch_poses(7), D=D2, rgb=frame_for(m, G, K, D2, 1))
    elif name.startswith("scene_"):                               # the four equivalents of the truth on a noisy scene, the scene's own 512^2 texture
        s = scene(int(name[6:]))
        c.update(mesh=mesh3(), poses=scene_equivalents(int(name[6:])), D=s.depth, rgb=s.rgb)
    elif name == "vertex_colors":
        m = ico2("512")
        col = vertex_colors(m)
        c.update(mesh=m, poses=IC.batch_poses(3), D=D2, colors=col, rgb=noise_rgb(2))
    elif name == "ragged":                                        # 3 x 3 tiles, the last row ragged, NaN and 0 in the window's depth
        m = ico2("512")
        D = np.ascontiguousarray(IC.record_case("nan_and_zero")[2][RY0:RY0 + RH, RX0:RX0 + RW], f32)
        c.update(mesh=m, poses=IC.batch_poses(3), K=RK, D=D, rgb=frame_for(m, G, RK, D, 3))
    elif name == "nan_zero_inf":
        m = ico2("512")
        D = SC.holes()
        c.update(mesh=m, poses=np.stack([G, syn.perturb_pose(G, deg=4.0, trans=0.004, seed=3)]), D=D, rgb=frame_for(m, G, K, D2, 4))
    elif name == "plate_in_front":                                # everything the camera sees is 0.20 m away: nothing of the model is visible
        m = ico2("512")
        c.update(mesh=m, poses=G[None], D=np.full((H, W), f32(0.20)), rgb=noise_rgb(5))
    elif name == "uv_wrap":
        m = quad()
        D = np.full((H, W), IC.WALL, f32)
        c.update(mesh=m, poses=np.stack([QUAD_P, IC.pose(_rot_y(-20.0), (0.02, 0.01, 0.3))]), D=D, rgb=frame_for(m, QUAD_P, K, D, 6))
    elif name == "refused":                                       # a near-refused and a range-refused pose between good ones
        m = ico2("512")
        c.update(mesh=m, poses=np.stack([G, BEHIND, IC.batch_poses(2)[1], BEYOND, G]), D=D2, rgb=frame_for(m, G, K, D2, 7))
    elif name == "grey":                                          # the 2 x 2 grey default texture: no variance
        c.update(mesh=IC.ico(2), poses=G[None], D=D2, rgb=noise_rgb(8))
    elif name in ("hand_2x2", "hand_3x2"):
        c.update(mesh=hand_mesh(2 if name == "hand_2x2" else 3), poses=HAND_P[None], D=np.full((H, W), IC.WALL, f32), rgb=hand_rgb())
    elif name == "hand_vcol":
        c.update(mesh=hand_mesh(2), poses=HAND_P[None], D=np.full((H, W), IC.WALL, f32), rgb=hand_rgb(), colors=HAND_COLORS)
    else:
        raise KeyError(name)
    return c


CASES = ("batch_47x1", "batch_512") + tuple(f"scene_{s}" for s in GPU_SEEDS) + ("vertex_colors", "ragged", "nan_zero_inf", "plate_in_front",
                                                                                 "uv_wrap", "refused", "grey", "hand_2x2", "hand_3x2", "hand_vcol")


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    m = c["mesh"]
    return [CR.sums(FR.centred(m), m.faces, P, c["K"], c["rgb"], c["D"], TOL, uvs=CR.stored_uvs(m), tex=m.texture, colors=c["colors"]) for P in c["poses"]]


# ---- hand answers ------------------------------------------------------------------------------------------------------------------------
# One right triangle seen head-on at z = 1 m through f = 100 px: legs of 0.12 m = 12 px, corners at the pixels A (94, 69), B (106, 69),
# C (94, 81).  The top and the left edge belong to it, the hypotenuse does not: the pixels (94 + k, 69 + j) with k, j >= 0 and k + j <= 11,
# 78 of them.  The depth is 1 everywhere on it, so every attribute is affine in (k, j): with the corner coordinates below
#   u = 0.04 + 0.86 k / 12,  V = 1 - v = 0.96 - 0.86 j / 12
# and the texel boundaries fall between the sample points (the nearest is u = 0.3267 at k = 4 against 1/3):
#   2 texels wide:  tx = 0 for k <= 6, else 1          3 texels wide:  tx = 0 for k <= 4, 1 for k <= 8, else 2
#   2 texels high:  ty = 1 for j <= 6, else 0
HAND_P = IC.pose(t=(0.0, 0.0, 1.0))
HAND_TEX = {2: np.array([[[10, 20, 30], [40, 50, 60]], [[70, 80, 90], [100, 110, 120]]], np.uint8),
            3: np.array([[[10, 20, 30], [40, 50, 60], [200, 210, 220]], [[70, 80, 90], [100, 110, 120], [130, 140, 150]]], np.uint8)}
# vertex colours of A, B, C: at the corner A the pixel has A's colour; at the midpoint (100, 69) of A B the weights are exactly 1/2, 1/2, 0
# and the channels give 12.5 -> 12 and 13.5 -> 14 (half to even) and 40; at the centroid (98, 73) they are 1/3 each
HAND_COLORS = np.array([[10, 13, 30], [15, 14, 50], [35, 90, 100]], np.uint8)
HAND_VCOL_AT = {(94, 69): (10, 13, 30), (100, 69): (12, 14, 40), (98, 73): (20, 39, 60)}


def hand_mesh(tw):
    h = 0.06
    v = np.array([[-h, -h, 0], [h, -h, 0], [-h, h, 0]], f32)
    n = np.tile(np.array([[0, 0, 1]], f32), (3, 1))
    uv = np.array([[0.04, 0.04], [0.90, 0.04], [0.04, 0.90]], f32)
    return syn.Mesh(f"hand{tw}", v, n, uv, np.array([[0, 1, 2]], np.int32), HAND_TEX[tw]).finalize()


def hand_rgb():
    """the frame of the hand cases: o = (3 c + 5 r + 7 ch) mod 200"""
    r, c, ch = np.mgrid[0:H, 0:W, 0:3]
    return ((3 * c + 5 * r + 7 * ch) % 200).astype(np.uint8)


def hand_pixels():
    return [(94 + k, 69 + j, k, j) for j in range(12) for k in range(12 - j)]


def hand_expected(tw):
    """the record of the textured hand case, in plain integer arithmetic from the table above"""
    m, o = [], []
    for c, r, k, j in hand_pixels():
        tx = (0 if k <= 6 else 1) if tw == 2 else (0 if k <= 4 else 1 if k <= 8 else 2)
        ty = 1 if j <= 6 else 0
        m.append([int(x) for x in HAND_TEX[tw][ty][tx]])
        o.append([(3 * c + 5 * r + 7 * ch) % 200 for ch in range(3)])
    return CR.record(78, 78, 0, m, o)
