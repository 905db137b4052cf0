"""The scenes tests/test_vsd_gpu.py hands to fp_pose_vsd, built without a GPU so that tests/test_vsd_ref_cpu.py can hold each to what it
is for before a kernel sees it.  An 88 x 72 frame (3 x 3 tiles of 32 px, ragged on both edges) with f = 44 px, the 12-triangle box and
the 320-face icosphere (a 256-thread stride loops twice).  Scene depths keep the comparisons of the metric far from their thresholds:
the observed depth is the truth's own rendering, a plate 8 cm in front of it, a wall at 2 m, or missing; estimates differ from the
truth by nothing, by 0.3 diameters in depth (thresholds 0.2 / 0.4), or sideways (one huge threshold).  References are computed once
and shared; callers must not modify them."""
import functools

import numpy as np

import frame_render_ref as FR
import vsd_ref as VR
from foundationpose_cpp_amd import synthetic as syn

W, H = 88, 72
K = syn.intrinsics(W, H)                  # fx = fy = 44, cx = 44, cy = 36
WALL = np.float32(2.0)
BOP19_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))


@functools.lru_cache(maxsize=None)
def box():
    h = np.array([0.10, 0.075, 0.05])
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int32)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    return syn.Mesh("box", v.astype(np.float32), n.astype(np.float32), np.zeros((8, 2), np.float32), faces, np.full((2, 2, 3), 100, np.uint8)).finalize()


@functools.lru_cache(maxsize=None)
def ico():
    return syn.make_mesh(2, textured=False, name="ico")      # 162 vertices, 320 faces


def mesh_of(name):
    return {"box": box, "ico": ico}[name]()


def pose(R=np.eye(3), t=(0, 0, 0)):
    return syn.pose_matrix(np.asarray(R, np.float64), t)


def moved(P, dt):
    Q = np.array(P, np.float32)
    Q[:3, 3] += np.asarray(dt, np.float32)
    return Q


def rendering(mesh, P, background=WALL):
    """the depth a sensor would see of the mesh under P in front of a wall: the f32 rendering itself"""
    z = VR.model_depth(FR.centred(mesh), mesh.faces, np.asarray(P, np.float32), K, H, W)
    return np.where(z != 0, z, np.float32(background)).astype(np.float32)


BOX_G = pose(t=(0.0, 0.0, 0.23))                 # face-on, front face at 0.18 m: 49 x 37 px
BOX_SHIFT = np.float32(0.3) * np.float32(box().diameter)


def _case(mesh, est, gt, D, delta=0.015, taus=BOP19_TAUS, normalized=True):
    return dict(mesh=mesh, est=np.asarray(est, np.float32).reshape(-1, 4, 4), gt=np.asarray(gt, np.float32).reshape(-1, 4, 4),
                D=np.ascontiguousarray(D, np.float32), delta=delta, taus=tuple(taus), normalized=normalized)


@functools.lru_cache(maxsize=None)
def case(name):
    zeros = np.zeros((H, W), np.float32)
    if name == "box_same":                       # est == gt on the truth's own rendering
        return _case("box", [BOX_G], [BOX_G], rendering(box(), BOX_G))
    if name == "box_same_nan":                   # ... with one pixel of the object's depth a NaN
        D = rendering(box(), BOX_G)
        D[36, 40] = np.nan
        return _case("box", [BOX_G], [BOX_G], D)
    if name == "box_same_missing":               # ... with no depth at all
        return _case("box", [BOX_G], [BOX_G], zeros)
    if name == "box_tau0":                       # a threshold of 0 equals every distance difference of est == gt: >= fails them all
        return _case("box", [BOX_G], [BOX_G], rendering(box(), BOX_G), taus=(0.0, 0.05))
    if name == "box_zshift":                     # 0.3 diameters deeper: between the thresholds 0.2 and 0.4
        return _case("box", [moved(BOX_G, (0, 0, BOX_SHIFT))], [BOX_G], zeros, taus=(0.2, 0.4))
    if name == "box_scaled":                     # every point 1.5 times as far along its own ray: the same silhouette, 0.3 diameters deeper
        G = pose(t=(0.0, 0.0, BOX_SHIFT * 2 + np.float32(0.05)))
        E = np.array(G, np.float32)
        E[:3] *= np.float32(1.5)
        return _case("box", [E], [G], zeros, taus=(0.2, 0.4))
    if name == "box_lateral":                    # half the object sideways, one huge threshold in metres: only the masks count
        return _case("box", [moved(BOX_G, (0.1, 0, 0))], [BOX_G], zeros, taus=(10.0,), normalized=False)
    if name == "box_est_outside":
        return _case("box", [moved(BOX_G, (2.0, 0, 0))], [BOX_G], rendering(box(), BOX_G))
    if name == "box_both_outside":
        return _case("box", [moved(BOX_G, (2.0, 0, 0))], [moved(BOX_G, (0, -3.0, 0))], np.full((H, W), WALL, np.float32))
    if name == "box_half_outside":               # the truth's centre on the frame's right edge, the estimate 5 mm off
        G = moved(BOX_G, (0.22, 0.0, 0.0))
        return _case("box", [moved(G, (0.005, 0.003, 0.0))], [G], rendering(box(), G))
    if name == "box_plate":                      # a plate 8 cm in front of the left half of the object
        D = rendering(box(), BOX_G)
        D[:, :44] = np.float32(0.10)
        return _case("box", [BOX_G], [BOX_G], D)
    if name == "box_corner":                     # near the frame's corner, where a distance is 1.1 .. 1.6 times z: the threshold lies between
        G = pose(t=(0.32, 0.27, 0.5))            # the z difference (0.3 diameters) and the smallest distance difference
        return _case("box", [moved(G, (0, 0, BOX_SHIFT))], [G], rendering(box(), G), taus=(0.315,))
    if name == "ico_behind":                     # the estimate 0.3 diameters behind the observed truth and turned by 5 degrees: hidden by the
        m = ico()                                # rule, visible by BOP's clause wherever the truth is
        G = pose(syn.random_rotation(4), (0.01, -0.005, 0.25))
        E = moved(syn.perturb_pose(G, deg=5.0, trans=0.0, seed=2), (0, 0, np.float32(0.3) * np.float32(m.diameter)))
        D = rendering(m, G)
        D[30, 46] = np.nan
        return _case("ico", [E], [G], D, taus=(0.2, 0.4))
    if name == "ico_batch":                      # three estimates against one truth, BOP19's thresholds
        m = ico()
        G = pose(syn.random_rotation(6), (-0.02, 0.01, 0.22))
        est = [syn.perturb_pose(G, deg=4.0 + 3 * i, trans=0.004 * (i + 1), seed=10 + i) for i in range(3)]
        return _case("ico", est, [G], rendering(m, G))
    raise KeyError(name)


CASES = ("box_same", "box_same_nan", "box_same_missing", "box_tau0", "box_zshift", "box_scaled", "box_lateral", "box_est_outside",
         "box_both_outside", "box_half_outside", "box_plate", "box_corner", "ico_behind", "ico_batch")
# the cases whose comparisons stay out of reach of their thresholds, which is what the float64 intervals ask for.  Not box_tau0, whose
# threshold sits ON every distance difference on purpose, and not ico_batch, whose ten thresholds lie inside the range of its distance
# differences: there a vertex snapped by 1/32 px moves a sloped surface's depth by 1e-4 m, more than the comparison band.
F64_CASES = tuple(c for c in CASES if c not in ("box_tau0", "ico_batch"))


@functools.lru_cache(maxsize=None)
def expected(name, wrong=None):
    """the records fp_pose_vsd must return for the case"""
    c = case(name)
    return VR.vsd(mesh_of(c["mesh"]), c["est"], c["gt"], c["D"], K, c["delta"], c["taus"], c["normalized"], wrong)


def batch_poses(n, seed=0):
    """n estimates around ico_batch's truth, some of them partly outside the frame"""
    G = case("ico_batch")["gt"][0]
    rng = np.random.default_rng(seed)
    return np.stack([moved(syn.perturb_pose(G, deg=float(rng.uniform(0, 25)), trans=float(rng.uniform(0, 0.02)), seed=100 + i),
                           (float(rng.uniform(-0.15, 0.15)) if i % 5 == 0 else 0.0, 0.0, 0.0)) for i in range(n)])
