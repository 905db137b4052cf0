"""numpy restatement of DESIGN.md section 4.8 (fp_render_pose): float32 operations in the stated order, int64 coverage.

Shared by tests/test_frame_render_ref_cpu.py (which holds it to an analytic ray-cast and to hand-derived cases) and
tests/test_frame_render_gpu.py (which holds the kernels to it, bit for bit).  One Python loop over triangles; everything inside a
triangle's bounding box is vectorised."""
import numpy as np

f32 = np.float32
NEAR = f32(0.01)            # FP_RENDER_NEAR_M
SNAP_MAX = f32(2 ** 26)     # FP_RENDER_SNAP_MAX
MIN_DEPTH = f32(0.001)      # validity threshold of an observed depth
TINT = (40, 220, 120)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
OUTPUTS = ("model_depth", "model_mask", "visible_mask", "tri_id", "overlay")


class Refused(Exception):
    """the pose needs a clipper (near) or leaves the exact integer range (range)"""


def centred(mesh):
    """the vertices the library renders: mesh frame minus the mesh centre, one f32 subtraction"""
    return mesh.vertices.astype(f32) - np.asarray(mesh.center, f32)


def stored_faces(verts, faces):
    """the faces the library renders: a face whose CENTRED corners are exactly collinear is stored as (i0, i0, i0), because three collinear
    points may snap to a sliver that covers a sample, while a repeated index snaps to one point under every pose"""
    f = np.array(faces, np.int64).reshape(-1, 3)
    v = np.asarray(verts, f32).astype(np.float64)
    ok = np.nonzero(((f >= 0) & (f < len(v))).all(1))[0]
    a, b = v[f[ok, 1]] - v[f[ok, 0]], v[f[ok, 2]] - v[f[ok, 0]]
    flat = (a[:, 1] * b[:, 2] == a[:, 2] * b[:, 1]) & (a[:, 2] * b[:, 0] == a[:, 0] * b[:, 2]) & (a[:, 0] * b[:, 1] == a[:, 1] * b[:, 0])
    f[ok[flat]] = f[ok[flat], :1]
    return f


def project(verts, pose, K):
    """-> (cam [V,3] f32, snapped [V,2] i64, near [V] bool, out_of_range [V] bool).  pose: numpy 4x4 (row-major as numpy prints it)."""
    v = np.asarray(verts, f32)
    P = np.asarray(pose, f32)
    K = np.asarray(K, f32).reshape(3, 3)
    cam = np.empty_like(v)
    for r in range(3):
        cam[:, r] = ((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) + P[r, 3]
    x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
    near = ~(z >= NEAR)
    with np.errstate(all="ignore"):
        us = (K[0, 0] * (x / z) + K[0, 2]) * f32(16)
        ws = (K[1, 1] * (y / z) + K[1, 2]) * f32(16)
        far = ~near & (~(np.abs(us) <= SNAP_MAX) | ~(np.abs(ws) <= SNAP_MAX))
    ok = ~near & ~far
    snap = np.zeros((len(v), 2), np.int64)
    snap[ok, 0] = np.rint(us[ok]).astype(np.int64)
    snap[ok, 1] = np.rint(ws[ok]).astype(np.int64)
    return cam, snap, near, far


def refused(verts, pose, K):
    """None, or why fp_render_pose must refuse the pose ("near" before "range", like the library's messages)"""
    _, _, near, far = project(verts, pose, K)
    return "near" if near.any() else "range" if far.any() else None


def _bias(dx, dy):
    """top-left rule: smallest edge-function value that counts as covered, for an edge of direction (dx, dy) of a positive-area triangle"""
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1


def rasterize(cam, snap, faces, H, W):
    """-> z-buffer keys [H,W] u64: bits(z) << 32 | triangle, EMPTY where no triangle covers the sample point (16 c, 16 r)"""
    keys = np.full((H, W), EMPTY, np.uint64)
    V = len(cam)
    for t, (i0, i1, i2) in enumerate(np.asarray(faces, np.int64)):
        if not (0 <= i0 < V and 0 <= i1 < V and 0 <= i2 < V):
            continue
        (ax, ay), (bx, by), (cx, cy) = (int(snap[i0, 0]), int(snap[i0, 1])), (int(snap[i1, 0]), int(snap[i1, 1])), (int(snap[i2, 0]), int(snap[i2, 1]))
        px0, px1 = max(-(-min(ax, bx, cx) // 16), 0), min(max(ax, bx, cx) // 16, W - 1)
        py0, py1 = max(-(-min(ay, by, cy) // 16), 0), min(max(ay, by, cy) // 16, H - 1)
        if px0 > px1 or py0 > py1:
            continue
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0:
            continue
        s = -1 if area < 0 else 1
        A = s * area
        sx = 16 * np.arange(px0, px1 + 1, dtype=np.int64)[None, :]
        sy = 16 * np.arange(py0, py1 + 1, dtype=np.int64)[:, None]
        es = []
        inside = True
        for (qx, qy), (rx, ry) in (((bx, by), (cx, cy)), ((cx, cy), (ax, ay)), ((ax, ay), (bx, by))):   # edge i is opposite corner i
            dx, dy = s * (rx - qx), s * (ry - qy)
            e = dx * (sy - qy) - dy * (sx - qx)
            inside = inside & (e >= _bias(dx, dy))
            es.append(e)
        if not inside.any():
            continue
        fA = f32(A)
        w = [e.astype(f32) / fA for e in es]
        z0, z1, z2 = cam[i0, 2], cam[i1, 2], cam[i2, 2]
        with np.errstate(all="ignore"):
            z = f32(1) / ((w[0] / z0 + w[1] / z1) + w[2] / z2)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        win = keys[py0:py1 + 1, px0:px1 + 1]
        np.minimum(win, np.where(inside, key, EMPTY), out=win)
    return keys


def shade(cam, faces, tri):
    """integer shade k in [64, 255] of triangles `tri` (an index array): flat, two-sided Lambert term of the camera-space normal"""
    f = np.asarray(faces, np.int64)[tri]
    p0, p1, p2 = cam[f[:, 0]], cam[f[:, 1]], cam[f[:, 2]]
    a, b = p1 - p0, p2 - p0
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    len2 = (nx * nx + ny * ny) + nz * nz
    with np.errstate(all="ignore"):
        lam = np.where(len2 > 0, np.abs(nz) / np.sqrt(len2), f32(0)).astype(f32)
    return 64 + np.rint(lam * f32(191)).astype(np.int64)


def render(verts, faces, pose, K, rgb, depth, tol_m=0.005):
    """fp_render_pose on the frame (rgb [H,W,3] u8, depth [H,W] f32): dict of the five outputs; raises Refused like the library errors.
    verts: CENTRED vertices (centred(mesh))."""
    cam, snap, near, far = project(verts, pose, K)
    if near.any():
        raise Refused("near")
    if far.any():
        raise Refused("range")
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    faces = stored_faces(verts, faces)
    keys = rasterize(cam, snap, faces, H, W)
    model = keys != EMPTY
    z = np.where(model, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    tri = np.where(model, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    with np.errstate(invalid="ignore"):
        occluded = model & ~(depth < MIN_DEPTH) & (depth < z - f32(tol_m))
    visible = model & ~occluded
    overlay = np.asarray(rgb, np.uint8).copy()
    if visible.any():
        k = shade(cam, faces, tri[visible])
        src = overlay[visible].astype(np.int64)
        tint = (np.asarray(TINT, np.int64)[None, :] * k[:, None] + 127) // 255
        overlay[visible] = ((src + tint + 1) >> 1).astype(np.uint8)
    return dict(model_depth=z, model_mask=np.where(model, 255, 0).astype(np.uint8), visible_mask=np.where(visible, 255, 0).astype(np.uint8),
                tri_id=(tri + 1).astype(np.int32), overlay=overlay)
