"""Float64 references of texture shading and of the crop warp, written from the rules in DESIGN.md (sections 2.1, 4.1) and the header of
fp_geometry.hip -- NOT from oracle/fp_oracle.c or the kernels, whose expressions (mad<> / dot3<>, MAD / DOT3) come from one hand.

Everything is numpy float64; the only f32 values are the ones the rules name as data: the mesh as the loader leaves it (vertices centred
in f32), the pose, K, the crop window `tf`, the rasteriser's own output, and the warp's inverse coefficients ("inverse in double, cast
to f32").

    texture_ref   the texture unit: u8 / 255, wrap = frac(u), texel centre at u * TW - 0.5, bilinear with neighbours modulo the size
    shade_ref     the shader, GIVEN the rasteriser's output (b0, b1, z/w, id): interpolation, Lambert term, colour, xyz, cuts, flip
    bary_ref      the geometry behind that output: ray through the crop pixel's sample point against the triangle's plane
    warp_ref      the crop warp: bilinear u8 with a zero border and round-half-even, nearest xyz tap, back-projection, cuts

The pieces warp_ref is made of (warp_source, bilinear_taps, nearest_xyz) are public so that a test can state a tie window or build a
deliberately wrong warp out of them."""
import numpy as np

CROP = 160
ZNEAR, ZFAR = 0.1, 100.0
MIN_DEPTH, MAX_XYZ = 0.001, 4.0


def _f64(a):
    return np.asarray(a, np.float64)


# ---- the texture unit ---------------------------------------------------------------------------------------------------------------
def texture_ref(tex_u8, u, v):
    """[..., 3] float64: tex_u8 [TH, TW, 3] sampled at (u, v), row 0 at v = 0"""
    tex = np.asarray(tex_u8)
    assert tex.dtype == np.uint8 and tex.ndim == 3
    th, tw = tex.shape[:2]
    t = tex.astype(np.float64) / 255.0
    u, v = np.broadcast_arrays(_f64(u), _f64(v))
    x = (u - np.floor(u)) * tw - 0.5
    y = (v - np.floor(v)) * th - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    ix0, iy0 = x0.astype(np.int64) % tw, y0.astype(np.int64) % th
    ix1, iy1 = (ix0 + 1) % tw, (iy0 + 1) % th
    top = t[iy0, ix0] * (1 - ax) + t[iy0, ix1] * ax
    bot = t[iy1, ix0] * (1 - ax) + t[iy1, ix1] * ax
    return top * (1 - ay) + bot * ay


# ---- the mesh as the renderer holds it ----------------------------------------------------------------------------------------------
def _pose(pose):
    p = _f64(np.asarray(pose, np.float32))
    return p[:3, :3], p[:3, 3]


def camera_vertices(mesh, pose):
    """[V, 3] float64 camera-space vertices: centred in f32 exactly as the loader does, then widened"""
    R, t = _pose(pose)
    v = (np.asarray(mesh.vertices, np.float32) - np.asarray(mesh.center, np.float32)[None, :]).astype(np.float64)
    return v @ R.T + t


def vertex_uv(mesh):
    """[V, 2] float64 (u, 1 - v)"""
    uv = _f64(np.asarray(mesh.texcoords, np.float32)[:, :2])
    return np.stack([uv[:, 0], 1.0 - uv[:, 1]], 1)


def vertex_diffuse(mesh, pose):
    """[V] float64 clamp(-n_cam.z / |n_cam|, 0, 1), 0 for a zero normal"""
    R, _ = _pose(pose)
    n = _f64(np.asarray(mesh.normals, np.float32)) @ R.T
    ln = np.linalg.norm(n, axis=1)
    return np.clip(np.where(ln == 0, 0.0, -n[:, 2] / np.where(ln == 0, 1.0, ln)), 0.0, 1.0)


def radius_of(mesh):
    return float(np.float32(mesh.diameter)) / 2.0


# ---- the shader ---------------------------------------------------------------------------------------------------------------------
def shade_ref(mesh, pose, rast, sample=texture_ref, details=False):
    """[160, 160, 6] float64 render tensor (rgb, xyz) of one pose from the rasteriser's own output `rast` [160, 160, 4] = (b0, b1, z/w, id) in
    y-up raster order.  `sample(texture, u, v)` is the texture unit.  details=True also returns what a bound needs: the foreground mask,
    the interpolated uv, the camera-space point and the xyz before the cuts, all in the output's (flipped) orientation."""
    R, t = _pose(pose)
    r = _f64(rast)[::-1]                                     # y-up -> the vertical flip of the output
    tid = r[..., 3].astype(np.int64)
    fg = tid > 0
    f = np.asarray(mesh.faces, np.int64)[np.where(fg, tid - 1, 0)]
    b0, b1 = r[..., 0], r[..., 1]
    b2 = 1.0 - b0 - b1

    def interp(a):
        return b0[..., None] * a[f[..., 0]] + b1[..., None] * a[f[..., 1]] + b2[..., None] * a[f[..., 2]]

    p = interp(camera_vertices(mesh, pose))
    uv = interp(vertex_uv(mesh))
    dif = interp(vertex_diffuse(mesh, pose)[:, None])[..., 0]
    col = np.clip(sample(mesh.texture, uv[..., 0], uv[..., 1]) * (0.8 + 0.5 * dif)[..., None], 0.0, 1.0)
    q = (p - t) / radius_of(mesh)
    cut = (p[..., 2:3] < MIN_DEPTH) | (np.abs(q) > MAX_XYZ)
    out = np.where(fg[..., None], np.concatenate([col, np.where(cut, 0.0, q)], -1), 0.0)
    if details:
        return out, dict(fg=fg, uv=uv, p=p, q=q)
    return out


# ---- the geometry behind the rasteriser's output --------------------------------------------------------------------------------------
def sample_points(tf, offset=(0.5, 0.5)):
    """image coordinates (sx [160] by crop column, sy [160] by OUTPUT row) the crop pixels look at: b0 + (x + 0.5) (b2 - b0) / 160 with
    (b0, b2) = tf^-1 (0, 159), the convention the analytic ellipsoid test established"""
    inv = np.linalg.inv(_f64(tf).reshape(3, 3))
    lo = inv @ np.array([0.0, 0.0, 1.0])
    hi = inv @ np.array([CROP - 1.0, CROP - 1.0, 1.0])
    i = np.arange(CROP, dtype=np.float64)
    return (lo[0] + (i + offset[0]) * (hi[0] - lo[0]) / CROP, lo[1] + (i + offset[1]) * (hi[1] - lo[1]) / CROP)


def bary_ref(mesh, pose, K, tf, tri_id, offset=(0.5, 0.5)):
    """[160, 160, 3] float64 (b0, b1, z/w) in the y-up raster order of tri_id [160, 160] (triangle + 1, 0 = background): the ray through each
    pixel's sample point meets the plane of its triangle in camera space.  Barycentrics are NOT clamped (a caller can see where the
    rasteriser's rule clamps); z/w is the clip-space depth for znear 0.1 / zfar 100, clamped to [-1, 1].  Background is nan."""
    K = _f64(np.asarray(K, np.float32))
    sx, sy = sample_points(tf, offset)
    sy = sy[::-1]                                            # output row 159 - py is raster row py
    d = np.stack(np.broadcast_arrays((sx[None, :] - K[0, 2]) / K[0, 0], (sy[:, None] - K[1, 2]) / K[1, 1], 1.0), -1)
    tid = np.asarray(tri_id, np.int64)
    fg = tid > 0
    f = np.asarray(mesh.faces, np.int64)[np.where(fg, tid - 1, 0)]
    pc = camera_vertices(mesh, pose)
    p0, p1, p2 = pc[f[..., 0]], pc[f[..., 1]], pc[f[..., 2]]
    # s d = b0 p0 + b1 p1 + b2 p2 with b0 + b1 + b2 = 1: Cramer's rule on [p0 p1 p2] w = d, then b = w / sum(w) and s = 1 / sum(w)
    w0 = (d * np.cross(p1, p2)).sum(-1)
    w1 = (d * np.cross(p2, p0)).sum(-1)
    w2 = (d * np.cross(p0, p1)).sum(-1)
    det = (p0 * np.cross(p1, p2)).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ws = w0 + w1 + w2
        z = det / ws                                         # the point is s d and d.z = 1
        zw = (ZFAR + ZNEAR) / (ZFAR - ZNEAR) - 2.0 * ZFAR * ZNEAR / ((ZFAR - ZNEAR) * z)
        out = np.stack([w0 / ws, w1 / ws, np.clip(zw, -1.0, 1.0)], -1)
    return np.where(fg[..., None], out, np.nan)


# ---- the crop warp ------------------------------------------------------------------------------------------------------------------
def warp_source(tf):
    """source coordinates (sx [160], sy [160]) of the crop's columns / rows: tf is a scale and a shift, its inverse is taken in double,
    the coefficients are cast to f32, m0 x + m2 and m4 y + m5 are evaluated in float64"""
    tf = _f64(np.asarray(tf, np.float32)).reshape(3, 3)
    assert tf[0, 1] == 0 and tf[1, 0] == 0 and tf[2, 0] == 0 and tf[2, 1] == 0 and tf[2, 2] == 1
    m0, m2, m4, m5 = _f64(np.array([1.0 / tf[0, 0], -tf[0, 2] / tf[0, 0], 1.0 / tf[1, 1], -tf[1, 2] / tf[1, 1]]).astype(np.float32))
    i = np.arange(CROP, dtype=np.float64)
    return m0 * i + m2, m4 * i + m5


def bilinear_taps(img_u8, sx, sy):
    """the four taps (p00, p10, p01, p11: [160, 160, C] float64, zero outside the frame; first index = x offset) around (sx, sy) and the
    weights ax [1, 160, 1], ay [160, 1, 1]"""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8
    H, W = img.shape[:2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)

    def tap(yi, xi):
        ok = ((yi >= 0) & (yi < H))[:, None] & ((xi >= 0) & (xi < W))[None, :]
        val = img[np.clip(yi, 0, H - 1)[:, None], np.clip(xi, 0, W - 1)[None, :]].astype(np.float64)
        return np.where(ok[..., None], val, 0.0)

    return (tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)), (sx - x0)[None, :, None], (sy - y0)[:, None, None]


def bilinear_value(taps, ax, ay):
    p00, p10, p01, p11 = taps
    return (p00 * (1 - ax) + p10 * ax) * (1 - ay) + (p01 * (1 - ax) + p11 * ax) * ay


def tap_spread(taps):
    """sum of the |differences| along the four edges of the tap square: what a unit shift of the sample position can move the value by"""
    p00, p10, p01, p11 = taps
    return np.abs(p10 - p00) + np.abs(p11 - p01) + np.abs(p01 - p00) + np.abs(p11 - p10)


def nearest_xyz(depth, K, pose, diameter, cx, cy, details=False):
    """[160, 160, 3] float64 normalised xyz from the depth tap at column cx [160], row cy [160] (integers; zero border, depth < 0.001 invalid):
    back-projected with K, minus t, over the radius, zeroed per component beyond 4.0 and as a whole where invalid"""
    depth = np.asarray(depth, np.float32)
    K = _f64(np.asarray(K, np.float32))
    _, t = _pose(pose)
    H, W = depth.shape
    ok = ((cy >= 0) & (cy < H))[:, None] & ((cx >= 0) & (cx < W))[None, :]
    d = np.where(ok, _f64(depth[np.clip(cy, 0, H - 1)[:, None], np.clip(cx, 0, W - 1)[None, :]]), 0.0)
    valid = ok & ~(d < MIN_DEPTH)
    p = np.stack([(cx[None, :] - K[0, 2]) * d / K[0, 0], (cy[:, None] - K[1, 2]) * d / K[1, 1], d], -1)
    q = (p - t) / (float(np.float32(diameter)) / 2.0)
    out = np.where(valid[..., None] & ~(np.abs(q) > MAX_XYZ), q, 0.0)
    if details:
        return out, dict(valid=valid, p=p, q=q)
    return out


def warp_ref(rgb, depth, K, pose, tf, diameter):
    """[160, 160, 6] float64 observed crop (rgb, xyz) of one pose's window tf [9] f32"""
    sx, sy = warp_source(tf)
    taps, ax, ay = bilinear_taps(rgb, sx, sy)
    col = np.clip(np.rint(bilinear_value(taps, ax, ay)), 0.0, 255.0) / 255.0          # np.rint rounds half to even
    xyz = nearest_xyz(depth, K, pose, diameter, np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64))
    return np.concatenate([col, xyz], -1)
