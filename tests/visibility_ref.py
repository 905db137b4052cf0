"""Float64 ray-cast of WHICH triangle, if any, a pixel shows, and the rules a rasteriser's (id, depth) image is held to (DESIGN.md
section 2.3).  Written from the rules alone: numpy float64, no expression of oracle/fp_oracle.c, of the kernels or of
tests/frame_render_ref.py.  f32 enters only as data (the mesh as the loader centres it, the pose, K, the crop window `tf`).

Raster coordinates: the crop rasteriser's output pixel (x, y) looks at (x + 1/2, y + 1/2), mapped to the image by the convention of
shade_warp_ref.sample_points; the frame rasteriser's pixel (c, r) looks at the image point (c, r) itself.  A `Grid` carries the map and
the sample coordinates, so one code serves both.  Images are in OUTPUT orientation (row y looks at sample_points' sy[y]): the crop
rasteriser's y-up buffers are turned with `crop_images` first.

Per triangle k:  P_k = the camera-space triangle clipped to z >= znear, projected (3 or 4 corners, none when wholly nearer);
d_k(s) = min of the normalised edge functions of P_k after orienting it (positive inside, in pixels; nothing is culled);
zw_k(s) = the depth of the triangle's plane along the ray of s (clip-space z/w, or camera z);  G_k(s) = |d zw_k / dx| + |d zw_k / dy| per
pixel by central differences at +- 1/2 px.  hit(s): some k has d_k >= 0 with z in range, the nearest such k is the reference's triangle.
An OPEN edge is an edge of some P_k that is not shared by exactly one other triangle which is unclipped, not degenerate and lies on the
other side of it; D(s) is the distance to the nearest open edge.  The rules R1-R4 are in `check`."""
import dataclasses

import numpy as np

import shade_warp_ref as sw

ZNEAR, ZFAR = sw.ZNEAR, sw.ZFAR
SNAP = np.sqrt(2.0) / 32.0          # px: a vertex snapped to 1/16 px moves by at most 1/32 per axis, so no point of an edge moves further
DELTA_CROP = SNAP + 6.0e-4          # + the f32 projection allowance of section 2.1 (ETA)
DELTA_FRAME = SNAP + 2.0e-3         # + the frame path's own f32 allowance (1/1024 px per axis), rounded up
ZTOL = 1.0e-6                       # absolute depth tolerance of R4 (f32 storage of the depth)
D_CAP = 1.0                         # px: D(s) is exact up to here, "further" beyond
MAX_EXTENT = 2047.0                 # px: an unclipped triangle wider than this also goes through the crop rasteriser's clipper


# ---- sample grids -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Grid:
    """raster = a * image + b per axis; output pixel (i, j) samples raster point (xs[i], ys[j]); xs, ys have unit steps (either sign)"""
    xs: np.ndarray
    ys: np.ndarray
    ax: float
    bx: float
    ay: float
    by: float

    @property
    def shape(self):
        return len(self.ys), len(self.xs)


def crop_grid(tf, half_pixel=True, flip=True):
    """the 160 x 160 crop of window tf [9].  half_pixel=False and flip=False are the wrong conventions of the negative controls: samples at
    (x, y) instead of (x + 1/2, y + 1/2); output row y showing what row 159 - y should"""
    sx, sy = sw.sample_points(tf)                           # image coordinates of raster (i + 1/2)
    n = sw.CROP
    ax, ay = (n - 1.0) / (sx[-1] - sx[0]), (n - 1.0) / (sy[-1] - sy[0])
    i = np.arange(n, dtype=np.float64) + (0.5 if half_pixel else 0.0)
    return Grid(i, i if flip else i[::-1].copy(), ax, 0.5 - sx[0] * ax, ay, 0.5 - sy[0] * ay)


def frame_grid(H, W):
    return Grid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), 1.0, 0.0, 1.0, 0.0)


def crop_images(tri, rast):
    """(id [160,160] i64, zw [160,160] f64) in output orientation from debug buffers in y-up raster order"""
    return np.asarray(tri, np.int64)[::-1], np.asarray(rast, np.float64)[::-1, :, 2]


def _index_range(lo, hi, c):
    """first and last index i with lo <= c[i] <= hi (c = c0 +- i), clipped to the grid; first > last when there is none"""
    c0, step = c[0], c[1] - c[0]
    if step > 0:
        i0, i1 = np.ceil(lo - c0), np.floor(hi - c0)
    else:
        i0, i1 = np.ceil(c0 - hi), np.floor(c0 - lo)
    return np.clip(i0, 0, len(c)).astype(np.int64), np.clip(i1, -1, len(c) - 1).astype(np.int64)


def _pairs(lo, hi, grid):
    """every (item, pixel) with the pixel's sample inside the item's box [lo, hi] ([M,2] each) -> (item [T], ix [T], iy [T])"""
    x0, x1 = _index_range(lo[:, 0], hi[:, 0], grid.xs)
    y0, y1 = _index_range(lo[:, 1], hi[:, 1], grid.ys)
    nx, ny = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = nx * ny
    item = np.repeat(np.arange(len(cnt)), cnt)
    local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    w = np.maximum(nx[item], 1)
    return item, x0[item] + local % w, y0[item] + local // w


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def _clip_near(tri, znear):
    """one camera-space triangle [3,3] against z >= znear -> list of 0, 3 or 4 corners, in the triangle's own order"""
    out = []
    for i in range(3):
        a, b = tri[i], tri[(i + 1) % 3]
        if a[2] >= znear:
            out.append(a)
        if (a[2] >= znear) != (b[2] >= znear):
            t = (znear - a[2]) / (b[2] - a[2])
            p = a + t * (b - a)
            p[2] = znear
            out.append(p)
    return out


class Geometry:
    """the polygons P_k of one mesh under one pose on one grid, and what d_k, zw_k and the open edges need"""

    def __init__(self, mesh, pose, K, grid, znear=ZNEAR, zfar=ZFAR, depth="zw", sense=1.0):
        self.grid, self.znear, self.zfar, self.depth, self.sense = grid, float(znear), float(zfar), depth, float(sense)
        K = np.asarray(np.asarray(K, np.float32), np.float64).reshape(3, 3)
        assert K[0, 1] == 0 and K[1, 0] == 0
        self.fx, self.fy, self.cx, self.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        cam = sw.camera_vertices(mesh, pose)
        faces = np.asarray(mesh.faces, np.int64)
        V, F = len(cam), len(faces)
        self.F = F
        valid = ((faces >= 0) & (faces < V)).all(1)                       # a face with an index outside the mesh is dropped
        f = np.where(valid[:, None], faces, 0)
        tri = cam[f]                                                      # [F,3,3]
        # exactly zero area: a repeated index, or corners collinear after centring (the cross product of f32 data is exact enough to be 0)
        centred = (np.asarray(mesh.vertices, np.float32) - np.asarray(mesh.center, np.float32)[None, :]).astype(np.float64)[f]
        self.zero = valid & ((np.cross(centred[:, 1] - centred[:, 0], centred[:, 2] - centred[:, 0]) == 0).all(1)
                             | (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
        inside = tri[:, :, 2] >= self.znear
        self.clipped = valid & ~inside.all(1)
        self.n = np.where(valid & inside.all(1), 3, 0)
        P = np.zeros((F, 4, 3))
        P[:, :3] = tri
        P[:, 3] = tri[:, 2]
        for k in np.nonzero(valid & inside.any(1) & ~inside.all(1))[0]:
            c = _clip_near(tri[k], self.znear)
            self.n[k] = len(c)
            P[k, :len(c)] = c
            P[k, len(c):] = c[-1]
        P[self.n == 0] = [0.0, 0.0, 1.0]
        self.Q = self.project(P)                                          # [F,4,2] raster corners (a 3-corner polygon repeats its last)
        x, y = self.Q[..., 0], self.Q[..., 1]
        xn, yn = np.roll(x, -1, 1), np.roll(y, -1, 1)
        self.area = 0.5 * (x * yn - xn * y).sum(1)
        self.area[self.n == 0] = 0.0
        self.sign = np.sign(self.area)
        ok = (self.n == 3) & ~self.clipped
        if ok.any():
            ext = (self.Q[ok].max(1) - self.Q[ok].min(1)).max()
            assert ext <= MAX_EXTENT, f"an unclipped triangle spans {ext:.0f} px: the crop rasteriser would clip it to the window"
        # the plane of the UNCLIPPED triangle: nrm . p = c0
        self.nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        self.c0 = (self.nrm * tri[:, 0]).sum(1)
        self.faces, self.valid, self.V = f, valid, V
        with np.errstate(divide="ignore", invalid="ignore"):
            self.vert_raster = self.project(np.where((cam[:, 2:3] >= self.znear), cam, np.nan))   # [V,2], nan where it has no projection

    def project(self, p):
        with np.errstate(divide="ignore", invalid="ignore"):
            u = self.fx * p[..., 0] / p[..., 2] + self.cx
            v = self.fy * p[..., 1] / p[..., 2] + self.cy
        return np.stack([self.grid.ax * u + self.grid.bx, self.grid.ay * v + self.grid.by], -1)

    def dist(self, k, sx, sy):
        """d_k(s) for triangles k [T] at raster points (sx, sy) [T]; -inf for a triangle without a polygon; for a polygon of zero area minus
        the distance to the line it lies on"""
        q = self.Q[k]                                                     # [T,4,2]
        qn = np.roll(q, -1, 1)
        ex, ey = qn[..., 0] - q[..., 0], qn[..., 1] - q[..., 1]
        ln = np.hypot(ex, ey)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = (ex * (sy[:, None] - q[..., 1]) - ey * (sx[:, None] - q[..., 0])) / ln     # > 0 on the left of the edge's direction
        s = self.sign[k][:, None]
        d = np.where(ln > 0, np.where(s != 0, s * e, -np.abs(e)), np.inf).min(1)
        return np.where(self.n[k] >= 3, d, -np.inf)

    def z(self, k, sx, sy):
        """camera z where the ray of raster point (sx, sy) meets the plane of triangle k (inf / nan for a ray in the plane)"""
        dx = ((sx - self.grid.bx) / self.grid.ax - self.cx) / self.fx
        dy = ((sy - self.grid.by) / self.grid.ay - self.cy) / self.fy
        n = self.nrm[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.c0[k] / (n[:, 0] * dx + n[:, 1] * dy + n[:, 2])

    def value(self, z):
        """the depth the rasteriser stores for camera z: clip-space z/w of znear 0.1 / zfar 100, or z itself; times `sense` (-1 turns the
        depth order round: the `farthest` control, whose caller negates the image's depth too)"""
        if self.depth == "z":
            return self.sense * z
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sense * ((ZFAR + ZNEAR) / (ZFAR - ZNEAR) - 2.0 * ZFAR * ZNEAR / ((ZFAR - ZNEAR) * z))

    def zw_and_gradient(self, k, sx, sy):
        """(z, zw_k, G_k) at raster points; G may be inf / nan where the triangle is seen edge-on"""
        z = self.z(k, sx, sy)
        gx = self.value(self.z(k, sx + 0.5, sy)) - self.value(self.z(k, sx - 0.5, sy))
        gy = self.value(self.z(k, sx, sy + 0.5)) - self.value(self.z(k, sx, sy - 0.5))
        return z, self.value(z), np.abs(gx) + np.abs(gy)

    def in_range(self, z):
        with np.errstate(invalid="ignore"):
            return (z >= self.znear * (1.0 - 1e-12)) & (z <= self.zfar)

    def covers(self, keep=None):
        """every (triangle, pixel) with d_k >= 0 and z in range -> dict(k, pix, d, zw, G); `keep` [F] bool leaves triangles out"""
        use = (self.n >= 3) & ~self.zero & (self.sign != 0)
        if keep is not None:
            use &= keep
        ks = np.nonzero(use)[0]
        lo = np.where(np.arange(4)[None, :, None] < self.n[ks][:, None, None], self.Q[ks], np.inf).min(1)
        hi = np.where(np.arange(4)[None, :, None] < self.n[ks][:, None, None], self.Q[ks], -np.inf).max(1)
        item, ix, iy = _pairs(lo, hi, self.grid)
        k = ks[item]
        sx, sy = self.grid.xs[ix], self.grid.ys[iy]
        d = self.dist(k, sx, sy)
        m = d >= 0
        k, ix, iy, sx, sy, d = k[m], ix[m], iy[m], sx[m], sy[m], d[m]
        z, zw, G = self.zw_and_gradient(k, sx, sy)
        m = self.in_range(z)
        return dict(k=k[m], pix=(iy * len(self.grid.xs) + ix)[m], d=d[m], zw=zw[m], G=G[m])

    def open_edges(self):
        """[E,2,2] raster segments"""
        good = (self.n == 3) & ~self.clipped & ~self.zero & (self.sign != 0)
        fv = np.nonzero(self.valid)[0]
        a = self.faces[fv][:, [0, 1, 2]].ravel()
        b = self.faces[fv][:, [1, 2, 0]].ravel()
        c = self.faces[fv][:, [2, 0, 1]].ravel()
        face = np.repeat(fv, 3)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        nz = lo != hi                                                     # (the zero-length edge of a repeated index is no edge)
        lo, hi, c, face = lo[nz], hi[nz], c[nz], face[nz]
        qa, qb, qc = self.vert_raster[lo], self.vert_raster[hi], self.vert_raster[c]
        with np.errstate(invalid="ignore"):
            side = np.sign((qb[:, 0] - qa[:, 0]) * (qc[:, 1] - qa[:, 1]) - (qb[:, 1] - qa[:, 1]) * (qc[:, 0] - qa[:, 0]))
        key = lo * self.V + hi
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        n_good = np.bincount(inv, good[face], len(cnt))
        side_sum = np.bincount(inv, np.where(good[face], side, 0.0), len(cnt))
        closed = (cnt == 2) & (n_good == 2) & (side_sum == 0)             # two good triangles, one on each side
        has_poly = (self.n[face] == 3) & ~self.clipped[face]              # (a clipped triangle's edges are added below, as it shows them)
        m = ~closed[inv] & has_poly
        seg = [np.stack([qa[m], qb[m]], 1)]
        for k in np.nonzero(self.clipped & (self.n >= 3))[0]:
            q = self.Q[k, :self.n[k]]
            seg.append(np.stack([q, np.roll(q, -1, 0)], 1))
        seg = np.concatenate(seg)
        return seg[(seg[:, 0] != seg[:, 1]).any(1)]

    def edge_distance(self):
        """D(s) [H,W]: exact where it is <= D_CAP, larger (or inf) elsewhere"""
        H, W = self.grid.shape
        D = np.full(H * W, np.inf)
        seg = self.open_edges()
        if len(seg):
            item, ix, iy = _pairs(seg.min(1) - D_CAP, seg.max(1) + D_CAP, self.grid)
            p, q = seg[item, 0], seg[item, 1]
            s = np.stack([self.grid.xs[ix], self.grid.ys[iy]], 1)
            e = q - p
            t = np.clip(((s - p) * e).sum(1) / (e * e).sum(1), 0.0, 1.0)
            np.minimum.at(D, iy * W + ix, np.hypot(*(s - (p + t[:, None] * e)).T))
        return D.reshape(H, W)


# ---- the reference image and what the rules need --------------------------------------------------------------------------------------
def _pick(c, shape, farthest=False):
    """(id [H,W] i64, zw [H,W]) of the nearest (farthest) cover per pixel; ties take the lower triangle (ties are out of scope)"""
    H, W = shape
    tid, zw = np.zeros(H * W, np.int64), np.zeros(H * W)
    if len(c["k"]):
        order = np.lexsort((c["k"], -c["zw"] if farthest else c["zw"], c["pix"]))
        pix = c["pix"][order]
        first = np.concatenate([[True], pix[1:] != pix[:-1]])
        tid[pix[first]] = c["k"][order][first] + 1
        zw[pix[first]] = c["zw"][order][first]
    return tid.reshape(H, W), zw.reshape(H, W)


@dataclasses.dataclass
class Reference:
    geo: Geometry
    delta: float
    hit: np.ndarray            # [H,W] bool
    tid: np.ndarray            # [H,W] the reference's triangle + 1
    zw: np.ndarray             # [H,W] its depth
    n_certain: np.ndarray      # [H,W] number of k with d_k >= delta and z in range
    zcap: np.ndarray           # [H,W] min over them of zw_k + delta G_k (inf without one)
    zfloor: np.ndarray         # [H,W] max over them of zw_k - delta G_k (-inf without one)
    D: np.ndarray              # [H,W] distance to the nearest open edge


def reference(mesh, pose, K, grid, delta, znear=ZNEAR, zfar=ZFAR, depth="zw", sense=1.0):
    """the Reference of one pose.  znear and sense are what the rules say (0.1, nearest); other values make the WRONG references that a
    rasteriser's own image must fail (negative controls)"""
    geo = Geometry(mesh, pose, K, grid, znear, zfar, depth, sense)
    H, W = grid.shape
    c = geo.covers()
    tid, zw = _pick(c, (H, W))
    m = c["d"] >= delta
    n_certain = np.bincount(c["pix"][m], minlength=H * W)
    zcap, zfloor = np.full(H * W, np.inf), np.full(H * W, -np.inf)
    with np.errstate(invalid="ignore"):
        hi, lo = c["zw"][m] + delta * c["G"][m], c["zw"][m] - delta * c["G"][m]
    np.minimum.at(zcap, c["pix"][m], np.where(np.isfinite(hi), hi, np.inf))
    np.maximum.at(zfloor, c["pix"][m], np.where(np.isfinite(lo), lo, -np.inf))
    return Reference(geo, float(delta), tid > 0, tid, zw, n_certain.reshape(H, W), zcap.reshape(H, W), zfloor.reshape(H, W), geo.edge_distance())


def check(ref, tid, zw):
    """the rules for one image (tid [H,W] triangle + 1 or 0, zw [H,W] its depth, output orientation):
      R1 coverage      D(s) > delta  =>  (id > 0) == hit(s)
      R2 no hole       some k has d_k(s) >= delta with z in range  =>  id > 0            (inside the uncertain band too)
      R3 membership    id > 0  =>  d_id(s) >= -delta, and id is no triangle of exactly zero area
      R4 depth order   id > 0  =>  zw <= min over k with d_k >= delta of (zw_k + delta G_k) + delta G_id + 1e-6
    -> dict: R1..R4 = violating pixels; n = |foreground u hit|, uncertain = those of them with D <= delta, fg, live = foreground pixels
    where R4 can fail (a second certain cover deeper than the tolerance), dmax = the largest D at which coverage differs from hit"""
    g, delta = ref.geo, ref.delta
    tid = np.asarray(tid, np.int64)
    zw = np.asarray(zw, np.float64)
    assert tid.shape == ref.hit.shape == zw.shape
    assert ((tid >= 0) & (tid <= g.F)).all(), "a triangle id outside the mesh"
    fg = tid > 0
    differs = fg != ref.hit
    sure = ref.D > delta
    r1 = sure & differs
    r2 = (ref.n_certain > 0) & ~fg
    iy, ix = np.nonzero(fg)
    k = tid[iy, ix] - 1
    sx, sy = g.grid.xs[ix], g.grid.ys[iy]
    d = g.dist(k, sx, sy)
    r3 = np.zeros_like(fg)
    r3[iy, ix] = ~(d >= -delta) | g.zero[k]
    _, _, G = g.zw_and_gradient(k, sx, sy)
    with np.errstate(invalid="ignore"):
        bound = ref.zcap[iy, ix] + delta * np.where(np.isfinite(G), G, np.inf) + ZTOL
    r4 = np.zeros_like(fg)
    r4[iy, ix] = zw[iy, ix] > bound
    union = fg | ref.hit
    live = fg & (ref.n_certain >= 2) & (ref.zfloor > ref.zcap + ZTOL)
    return dict(R1=int(r1.sum()), R2=int(r2.sum()), R3=int(r3.sum()), R4=int(r4.sum()), n=int(union.sum()), uncertain=int((union & ~sure).sum()),
                fg=int(fg.sum()), live=int(live.sum()), dmax=float(ref.D[differs].max()) if differs.any() else 0.0)


RULES = ("R1", "R2", "R3", "R4")


# ---- the reference's own image under a named rule: for negative controls only ----------------------------------------------------------
def render_by_rule(mesh, pose, K, grid, rule="nearest", depth="zw", zfar=ZFAR, grid_of=None):
    """(id, zw) [H,W] of the reference itself under `rule`: "nearest" (the rule), "farthest", "cull_back", "znear=<metres>",
    "no_half_pixel", "no_flip", "drop_triangle=<t>".  The two sampling rules need `grid_of(half_pixel=, flip=)` to build their grid."""
    znear, keep, farthest = ZNEAR, None, False
    if rule == "farthest":
        farthest = True
    elif rule.startswith("znear="):
        znear = float(rule[6:])
    elif rule == "no_half_pixel":
        grid = grid_of(half_pixel=False)
    elif rule == "no_flip":
        grid = grid_of(flip=False)
    elif rule not in ("nearest", "cull_back") and not rule.startswith("drop_triangle="):
        raise KeyError(rule)
    geo = Geometry(mesh, pose, K, grid, znear, zfar, depth)
    if rule == "cull_back":
        keep = geo.c0 < 0                                                 # the plane's normal points at the camera: nrm . p0 < 0
    elif rule.startswith("drop_triangle="):
        keep = np.arange(geo.F) != int(rule[14:])
    return _pick(geo.covers(keep), grid.shape, farthest)
