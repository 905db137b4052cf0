"""References of fp_pose_color and fp_resolve_symmetry, shared by tests/test_color_ref_cpu.py and the GPU tests.

(a) `sums` restates the section's per-pixel rules in numpy float32, operation by operation, on top of frame_render_ref's rasteriser (the
restatement of fp_render_pose the kernels are held to bit for bit): the four counts and the 15 integer sums the device record must EQUAL,
then the status and the zncc the host derives from them.

(b) `color64` is the float64 reference and shares no expression with (a): it ray-casts the mesh from the unsnapped float64 vertices (the
ray-cast of icp_ref), takes the barycentric coordinates of the hit point in the 3-D triangle from cross products, forms the texture
coordinate with vector algebra and takes floor of the wrapped coordinate.

`compare` holds (a)'s maps to (b)'s: the share of pixels that differ in coverage or in the winning triangle, and, over the others that
both compare, the share that picks another texel."""
import numpy as np

import frame_render_ref as FR
import icp_ref as IR

f32 = np.float32
MIN_PIXELS = 32
REFUSED_NEAR, REFUSED_RANGE, TOO_FEW, FLAT = 1, 2, 4, 8
COUNTS = ("n_model", "n_visible", "n_compared", "n_nocolor")
SUMS = ("sum_m", "sum_o", "sum_mm", "sum_oo", "sum_mo")
WRONG = ("v_not_flipped", "uv_swapped", "affine", "half_pixel", "clamp", "bgr")


def stored_uvs(mesh):
    """the texture coordinates the library keeps: (u, 1 - v), one f32 subtraction"""
    uv = np.asarray(mesh.texcoords, f32)
    return np.stack([uv[:, 0], f32(1) - uv[:, 1]], 1)


def packed_colors(colors):
    """[V,3] u8 -> what the corner bytes are as float"""
    return np.asarray(colors, np.uint8).astype(f32)


def zncc_of(n, sum_m, sum_o, sum_mm, sum_oo, sum_mo):
    """-> (status bits, zncc as the double the host rounds once): the host's formula on the record's integers"""
    if n < MIN_PIXELS:
        return TOO_FEW, 0.0
    n = float(n)
    cov = var_m = var_o = 0.0
    for ch in range(3):
        sm, so = float(sum_m[ch]), float(sum_o[ch])
        cov += float(sum_mo[ch]) - sm * so / n
        var_m += float(sum_mm[ch]) - sm * sm / n
        var_o += float(sum_oo[ch]) - so * so / n
    if not var_m > 0.0 or not var_o > 0.0:
        return FLAT, 0.0
    return 0, cov / np.sqrt(var_m * var_o)


def record(n_model, n_visible, n_nocolor, m, o):
    """the record of compared model values m [n,3] and observed values o [n,3] (integers)"""
    m, o = np.asarray(m, np.int64).reshape(-1, 3), np.asarray(o, np.int64).reshape(-1, 3)
    r = dict(n_model=int(n_model), n_visible=int(n_visible), n_compared=len(m), n_nocolor=int(n_nocolor),
             sum_m=[int(x) for x in m.sum(0)], sum_o=[int(x) for x in o.sum(0)], sum_mm=[int(x) for x in (m * m).sum(0)],
             sum_oo=[int(x) for x in (o * o).sum(0)], sum_mo=[int(x) for x in (m * o).sum(0)])
    r["status"], z = zncc_of(r["n_compared"], *(r[k] for k in SUMS))
    r["zncc64"], r["zncc"] = float(z), f32(z)
    return r


def refused_record(bits):
    r = record(0, 0, 0, np.zeros((0, 3)), np.zeros((0, 3)))
    r["status"] = bits
    return r


# ---- (a) the f32 restatement ------------------------------------------------------------------------------------------------------------
def sums(verts, faces, pose, K, rgb, D, tol_m, uvs=None, tex=None, colors=None, wrong=None, maps=False):
    """verts: CENTRED vertices; uvs: the STORED coordinates (stored_uvs) with tex [TH,TW,3] u8, or colors [V,3] u8 (the vertex-colour
    source, which wins like the library's); pose 4x4 (numpy, row-major); rgb [H,W,3] u8; D [H,W] f32 raw depth -> the record (a dict).
    wrong: a rule broken on purpose (negative controls, WRONG).  maps: also model / tri / texel [H,W] (texel: ty * TW + tx, -1 where the
    pixel is not compared)."""
    P = np.asarray(pose, f32)
    K = np.asarray(K, f32).reshape(3, 3)
    D = np.asarray(D, f32)
    rgb = np.asarray(rgb, np.uint8)
    H, W = D.shape
    cam, snap, near, far = FR.project(verts, P, K)
    if near.any() or far.any():
        return refused_record((REFUSED_NEAR if near.any() else 0) | (REFUSED_RANGE if far.any() else 0))
    fs = FR.stored_faces(verts, faces)
    keys = FR.rasterize(cam, snap, fs, H, W)
    model = keys != FR.EMPTY
    z_all = np.where(model, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    with np.errstate(invalid="ignore"):
        visible = model & ~(~(D < FR.MIN_DEPTH) & (D < z_all - f32(tol_m)))
    rr, cc = np.nonzero(visible)
    z = z_all[visible]
    tri = (keys[visible] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    f = fs[tri]
    a, b, c = snap[f[:, 0]], snap[f[:, 1]], snap[f[:, 2]]                                # [n,2] i64
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    s = np.where(area < 0, -1, 1).astype(np.int64)
    A = s * area
    sx, sy = 16 * cc.astype(np.int64), 16 * rr.astype(np.int64)
    if wrong == "half_pixel":
        sx, sy = sx + 8, sy + 8
    es = []
    for q, r in ((b, c), (c, a), (a, b)):                                                # edge i is opposite corner i
        dx, dy = s * (r[:, 0] - q[:, 0]), s * (r[:, 1] - q[:, 1])
        es.append(dx * (sy - q[:, 1]) - dy * (sx - q[:, 0]))
    fA = A.astype(f32)
    with np.errstate(all="ignore"):
        w = [e.astype(f32) / fA for e in es]
        zk = [cam[f[:, k], 2] for k in range(3)]
        g = w if wrong == "affine" else [(w[k] / zk[k]) * z for k in range(3)]
        assert all(x.dtype == f32 for x in g)
        if colors is not None:
            col = packed_colors(colors)
            v = np.stack([(g[0] * col[f[:, 0], ch] + g[1] * col[f[:, 1], ch]) + g[2] * col[f[:, 2], ch] for ch in range(3)], 1)
            has = ~np.isnan(v).any(1)
            m = np.rint(np.minimum(np.maximum(np.where(np.isnan(v), f32(0), v), f32(0)), f32(255))).astype(np.int64)
            texel = np.where(has, 0, -1)
        else:
            uv = np.asarray(uvs, f32)
            if wrong == "v_not_flipped":
                uv = np.stack([uv[:, 0], f32(1) - uv[:, 1]], 1)
            if wrong == "uv_swapped":
                uv = uv[:, ::-1]
            TH, TW = tex.shape[:2]
            U = (g[0] * uv[f[:, 0], 0] + g[1] * uv[f[:, 1], 0]) + g[2] * uv[f[:, 2], 0]
            Vt = (g[0] * uv[f[:, 0], 1] + g[1] * uv[f[:, 1], 1]) + g[2] * uv[f[:, 2], 1]
            assert U.dtype == f32 and Vt.dtype == f32
            has = np.isfinite(U) & np.isfinite(Vt)
            Uo, Vo = np.where(has, U, f32(0)), np.where(has, Vt, f32(0))
            if wrong == "clamp":
                fu, fv = np.clip(Uo, f32(0), f32(1)), np.clip(Vo, f32(0), f32(1))
            else:
                fu, fv = Uo - np.floor(Uo), Vo - np.floor(Vo)
            tx = np.minimum((fu * f32(TW)).astype(np.int64), TW - 1)
            ty = np.minimum((fv * f32(TH)).astype(np.int64), TH - 1)
            m = np.asarray(tex, np.uint8)[ty, tx].astype(np.int64)
            if wrong == "bgr":
                m = m[:, ::-1]
            texel = np.where(has, ty * TW + tx, -1)
    o = rgb[rr, cc].astype(np.int64)
    out = record(model.sum(), visible.sum(), (~has).sum(), m[has], o[has])
    if maps:
        tmap = np.full((H, W), -1, np.int64)
        tmap[model] = (keys[model] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        xmap = np.full((H, W), -1, np.int64)
        xmap[rr, cc] = texel
        mmap = np.zeros((H, W, 3), np.int64)
        mmap[rr[has], cc[has]] = m[has]
        out.update(model=model, visible=visible, tri=tmap, texel=xmap, values=mmap)
    return out


def sums_of_mesh(mesh, pose, K, rgb, D, tol_m=0.005, **kw):
    """`sums` of a synthetic Mesh with the colour source the library would use for it"""
    colors = mesh.vertex_colors if getattr(mesh, "color_source", 0) == 1 else None
    return sums(FR.centred(mesh), mesh.faces, pose, K, rgb, D, tol_m, uvs=stored_uvs(mesh), tex=mesh.texture, colors=colors, **kw)


def painted(rec_maps, rgb):
    """rgb with every compared pixel painted with the model's own value there (rec_maps: a record with maps)"""
    out = np.array(rgb, np.uint8)
    at = rec_maps["texel"] >= 0
    out[at] = rec_maps["values"][at].astype(np.uint8)
    return out


# ---- (b) the float64 reference ----------------------------------------------------------------------------------------------------------
def color64(mesh, pose, K, rgb, D, tol_m=0.005, tex=None):
    """float64, by other means -> the record, with maps (model, tri, texel).  Texture source only."""
    tex = mesh.texture if tex is None else tex
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    P = np.asarray(pose, np.float64)
    K = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    D = np.asarray(np.asarray(D, f32), np.float64)
    H, W = D.shape
    cam = v @ P[:3, :3].T + P[:3, 3]
    assert (cam[:, 2] > 0.02).all(), "the float64 reference is for poses well in front of the camera"
    faces = np.asarray(mesh.faces, np.int64)
    depth, win = IR._cast64(cam, faces, K, H, W)
    model = win >= 0
    with np.errstate(invalid="ignore"):
        hidden = (D >= float(FR.MIN_DEPTH)) & (D < depth - float(f32(tol_m)))
    visible = model & ~hidden
    rr, cc = np.nonzero(visible)
    ray = np.stack([(cc - K[0, 2]) / K[0, 0], (rr - K[1, 2]) / K[1, 1], np.ones(len(cc))], 1)
    hit = depth[visible][:, None] * ray
    t3 = cam[faces[win[visible]]]                                                       # [n,3,3]
    n = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
    nn = (n * n).sum(1)
    bary = np.stack([(np.cross(t3[:, (k + 2) % 3] - t3[:, (k + 1) % 3], hit - t3[:, (k + 1) % 3]) * n).sum(1) / nn for k in range(3)], 1)
    tc = np.asarray(mesh.texcoords, f32).astype(np.float64)
    tc = np.stack([tc[:, 0], 1.0 - tc[:, 1]], 1)                                        # the renderer samples (u, 1 - v)
    uv = np.einsum("nk,nkc->nc", bary, tc[faces[win[visible]]])
    TH, TW = tex.shape[:2]
    wrapped = uv - np.floor(uv)
    tx = np.minimum(np.floor(wrapped[:, 0] * TW).astype(np.int64), TW - 1)
    ty = np.minimum(np.floor(wrapped[:, 1] * TH).astype(np.int64), TH - 1)
    m = np.asarray(tex, np.uint8)[ty, tx].astype(np.int64)
    o = np.asarray(rgb, np.uint8)[rr, cc].astype(np.int64)
    out = record(model.sum(), visible.sum(), 0, m, o)
    xmap = np.full((H, W), -1, np.int64)
    xmap[rr, cc] = ty * TW + tx
    out.update(model=model, visible=visible, tri=win, texel=xmap)
    return out


def compare(a, b):
    """(a) with maps against (b) -> (share of the pixels either covers that differ in coverage, visibility or triangle; share of the
    others, where both compare, that pick another texel; the number of those others)"""
    either = a["model"] | b["model"]
    differ = either & ((a["model"] != b["model"]) | (a["visible"] != b["visible"]) | (a["tri"] != b["tri"]))
    both = either & ~differ & (a["texel"] >= 0) & (b["texel"] >= 0)
    other = both & (a["texel"] != b["texel"])
    return differ.sum() / max(either.sum(), 1), other.sum() / max(both.sum(), 1), int(both.sum())


# ---- symmetry resolution -----------------------------------------------------------------------------------------------------------------
def _rigid_mul(Ra, ta, Rb, tb):
    """the host's product of two rigid transforms, float64, in its order of operations"""
    R = np.empty((3, 3))
    t = np.empty(3)
    for r in range(3):
        for c in range(3):
            R[r, c] = (Ra[r, 0] * Rb[0, c] + Ra[r, 1] * Rb[1, c]) + Ra[r, 2] * Rb[2, c]
        t[r] = ((Ra[r, 0] * tb[0] + Ra[r, 1] * tb[1]) + Ra[r, 2] * tb[2]) + ta[r]
    return R, t


def equivalents(pose, symmetries, center):
    """E_s = pose * S'_s, s = 0..S, as fp_resolve_symmetry forms them: S'_s the mesh-frame symmetry conjugated with the mesh centre,
    x' = R_s (x + c) + t_s - c, in float64; rounded to f32 once; E_0 the pose itself -> [S + 1, 4, 4] f32"""
    pose = np.asarray(pose, f32)
    P = pose.astype(np.float64)
    c = np.asarray(center, f32).astype(np.float64)
    out = [pose.copy()]
    for S in symmetries:
        S = np.asarray(S, f32).astype(np.float64)
        Rs = S[:3, :3]
        ts = np.array([(((Rs[r, 0] * c[0] + Rs[r, 1] * c[1]) + Rs[r, 2] * c[2]) + S[r, 3]) - c[r] for r in range(3)])
        R, t = _rigid_mul(P[:3, :3], P[:3, 3], Rs, ts)
        E = pose.copy()
        E[:3, :3], E[:3, 3] = R.astype(f32), t.astype(f32)
        out.append(E)
    return np.stack(out)


def resolve(records):
    """the winner among records (dicts or device records): the largest zncc with status 0, ties to the lower index; None without one"""
    get = (lambda r, k: r[k]) if isinstance(records[0], dict) else getattr
    best = None
    for i, r in enumerate(records):
        if get(r, "status") == 0 and (best is None or f32(get(r, "zncc")) > f32(get(records[best], "zncc"))):
            best = i
    return best
