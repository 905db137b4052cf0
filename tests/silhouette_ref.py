"""numpy restatement of DESIGN.md section 4.15 (fp_mask_distance, fp_pose_silhouette): the squared Euclidean distance transform by brute
force over the seeds, the pose's pixels by tests/frame_render_ref.py (project, rasterize, refused), integer counts and sums, and the host
formulas in float64 rounded once.

Shared by tests/test_silhouette_ref_cpu.py (which holds it to a second, separable transform and to hand answers) and
tests/test_pose_silhouette_gpu.py (which holds the kernels to it in every integer and in the bits of the three floats)."""
import numpy as np

import frame_render_ref as FR

f32 = np.float32
D2_NONE = 0x7FFFFFFF                 # FP_SIL_D2_NONE
REFUSED_NEAR, REFUSED_RANGE, EMPTY = 1, 2, 4
MAX_DIM, MAX_TRUNC_PX = 8192, 32767
INTS = ("n_model", "n_visible", "n_inter", "n_spill", "n_mask", "n_miss", "status", "sum_spill_d2", "sum_miss_d2")
FLOATS = ("iou", "rms_spill_px", "rms_miss_px")
FIELDS = ("n_model", "n_visible", "n_inter", "n_spill", "n_mask", "n_miss", "status", "reserved", "sum_spill_d2", "sum_miss_d2",
          "iou", "rms_spill_px", "rms_miss_px", "reserved_f")


def edt2(seed):
    """-> [H,W] int64: per pixel the smallest (r - r')^2 + (c - c')^2 over the pixels (r', c') where `seed` is true, D2_NONE when there is
    none.  Brute force: every pixel that is no seed against every seed (a seed's own distance is 0)."""
    seed = np.asarray(seed, bool)
    out = np.zeros(seed.shape, np.int64)
    sr, sc = np.nonzero(seed)
    if len(sr) == 0:
        out[:] = D2_NONE
        return out
    pr, pc = np.nonzero(~seed)
    sr, sc = sr.astype(np.int64), sc.astype(np.int64)
    step = max(1, 2_000_000 // len(sr))
    for i in range(0, len(pr), step):
        r, c = pr[i:i + step, None].astype(np.int64), pc[i:i + step, None].astype(np.int64)
        out[pr[i:i + step], pc[i:i + step]] = ((r - sr[None, :]) ** 2 + (c - sc[None, :]) ** 2).min(axis=1)
    return out


def maps(mask):
    """(d2_to_mask, d2_to_bg) of a u8 mask: a mask pixel is one whose byte is > 0"""
    on = np.asarray(mask) > 0
    return edt2(on), edt2(~on)


def clip(v, trunc):
    return np.minimum(v, trunc * trunc) if trunc > 0 else v


def host_formulas(r):
    """iou, rms_spill_px, rms_miss_px and the EMPTY bit from a record's integers: float64, rounded to f32 once"""
    union = r["n_mask"] + r["n_spill"]
    r["iou"] = f32(np.float64(r["n_inter"]) / np.float64(union)) if union else f32(0)
    r["rms_spill_px"] = f32(np.sqrt(np.float64(r["sum_spill_d2"]) / np.float64(r["n_spill"]))) if r["n_spill"] else f32(0)
    r["rms_miss_px"] = f32(np.sqrt(np.float64(r["sum_miss_d2"]) / np.float64(r["n_miss"]))) if r["n_miss"] else f32(0)
    if not union:
        r["status"] |= EMPTY
    return r


def zero_record(status=0):
    r = {k: 0 for k in INTS}
    r.update(status=status, iou=f32(0), rms_spill_px=f32(0), rms_miss_px=f32(0))
    return r


def pose_pixels(mesh, pose, K, depth, tol, amodal):
    """(model, visible) [H,W] bool of the mesh under `pose`, fp_render_pose's model_mask and visible_mask (amodal: visible is model)"""
    verts = FR.centred(mesh)
    H, W = np.asarray(depth).shape
    cam, snap, _, _ = FR.project(verts, pose, K)
    keys = FR.rasterize(cam, snap, FR.stored_faces(verts, mesh.faces), H, W)
    model = keys != FR.EMPTY
    if amodal:
        return model, model.copy()
    z = np.where(model, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    D = np.asarray(depth, f32)
    with np.errstate(invalid="ignore"):
        occluded = model & ~(D < FR.MIN_DEPTH) & (D < z - f32(tol))
    return model, model & ~occluded


def records(mesh, poses, K, depth, mask, tol=0.005, trunc=0, amodal=False, d2=None):
    """fp_pose_silhouette -> a dict per pose.  d2: maps(mask), when the caller has them already"""
    on = np.asarray(mask) > 0
    d2m, d2b = maps(mask) if d2 is None else d2
    n_mask = int(on.sum())
    total = int(clip(d2b[on], trunc).sum())
    out = []
    for P in np.asarray(poses, f32).reshape(-1, 4, 4):
        why = FR.refused(FR.centred(mesh), P, K)
        if why:
            out.append(zero_record(REFUSED_NEAR if why == "near" else REFUSED_RANGE))
            continue
        model, visible = pose_pixels(mesh, P, K, depth, tol, amodal)
        inter, spill = visible & on, visible & ~on
        r = zero_record()
        r.update(n_model=int(model.sum()), n_visible=int(visible.sum()), n_inter=int(inter.sum()), n_spill=int(spill.sum()), n_mask=n_mask)
        r["n_miss"] = n_mask - r["n_inter"]
        r["sum_spill_d2"] = int(clip(d2m[spill], trunc).sum())
        r["sum_miss_d2"] = total - int(clip(d2b[inter], trunc).sum())
        out.append(host_formulas(r))
    return out
