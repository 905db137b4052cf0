"""numpy restatement of DESIGN.md section 4.9 (fp_render_scene): K objects in one picture.

Per object the projection, coverage, depth and shade are frame_render_ref's (section 4.8), imported, not restated.  What this file
adds is what the scene call adds: keys composed with the GLOBAL triangle index (faces of the objects before o in the call + t), the
coverage word, the per-object records and the palette overlay -- each written here independently of the kernel.
Shared by tests/test_scene_render_ref_cpu.py (which holds it to the composition of K frame_render_ref.render calls) and
tests/test_scene_render_gpu.py (which holds the kernels to it, bit for bit)."""
import numpy as np

import frame_render_ref as FR

f32 = np.float32
MAX_OBJECTS = 64            # FP_SCENE_MAX_OBJECTS
PALETTE = ((40, 220, 120), (230, 80, 60), (70, 130, 240), (240, 200, 40), (200, 80, 220), (40, 210, 220), (250, 140, 30), (160, 230, 60))
OUTPUTS = ("model_depth", "instance_id", "visible_mask", "tri_id", "cover_bits", "overlay")
RECORD = ("n_covered", "n_front", "n_hidden", "n_visible", "n_occluded")
LOW32 = np.uint64(0xFFFFFFFF)


class Refused(Exception):
    """an object's pose needs a clipper or leaves the exact integer range; .index is the lowest such object"""

    def __init__(self, index, why):
        super().__init__(f"object {index}: {why}")
        self.index, self.why = index, why


def render(objects, K, rgb, depth, tol_m=0.005):
    """objects: a list of (centred vertices, faces, pose 4x4) in call order -> (dict of the six outputs, records [K, 5] int64 in the
    order of RECORD); raises Refused like the library errors"""
    assert 1 <= len(objects) <= MAX_OBJECTS
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    proj = []
    for o, (verts, faces, pose) in enumerate(objects):
        cam, snap, near, far = FR.project(verts, pose, K)
        if near.any() or far.any():
            raise Refused(o, "near" if near.any() else "range")
        proj.append((cam, snap))
    assert sum(len(f) for _, f, _ in objects) < 2 ** 32 - 1
    keys = np.full((H, W), FR.EMPTY, np.uint64)
    inst = np.zeros((H, W), np.int64)          # object + 1 of the smallest key so far
    local = np.zeros((H, W), np.int64)         # triangle + 1 within that object
    cover = np.zeros((H, W), np.uint64)
    start = 0                                  # faces of the objects before o
    for o, ((verts, faces, pose), (cam, snap)) in enumerate(zip(objects, proj)):
        own = FR.rasterize(cam, snap, FR.stored_faces(verts, faces), H, W)   # bits(z) << 32 | t
        hit = own != FR.EMPTY
        g = (own & LOW32) + np.uint64(start)                          # the global index: below 2^32 - 1 by the check above
        composed = np.where(hit, (own & ~LOW32) | g, FR.EMPTY)
        wins = composed < keys                                        # the smallest key: nearest, then lowest object, then lowest triangle
        keys = np.where(wins, composed, keys)
        inst = np.where(wins, o + 1, inst)
        local = np.where(wins, (own & LOW32).astype(np.int64) + 1, local)
        cover |= np.where(hit, np.uint64(1) << np.uint64(o), np.uint64(0))
        start += len(faces)
    model = keys != FR.EMPTY
    z = np.where(model, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    with np.errstate(invalid="ignore"):
        occluded = model & ~(depth < FR.MIN_DEPTH) & (depth < z - f32(tol_m))
    visible = model & ~occluded
    overlay = np.asarray(rgb, np.uint8).copy()
    records = np.zeros((len(objects), len(RECORD)), np.int64)
    for o, ((verts, faces, pose), (cam, snap)) in enumerate(zip(objects, proj)):
        front = inst == o + 1
        seen = front & visible
        n_cov = int(((cover >> np.uint64(o)) & np.uint64(1)).sum())
        n_front, n_vis = int(front.sum()), int(seen.sum())
        records[o] = (n_cov, n_front, n_cov - n_front, n_vis, n_front - n_vis)
        if n_vis:
            k = FR.shade(cam, faces, local[seen] - 1)
            src = overlay[seen].astype(np.int64)
            tint = (np.asarray(PALETTE[o % 8], np.int64)[None, :] * k[:, None] + 127) // 255
            overlay[seen] = ((src + tint + 1) >> 1).astype(np.uint8)
    out = dict(model_depth=z, instance_id=inst.astype(np.uint8), visible_mask=np.where(visible, 255, 0).astype(np.uint8),
               tri_id=local.astype(np.int32), cover_bits=cover, overlay=overlay)
    return out, records


def compose_singles(objects, K, rgb, depth, tol_m=0.005):
    """the per-pixel composition of K frame_render_ref.render calls: the min of the non-zero depths with the lowest index on ties ->
    (model_depth, instance, tri_id, visible_mask, [mask of object o]); the statement fp_render_scene's result is held to"""
    depth = np.asarray(depth, f32)
    best = np.zeros(depth.shape, f32)
    inst = np.zeros(depth.shape, np.int64)
    tri = np.zeros(depth.shape, np.int32)
    vis = np.zeros(depth.shape, np.uint8)
    masks = []
    for o, (verts, faces, pose) in enumerate(objects):
        one = FR.render(verts, faces, pose, K, rgb, depth, tol_m)
        m = one["model_mask"] > 0
        masks.append(m)
        # positive f32 order like their bit patterns; strictly nearer wins, so the lowest index keeps a tie
        wins = m & ((inst == 0) | (one["model_depth"] < best))
        best = np.where(wins, one["model_depth"], best)
        inst = np.where(wins, o + 1, inst)
        tri = np.where(wins, one["tri_id"], tri)
        vis = np.where(wins, one["visible_mask"], vis)
    return best, inst, tri, vis, masks
