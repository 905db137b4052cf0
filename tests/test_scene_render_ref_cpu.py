"""tests/scene_render_ref.py (the numpy restatement of DESIGN.md section 4.9 that tests/test_scene_render_gpu.py holds fp_render_scene to)
against the statement it restates: the result equals the per-pixel composition of K single-object renderings of
tests/frame_render_ref.py.  Then the cases of tests/scene_render_cases.py are held to what each is for, so that the GPU test compares
scenes that can break the kernels; and the pure host sizing of the binning block (fpt_scene_sizing) is checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import frame_render_ref as FR
import scene_render_cases as SC
import scene_render_ref as SR
from foundationpose_cpp_amd import _lib
from foundationpose_cpp_amd.api import _p

TILE = 32
COL = {n: i for i, n in enumerate(SR.RECORD)}


def _identities(out, rec):
    assert (rec[:, COL["n_covered"]] == rec[:, COL["n_front"]] + rec[:, COL["n_hidden"]]).all()
    assert (rec[:, COL["n_front"]] == rec[:, COL["n_visible"]] + rec[:, COL["n_occluded"]]).all()
    assert (rec >= 0).all()
    assert rec[:, COL["n_front"]].sum() == (out["instance_id"] > 0).sum()
    assert rec[:, COL["n_visible"]].sum() == (out["visible_mask"] > 0).sum()


@pytest.mark.parametrize("name", ["single", "overlap", "tie", "grid64", "binning", "wide"])
def test_reference_equals_the_composition_of_single_renderings(name):
    case = getattr(SC, name)()
    objects = SC.objects_of(case)
    out, rec = SC.reference(name)
    best, inst, tri, vis, masks = SR.compose_singles(objects, case[3], case[4], case[5])
    assert np.array_equal(out["model_depth"].view(np.uint32), best.view(np.uint32))
    assert np.array_equal(out["instance_id"], inst)
    assert np.array_equal(out["tri_id"], tri)
    assert np.array_equal(out["visible_mask"], vis)
    for o, m in enumerate(masks):
        assert np.array_equal((out["cover_bits"] >> np.uint64(o)) & np.uint64(1), m.astype(np.uint64)), f"amodal mask of object {o}"
    assert (out["cover_bits"] >> np.uint64(len(objects)) == 0).all() if len(objects) < 64 else True
    _identities(out, rec)


def test_single_object_is_frame_render_ref():
    case = SC.single()
    (verts, faces, pose), = SC.objects_of(case)
    out, rec = SC.reference("single")
    one = FR.render(verts, faces, pose, case[3], case[4], case[5])
    for n in ("model_depth", "visible_mask", "tri_id", "overlay"):       # PALETTE[0] is fp_render_pose's tint
        assert np.array_equal(out[n], one[n]), n
    assert np.array_equal(out["instance_id"] * 255, one["model_mask"])
    assert rec[0, COL["n_occluded"]] > 0 and rec[0, COL["n_visible"]] > 0 and rec[0, COL["n_hidden"]] == 0


def test_overlap_case_shows_what_it_is_for():
    out, rec = SC.reference("overlap")
    bits, inst = out["cover_bits"], out["instance_id"]
    assert (bits & (bits - np.uint64(1)) != 0).any()                      # some pixel has >= 2 coverage bits
    both = (bits & np.uint64(3)) == 3                                     # the overlap of the interpenetrating pair
    assert (inst[both] == 1).any() and (inst[both] == 2).any()            # each is in front somewhere inside it
    # ... and the winner changes inside one tile
    ty, tx = np.nonzero(both)
    tiles1 = {(y // TILE, x // TILE) for y, x in zip(ty, tx) if inst[y, x] == 1}
    tiles2 = {(y // TILE, x // TILE) for y, x in zip(ty, tx) if inst[y, x] == 2}
    assert tiles1 & tiles2
    assert (rec[:, COL["n_hidden"]] > 0).any() and (rec[:, COL["n_occluded"]] > 0).any()
    assert (rec[:, COL["n_covered"]] > 0).all()
    # two objects' translations are less than a radius apart
    t0, t1 = SC.overlap()[2][0][:3, 3], SC.overlap()[2][1][:3, 3]
    assert np.linalg.norm(t0 - t1) < 0.032


def test_tie_case_goes_to_the_lower_object():
    out, rec = SC.reference("tie")
    model = out["model_depth"] > 0
    assert model.sum() > 500
    assert (out["instance_id"][model] == 1).all() and (out["cover_bits"][model] == 3).all() and (out["cover_bits"][~model] == 0).all()
    assert rec[1, COL["n_front"]] == 0 and rec[1, COL["n_hidden"]] == rec[1, COL["n_covered"]] == rec[0, COL["n_covered"]] > 0
    single = SC.reference("single")[0]
    for n in ("model_depth", "tri_id", "visible_mask", "overlay"):
        assert np.array_equal(out[n], single[n]), n


def test_grid_of_64_uses_the_upper_half_of_the_word():
    out, rec = SC.reference("grid64")
    assert (rec[:, COL["n_covered"]] > 0).all()
    assert (out["instance_id"] > 32).any() and out["instance_id"].max() == 64
    bits = out["cover_bits"]
    high = bits >> np.uint64(32) != 0
    assert (high & (bits & (bits - np.uint64(1)) != 0)).any()             # a bit >= 32 together with another bit
    assert (rec[:, COL["n_hidden"]] > 0).sum() >= 16                      # neighbours overlap


def test_binning_case_shows_what_it_is_for():
    out, rec = SC.reference("binning")
    H, W = SC.binning()[6]
    box = (out["cover_bits"] & np.uint64(1)) != 0
    assert len({(y // TILE, x // TILE) for y, x in zip(*np.nonzero(box))}) >= 20
    tri, inst = out["tri_id"], out["instance_id"]
    same = (tri[:, TILE - 1:W - 1:TILE] == tri[:, TILE:W:TILE]) & (inst[:, TILE - 1:W - 1:TILE] == 1) & (inst[:, TILE:W:TILE] == 1)
    assert same.any()                                                     # a box triangle on both sides of a seam
    assert 0 < rec[2, COL["n_covered"]] < SC.reference("binning", True)[1][2, COL["n_covered"]] + 1
    assert (out["cover_bits"][:, 0] & np.uint64(4)).any()                 # object 2 reaches the frame's left edge: partly outside
    assert (rec[3] == 0).all()                                            # object 3: wholly outside, no error
    big, big_rec = SC.reference("binning", True)
    assert (big_rec[:, COL["n_covered"]] > 0).sum() == 7 and big_rec[:, COL["n_covered"]].sum() > 2 * rec[:, COL["n_covered"]].sum()


def test_wide_case_crosses_the_binning_chunk():
    out, rec = SC.reference("wide")
    H, W = SC.wide()[6]
    ntx = -(-W // TILE)
    assert ntx * -(-H // TILE) > 2048
    tile = (np.arange(H)[:, None] // TILE) * ntx + np.arange(W)[None, :] // TILE
    for o, where in ((0, tile < 2048), (1, tile < 2048), (1, tile >= 2048), (2, tile >= 2048)):
        assert (((out["cover_bits"] >> np.uint64(o)) & np.uint64(1)) != 0)[where].any(), (o, "tiles below 2048" if where[0, 0] else "tiles from 2048")
    assert (rec[:, COL["n_occluded"]] > 0).any() and (rec[:, COL["n_hidden"]] > 0).any()


def test_refusal_names_the_lowest_refused_object():
    ms, names, poses, K, rgb, depth, hw = SC.overlap()
    bad = list(poses)
    bad[2] = bad[2].copy(); bad[2][:3, 3] = (0, 0, 0.05)
    bad[3] = bad[3].copy(); bad[3][:3, 3] = (4000.0, 0, 0.2)
    with pytest.raises(SR.Refused) as e:
        SR.render(SC.objects_of((ms, names, bad)), K, rgb, depth)
    assert e.value.index == 2 and e.value.why == "near"


def test_sizing_of_the_binning_block():
    """fpt_scene_sizing: 32-px tiles rounded up on both axes; 258 fixed words (64 refusal words, the 64-bit total, 64 x 3 counters) and
    three per-tile arrays, one of them one longer; at most 2040 tiles at 1920 x 1080 (one workgroup scans them)"""
    L = _lib.test_lib()
    L.fpt_scene_sizing.argtypes = [C.c_int, C.c_int, C.c_void_p]
    for H, W in ((1, 1), (32, 32), (33, 32), (150, 208), (480, 640), (720, 1280), (1080, 1920), (2160, 3840)):
        out = np.zeros(3, np.int32)
        assert L.fpt_scene_sizing(H, W, _p(out)) == 0
        ntx, nty = -(-W // 32), -(-H // 32)
        assert tuple(out) == (ntx, nty, 258 + 3 * ntx * nty + 1)
    assert -(-1920 // 32) * -(-1080 // 32) == 2040
