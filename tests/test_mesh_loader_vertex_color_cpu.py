"""Mesh loader, per-vertex colours (include/foundationpose_amd.h FP_COLOR_TEXTURE / FP_COLOR_VERTEX): PLY `red green blue` in the three
encodings and as uchar or float, OBJ `v x y z r g b`; a file without UVs but with colours loads with the colour source VERTEX, a file
with UVs is what it always was.  Pure host code: runs on CPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from foundationpose_cpp_amd import FoundationPoseError, _lib, load_mesh, synthetic as syn
from foundationpose_cpp_amd.api import FP_COLOR_TEXTURE, FP_COLOR_VERTEX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fp_mesh_color_source", "fp_mesh_vertex_colors", "fp_set_vertex_colors", "fp_get_color_source"]


@pytest.fixture(scope="module")
def small_mesh():
    return syn.make_mesh(subdiv=2, offset=(0.01, -0.02, 0.03))   # 162 vertices, off-centre


@pytest.fixture(scope="module")
def colors(small_mesh):
    c = np.random.default_rng(7).integers(0, 256, (len(small_mesh.vertices), 3), dtype=np.uint8)
    c[0], c[1] = (0, 0, 0), (255, 255, 255)
    return c


def _write_ply(path, mesh, colors, fmt="ascii", ctype="uchar", normals=True, uv=False, names=("red", "green", "blue"), alpha=True,
               texture=None):
    """colors None: no colour properties.  ctype float: the colours as c / 255 in float32"""
    v, n, f = mesh.vertices, mesh.normals, mesh.faces
    e = ">" if fmt == "binary_big_endian" else "<"
    hdr = ["ply", f"format {fmt} 1.0"] + ([f"comment TextureFile {texture}"] if texture else [])
    hdr += [f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if normals:
        hdr += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        hdr += [f"property {ctype} {k}" for k in names] + ([f"property {ctype} alpha"] if alpha else [])
    if uv:
        hdr += ["property float texture_u", "property float texture_v"]
    hdr += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    body_a, body_b = [], b""
    for i in range(len(v)):
        row = list(v[i]) + (list(n[i]) if normals else [])
        la, lb = " ".join("%.9g" % x for x in row), struct.pack(e + "%df" % len(row), *row)
        if colors is not None:
            c = [int(x) for x in colors[i]] + ([255] if alpha else [])
            if ctype == "float":
                cf = [np.float32(x / 255.0) for x in c]
                la += " " + " ".join("%.9g" % x for x in cf)
                lb += struct.pack(e + "%df" % len(cf), *cf)
            else:
                la += " " + " ".join(str(x) for x in c)
                lb += bytes(c)
        if uv:
            la += " %.9g %.9g" % tuple(mesh.texcoords[i])
            lb += struct.pack(e + "2f", *mesh.texcoords[i])
        body_a.append(la)
        body_b += lb
    for t in f:
        body_a.append("3 " + " ".join(str(int(i)) for i in t))
        body_b += struct.pack(e + "B3i", 3, *[int(i) for i in t])
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode())
        fh.write(("\n".join(body_a) + "\n").encode() if fmt == "ascii" else body_b)
    return str(path)


def _write_obj(path, mesh, colors, colored=None, uv=False):
    """colored: the vertices whose `v` line carries r g b (default: all)"""
    with open(path, "w") as fh:
        for i, p in enumerate(mesh.vertices):
            line = "v %.9g %.9g %.9g" % tuple(p)
            if colors is not None and (colored is None or i in colored):
                line += " %.9g %.9g %.9g" % tuple(colors[i] / 255.0)
            fh.write(line + "\n")
        if uv:
            fh.writelines("vt %.9g %.9g\n" % tuple(p) for p in mesh.texcoords)
        fh.writelines("vn %.9g %.9g %.9g\n" % tuple(p) for p in mesh.normals)
        for a, b, c in mesh.faces + 1:
            fh.write(f"f {a}/{a}/{a} {b}/{b}/{b} {c}/{c}/{c}\n" if uv else f"f {a}//{a} {b}//{b} {c}//{c}\n")
    return str(path)


def _check_vertex_coloured(m, mesh, colors, case):
    assert m.color_source == FP_COLOR_VERTEX, case
    assert m.faces.shape == mesh.faces.shape and len(m.vertices) == len(mesh.vertices), case
    np.testing.assert_allclose(m.vertices[m.faces], mesh.vertices[mesh.faces], rtol=1e-6, err_msg=case)
    assert m.vertex_colors is not None and m.vertex_colors.dtype == np.uint8 and m.vertex_colors.shape == (len(m.vertices), 3), case
    np.testing.assert_array_equal(m.vertex_colors[m.faces], colors[mesh.faces], err_msg=case)     # per corner, through the de-duplication
    # the unchanged struct stays valid for fp_create: zero texcoords, the 2x2 grey default texture
    assert m.texcoords.shape == (len(m.vertices), 2) and (m.texcoords == 0).all(), case
    assert m.texture.shape == (2, 2, 3) and (m.texture == 100).all(), case


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no-normals"])
@pytest.mark.parametrize("ctype", ["uchar", "float"])
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_without_uvs_loads_with_its_vertex_colours(tmp_path, small_mesh, colors, fmt, ctype, normals):
    case = f"{fmt} {ctype} normals={normals}"
    m = load_mesh("c", _write_ply(tmp_path / "c.ply", small_mesh, colors, fmt=fmt, ctype=ctype, normals=normals))
    _check_vertex_coloured(m, small_mesh, colors, case)
    if normals:
        np.testing.assert_allclose(m.normals[m.faces], small_mesh.normals[small_mesh.faces], rtol=1e-6, err_msg=case)


def test_ply_aliases_and_out_of_range_floats(tmp_path, small_mesh, colors):
    m = load_mesh("c", _write_ply(tmp_path / "d.ply", small_mesh, colors, names=("diffuse_red", "diffuse_green", "diffuse_blue"), alpha=False))
    _check_vertex_coloured(m, small_mesh, colors, "diffuse_* aliases")
    # float colours are clamped to 0..1 and stored as rint(c * 255)
    tri = syn.Mesh("t", np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.float32([[0, 0, 1]] * 3), np.zeros((3, 2), np.float32),
                   np.int32([[0, 1, 2]]), np.zeros((2, 2, 3), np.uint8)).finalize()
    with open(tmp_path / "f.ply", "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float red\n"
                 "property float green\nproperty float blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                 "0 0 0 -0.5 0.5 1.5\n1 0 0 0.25 0.7490196 0.001\n0 1 0 1 0 0.998\n3 0 1 2\n")
    m = load_mesh("f", str(tmp_path / "f.ply"))
    np.testing.assert_array_equal(m.vertex_colors[m.faces[0]], [[0, 128, 255], [64, 191, 0], [255, 0, 254]])
    np.testing.assert_allclose(m.vertices[m.faces[0]], tri.vertices)


def test_textured_ply_that_also_carries_colours_is_what_it_was(tmp_path, small_mesh, colors):
    Image.fromarray(small_mesh.texture).save(tmp_path / "tex.png")
    a = load_mesh("a", _write_ply(tmp_path / "a.ply", small_mesh, None, fmt="binary_little_endian", uv=True, texture="tex.png"))
    b = load_mesh("b", _write_ply(tmp_path / "b.ply", small_mesh, colors, fmt="binary_little_endian", uv=True, texture="tex.png"))
    assert a.color_source == FP_COLOR_TEXTURE and b.color_source == FP_COLOR_TEXTURE
    for k in ("vertices", "normals", "texcoords", "faces", "texture", "center"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    assert a.diameter == b.diameter
    assert a.vertex_colors is None
    np.testing.assert_array_equal(b.vertex_colors[b.faces], colors[small_mesh.faces])     # still readable
    np.testing.assert_array_equal(b.texture, small_mesh.texture)


def test_obj_with_colours_on_the_v_lines(tmp_path, small_mesh, colors):
    m = load_mesh("o", _write_obj(tmp_path / "o.obj", small_mesh, colors))
    _check_vertex_coloured(m, small_mesh, colors, "obj")
    np.testing.assert_allclose(m.normals[m.faces], small_mesh.normals[small_mesh.faces], rtol=1e-6)
    # with UVs as well: the texture is the colour source, the colours stay readable
    t = load_mesh("o", _write_obj(tmp_path / "t.obj", small_mesh, colors, uv=True))
    assert t.color_source == FP_COLOR_TEXTURE
    np.testing.assert_allclose(t.texcoords[t.faces], small_mesh.texcoords[small_mesh.faces], rtol=1e-6)
    np.testing.assert_array_equal(t.vertex_colors[t.faces], colors[small_mesh.faces])


def test_dataset_writer_round_trips_a_vertex_coloured_mesh(tmp_path, small_mesh, colors):
    import dataclasses
    from foundationpose_cpp_amd import dataset
    twin = dataclasses.replace(small_mesh, vertex_colors=colors)
    twin.color_source = FP_COLOR_VERTEX
    _check_vertex_coloured(load_mesh("w", dataset.write_obj(str(tmp_path / "mesh"), twin)), small_mesh, colors, "dataset.write_obj")


def test_files_that_still_fail(tmp_path, small_mesh, colors):
    # only some `v` lines carry colours: no vertex colours, and without UVs the reference's error
    with pytest.raises(FoundationPoseError, match="invalid texturecoords"):
        load_mesh("p", _write_obj(tmp_path / "p.obj", small_mesh, colors, colored=set(range(0, len(colors), 2))))
    with pytest.raises(FoundationPoseError, match="invalid texturecoords"):
        load_mesh("n", _write_ply(tmp_path / "n.ply", small_mesh, None))
    with pytest.raises(FoundationPoseError, match="invalid texturecoords"):
        load_mesh("n", _write_obj(tmp_path / "n.obj", small_mesh, None))
    # a partially coloured OBJ WITH UVs is a textured mesh without colours
    t = load_mesh("p", _write_obj(tmp_path / "pt.obj", small_mesh, colors, colored={0, 5}, uv=True))
    assert t.color_source == FP_COLOR_TEXTURE and t.vertex_colors is None
    # truncated colour data: the malformed-body error
    for fmt in ("ascii", "binary_little_endian"):
        data = open(_write_ply(tmp_path / "full.ply", small_mesh, colors, fmt=fmt), "rb").read()
        end = data.index(b"end_header\n") + len(b"end_header\n")
        per_vertex = (len(data) - end) // (len(small_mesh.vertices) + len(small_mesh.faces))      # a cut inside the vertex element
        open(tmp_path / "cut.ply", "wb").write(data[:end + 40 * max(per_vertex, 8)])
        with pytest.raises(FoundationPoseError, match="truncated or malformed PLY body"):
            load_mesh("c", str(tmp_path / "cut.ply"))


def test_header_declares_and_both_libraries_export_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"include/foundationpose_amd.h does not declare {s}"
        assert s in _lib.SYMBOLS
    assert re.search(r"#define FP_COLOR_TEXTURE 0\b", src) and re.search(r"#define FP_COLOR_VERTEX 1\b", src)
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
        for s in NEW_SYMBOLS:
            assert s in exported, f"{os.path.basename(path)} does not export {s}"
