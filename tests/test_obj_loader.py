"""OBJ loader vs the reference's own artefacts: tobj 1.0's output for suzanne.obj is serialised in the
reference's scenes/suzanne.yml (kept here as scenes/suzanne_mesh.npz), and teapot.obj -> scenes/teapot.yml
(both kept byte for byte, xz-compressed, under tests/golden/)."""
import lzma
import os

import numpy as np

from firework_amd.obj import load_obj

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def unpacked(tmp_path, name):
    """tests/golden/<name>.xz written out as <tmp_path>/<name>."""
    dst = tmp_path / name
    with lzma.open(os.path.join(HERE, "golden", name + ".xz")) as f:
        dst.write_bytes(f.read())
    return str(dst)


def test_suzanne_obj_reproduces_the_reference_yaml_mesh():
    models = load_obj(os.path.join(HERE, "golden", "suzanne.obj"))
    assert len(models) == 1
    m = models[0]
    d = np.load(os.path.join(ROOT, "scenes", "suzanne_mesh.npz"))
    assert m["positions"].shape == (1966, 3) and m["indices"].shape == (2904,)
    assert np.array_equal(m["positions"], d["verts"])          # f32-equal
    assert np.array_equal(m["indices"], d["indicies"])


def test_teapot_obj_matches_reference_teapot_yml(tmp_path):
    from firework_amd.yaml_io import load_scene
    models = load_obj(unpacked(tmp_path, "teapot.obj"))          # CRLF file, 4 groups, vn normals
    sc = load_scene(unpacked(tmp_path, "teapot.yml"))
    meshes = [ro.obj for ro in sc.render_objects if type(ro.obj).__name__ == "TriangleMesh"]
    assert len(models) == len(meshes) == 4
    for m, ref in zip(models, meshes):
        assert np.array_equal(m["indices"], ref.indicies)
        assert np.array_equal(m["positions"], ref.verts)
        assert m["normals"] is not None and np.array_equal(m["normals"], ref.normals)
