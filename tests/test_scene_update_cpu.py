"""CPU-side checks of moving a resident scene's objects (fw_scene_update): the export and its declaration, the argument errors that come
back before a scene is looked at, and SceneDesc.placements — the placement-only description DeviceScene.update builds from a moved Scene
(new objects, the kept shape, material, texture and environment arrays, ValueError when an object's shape was swapped)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from firework_amd import _abi as A
from firework_amd import _lib, scenes
from firework_amd.api import RenderObject, Rotor3, Sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_export_and_null_arguments():
    lib = _lib.load()
    assert hasattr(lib, "fw_scene_update")
    assert lib.fw_abi_version() == 8 == A.FW_ABI_VERSION
    text = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    entry_points = text[text.index("/* ---- entry points"):]
    assert re.search(r"\bint fw_scene_update\s*\(fw_scene \*scene, const fw_scene_desc \*desc\);", entry_points)
    assert lib.fw_scene_update(None, None) == A.FW_ERR_BAD_ARG
    s, _r = scenes.cornell_box()
    assert lib.fw_scene_update(None, s.to_desc().ptr()) == A.FW_ERR_BAD_ARG
    not_a_scene = C.create_string_buffer(64)        # a NULL desc comes back before the scene is dereferenced
    assert lib.fw_scene_update(C.cast(not_a_scene, C.c_void_p), None) == A.FW_ERR_BAD_ARG


def _ptr(p):
    return C.cast(p, C.c_void_p).value


def test_placements_reflect_moved_objects_and_keep_the_arrays():
    s, _r = scenes.config("C4a_hdri_test", 8, 8, 1)
    kept = s.to_desc()
    ros = s.render_objects
    ros[0].position(1.5, -2.0, 3.25)
    ros[1].rotate(Rotor3.from_euler_angles(0.3, -0.2, 0.1))
    ros[2].flip_normals()
    new = kept.placements(s)
    fresh = s.to_desc()
    assert new.desc.n_objects == kept.desc.n_objects == len(ros)
    assert bytes(new.objects) == bytes(fresh.objects)        # the same fw_object records a new SceneDesc would hold
    assert bytes(new.objects) != bytes(kept.objects)
    o = new.objects
    assert (o[0].position.x, o[0].position.y, o[0].position.z) == (1.5, -2.0, 3.25)
    assert o[1].rotation.s != 1.0 and o[2].flip_normals == 1 and o[0].flip_normals == 0
    assert [o[i].shape for i in range(len(ros))] == [kept.objects[i].shape for i in range(len(ros))]
    for field, arr in (("shapes", kept.shapes), ("materials", kept.materials), ("textures", kept.textures)):
        assert _ptr(getattr(new.desc, field)) == C.addressof(arr) == _ptr(getattr(kept.desc, field)), field
        assert getattr(new.desc, "n_" + field) == getattr(kept.desc, "n_" + field)
    assert _ptr(new.desc.objects) == C.addressof(new.objects) != C.addressof(kept.objects)
    assert new.desc.environment.kind == A.FW_ENV_HDR
    assert _ptr(new.desc.environment.hdr_rgb) == _ptr(kept.desc.environment.hdr_rgb) != None  # noqa: E711
    assert bytes(new.desc.environment) == bytes(kept.desc.environment)
    assert new.content_hash() == fresh.content_hash()
    # placements of placements: still the first description's arrays
    ros[0].position(0.0, 0.0, 0.0)
    again = new.placements(s)
    assert _ptr(again.desc.shapes) == C.addressof(kept.shapes)


def test_placements_reject_other_shapes():
    s, _r = scenes.config("C2_cornell_box", 8, 8, 1)
    kept = s.to_desc()
    ros = s.render_objects
    ros[0].obj, ros[1].obj = ros[1].obj, ros[0].obj              # two shapes of the scene swapped between objects
    with pytest.raises(ValueError):
        kept.placements(s)
    ros[0].obj, ros[1].obj = ros[1].obj, ros[0].obj
    kept.placements(s)
    ros[0].obj = Sphere.new(1.0, 0)                              # a shape the description does not know
    with pytest.raises(ValueError):
        kept.placements(s)
    s2, _ = scenes.config("C2_cornell_box", 8, 8, 1)
    kept2 = s2.to_desc()
    s2.add_object(RenderObject.new(Sphere.new(1.0, 0)))          # one more object
    with pytest.raises(ValueError):
        kept2.placements(s2)


def test_device_scene_update_raises_before_the_library_is_called():
    """DeviceScene.update with a Scene whose object uses another shape: ValueError, and fw_scene_update is never reached."""
    s, _r = scenes.config("C2_cornell_box", 8, 8, 1)

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")

    ds = _lib.DeviceScene.__new__(_lib.DeviceScene)
    ds._lib, ds._desc, ds.handle, ds.device = NoLib(), s.to_desc(), None, 0
    s.render_objects[3].obj = s.render_objects[4].obj
    with pytest.raises(ValueError):
        ds.update(s)
    ds.handle = None


def test_placements_positions_are_float32():
    s, _r = scenes.config("C1_random_spheres", 8, 8, 1)
    kept = s.to_desc()
    s.render_objects[5].position_vec(np.array([0.1, 0.2, 0.3]))
    o = kept.placements(s).objects[5]
    assert (o.position.x, o.position.y, o.position.z) == tuple(float(v) for v in np.float32([0.1, 0.2, 0.3]))


def test_chained_updates_hold_a_bounded_set_of_buffers():
    """An animation loop: DeviceScene.update(scene) every frame keeps the latest description, which holds the first description's buffers
    and its own object array — never the object arrays of earlier frames."""
    s, _r = scenes.config("C1_random_spheres", 8, 8, 1)

    class AcceptingLib:                                          # fw_scene_update succeeds; nothing else may be called
        def fw_scene_update(self, handle, desc):
            return A.FW_OK

    ds = _lib.DeviceScene.__new__(_lib.DeviceScene)
    first = s.to_desc()
    ds._lib, ds._desc, ds.handle, ds.device = AcceptingLib(), first, None, 0
    rng = np.random.default_rng(4)
    earlier = []
    for frame in range(50):
        for ro in s.render_objects[:10]:
            ro.position_vec(ro._position + rng.uniform(-0.01, 0.01, 3).astype(np.float32))
        ds.update(s)
        assert len(ds._desc._keep) == len(first._keep) + 1, frame
        assert not any(any(a is e for e in earlier) for a in ds._desc._keep), frame
        assert _ptr(ds._desc.desc.shapes) == C.addressof(first.shapes)
        earlier.append(ds._desc.objects)
    assert bytes(ds._desc.objects) == bytes(s.to_desc().objects)
