"""The `rig` and `rig_merged` keys of the approach file (lidar_transfer_amd.config.Approach.rig): parsing, the sensor paths,
the names, the number of heads, the conflict with the top-level transformation -- and a file without the keys loads as before."""
import os

import numpy as np
import pytest

from lidar_transfer_amd.config import RIG_MAX_HEADS, load_approach, load_sensor, mount_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(adaption="mesh", preserve_float=False, voxel_size=0.1, number_of_scans=1, voxel_bounds=[-10, 10, -10, 10, -3, 3],
            ignore=[], moving=[], transformation=[], color_map={0: [0, 0, 0]})
PLAIN = dict(name="plain", fov_up=3.0, fov_down=-25.0, beams=16, angle_res_hor=360.0 / 64, fov_hor=360)
DOWN = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.4, 0, 0, 0, 1]   # a head 0.4 m below the source sensor


def _approach(**kw):
    return load_approach(dict(BASE, **kw))


def test_the_example_file():
    a = load_approach(os.path.join(ROOT, "config", "approach_rig_example.yaml"))
    heads = a.rig()
    assert [h.name for h in heads] == ["roof", "front"] and a.rig_merged is False
    # the sensor paths are relative to the approach file, wherever the process runs
    for h, fname in zip(heads, ("vlp32c_table_returns_1024.yaml", "front120_64x1024.yaml")):
        want = load_sensor(os.path.join(ROOT, "config", fname))
        assert h.sensor.as_tuple() == want.as_tuple() and h.sensor.target_model() == want.target_model()
    assert heads[0].sensor.return_model() is not None and heads[1].sensor.sector() is not None
    assert heads[0].mount is None
    T, P = heads[1].mount
    assert np.allclose(P[:3, 3], [0, 0, -0.4], atol=1e-12) and np.allclose(T @ P, np.eye(4), atol=1e-12)
    # 5 degrees down: the head's x axis points below the horizon of the source frame
    assert np.isclose(np.rad2deg(np.arcsin(-P[2, 0])), 5.0)
    assert a.mount() is None


def test_heads_from_mappings_and_paths(tmp_path):
    import yaml
    (tmp_path / "sensors").mkdir()
    with open(tmp_path / "sensors" / "s.yaml", "w") as f:
        yaml.safe_dump(dict(PLAIN, name="from a file"), f)
    with open(tmp_path / "approach.yaml", "w") as f:
        yaml.safe_dump(dict(BASE, rig=[dict(name="a", sensor=PLAIN), dict(name="b-2_X", sensor="sensors/s.yaml", transformation=DOWN),
                                       dict(name="c", sensor=str(tmp_path / "sensors" / "s.yaml"), transformation=[])],
                            rig_merged=True), f)
    a = load_approach(str(tmp_path / "approach.yaml"))
    heads = a.rig()
    assert [h.name for h in heads] == ["a", "b-2_X", "c"] and a.rig_merged is True
    assert [h.sensor.name for h in heads] == ["plain", "from a file", "from a file"]
    assert heads[0].mount is None and heads[2].mount is None
    assert np.array_equal(heads[1].mount[0], np.array(DOWN, np.float64).reshape(4, 4))
    assert np.array_equal(heads[1].mount[1], mount_of(DOWN)[1])
    # an identity transformation is none, as for the top-level key
    assert _approach(rig=[dict(name="a", sensor=PLAIN, transformation=np.eye(4).reshape(-1).tolist())]).rig()[0].mount is None


@pytest.mark.parametrize("n", [1, RIG_MAX_HEADS])
def test_one_to_eight_heads(n):
    heads = _approach(rig=[dict(name="h%d" % k, sensor=PLAIN) for k in range(n)]).rig()
    assert len(heads) == n and RIG_MAX_HEADS == 8


@pytest.mark.parametrize("n", [0, 9])
def test_zero_and_nine_heads_are_refused(n):
    a = _approach(rig=[dict(name="h%d" % k, sensor=PLAIN) for k in range(n)])   # (loading keeps the key ...)
    with pytest.raises(ValueError, match="1 to 8 heads"):
        a.rig()                                                                   # (... reading the rig validates it)


@pytest.mark.parametrize("name", ["", "a b", "a/b", "..", "front.1", 7, None])
def test_names_that_are_no_folder_names(name):
    with pytest.raises(ValueError, match="name"):
        _approach(rig=[dict(name=name, sensor=PLAIN)]).rig()


def test_names_are_unique():
    with pytest.raises(ValueError, match="'roof' is used twice"):
        _approach(rig=[dict(name="roof", sensor=PLAIN), dict(name="front", sensor=PLAIN), dict(name="roof", sensor=PLAIN)]).rig()


def test_entries_that_are_no_heads():
    for entry in ("roof", dict(name="a"), dict(sensor=PLAIN), dict(name="a", sensor=PLAIN, pose=DOWN), dict(name="a", sensor=3)):
        with pytest.raises(ValueError, match="rig"):
            _approach(rig=[entry]).rig()
    with pytest.raises(ValueError, match="1 to 8 heads"):
        _approach(rig=dict(name="a", sensor=PLAIN)).rig()
    with pytest.raises(ValueError, match="head 'a'.*transformation"):
        _approach(rig=[dict(name="a", sensor=PLAIN, transformation=[1, 2, 3])]).rig()
    with pytest.raises(KeyError):   # a sensor mapping is read like a sensor file
        _approach(rig=[dict(name="a", sensor=dict(name="x"))]).rig()


def test_top_level_transformation_conflicts_with_a_rig():
    rig = [dict(name="a", sensor=PLAIN)]
    with pytest.raises(ValueError, match="rig.*transformation|transformation.*rig"):
        _approach(rig=rig, transformation=DOWN).rig()
    # empty, absent-like and the exact identity are no conflict
    assert len(_approach(rig=rig, transformation=[]).rig()) == 1
    assert len(_approach(rig=rig, transformation=np.eye(4).reshape(-1).tolist()).rig()) == 1


def test_rig_merged():
    rig = [dict(name="a", sensor=PLAIN), dict(name="b", sensor=PLAIN, transformation=DOWN)]
    assert _approach(rig=rig).rig_merged is False
    assert _approach(rig=rig, rig_merged=True).rig_merged is True
    with pytest.raises(ValueError, match="rig_merged"):   # at load time, not when the rig is read
        _approach(rig_merged=True)
    for v in ("false", "true", 1, 0, None, []):           # a real boolean: the string "false" would be true
        with pytest.raises(ValueError, match="rig_merged"):
            _approach(rig=rig, rig_merged=v)


@pytest.mark.parametrize("fname", ["approach_mergemesh.yaml", "approach_mount_example.yaml"])
def test_a_file_without_the_key_loads_as_before(fname):
    a = load_approach(os.path.join(ROOT, "config", fname))
    assert a.rig() is None and a.rig_block is None and a.rig_merged is False
    assert (a.mount() is None) == (fname == "approach_mergemesh.yaml")
    b = _approach()
    assert b.rig() is None and b.mount() is None and b.base_dir is None
