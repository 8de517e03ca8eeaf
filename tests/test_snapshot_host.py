"""Host side of the snapshots (cosim_amd/snapshot.py): the file format and the metadata check, without a device.  The header /
EXPORTS agreement of the new entry points is enforced by test_host_logic.test_abi_library_exports_and_layouts."""
import json
import zipfile

import numpy as np
import pytest

from cosim_amd.snapshot import META_FIELDS, Snapshot, check_compatible

META = {"env_id": "flamingo_light_v1", "terrain": "flat", "precision": "medium", "snapshot_floats": 288, "state_stride": 224,
        "param_stride": 64, "state_dim": 52, "n_envs": 5, "env_id0": 0, "seed": 3}


def _snapshot():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((5, 288)).astype(np.float32)
    rows[:, 40:56] = np.arange(5 * 16, dtype=np.int32).reshape(5, 16).view(np.float32)   # meta words: int32 bits, denormals as floats
    rows[2, 7] = np.float32(np.nan)
    return Snapshot(rows, rng.standard_normal((5, 52)).astype(np.float32), rng.standard_normal((5, 4)).astype(np.float32), steps=37,
                    meta=META, policy_state={"t": np.array(37, dtype=np.int64), "h": rng.standard_normal((5, 6)).astype(np.float32)})


def test_save_load_round_trip_is_bit_exact_and_pickle_free(tmp_path):
    snap = _snapshot()
    path = str(tmp_path / "fleet.snap")                    # the name is kept as given
    snap.save(path)
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
    assert names == {"rows.npy", "obs.npy", "command.npy", "policy.t.npy", "policy.h.npy", "header_json.npy"}
    with np.load(path, allow_pickle=False) as z:           # every member loads without pickle; the header is JSON
        head = json.loads(z["header_json"].tobytes().decode())
        assert all(z[k].dtype != object for k in z.files)
    assert head == {"format": 1, "steps": 37, "meta": META}
    back = Snapshot.load(path)
    assert back.steps == 37 and back.meta == META and back.num_rows == 5 and back.steps_ago is None
    np.testing.assert_array_equal(back.rows.view(np.int32), snap.rows.view(np.int32))   # bits, NaN and denormals included
    np.testing.assert_array_equal(back.obs, snap.obs)
    np.testing.assert_array_equal(back.command, snap.command)
    assert int(back.policy_state["t"].reshape(-1)[0]) == 37 and back.policy_state["t"].dtype == np.int64
    np.testing.assert_array_equal(back.policy_state["h"], snap.policy_state["h"])
    on_cpu = Snapshot.load(path, device="cpu")             # tensors on request
    assert on_cpu.rows.dtype.is_floating_point and tuple(on_cpu.rows.shape) == (5, 288)
    np.testing.assert_array_equal(on_cpu.rows.numpy().view(np.int32), snap.rows.view(np.int32))


def test_history_style_snapshot_without_observation_rows(tmp_path):
    path = str(tmp_path / "ring.npz")
    Snapshot(_snapshot().rows, None, None, 25, META).save(path)
    back = Snapshot.load(path)
    assert back.obs is None and back.command is None and back.policy_state is None and back.steps == 25


def test_load_refuses_other_files(tmp_path):
    path = str(tmp_path / "other.npz")
    with open(path, "wb") as f:
        np.savez(f, rows=np.zeros((2, 32), dtype=np.float32))
    with pytest.raises(ValueError, match="not a snapshot file"):
        Snapshot.load(path)
    with open(path, "wb") as f:
        np.savez(f, rows=np.zeros((2, 32), dtype=np.float32),
                 header_json=np.frombuffer(json.dumps({"format": 99, "steps": 0, "meta": {}}).encode(), dtype=np.uint8))
    with pytest.raises(ValueError, match="format 99"):
        Snapshot.load(path)


def test_metadata_check_names_the_first_field_that_disagrees():
    check_compatible(dict(META), dict(META), need_n_envs=True)
    for field, other in (("env_id", "w4_p_v2"), ("terrain", "rocky_hard"), ("precision", "high"), ("snapshot_floats", 320),
                         ("state_stride", 256), ("param_stride", 96), ("state_dim", 64)):
        assert field in META_FIELDS
        with pytest.raises(ValueError, match=rf"{field} is .* in the snapshot, .* here"):
            check_compatible(dict(META, **{field: other}), dict(META), need_n_envs=False)
    # the first of several; n_envs only where rows map one to one; seed and env_id0 are recorded, never compared
    with pytest.raises(ValueError, match="terrain is 'rocky_hard' in the snapshot, 'flat' here"):
        check_compatible(dict(META, terrain="rocky_hard", precision="high", n_envs=9), dict(META), need_n_envs=True)
    check_compatible(dict(META, n_envs=9, seed=8, env_id0=64), dict(META), need_n_envs=False)
    with pytest.raises(ValueError, match="n_envs is 9 in the snapshot, 5 here"):
        check_compatible(dict(META, n_envs=9), dict(META), need_n_envs=True)
    broken = dict(META)
    del broken["precision"]
    with pytest.raises(ValueError, match="no field 'precision'"):
        check_compatible(broken, dict(META), need_n_envs=False)


def test_sinusoid_policy_state_round_trip():
    from cosim_amd.runner import SinusoidPolicy
    pol = SinusoidPolicy(4, 3, "cpu", seed=2)
    for _ in range(5):
        pol.get_action(None)
    st = pol.state()
    nxt = pol.get_action(None).clone()
    fresh = SinusoidPolicy(4, 3, "cpu", seed=2)
    fresh.load_state(st, src=[3, 2, 1, 0])
    assert fresh.t == 5
    np.testing.assert_array_equal(fresh.get_action(None).numpy(), nxt.numpy())
