"""autodecode --batch on the CPU: run() with a recording fake fitter - grouping, the short last batch, the order of the records and
[start, end) - and the bookkeeping of the new entry points (asdf_fit_codes, asdf_fit_codes_workspace_bytes)."""
import json
import os

import numpy as np
import pytest

from alignsdf_amd import autodecode as ad
from alignsdf_amd import synthetic as syn

L = 256


def _tree(root, names):
    for sub in ("mesh_hand", "mesh_obj"):
        os.makedirs(os.path.join(root, "obman", "test", sub), exist_ok=True)
        for n in names:
            with open(os.path.join(root, "obman", "test", sub, n + ".obj"), "w") as fh:
                fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")


class Recorder:
    """A fitter that fits nothing: the code is the start plus the name's number, the record names the sample."""

    def __init__(self):
        self.single, self.batches = [], []

    def _fit(self, name, start):
        return start + float(int(name)), {"first": 2.0 + int(name), "last": 1.0, "steps": 3, "mesh_info": {}}

    def __call__(self, name, hand_path, obj_path, poses, start):
        self.single.append(name)
        return self._fit(name, start)

    def fit_many(self, jobs):
        assert all(h.endswith(os.path.join("mesh_hand", n + ".obj")) and o.endswith(os.path.join("mesh_obj", n + ".obj")) for n, h, o, _, _ in jobs)
        self.batches.append([(n, float(start[0]), sorted(poses)) for n, _, _, poses, start in jobs])
        return [self._fit(n, start) for n, _, _, _, start in jobs]


def _files(out):
    return {n: dict(np.load(os.path.join(out, n))) for n in sorted(os.listdir(out)) if n.endswith(".npz")}


def test_batches_group_the_pairs_in_order(tmp_path):
    names = ["00000008", "00000002", "00000011", "00000005", "00000003", "00000013", "00000001"]
    data, init = str(tmp_path / "data"), str(tmp_path / "init")
    _tree(data, names)
    os.makedirs(init)
    for n in names:
        np.savez(os.path.join(init, n + ".npz"), latent=np.full((1, L), 0.25 * int(n), np.float32))
    specs = syn.specs_for("nerf3")
    order = sorted(names)
    # --batch 1: the one-sample fitter, never the many-sample call
    one = Recorder()
    path1, records1 = ad.run(specs, one, "obman", data, str(tmp_path / "b1"), init_dir=init)
    assert one.single == order and not one.batches and [r["name"] for r in records1] == order
    # --batch 3 over 7 pairs: 3 + 3 + 1, in discovery order
    three = Recorder()
    path3, records3 = ad.run(specs, three, "obman", data, str(tmp_path / "b3"), init_dir=init, batch=3)
    assert not three.single and [[j[0] for j in b] for b in three.batches] == [order[0:3], order[3:6], order[6:7]]
    assert all(j[1] == 0.25 * int(j[0]) and j[2] == [] for b in three.batches for j in b)
    assert records3 == records1 and json.load(open(path3)) == json.load(open(path1))
    f1, f3 = _files(str(tmp_path / "b1")), _files(str(tmp_path / "b3"))
    assert list(f1) == [n + ".npz" for n in order] == list(f3)
    for n in f1:
        assert list(f1[n]) == list(f3[n]) == ["latent"] and np.array_equal(f1[n]["latent"], f3[n]["latent"])
        assert f1[n]["latent"].shape == (1, L) and float(f1[n]["latent"][0, 0]) == 1.25 * int(n[:-4])
    # [start, end) is taken before the grouping; a batch larger than what is left is one short batch
    part = Recorder()
    _, records = ad.run(specs, part, "obman", data, str(tmp_path / "part"), init_dir=init, start=1, end=6, batch=2)
    assert [[j[0] for j in b] for b in part.batches] == [order[1:3], order[3:5], order[5:6]] and [r["name"] for r in records] == order[1:6]
    big = Recorder()
    _, records = ad.run(specs, big, "obman", data, str(tmp_path / "big"), init_dir=init, end=2, batch=8)
    assert [[j[0] for j in b] for b in big.batches] == [order[0:2]] and [r["name"] for r in records] == order[0:2]
    # nothing found: no call at all
    none = Recorder()
    _, records = ad.run(specs, none, "obman", data, str(tmp_path / "none"), start=7, batch=4)
    assert records == [] and not none.batches and not none.single
    with pytest.raises(ValueError, match="batch"):
        ad.run(specs, none, "obman", data, str(tmp_path / "bad"), batch=0)
    # a fitter that loses a sample is an error, not a shifted file
    class Short(Recorder):
        def fit_many(self, jobs):
            return super().fit_many(jobs)[:-1]
    with pytest.raises(RuntimeError, match="results"):
        ad.run(specs, Short(), "obman", data, str(tmp_path / "short"), batch=2)


def test_pose_check_comes_before_any_batch(tmp_path):
    names = ["00000001", "00000002", "00000003"]
    data, poses = str(tmp_path / "data"), str(tmp_path / "poses")
    _tree(data, names)
    specs = syn.specs_for("both9")
    rec = Recorder()
    with pytest.raises(ValueError, match="poses"):
        ad.run(specs, rec, "obman", data, str(tmp_path / "never"), batch=2)
    assert not rec.batches and not rec.single and not os.path.exists(str(tmp_path / "never"))
    # with poses every job of a batch carries its own; a file that lacks an array stops the run before that batch is fitted
    os.makedirs(poses)
    _, mano, obj = syn.sample_inputs("both9", 1)
    for i, n in enumerate(names):
        np.savez(os.path.join(poses, n + ".npz"), global_trans=mano["global_trans"], rot_center=mano["rot_center"] + i, obj_trans=obj["obj_trans"])
    out = str(tmp_path / "codes")
    ad.run(specs, rec, "obman", data, out, poses, batch=2)
    assert [[j[0] for j in b] for b in rec.batches] == [names[:2], names[2:]]
    assert all(j[2] == ["global_trans", "obj_trans", "rot_center"] for b in rec.batches for j in b)
    for i, n in enumerate(names):
        assert np.array_equal(np.load(os.path.join(out, n + ".npz"))["rot_center"], (mano["rot_center"] + i).astype(np.float32))
    np.savez(os.path.join(poses, "00000003.npz"), global_trans=mano["global_trans"], rot_center=mano["rot_center"])
    late = Recorder()
    with pytest.raises(ValueError, match=r"00000003\.npz.*obj_trans"):
        ad.run(specs, late, "obman", data, str(tmp_path / "partial"), poses, batch=2)
    assert [[j[0] for j in b] for b in late.batches] == [names[:2]]


def test_command_line_takes_a_batch():
    import inspect
    assert "--batch" in inspect.getsource(ad.main) and inspect.signature(ad.run).parameters["batch"].default == 1
    assert callable(getattr(ad.DeviceFitter, "fit_many"))


def test_abi_bookkeeping():
    from alignsdf_amd import _native
    assert _native.ABI_VERSION == 132
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "alignsdf_hip.h")) as fh:
        text = fh.read()
    for name in ("asdf_fit_codes", "asdf_fit_codes_workspace_bytes"):
        assert name in _native.EXPORTS and "int %s(" % name in text
    with open(os.path.join(here, "..", "alignsdf_amd", "csrc", "decoder.hip")) as fh:
        assert "return 132;" in fh.read().split("asdf_version")[1][:200]
    from alignsdf_amd.build_native import SOURCES, TU_FLAGS
    assert "k1vb_kernels.hip" in SOURCES and TU_FLAGS["k1vb_kernels.hip"] == TU_FLAGS["k1v_kernels.hip"]
