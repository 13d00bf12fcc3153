"""The mesh signed distance kernels (csrc/mesh_sdf.hip; alignsdf_amd.mesh_sdf, alignsdf_amd.gt_interaction) held to the fp64 rule of
tests/mesh_sdf_cases.py.  Yardsticks (mesh_sdf_cases.compare): |d| and - off the surface - w within 4 x the fp32 model's own maxima
against the truth; signs wherever the truth decides them; face by value; closest on its face and at |sdf|.  Every line printed with the
prefix MESHSDF is one case's measured errors (profiles/mesh_sdf_fp64_errors.txt)."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import interaction_cases as ic
from tests import mesh_sdf_cases as mc

pytestmark = pytest.mark.gpu
EINVAL = -1          # ASDF_EINVAL
SHAPES = ("whole", "split")


def _field(verts, faces):
    from alignsdf_amd.mesh_sdf import MeshField
    return MeshField(verts, faces)


@contextlib.contextmanager
def _shape(name):
    """Force a launch shape through the unit's environment variable (read at every call)."""
    before = os.environ.get("ASDF_MESH_SDF_SHAPE")
    os.environ["ASDF_MESH_SDF_SHAPE"] = name
    try:
        yield
    finally:
        if before is None:
            del os.environ["ASDF_MESH_SDF_SHAPE"]
        else:
            os.environ["ASDF_MESH_SDF_SHAPE"] = before


def _at(field, xyz, shape="auto"):
    """Everything MeshField.at gives, as numpy arrays."""
    with _shape(shape):
        r = field.at(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).cuda(), winding=True, face=True, closest=True)
    return {"sdf": r.sdf.cpu().numpy(), "w": r.winding.cpu().numpy(), "face": r.face.cpu().numpy(), "closest": r.closest.cpu().numpy()}


def _same_bits(a, b, keys=("sdf", "w", "face", "closest")):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in keys)


# ---- 1. truth at the edges

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", mc.CASES)
def test_truth_on_every_case(name, shape):
    v, f, xyz = mc.case(name)
    got = _at(_field(v, f), xyz, shape)
    e_d, e_w, left = mc.compare(name, got, "gpu " + shape)
    print("MESHSDF gpu %-5s %-13s T %4d M %5d | max |dd| %.2e (bound %.2e)  max |dw| %.2e (bound %.2e) | sign left out %d" % (
        shape, name, len(f), len(xyz), e_d, mc.D_BOUND, e_w, mc.W_BOUND, left))


@pytest.mark.parametrize("M", mc.LIST_LENGTHS)
def test_truth_on_every_list_length(M):
    v, f, xyz = mc.case("box")
    field = _field(v, f)
    for shape in SHAPES:
        got = _at(field, xyz[:M], shape)
        assert all(len(a) == M for a in got.values())
        mc.compare("box", got, "gpu %s M=%d" % (shape, M), take=slice(0, M))


# ---- 2. bit-repeatability

def test_results_depend_on_the_query_and_the_mesh_alone():
    v, f, xyz = mc.case("torus_open")                     # 523 faces: 5 chunks, the last one part of a block
    field = _field(v, f)
    base = _at(field, xyz, "whole")
    assert _same_bits(base, _at(field, xyz, "whole"))                                          # two calls
    for shape in ("split", "auto"):
        assert _same_bits(base, _at(field, xyz, shape)), shape                                # launch shapes
    perm = np.argsort(syn.uniform((len(xyz),), 44000), kind="stable")
    for shape in SHAPES:
        got = _at(field, xyz[perm], shape)
        assert _same_bits({k: a[perm] for k, a in base.items()}, got), shape                  # place in the list
        for take in (slice(0, 1), slice(5, 70), slice(100, 357), slice(1000, 1001)):           # M
            assert _same_bits({k: a[take] for k, a in base.items()}, _at(field, xyz[take], shape)), (shape, take)
    # a second field of the same mesh: nothing of the first call's state enters
    assert _same_bits(base, _at(_field(v, f), xyz, "split"))


def test_inward_and_outward_orientation_give_the_same_sdf_bits_and_opposite_w():
    (v, f, xyz), (vi, fi, xyzi) = mc.case("torus"), mc.case("torus_inward")
    assert np.array_equal(xyz, xyzi) and np.array_equal(f[:, ::-1], fi)
    for shape in SHAPES:
        out, inw = _at(_field(v, f), xyz, shape), _at(_field(vi, fi), xyz, shape)
        assert _same_bits(out, inw, ("sdf", "face", "closest")), shape
        assert np.array_equal(-inw["w"], out["w"]), shape                 # (as values: a sum that is 0 is +0 for both)
        assert (np.abs(out["w"]) > 0.9).sum() > 100                                            # (there are inside points)


# ---- 3. edges of the rule

def _bad_faces(num_verts):
    return np.array([[0, 1, num_verts], [-1, 2, 3], [2, 2 ** 31 - 1, 1], [0, 1, num_verts + 1], [-2 ** 31, 0, 1]], np.int32)


def test_appended_bad_faces_are_skipped_counted_and_change_no_bit():
    v, f, xyz = mc.case("torus_open")
    vn = np.concatenate([v, np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]], np.float32)])          # two non-finite vertices
    bad = np.concatenate([_bad_faces(len(vn)), [[0, 1, len(v)], [len(v) + 1, 5, 6]]]).astype(np.int32)
    more = np.concatenate([f, np.tile(bad, (40, 1))])                                                # 280 more: chunks of nothing but these
    field = _field(vn, more)
    assert field.info == {"skipped": 280, "zero_area": 0} and _field(v, f).info == {"skipped": 0, "zero_area": 0}
    for shape in SHAPES:
        assert _same_bits(_at(_field(v, f), xyz, shape), _at(field, xyz, shape)), shape


def test_interleaved_bad_faces_leave_the_distance_bits_and_move_the_indices():
    v, f, xyz = mc.case("torus_open")
    bad = _bad_faces(len(v))
    slots = np.sort(np.argsort(syn.uniform((len(f) + 60,), 45000), kind="stable")[:60])            # where the bad ones go
    mixed = np.empty((len(f) + 60, 3), np.int32)
    is_bad = np.zeros(len(mixed), bool)
    is_bad[slots] = True
    mixed[is_bad], mixed[~is_bad] = bad[np.arange(60) % len(bad)], f
    new_index = np.flatnonzero(~is_bad)
    field = _field(v, mixed)
    assert field.info["skipped"] == 60
    tr = mc.truth("torus_open")
    for shape in SHAPES:
        want, got = _at(_field(v, f), xyz, shape), _at(field, xyz, shape)
        assert np.array_equal(np.abs(got["sdf"]).view(np.int32), np.abs(want["sdf"]).view(np.int32))      # the minimum is exact in any grouping
        assert np.array_equal(got["face"], new_index[want["face"]]) and _same_bits(want, got, ("closest",))
        # the chunks hold other faces now: w is another fp32 sum of the same terms, each within the bound of the one truth
        off = mc.off_surface(tr)
        assert np.abs(got["w"].astype(np.float64) - tr["w"])[off].max() <= mc.W_BOUND
        clear = mc.clear_sign(tr)
        assert np.array_equal(np.signbit(got["sdf"][clear]), np.signbit(tr["sdf"][clear]))


def test_zero_area_faces_leave_w_alone_and_take_part_in_d():
    (v, f, _), (vf, ff, xyz) = mc.case("box"), mc.case("box_flat")
    field = _field(vf, ff)
    assert field.info == {"skipped": 0, "zero_area": 3}
    for shape in SHAPES:
        plain, flat = _at(_field(v, f), xyz, shape), _at(field, xyz, shape)
        assert np.array_equal(plain["w"].view(np.int32), flat["w"].view(np.int32)), shape
        # the first queries of the case sit at and around the segment (1..2, 0, 0) and the point (0, 1, 0.25)
        assert list(flat["sdf"][:6]) == [0.0, 0.5, 0.25, 0.0, 0.125, 0.25] and list(flat["face"][:5]) == [12, 12, 12, 13, 13]
        assert np.array_equal(flat["closest"][:5], np.array([[1.25, 0, 0], [2, 0, 0], [1.5, 0, 0], [0, 1, 0.25], [0, 1, 0.25]], np.float32))
        far = flat["face"] < 12
        assert _same_bits({k: a[far] for k, a in plain.items()}, {k: a[far] for k, a in flat.items()})


def test_empty_mesh_and_non_finite_queries():
    v, f = mc.box()
    q = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, -np.inf]], np.float32)
    for shape in SHAPES:
        for verts, faces in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (v, _bad_faces(len(v)))):
            got = _at(_field(verts, faces), q, shape)
            fin = [0, 3]
            assert np.isposinf(got["sdf"][fin]).all() and (got["w"][fin] == 0).all() and (got["face"] == -1).all()
            assert np.isnan(got["closest"]).all() and np.isnan(got["sdf"][[1, 2, 4]]).all() and np.isnan(got["w"][[1, 2, 4]]).all()
        got = _at(_field(v, f), q, shape)
        assert list(got["sdf"][fin]) == [-0.25, 1.5] and list(got["face"][[1, 2, 4]]) == [-1, -1, -1] and (got["face"][fin] >= 0).all()
        assert np.isnan(got["sdf"][[1, 2, 4]]).all() and np.isnan(got["w"][[1, 2, 4]]).all() and np.isnan(got["closest"][[1, 2, 4]]).all()
        assert np.isfinite(got["closest"][fin]).all()


def _raw_call(field, xyz_t, outs, scratch):
    ptr = lambda t: None if t is None else t.data_ptr()
    return _native.lib().asdf_mesh_sdf_points(field._ws.data_ptr(), field.num_faces, ptr(xyz_t), xyz_t.shape[0] if xyz_t is not None else 0,
                                              *[ptr(o) for o in outs], ptr(scratch), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_null_outputs_leave_the_others_untouched():
    v, f, xyz = mc.case("prefix259")
    field = _field(v, f)
    x = torch.from_numpy(xyz).cuda()
    M = len(xyz)
    full = _at(field, xyz, "whole")
    keys = ("sdf", "w", "face", "closest")
    nbytes = ctypes.c_size_t()
    assert _native.lib().asdf_mesh_sdf_workspace_bytes(len(f), M, ctypes.byref(nbytes)) == 0
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    for shape in SHAPES:
        with _shape(shape):
            for wanted in ((0,), (1,), (2,), (3,), (0, 3), (1, 2), ()):
                # one allocation, the outputs side by side with guard words between them: a NULL output's neighbours keep every bit
                arena = torch.full((8 * M + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
                views = [arena[16:16 + M], arena[M + 32:2 * M + 32], arena[2 * M + 48:3 * M + 48], arena[3 * M + 64:6 * M + 64]]
                outs = [views[i].view(torch.float32) if i != 2 else views[i] for i in range(4)]
                assert _raw_call(field, x, [outs[i] if i in wanted else None for i in range(4)], scratch) == 0
                host = arena.cpu().numpy()
                written = np.zeros(len(host), bool)
                for i, (lo, n) in enumerate(((16, M), (M + 32, M), (2 * M + 48, M), (3 * M + 64, 3 * M))):
                    if i in wanted:
                        written[lo:lo + n] = True
                        assert np.array_equal(host[lo:lo + n], full[keys[i]].reshape(-1).view(np.int32)), (shape, wanted, keys[i])
                assert (host[~written] == 0x5a5a5a5a).all(), (shape, wanted)


def test_argument_errors_of_the_c_abi():
    L = _native.lib()
    v, f, xyz = mc.case("prefix2")
    field = _field(v, f)
    x = torch.from_numpy(xyz).cuda()
    out = torch.empty(len(xyz), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = ctypes.c_size_t()
    assert L.asdf_mesh_sdf_workspace_bytes(-1, 0, ctypes.byref(n)) == EINVAL and L.asdf_mesh_sdf_workspace_bytes(1, -1, ctypes.byref(n)) == EINVAL
    assert L.asdf_mesh_sdf_workspace_bytes(1, 0, None) == EINVAL
    assert L.asdf_mesh_sdf_workspace_bytes(0, 0, ctypes.byref(n)) == 0 and n.value == 16
    assert L.asdf_mesh_sdf_workspace_bytes(1, 0, ctypes.byref(n)) == 0 and n.value == 16 + _native.MESH_SDF_CHUNK_FACES * _native.MESH_SDF_RECORD_BYTES
    assert L.asdf_mesh_sdf_workspace_bytes(1, 5, ctypes.byref(n)) == 0 and n.value >= 16
    ws, vd, fd = field._ws.data_ptr(), field.verts.data_ptr(), field.faces.data_ptr()
    assert L.asdf_mesh_sdf_prepare(vd, -1, fd, 2, ws, None, st) == EINVAL and L.asdf_mesh_sdf_prepare(vd, len(v), fd, -1, ws, None, st) == EINVAL
    assert L.asdf_mesh_sdf_prepare(vd, len(v), fd, 2, None, None, st) == EINVAL and L.asdf_mesh_sdf_prepare(vd, len(v), None, 2, ws, None, st) == EINVAL
    assert L.asdf_mesh_sdf_prepare(None, len(v), fd, 2, ws, None, st) == EINVAL and L.asdf_mesh_sdf_prepare(vd, len(v), fd, 2, ws + 4, None, st) == EINVAL
    assert L.asdf_mesh_sdf_prepare(vd, len(v), fd, 2, ws, None, st) == 0                      # info is optional
    assert L.asdf_mesh_sdf_points(ws, -1, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL
    assert L.asdf_mesh_sdf_points(ws, 2, x.data_ptr(), -1, out.data_ptr(), None, None, None, None, st) == EINVAL
    assert L.asdf_mesh_sdf_points(None, 2, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL
    assert L.asdf_mesh_sdf_points(ws, 2, None, len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL
    assert L.asdf_mesh_sdf_points(ws, 2, None, 0, None, None, None, None, None, st) == 0        # M = 0
    assert L.asdf_mesh_sdf_points(ws, 2, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == 0      # no scratch: the whole shape
    with _shape("split"):
        assert L.asdf_mesh_sdf_points(ws, 2, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL      # a split needs scratch
    with _shape("diagonal"):
        assert L.asdf_mesh_sdf_points(ws, 2, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL      # no such shape
    top = 2 ** 31 - 1
    assert L.asdf_mesh_sdf_workspace_bytes(top, 0, ctypes.byref(n)) == EINVAL and L.asdf_mesh_sdf_prepare(vd, len(v), fd, top, ws, None, st) == EINVAL
    assert L.asdf_mesh_sdf_points(ws, top, x.data_ptr(), len(xyz), out.data_ptr(), None, None, None, None, st) == EINVAL
    # a split that would take more scratch than the unit allows is not offered: the size call says 16 bytes, the whole shape runs
    assert L.asdf_mesh_sdf_workspace_bytes(4_000_000, 100_000, ctypes.byref(n)) == 0 and n.value == 16
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), _at(field, xyz)["sdf"].view(np.int32))
    # a face count beyond what was prepared reads nothing beyond it
    big = torch.empty(len(xyz), dtype=torch.float32, device="cuda")
    assert L.asdf_mesh_sdf_points(ws, 100000, x.data_ptr(), len(xyz), big.data_ptr(), None, None, None, None, st) == 0
    assert torch.equal(big, out)


# ---- 4. round trip through marching cubes

@pytest.mark.parametrize("N, sample", [(24, 0), (33, 1)])
def test_marching_cubes_round_trip_keeps_every_sign(N, sample):
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.utils.mesh import lattice_points
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / (N - 1)
    idx = np.stack(np.meshgrid(*[np.arange(N, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice_points(torch.from_numpy(idx), origin, voxel).numpy()
    for head, values in zip(("hand", "obj"), syn.grasp_sdf(pts, sample)):
        vol = torch.from_numpy(values.astype(np.float32).reshape(N, N, N)).cuda()
        verts, faces = marching_cubes_device(vol, 0.0)
        field = _field(lattice_points(verts, origin, voxel), faces)
        assert field.info == {"skipped": 0, "zero_area": 0}
        for shape in SHAPES:
            with _shape(shape):
                back = field.volume(origin, voxel, (N, N, N))
            wrong = int(((back < 0) != (vol < 0)).sum())
            print("MESHSDF round trip N %d sample %d %-4s %-5s: %d faces, %d voxels negative, %d signs differ" % (
                N, sample, head, shape, len(faces), int((vol < 0).sum()), wrong))
            assert wrong == 0 and int((vol < 0).sum()) > 0, (head, shape, wrong)


# ---- 5. consumers

def _write_obj(path, verts, faces):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for p in np.asarray(verts, np.float32):
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in p))
        for t in np.asarray(faces):
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


GT_VOXEL, GT_CONTACT = 0.0625, 0.02          # file units = metres here (unit_m 1)


def _gt_pairs():
    """Stand-ins for two synthetic grasps: marching-cubes meshes of synthetic.grasp_sdf have thousands of faces, and the numpy truth
    that every voxel and vertex is held to manages M T <= 2 10^6 - so the "hand" is the 260-face torus and the "object" the box, whose
    enclosed volume is analytic.
    name -> (hand mesh, object mesh): a torus that cuts through a corner region of the box, placed so that the lower corner of the
    boxes' intersection is the torus's (the lattice starts one voxel below that corner: on the box's own planes every voxel would sit
    ON its surface), and the same torus three units away."""
    hv, hf = mc.torus(*mc.TORUS_EDGE)
    bv, bf = mc.box()
    place = lambda t: (hv + np.float32(t)).astype(np.float32)
    return {"apart": (place([3.0, 0.0, 0.0]), hf, bv, bf), "through": (place([0.35, 0.55, 0.3]), hf, bv, bf)}


def test_gt_interaction_flow_equals_the_statements_on_the_truth(tmp_path):
    from alignsdf_amd import gt_interaction as gi
    from alignsdf_amd.mesh_sdf import mesh_bounds
    pairs = _gt_pairs()
    for name, (hv, hf, bv, bf) in pairs.items():
        _write_obj(str(tmp_path / "data" / "obman" / "test" / "mesh_hand" / (name + ".obj")), hv, hf)
        _write_obj(str(tmp_path / "data" / "obman" / "test" / "mesh_obj" / (name + ".obj")), bv, bf)
    gi.main(["-e", str(tmp_path / "exp"), "-t", "obman", "--data_root", str(tmp_path / "data"), "--contact_mm", str(1e3 * GT_CONTACT),
             "--voxel_mm", str(1e3 * GT_VOXEL), "--unit_m", "1.0"])
    body = json.loads((tmp_path / "exp" / "Eval_obman" / "interaction_gt.json").read_text())
    assert (tmp_path / "exp" / "Eval_obman" / "interaction_gt.txt").exists() and [s["name"] for s in body["samples"]] == ["apart", "through"]
    f32 = np.float32
    for rec in body["samples"]:
        hv, hf, bv, bf = pairs[rec["name"]]
        lat = gi.overlap_lattice(mesh_bounds(hv, hf), mesh_bounds(bv, bf), GT_VOXEL)
        assert (lat is None) == (rec["name"] == "apart")
        if lat is None:
            ov = gi.empty_overlap_words()
        else:
            idx = np.stack(np.meshgrid(*[np.arange(n, dtype=f32) for n in lat[1]], indexing="ij"), -1).reshape(-1, 3)
            pts = idx * f32(GT_VOXEL) + np.asarray(lat[0], np.float64).astype(f32)          # lattice_points' fp32 arithmetic
            assert len(pts) * (len(hf) + len(bf)) <= 2_000_000
            th, to = mc.rule(hv, hf, pts), mc.rule(bv, bf, pts)
            assert mc.clear_sign(th).all() and mc.clear_sign(to).all()                      # the truth decides every voxel
            ov = ic.overlap_statement(th["sdf"].reshape(lat[1]), to["sdf"].reshape(lat[1]))
        want = {"overlap": ov}
        values = {"hand": mc.rule(bv, bf, hv), "obj": mc.rule(hv, hf, bv)}                   # each surface's vertices in the OTHER field
        for part, tr in values.items():
            f = tr["sdf"]
            assert mc.clear_sign(tr).all() and (np.abs(f - GT_CONTACT) > mc.D_BOUND).all()     # ... and every vertex's two comparisons
            want[part] = ic.contact_statement(f.astype(f32), GT_CONTACT)
        from alignsdf_amd import interaction as ia
        exp = ia.interaction_record(want, GT_VOXEL, 2.0, GT_CONTACT)
        for key in ("intersection_voxels", "intersection_box", "nan_voxels", "contact", "hand_vertices", "hand_vertices_inside",
                    "hand_vertices_in_contact", "obj_vertices", "obj_vertices_inside", "obj_vertices_in_contact", "nan_vertices", "contact_m"):
            assert rec[key] == exp[key], (rec["name"], key, rec[key], exp[key])
        assert abs(rec["intersection_volume_cm3"] - exp["intersection_volume_cm3"]) <= 1e-9 * max(1.0, exp["intersection_volume_cm3"])
        for key in ("penetration_depth_cm", "penetration_depth_obj_cm", "min_distance_cm"):
            assert abs(rec[key] - exp[key]) <= 100.0 * mc.D_BOUND, (rec["name"], key, rec[key], exp[key])
        # the deepest vertex by value: the truth's value there is the truth's minimum within the bound
        for part, tr in values.items():
            assert abs(tr["sdf"][rec[part + "_deepest_vertex"]] - tr["sdf"].min()) <= 2 * mc.D_BOUND
        assert rec["hand_voxels"] is None and rec["obj_voxels"] is None and rec["skipped_faces"] == 0
        box_cm3 = 8.0 * np.prod(np.float64(mc.BOX_HALF)) * 1e6
        assert abs(rec["obj_volume_cm3"] - box_cm3) <= 1e-12 * box_cm3                       # the box has its analytic volume
        assert rec["hand_volume_cm3"] > 0
    through = body["samples"][1]
    assert through["intersection_voxels"] > 0 and through["hand_vertices_inside"] > 0 and through["contact"] is True
    assert body["samples"][0]["intersection_voxels"] == 0 and body["samples"][0]["contact"] is False
    assert body["summary"]["samples"] == 2 and body["summary"]["contact_ratio"] == 0.5


def test_sdf_samples_are_seeded_and_valued_by_the_field():
    from alignsdf_amd.mesh_sdf import sdf_samples
    v, f = mc.torus(18, 16)
    field = _field(v.astype(np.float64), f.astype(np.int64))
    xyz, sdf = sdf_samples(field, 1500, 500, seed=3)
    xyz2, sdf2 = sdf_samples(_field(v, f), 1500, 500, seed=3)
    assert xyz.shape == (2000, 3) and sdf.shape == (2000,) and xyz.is_cuda and sdf.is_cuda
    assert torch.equal(xyz.view(torch.int32), xyz2.view(torch.int32)) and torch.equal(sdf.view(torch.int32), sdf2.view(torch.int32))
    assert torch.equal(field.at(xyz).sdf.view(torch.int32), sdf.view(torch.int32))
    other = sdf_samples(field, 1500, 500, seed=4)[0]
    assert not torch.equal(other, xyz)
    s = sdf.cpu().numpy()
    near, far = np.abs(s[:1500]), xyz[1500:].cpu().numpy()
    # near the surface: displaced by sigma 0.005 / 0.02 in turn (|sdf| <= the displacement's length); both sides are hit
    assert np.median(near[0::2]) < np.median(near[1::2]) < 0.03 and (s[:1500] < 0).sum() > 300 and (s[:1500] > 0).sum() > 300
    lo, hi = field.bounds()
    pad = 0.05 * (hi - lo)
    assert (far >= lo - pad - 1e-6).all() and (far <= hi + pad + 1e-6).all() and (far.max(0) - far.min(0) > 0.95 * (hi - lo)).all()
    empty = sdf_samples(field, 0, 7, seed=0)
    assert empty[0].shape == (7, 3) and empty[1].shape == (7,)


def test_device_int64_indices_that_do_not_fit_int32_are_bad_indices():
    v, f = mc.box()
    wide = torch.from_numpy(f.astype(np.int64)).cuda()
    wide = torch.cat([wide, torch.tensor([[2 ** 32, 1, 2], [0, 2 ** 32 + 3, 5], [-2 ** 33, 0, 1]], dtype=torch.int64, device="cuda")])
    field = _field(torch.from_numpy(v).cuda(), wide)          # (2^32 would wrap to vertex 0, 2^32 + 3 to vertex 3)
    assert field.info == {"skipped": 3, "zero_area": 0}
    xyz = mc.case("box")[2][:257]
    assert _same_bits(_at(field, xyz), _at(_field(v, f), xyz))


# ---- the fit to (xyz, sdf) samples

def _fit_targets():
    from alignsdf_amd.mesh_sdf import sdf_samples
    out = []
    for head, (v, f) in enumerate(mc.fit_meshes()):
        xyz, sdf = sdf_samples(_field(v, f), mc.FIT_NEAR, mc.FIT_UNIFORM, seed=mc.FIT_SEED + head)
        assert np.array_equal(xyz.cpu().numpy().view(np.int32), mc.fit_points(head).view(np.int32))      # the reference's positions
        out.append((xyz, sdf))
    return out


@pytest.fixture(scope="module")
def fit_decoder():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from tests import sdf_grad_cases as gc
    from tests import sdf_vjp_cases as vc
    hip = HipSdfDecoder(gc.module_for(vc.FIT_TAG))
    yield hip
    hip.close()


@pytest.mark.parametrize("path", ["native", "module"])
def test_fit_to_sdf_samples_of_the_ground_truth_meshes(path, fit_decoder):
    """fit_sample's defaults (40 steps, lr 2e-3, prior 1e-3, clamp 0.05) with sdf_hand / sdf_obj alone: 384 near-surface and 128 uniform
    (xyz, sdf) samples per head around the ground-truth meshes of the scene the decoder was trained on, from the start of
    tests/test_gpu_sdf_vjp.py's fit (code moved by 0.3 |z|, heads shifted by 0.03).  The reference, the same fit in fp64 on the CPU
    through the package's module (mesh_sdf_cases.fit_reference_fp64; tests/test_mesh_sdf_truth.py holds the figure): loss 3.627e-2 ->
    8.520e-3, ratio 0.235 (0.215 at lr 5e-3).  The bound is that plus the existing fit test's margin over its reference
    (0.25 - 0.055): 0.43."""
    from alignsdf_amd.fit import fit_sample
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from tests import sdf_grad_cases as gc
    from tests import sdf_vjp_cases as vc
    z0, E0 = mc.fit_start()
    hand, obj = _fit_targets()
    dec = fit_decoder if path == "native" else TorchModuleDecoder(gc.module_for(vc.FIT_TAG), syn.specs_for(vc.FIT_TAG), "fit on the module path")
    z, E, shifts, history = fit_sample(dec, z0, E0, sdf_hand=hand, sdf_obj=obj)
    ratio = history[-1] / history[0]
    print("MESHSDF fit %-6s loss %.3e -> %.3e ratio %.3f (fp64 reference %.3f, bound %.3f) | history %s" % (
        path, history[0], history[-1], ratio, mc.FIT_REFERENCE_RATIO, mc.FIT_RATIO_BOUND, " ".join("%.2e" % v for v in history[::5])))
    assert len(history) == 40 and ratio <= mc.FIT_RATIO_BOUND, (path, history[0], history[-1])
    assert abs(history[0] - 3.627e-2) <= 1e-3                              # the same start and the same targets as the reference


def _fit_sample_before(decoder, latent, embed, surface_hand, surface_obj, steps, lr=2e-3, prior=1e-3):
    """fit.fit_sample as it was before it took (xyz, sdf) targets (both surfaces given, no penetration term), statement for statement."""
    from alignsdf_amd.fit import sdf_at_points, shift_embed
    dev = decoder.device
    z0 = latent.detach().reshape(-1).to(dev, torch.float32)
    z = z0.clone().requires_grad_()
    E0 = [e.detach().to(dev, torch.float32) for e in embed]
    shifts = torch.zeros(2, 3, dtype=torch.float32, device=dev, requires_grad=True)
    sets = [s.detach().to(dev, torch.float32).reshape(-1, 3) for s in (surface_hand, surface_obj)]
    pts = torch.cat(sets, 0)
    n_hand = sets[0].shape[0]
    opt = torch.optim.Adam([z, shifts], lr=lr)
    history = []
    for _ in range(steps):
        opt.zero_grad()
        E = (shift_embed(E0[0], shifts[0]), shift_embed(E0[1], shifts[1]))
        f_hand, f_obj = sdf_at_points(decoder, z, E, pts)
        data = torch.zeros((), dtype=torch.float32, device=dev)
        data = data + f_hand[:n_hand].abs().mean()
        data = data + f_obj[n_hand:].abs().mean()
        loss = data + prior * ((z - z0) ** 2).mean()
        history.append(data.detach())
        loss.backward()
        opt.step()
    E = tuple(shift_embed(E0[h], shifts[h]).detach() for h in range(2))
    return z.detach(), E, shifts.detach(), [float(v) for v in torch.stack(history).cpu()]


def test_fit_without_the_new_arguments_returns_what_it_returned_before(fit_decoder):
    from alignsdf_amd.fit import fit_sample
    from tests import sdf_vjp_cases as vc
    z0, E0, sh, so = vc.fit_scenario(fit_decoder)
    want = _fit_sample_before(fit_decoder, z0, E0, sh, so, steps=8)
    got = fit_sample(fit_decoder, z0, E0, sh, so, steps=8)
    assert torch.equal(want[0], got[0]) and torch.equal(want[2], got[2]) and want[3] == got[3]
    assert all(torch.equal(a, b) for a, b in zip(want[1], got[1]))
    with pytest.raises(ValueError):
        fit_sample(fit_decoder, z0, E0)
