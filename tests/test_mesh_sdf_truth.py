"""The mesh signed distance unit without a GPU (csrc/mesh_sdf.hip, alignsdf_amd/mesh_sdf.py, alignsdf_amd/gt_interaction.py):

  - the fp32 model of the rule against its fp64 truth on every case of tests/mesh_sdf_cases.py: its maxima are the constants the GPU's
    bounds are 4 x of (every line printed with the prefix MESHSDF is one case; profiles/mesh_sdf_fp64_errors.txt),
  - the compile-time budget of the kernels, read from the compiler's resource remarks,
  - the C ABI's bookkeeping: exports, SOURCES, the constants of header and bindings,
  - the host functions of the ground-truth interaction flow.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alignsdf_amd import _native
from tests import mesh_sdf_cases as mc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alignsdf_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "alignsdf_hip.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the model against the truth

@pytest.mark.parametrize("name", mc.CASES)
def test_fp32_model_stays_within_its_recorded_maxima(name):
    v, f, xyz = mc.case(name)
    assert len(xyz) * len(f) <= 2_000_000
    tr, mo = mc.truth(name), mc.model(name)
    off = mc.off_surface(tr)
    e_d = np.abs(mo["d"].astype(np.float64) - tr["d"]).max()
    e_w = np.abs(mo["w"].astype(np.float64) - tr["w"])[off].max()
    print("MESHSDF model %-13s T %4d M %5d | max |dd| %.2e  max |dw| %.2e (off the surface: %d of %d) | sign left out %d" % (
        name, len(f), len(xyz), e_d, e_w, off.sum(), len(xyz), (off & ~mc.clear_sign(tr)).sum()))
    assert e_d <= mc.MODEL_MAX_D and e_w <= mc.MODEL_MAX_W
    # the model meets the yardsticks the GPU is held to (signs, face by value, closest) - the cases are fair
    mc.compare(name, {"sdf": mo["sdf"], "w": mo["w"], "face": mo["face"], "closest": mo["closest"]}, "model")


def test_bounds_are_four_times_the_model_maxima():
    assert mc.D_BOUND == 4.0 * mc.MODEL_MAX_D and mc.W_BOUND == 4.0 * mc.MODEL_MAX_W
    assert mc.FACE_COUNTS == (1, 2, mc.BLOCK - 1, mc.BLOCK, mc.BLOCK + 1, mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1, 2 * mc.CHUNK + 3)
    assert len(set(mc.FACE_COUNTS)) == 9 and mc.CHUNK % mc.BLOCK == 0


def test_closed_meshes_leave_no_off_surface_sign_out():
    for name in ("box", "torus", "torus_inward", "box_flat"):
        tr = mc.truth(name)
        off = mc.off_surface(tr)
        assert (np.abs(np.abs(tr["w"][off]) - 0.5) > 0.49).all(), name          # |w| is 0 or 1 off a closed surface
    inward, outward = mc.truth("torus_inward"), mc.truth("torus")
    assert np.array_equal(inward["sdf"], outward["sdf"]) and np.array_equal(inward["w"], -outward["w"])


def test_rule_edges_in_numpy():
    v, f = mc.box()
    q = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.5, 0.375, 0.25]], np.float32)
    r = mc.rule(v, f, q)
    assert r["sdf"][0] == -0.25 and r["sdf"][1] == 1.5 and np.isnan(r["sdf"][2]) and r["face"][2] == -1 and r["d"][3] == 0.0
    bad = np.concatenate([f, [[0, 1, 99], [-1, 2, 3]]]).astype(np.int32)
    rb = mc.rule(v, bad, q)
    assert rb["skipped"] == 2 and np.array_equal(rb["sdf"][:2], r["sdf"][:2])
    none = mc.rule(v, bad[-2:], q)
    assert np.isinf(none["sdf"][0]) and none["sdf"][0] > 0 and none["w"][0] == 0 and none["face"][0] == -1 and np.isnan(none["closest"][0]).all()
    vf, ff = mc.box_with_flat_faces()
    rf = mc.rule(vf, ff, np.array([[1.25, 0.0, 0.0], [2.5, 0.0, 0.0], [0.0, 1.125, 0.25]], np.float32))
    assert rf["zero_area"] == 3 and list(rf["d"]) == [0.0, 0.5, 0.125] and list(rf["face"]) == [12, 12, 13]
    assert np.array_equal(rf["w"], mc.rule(*mc.box(), np.array([[1.25, 0.0, 0.0], [2.5, 0.0, 0.0], [0.0, 1.125, 0.25]], np.float32))["w"])


# ---- the kernels' compile-time budget

KERNELS = ("mesh_sdf_prepare_kernel", "mesh_sdf_pair_kernel", "mesh_sdf_combine_kernel")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "mesh_sdf.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "mesh_sdf.hip" in SOURCES and "-ffp-contract=off" in FLAGS and "mesh_sdf.hip" not in TU_FLAGS          # the common flags
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "mesh_sdf.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return proc.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("kernel", KERNELS)
def test_mesh_sdf_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    blocks = [b for b in re.split(r"remark: Function Name: ", remarks)[1:] if kernel in b.split()[0]]
    assert len(blocks) == {"mesh_sdf_prepare_kernel": 1, "mesh_sdf_pair_kernel": 4, "mesh_sdf_combine_kernel": 2}[kernel]
    for block in blocks:
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        assert get(r"ScratchSize \[bytes/lane\]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0
        assert get("AGPRs") == 0 and get("VGPRs") <= 96 and get(r"Occupancy \[waves/SIMD\]") >= 5
        lds = get(r"LDS Size \[bytes/block\]")
        assert lds == (_native.MESH_SDF_BLOCK_FACES * _native.MESH_SDF_RECORD_BYTES if kernel == "mesh_sdf_pair_kernel" else 0)


# ---- bookkeeping

def test_exports_sources_and_constants():
    names = {"asdf_mesh_sdf_workspace_bytes", "asdf_mesh_sdf_prepare", "asdf_mesh_sdf_points"}
    assert names <= set(_native.EXPORTS) and _native.ABI_VERSION == 132
    from alignsdf_amd.build_native import SOURCES
    assert "mesh_sdf.hip" in SOURCES
    with open(HEADER) as fh:
        text = fh.read()
    for n in names:
        assert "int %s(" % n in text
    found = {n: int(v) for n, v in re.findall(r"^#define ASDF_(MESH_SDF_\w+)\s+(\d+)\s*$", text, flags=re.M)}
    assert len(found) == 10
    for n, v in found.items():
        assert getattr(_native, n) == v, n
    assert found["MESH_SDF_CHUNK_FACES"] % found["MESH_SDF_BLOCK_FACES"] == 0 and found["MESH_SDF_RECORD_BYTES"] % 16 == 0


def test_fit_reference_ratio_is_the_recorded_one():
    """The fp64 fit to (xyz, sdf) samples on the CPU (mesh_sdf_cases.fit_reference_fp64): the ratio the GPU fits' bound is built on."""
    history = mc.fit_reference_fp64()
    ratio = history[-1] / history[0]
    print("MESHSDF fit fp64 reference: loss %.3e -> %.3e ratio %.3f" % (history[0], history[-1], ratio))
    assert len(history) == 40 and abs(ratio - mc.FIT_REFERENCE_RATIO) <= 0.005
    assert mc.FIT_RATIO_BOUND < 0.5


# ---- the host side of the ground-truth interaction flow

def test_discovery_takes_the_names_that_exist_as_a_pair(tmp_path):
    from alignsdf_amd import gt_interaction as gi
    base = tmp_path / "data" / "obman" / "test"
    for sub, names in (("mesh_hand", ("b", "a", "only_hand", "c.txt")), ("mesh_obj", ("a", "b", "only_obj"))):
        (base / sub).mkdir(parents=True)
        for n in names:
            (base / sub / (n if "." in n else n + ".obj")).write_text("")
    found = gi.discover(str(tmp_path / "data"), "obman")
    assert [n for n, _, _ in found] == ["a", "b"]
    assert found[0][1].endswith(os.path.join("mesh_hand", "a.obj")) and found[0][2].endswith(os.path.join("mesh_obj", "a.obj"))
    assert gi.discover(str(tmp_path / "data"), "dexycb") == []


def test_overlap_lattice_covers_the_intersection_grown_by_one_voxel():
    from alignsdf_amd import gt_interaction as gi
    a = (np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0]))
    b = (np.array([0.5, -1.0, 0.25]), np.array([2.0, 0.5, 0.5]))
    origin, dims = gi.overlap_lattice(a, b, 0.125)
    assert origin == [0.375, -0.125, 0.125] and dims == [7, 7, 5]
    last = np.array(origin) + (np.array(dims) - 1) * 0.125
    assert (last >= np.array([1.0, 0.5, 0.5]) + 0.125 - 1e-12).all()
    origin, dims = gi.overlap_lattice(a, b, 0.1)                       # a spacing that does not divide the box
    assert (np.array(origin) + (np.array(dims) - 1) * 0.1 >= np.array([1.0, 0.5, 0.5]) + 0.1 - 1e-12).all()
    assert gi.overlap_lattice(a, (np.array([1.5, 0, 0]), np.array([2.0, 1, 1])), 0.125) is None          # apart along one axis
    touching = gi.overlap_lattice(a, (np.array([1.0, 0, 0]), np.array([2.0, 1, 1])), 0.125)            # a shared face is an intersection
    assert touching is not None and touching[1][0] == 3


def test_enclosed_volume_of_a_box_is_analytic():
    from alignsdf_amd.mesh_sdf import enclosed_volume, mesh_bounds
    half = np.array([0.37, 0.211, 0.153])
    v, f = mc.box()
    verts = v.astype(np.float64) / np.array(mc.BOX_HALF) * half + np.array([0.3, -0.2, 0.7])
    want = 8.0 * half.prod()
    assert abs(enclosed_volume(verts, f) - want) <= 1e-12 * want
    assert abs(enclosed_volume(verts, f[:, ::-1]) - want) <= 1e-12 * want          # either orientation
    bad = np.concatenate([f, [[0, 1, 99]]])
    assert abs(enclosed_volume(verts, bad) - want) <= 1e-12 * want                 # absent faces are left out
    lo, hi = mesh_bounds(verts, f)
    assert np.allclose(hi - lo, 2 * half, rtol=0, atol=1e-15)


def test_gt_record_and_json_layout(tmp_path):
    from alignsdf_amd import gt_interaction as gi
    from alignsdf_amd import interaction as ia
    N = _native
    ov = gi.empty_overlap_words()
    assert ia.interaction_record({"overlap": ov, "hand": None, "obj": None}, 0.01, 2.0, 0.005)["intersection_box"] is None
    ov[[N.OVERLAP_HAND, N.OVERLAP_OBJ, N.OVERLAP_BOTH]] = 40, 30, 5
    ov[N.OVERLAP_MIN:N.OVERLAP_MIN + 3], ov[N.OVERLAP_MAX:N.OVERLAP_MAX + 3] = (1, 2, 3), (2, 3, 4)
    contact = lambda n, inside, near, low, arg: np.array([n, inside, near, 0, np.array([low], np.float32).view(np.int32)[0], arg, 0, 0], np.int32)
    words = {"overlap": ov, "hand": contact(778, 3, 9, -0.004, 17), "obj": contact(500, 0, 2, 0.001, 4)}
    # files in millimetres: unit_m = 1e-3, voxel 2 mm = 2 file units
    rec = gi.gt_record(words, 2.0, 1e-3, 0.005, hand_volume=350e3, obj_volume=120e3)
    assert rec["hand_voxels"] is None and rec["obj_voxels"] is None and rec["intersection_voxels"] == 5
    assert abs(rec["intersection_volume_cm3"] - 5 * 0.008) < 1e-12 and abs(rec["hand_volume_cm3"] - 350.0) < 1e-9
    assert abs(rec["obj_volume_cm3"] - 120.0) < 1e-9 and abs(rec["penetration_depth_cm"] - 0.0004) < 1e-9 and rec["contact"] is True
    samples = [dict({"index": 0, "name": "a"}, **rec), dict({"index": 1, "name": "b"}, **gi.gt_record(
        {"overlap": gi.empty_overlap_words(), "hand": contact(10, 0, 0, 9.0, 2), "obj": contact(10, 0, 0, 9.5, 1)}, 2.0, 1e-3, 0.005, 1.0, 1.0))]
    out = tmp_path / "Eval_obman"
    path, summary, line = gi.write_outputs(str(out), samples, 0.005, 0.002, 1e-3)
    assert line is None and os.path.basename(path) == "interaction_gt.json" and (out / "interaction_gt.txt").exists()
    body = json.loads((out / "interaction_gt.json").read_text())
    assert set(body) == {"summary", "contact_m", "voxel_m", "unit_m", "samples"} and body["summary"] == summary
    assert summary["samples"] == 2 and summary["contact_ratio"] == 0.5 and [s["name"] for s in body["samples"]] == ["a", "b"]
    assert "samples:2" in (out / "interaction_gt.txt").read_text()
    # with a prediction run's interaction.json next to it: one line that compares the two summaries
    (out / "interaction.json").write_text(json.dumps({"summary": {"samples": 2, "mean_penetration_depth_cm": 0.5,
                                                                  "mean_intersection_volume_cm3": 1.25, "contact_ratio": 1.0}}))
    line = gi.write_outputs(str(out), samples, 0.005, 0.002, 1e-3)[2]
    assert line.startswith("ground truth vs prediction") and "0.5000" in line and "1.000" in line
