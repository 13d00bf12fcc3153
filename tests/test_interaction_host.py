"""The host side of the interaction metrics (alignsdf_amd/interaction.py), without a GPU: units, records, summaries and merges, the
command-line flags, the `quality` column of the PLY files, and the numpy statements the GPU tests hold the kernels to."""
import argparse
import json
import os

import numpy as np
import pytest

from alignsdf_amd import _native
from alignsdf_amd import interaction as ia
from alignsdf_amd.ply import read_ply, write_ply
from tests import interaction_cases as ic

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "alignsdf_hip.h")


def _bits(x):
    return int(np.array([x], np.float32).view(np.int32)[0])


def _words(both=8, hand=100, obj=50, nan=0, lo=(1, 2, 3), hi=(2, 3, 4), hand_rec=(10, 3, 4, 0, -0.004, 7), obj_rec=(20, 0, 1, 0, 0.001, 2)):
    ov = np.zeros(16, np.int32)
    ov[:4] = hand, obj, both, nan
    ov[4:7], ov[7:10] = lo, hi
    pts = lambda r: None if r is None else np.array([r[0], r[1], r[2], r[3], _bits(r[4]), r[5], 0, 0], np.int32)
    return {"overlap": ov, "hand": pts(hand_rec), "obj": pts(obj_rec)}


# ---- units and records ------------------------------------------------------------------------------------------------------------------
def test_unit_conversion_by_hand():
    """SdfScaleFactor 7: one normalised unit is 2 / 7 m.  A fine voxel of 0.014 normalised is 0.4 cm, so 8 voxels are 8 x 0.064 = 0.512
    cm^3; a minimum of -0.0035 normalised is a depth of 0.1 cm; tau for 5 mm is 0.005 x 7 / 2 = 0.0175."""
    w = _words(both=8, hand=1000, obj=125, hand_rec=(10, 3, 4, 0, -0.0035, 7), obj_rec=(20, 0, 1, 0, 0.00175, 2))
    r = ia.interaction_record(w, 0.014, 7.0, 0.005)
    assert r["intersection_volume_cm3"] == pytest.approx(0.512, rel=1e-12) and r["hand_volume_cm3"] == pytest.approx(64.0, rel=1e-12)
    assert r["obj_volume_cm3"] == pytest.approx(8.0, rel=1e-12)
    assert r["penetration_depth_cm"] == pytest.approx(0.1, rel=1e-6) and r["penetration_depth_obj_cm"] == 0.0
    assert r["min_distance_cm"] == pytest.approx(-0.1, rel=1e-6) and r["contact"] is True and r["contact_m"] == 0.005
    assert (r["intersection_voxels"], r["hand_voxels"], r["obj_voxels"], r["nan_voxels"], r["nan_vertices"]) == (8, 1000, 125, 0, 0)
    assert (r["hand_vertices"], r["hand_vertices_inside"], r["hand_vertices_in_contact"], r["hand_deepest_vertex"]) == (10, 3, 4, 7)
    assert (r["obj_vertices"], r["obj_vertices_inside"], r["obj_vertices_in_contact"], r["obj_deepest_vertex"]) == (20, 0, 1, 2)
    assert r["intersection_box"] == [[1, 2, 3], [2, 3, 4]]
    assert ia.contact_tau(0.005, 7.0) == pytest.approx(0.0175, rel=1e-12)
    json.dumps(r)                                  # a plain dict


def test_record_of_a_missing_surface_and_of_nans():
    # no hand surface (marching-cubes error): its vertex fields are None, contact comes from the object's vertices
    r = ia.interaction_record(_words(hand_rec=None, obj_rec=(20, 2, 5, 0, -0.01, 4)), 0.01, 2.0, 0.005)
    assert r["penetration_depth_cm"] is None and r["hand_vertices"] is None and r["hand_vertices_inside"] is None
    assert r["hand_vertices_in_contact"] is None and r["penetration_depth_obj_cm"] == pytest.approx(1.0, rel=1e-6)
    assert r["contact"] is True and r["min_distance_cm"] == pytest.approx(-1.0, rel=1e-6)
    # neither: nothing to touch with
    r = ia.interaction_record(_words(hand_rec=None, obj_rec=None), 0.01, 2.0, 0.005)
    assert r["contact"] is False and r["min_distance_cm"] is None and r["penetration_depth_obj_cm"] is None
    # apart: positive minima, no vertex within tau
    r = ia.interaction_record(_words(both=0, lo=(ic.INT_MAX,) * 3, hi=(-1,) * 3, hand_rec=(5, 0, 0, 0, 0.3, 1), obj_rec=(6, 0, 0, 0, 0.2, 0)), 0.01, 2.0, 0.005)
    assert r["contact"] is False and r["penetration_depth_cm"] == 0.0 and r["min_distance_cm"] == pytest.approx(20.0, rel=1e-6)
    assert r["intersection_box"] is None and r["intersection_volume_cm3"] == 0.0
    # NaNs are counted and do not poison the figures; a list of NaNs alone has no minimum
    w = _words(nan=3, hand_rec=(4, 0, 0, 4, np.inf, -1), obj_rec=(9, 1, 1, 2, -0.002, 3))
    r = ia.interaction_record(w, 0.01, 2.0, 0.005)
    assert r["nan_voxels"] == 3 and r["nan_vertices"] == 6 and r["penetration_depth_cm"] == 0.0 and r["hand_deepest_vertex"] is None
    assert r["min_distance_cm"] == pytest.approx(-0.2, rel=1e-6) and r["contact"] is True
    json.dumps(r)
    # split_words: the pipeline's 32 words
    flat = np.concatenate([w["overlap"], w["hand"], w["obj"]])
    assert len(flat) == ia.WORDS == 32
    s = ia.split_words(flat, ["obj"])
    assert s["hand"] is None and np.array_equal(s["obj"], w["obj"]) and np.array_equal(s["overlap"], w["overlap"])


def _sample(index, depth, volume, contact, name=None):
    return {"index": index, "name": name or "%08d" % index, "interaction": {
        "penetration_depth_cm": depth, "intersection_volume_cm3": volume, "contact": contact, "min_distance_cm": None if depth is None else -depth}}


def test_summarise():
    recs = [_sample(0, 0.5, 2.0, True), _sample(1, 0.0, 0.0, False), _sample(2, None, 1.0, True), {"index": 3, "name": "x"}]
    s = ia.summarise(recs)
    assert s == {"samples": 3, "mean_penetration_depth_cm": 0.25, "mean_intersection_volume_cm3": 1.0, "contact_ratio": pytest.approx(2 / 3)}
    assert ia.summarise([r["interaction"] for r in recs[:2]])["samples"] == 2
    empty = ia.summarise([])
    assert empty == {"samples": 0, "mean_penetration_depth_cm": None, "mean_intersection_volume_cm3": None, "contact_ratio": None}
    assert "n/a" in ia.summary_line(empty) and "3 samples" in ia.summary_line(s) and "0.2500" in ia.summary_line(s)


def test_shard_files_and_merge(tmp_path):
    out = str(tmp_path)
    assert ia.merge_interaction_json(out) is None and os.listdir(out) == []          # a run without the option: nothing is written
    ia.write_interaction_json(out, 0, 2, [_sample(0, 0.5, 2.0, True), _sample(1, 0.1, 0.5, False)], 0.005)
    ia.write_interaction_json(out, 2, 5, [_sample(3, 0.9, 4.0, True), {"index": 4, "name": "none"}], 0.005)
    ia.write_interaction_json(out, 7, 9, [_sample(8, 9.0, 9.0, True)], 0.005, stride=2)          # an earlier run's shard
    body = json.load(open(os.path.join(out, "interaction_2_5.json")))
    assert body["range"] == [2, 5] and body["contact_m"] == 0.005 and [s["index"] for s in body["samples"]] == [3]
    assert json.load(open(os.path.join(out, "interaction_7_9.json")))["stride"] == 2
    # --merge-only: the ranges of THIS run only, a missing shard counted
    path = ia.merge_interaction_json(out, ranges=[(0, 2), (2, 5), (5, 7)])
    merged = json.load(open(path))
    assert os.path.basename(path) == "interaction.json" and merged["shards_missing"] == 1 and merged["contact_m"] == 0.005
    assert [s["index"] for s in merged["samples"]] == [0, 1, 3] and merged["summary"]["samples"] == 3
    assert merged["summary"]["mean_penetration_depth_cm"] == pytest.approx(0.5) and merged["summary"]["contact_ratio"] == pytest.approx(2 / 3)
    lines = open(os.path.join(out, "interaction.txt")).read().splitlines()
    assert lines[0].startswith("summary of interaction")
    assert [l.split(",")[0] for l in lines[1:4]] == ["00000003", "00000000", "00000001"]          # by decreasing penetration depth
    assert lines[4] == "mean penetration depth:0.5" and lines[5].startswith("mean intersection volume:") and lines[6].startswith("contact ratio:")
    assert lines[7] == "samples:3"
    # every shard present
    assert json.load(open(ia.merge_interaction_json(out)))["summary"]["samples"] == 4
    assert not [n for n in os.listdir(out) if ".tmp" in n]


def test_merge_only_of_dist_reconstruct_merges_the_interaction_shards(tmp_path, capsys):
    from alignsdf_amd import dist_reconstruct as dr
    exp = tmp_path / "exp"
    out = exp / "Eval_obman"
    os.makedirs(out)
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["rgb/%08d.jpg" % i for i in range(4)]}, fh)
    for a, b in ((0, 2), (2, 4)):
        dr.write_shard_records(str(out), a, b, a // 2, [{"index": i, "name": "%08d" % i, "V_hand": 1, "F_hand": 1, "V_obj": 1, "F_obj": 1,
                                                        "milliseconds": 1.0} for i in range(a, b)])
        ia.write_interaction_json(str(out), a, b, [_sample(i, 0.1 * (i + 1), 1.0, i != 3) for i in range(a, b)], 0.005)
    ia.write_interaction_json(str(out), 0, 4, [_sample(0, 50.0, 50.0, True)], 0.005)          # (a one-rank run's leftover: not merged)
    with pytest.raises(SystemExit) as e:
        dr.main(["-e", str(exp), "--split", split, "--merge-only", "2"])
    assert e.value.code == 0
    merged = json.load(open(out / "interaction.json"))
    assert [s["index"] for s in merged["samples"]] == [0, 1, 2, 3] and merged["summary"]["contact_ratio"] == 0.75
    assert merged["summary"]["mean_penetration_depth_cm"] == pytest.approx(0.25)
    printed = capsys.readouterr().out
    assert "interaction: 4 samples" in printed and os.path.exists(out / "interaction.txt")


def test_flag_parsing():
    from alignsdf_amd import reconstruct as rc
    p = argparse.ArgumentParser()
    rc.add_interaction_arguments(p)
    off = p.parse_args([])
    assert off.interaction is False and off.contact_mm == 5.0 and rc.interaction_from_args(off) == {}
    on = p.parse_args(["--interaction"])
    assert rc.interaction_from_args(on) == {"interaction": {"contact_m": 0.005}}
    assert rc.interaction_from_args(p.parse_args(["--interaction", "--contact_mm", "2.5"])) == {"interaction": {"contact_m": 0.0025}}
    # the option itself: a branch switched off, a negative distance
    both = {"SdfScaleFactor": 7.0}
    assert ia.check_option({"contact_m": 0.01}, both) == 0.01 and ia.check_option(True, both) == ia.DEFAULT_CONTACT_M == 0.005
    for specs in ({"HandBranch": False}, {"ObjectBranch": False}):
        with pytest.raises(ValueError):
            ia.check_option({"contact_m": 0.005}, specs)
    with pytest.raises(ValueError):
        ia.check_option({"contact_m": -1.0}, both)
    with pytest.raises(ValueError):
        ia.check_option({"contact_m": float("nan")}, both)


def test_a_branch_switched_off_raises_before_anything_is_asked_of_the_decoder():
    from alignsdf_amd.sample_pipeline import pipelined_two_pass

    def samples():
        raise AssertionError("a sample was fetched")
        yield

    for specs in ({"HandBranch": False, "SdfScaleFactor": 7.0}, {"ObjectBranch": False, "SdfScaleFactor": 7.0}):
        with pytest.raises(ValueError):
            next(pipelined_two_pass(object(), specs, samples(), 32, host_copy=True, interaction={"contact_m": 0.005}))
    # without host_copy there are no kept vertices to measure: an error, not a run that quietly reports nothing
    with pytest.raises(ValueError, match="host_copy"):
        next(pipelined_two_pass(object(), {"SdfScaleFactor": 7.0}, samples(), 32, interaction={"contact_m": 0.005}))


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------
V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5], [0.25, -2, 3]], np.float32)
F = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
NRM = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]], np.float32)
# what write_ply(path, V, F) and write_ply(path, V, F, NRM) wrote before the `quality` column existed
PLAIN_BYTES = (b'ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n'
               b'property list uchar int vertex_indices\nend_header\n'
               b'\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?'
               b'\x00\x00\x00?\x00\x00\x80>\x00\x00\x00\xc0\x00\x00@@'
               b'\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00\x03\x02\x00\x00\x00\x01\x00\x00\x00\x03\x00\x00\x00')
NORMALS_BYTES = (b'ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n'
                 b'property float ny\nproperty float nz\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n'
                 b'\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?'
                 b'\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00\x00'
                 b'\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00?\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00\x00'
                 b'\x00\x00\x80>\x00\x00\x00\xc0\x00\x00@@\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80\xbf'
                 b'\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00\x03\x02\x00\x00\x00\x01\x00\x00\x00\x03\x00\x00\x00')


def test_files_without_quality_are_byte_identical_to_the_earlier_writer(tmp_path):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_ply(a, V, F)
    write_ply(b, V, F, NRM)
    assert open(a, "rb").read() == PLAIN_BYTES and open(b, "rb").read() == NORMALS_BYTES
    write_ply(a, V, F, None, None)
    assert open(a, "rb").read() == PLAIN_BYTES


def test_quality_round_trip_in_both_layouts(tmp_path):
    q = np.array([-0.004, 0.0, 0.0125, np.inf], np.float32)
    plain, withn = str(tmp_path / "q.ply"), str(tmp_path / "nq.ply")
    write_ply(plain, V, F, quality=q)
    write_ply(withn, V, F, NRM, q)
    head = open(withn, "rb").read().split(b"end_header\n")[0].decode().splitlines()
    assert head[3:10] == ["property float " + k for k in ("x", "y", "z", "nx", "ny", "nz", "quality")]
    assert open(plain, "rb").read().split(b"end_header\n")[0].decode().splitlines()[3:7] == ["property float " + k for k in ("x", "y", "z", "quality")]
    for path, normals in ((plain, None), (withn, NRM)):
        v, f = read_ply(path)                                   # the two-value form keeps working on both layouts
        assert np.array_equal(v, V) and np.array_equal(f, F)
        v, f, n = read_ply(path, with_normals=True)
        assert np.array_equal(v, V) and (n is None if normals is None else np.array_equal(n, normals))
        v, f, n, got = read_ply(path, with_normals=True, with_quality=True)
        assert np.array_equal(f, F) and got.dtype == np.float32 and np.array_equal(got, q)
        assert np.array_equal(read_ply(path, with_quality=True)[2], q)
    old = str(tmp_path / "old.ply")
    with open(old, "wb") as fh:
        fh.write(NORMALS_BYTES)
    v, f, n, got = read_ply(old, with_normals=True, with_quality=True)
    assert got is None and np.array_equal(n, NRM) and np.array_equal(v, V)
    with pytest.raises(ValueError):
        write_ply(plain, V, F, quality=q[:3])


# ---- the record layout and the numpy statements ------------------------------------------------------------------------------------------
def test_record_words_are_named_once_in_the_header_and_mirrored():
    import re
    text = open(HEADER).read()
    found = {name: int(value) for name, value in re.findall(r"^#define ASDF_((?:OVERLAP|CONTACT)_\w+)\s+(\d+)\s", text, flags=re.M)}
    assert found == {"OVERLAP_HAND": 0, "OVERLAP_OBJ": 1, "OVERLAP_BOTH": 2, "OVERLAP_NAN": 3, "OVERLAP_MIN": 4, "OVERLAP_MAX": 7,
                     "OVERLAP_WORDS": 16, "CONTACT_COUNT": 0, "CONTACT_INSIDE": 1, "CONTACT_NEAR": 2, "CONTACT_NAN": 3,
                     "CONTACT_MIN_BITS": 4, "CONTACT_ARGMIN": 5, "CONTACT_WORDS": 8}
    for name, value in found.items():
        assert getattr(_native, name) == value, name
    assert _native.ABI_VERSION == 132 and {"asdf_interaction_lattice", "asdf_interaction_points"} <= set(_native.EXPORTS)
    from alignsdf_amd.build_native import SOURCES
    assert "interaction.hip" in SOURCES


def test_overlap_statement_on_hand_made_volumes():
    a = np.array([[[-1.0, 2.0], [-0.0, -3.0]], [[np.nan, -1.0], [-1e-40, 5.0]]], np.float32)
    b = np.array([[[-2.0, -1.0], [-1.0, 1.0]], [[-1.0, np.nan], [-np.inf, np.inf]]], np.float32)
    # hand negative: (0,0,0) (0,1,1) (1,0,1) (1,1,0) - not -0.0, not NaN;  object: (0,0,0) (0,0,1) (0,1,0) (1,0,0) (1,1,0)
    # both: (0,0,0) and (1,1,0);  NaN in either: (1,0,0) (1,0,1)
    assert ic.overlap_statement(a, b).tolist() == [4, 5, 2, 2, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    apart = ic.overlap_statement(np.abs(a), b)
    assert apart.tolist() == [0, 5, 0, 2] + [ic.INT_MAX] * 3 + [-1] * 3 + [0] * 6
    every = ic.overlap_statement(-np.ones((2, 2, 2), np.float32), -np.ones((2, 2, 2), np.float32))
    assert every.tolist() == [8, 8, 8, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_contact_statement_on_hand_made_lists():
    f = np.array([0.5, -0.25, np.nan, -0.25, 0.01], np.float32)
    tau = 0.01
    assert ic.contact_statement(f, tau).tolist() == [5, 2, 3, 1, _bits(-0.25), 1, 0, 0]          # the tie goes to index 1; f == tau counts
    assert ic.contact_statement(f, np.nextafter(np.float32(tau), np.float32(-1))).tolist()[2] == 2
    assert ic.contact_statement(f, tau, count=1).tolist() == [1, 0, 0, 0, _bits(0.5), 0, 0, 0]
    assert ic.contact_statement(f, tau, count=-3).tolist() == [0, 0, 0, 0, ic.INF_BITS, -1, 0, 0]
    assert ic.contact_statement(f, tau, count=99).tolist() == ic.contact_statement(f, tau).tolist()
    assert ic.contact_statement(np.full(5, np.nan, np.float32), tau).tolist() == [5, 0, 0, 5, ic.INF_BITS, -1, 0, 0]
    zeros = np.array([0.0, -0.0, 0.0, -0.0, 1.0], np.float32)
    assert ic.contact_statement(zeros, 0.0).tolist() == [5, 0, 4, 0, _bits(-0.0), 1, 0, 0]      # -0.0 is not negative, and below +0.0
    assert ic.contact_statement(np.array([np.inf, np.inf], np.float32), 0.0).tolist() == [2, 0, 0, 0, ic.INF_BITS, 0, 0, 0]


def test_generators_carry_the_special_values():
    v = ic.mixed_volume((33, 33, 33), 5)
    assert v.dtype == np.float32 and np.isnan(v).any() and np.isinf(v).any() and (np.signbit(v) & (v == 0)).any()
    assert ((v < 0) & (np.abs(v) < np.finfo(np.float32).tiny)).any() and np.array_equal(v, ic.mixed_volume((33, 33, 33), 5), equal_nan=True)


def test_oracle_table_of_the_grasp9_fine_volumes():
    """oracle.sdf_oracle.two_pass_volumes (fp32, CPU) on grasp9 samples 0..3 at N = 32: the both-negative counts of the table."""
    counts = [int(ic.overlap_statement(*ic.oracle_volumes(s, 32)[:2])[2]) for s in range(4)]
    assert tuple(counts) == ic.ORACLE_BOTH_NEGATIVE[32] == (23, 6, 19, 14)
    assert max(ic.near_level_voxels(s, 32) for s in range(4)) <= 1
