"""The interaction metrics on the GPU (csrc/interaction.hip, alignsdf_amd/interaction.py): both kernels against the numpy statements of
tests/interaction_cases.py in every word, the C ABI, the pass inside the sample pipeline (grasp9, N = 32) against the same statements
over the sample's own volumes and kept vertices, the CPU oracle's table, and the files of reconstruct()."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import interaction as ia
from alignsdf_amd import synthetic as syn
from tests import interaction_cases as ic
from tests import sdf_grad_cases as gc

pytestmark = pytest.mark.gpu
EINVAL = -1
PARTS = ("hand", "obj")
CONTACT_M = 0.005
N = 32


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bits1(x):
    return _bits(x).reshape(-1)[0]


def _offset_view(a):
    """The same values in a buffer that starts one float past a 16-byte boundary."""
    buf = torch.empty(a.numel() + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ---- 1. the lattice kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ic.LATTICE_SHAPES)
def test_lattice_kernel_equals_the_numpy_statement_in_every_word(shape):
    a, b = ic.mixed_volume(shape, 11 + shape[2]), ic.mixed_volume(shape, 12 + shape[2])
    want = ic.overlap_statement(a, b)
    da, db = _dev(a), _dev(b)
    got = ia.lattice_overlap(da, db)
    again = ia.lattice_overlap(da, db)
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist(), (shape, got.cpu().numpy(), want)
    assert torch.equal(got, again)
    # inputs unchanged
    assert np.array_equal(_bits(da.cpu().numpy()), _bits(a)) and np.array_equal(_bits(db.cpu().numpy()), _bits(b))
    # misaligned by one float: both, the hand volume alone, the object volume alone
    for oa, ob in ((True, True), (True, False), (False, True)):
        va, vb = _offset_view(da) if oa else da, _offset_view(db) if ob else db
        assert ia.lattice_overlap(va, vb).cpu().numpy().tolist() == want.tolist(), (shape, oa, ob)
    # the roles are not symmetric in words 0 / 1
    swapped = ia.lattice_overlap(db, da).cpu().numpy()
    assert swapped.tolist() == ic.overlap_statement(b, a).tolist()


@pytest.mark.parametrize("shape", ((2, 3, 5), (33, 33, 33)))
def test_lattice_kernel_on_all_positive_and_all_negative_pairs(shape):
    pos = np.abs(ic.mixed_volume(shape, 3))
    pos[np.isnan(pos)] = 1.0
    neg = -pos - 1.0
    apart = ia.lattice_overlap(_dev(pos), _dev(neg)).cpu().numpy()
    n = int(np.prod(shape))
    assert apart.tolist() == [0, n, 0, 0] + [ic.INT_MAX] * 3 + [-1] * 3 + [0] * 6 == ic.overlap_statement(pos, neg).tolist()
    every = ia.lattice_overlap(_offset_view(_dev(neg)), _dev(neg)).cpu().numpy()
    assert every.tolist() == [n, n, n, 0, 0, 0, 0, shape[0] - 1, shape[1] - 1, shape[2] - 1] + [0] * 6


# ---- 2. the points kernel -----------------------------------------------------------------------------------------------------------------
def _count(v):
    return None if v is None else torch.tensor([v, 12345, -7], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("M", ic.LIST_LENGTHS)
def test_points_kernel_equals_the_numpy_statement_in_every_word(M):
    f = ic.mixed_values(M, 200 + M)
    tau = 0.0175
    d = _dev(f)
    for count in (None, 0, M // 2, M - 1, M, M + 5, 2 ** 31 - 1, -1, -2 ** 31):
        want = ic.contact_statement(f, tau, count)
        got = ia.surface_contact(d, tau, _count(count))
        assert got.cpu().numpy().tolist() == want.tolist(), (M, count, got.cpu().numpy(), want)
    assert torch.equal(ia.surface_contact(d, tau), ia.surface_contact(d, tau))
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(f))
    if M:
        assert ia.surface_contact(_offset_view(d), tau).cpu().numpy().tolist() == ic.contact_statement(f, tau).tolist()


def test_points_kernel_ties_tau_edges_and_nan_lists():
    rng = np.random.default_rng(9)
    f = rng.uniform(0.1, 1.0, 4097).astype(np.float32)
    f[[4000, 77, 3000, 300]] = -0.5                         # a tie on the minimum, spread over workgroups: the lowest index wins
    got = ia.surface_contact(_dev(f), 0.01).cpu().numpy()
    assert got.tolist() == ic.contact_statement(f, 0.01).tolist() and got[_native.CONTACT_ARGMIN] == 77
    assert got[_native.CONTACT_MIN_BITS] == _bits(np.float32(-0.5)) and got[_native.CONTACT_INSIDE] == 4
    # f == tau counts, the next float above does not
    tau = np.float32(0.0175)
    edge = np.array([tau, np.nextafter(tau, np.float32(np.inf)), 1.0], np.float32)
    got = ia.surface_contact(_dev(edge), float(tau)).cpu().numpy()
    assert got.tolist() == ic.contact_statement(edge, tau).tolist() and got[_native.CONTACT_NEAR] == 1
    # tau = 0: -0.0 and +0.0 are within it and neither is negative; -0.0 orders below +0.0
    zeros = np.array([1.0, 0.0, -0.0, 0.0, -0.0, -1e-40], np.float32)
    got = ia.surface_contact(_dev(zeros[:5]), 0.0).cpu().numpy()
    assert got.tolist() == ic.contact_statement(zeros[:5], 0.0).tolist() == [5, 0, 4, 0, int(_bits1(np.float32(-0.0))), 2, 0, 0]
    got = ia.surface_contact(_dev(zeros), 0.0).cpu().numpy()
    assert got.tolist() == ic.contact_statement(zeros, 0.0).tolist() and got[_native.CONTACT_INSIDE] == 1 and got[_native.CONTACT_ARGMIN] == 5
    # nothing but NaNs
    for M in (1, 64, 300):
        nan = np.full(M, np.nan, np.float32)
        assert ia.surface_contact(_dev(nan), 0.01).cpu().numpy().tolist() == [M, 0, 0, M, ic.INF_BITS, -1, 0, 0]


# ---- 3. the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_version_invalid_arguments_and_empty_list(native_lib):
    L = native_lib
    assert L.asdf_version() == 132
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vol = torch.ones((2, 3, 4), dtype=torch.float32, device="cuda")
    rec = torch.full((16,), 99, dtype=torch.int32, device="cuda")
    lattice = lambda a, b, n0, n1, n2, r: L.asdf_interaction_lattice(a, b, n0, n1, n2, r, st)
    p, r = vol.data_ptr(), rec.data_ptr()
    assert lattice(None, p, 2, 3, 4, r) == EINVAL and lattice(p, None, 2, 3, 4, r) == EINVAL and lattice(p, p, 2, 3, 4, None) == EINVAL
    for dims in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4), (1025, 1024, 1024)):
        assert lattice(p, p, *dims, r) == EINVAL, dims
    torch.cuda.synchronize()
    assert rec.cpu().tolist() == [99] * 16                  # a refused call writes nothing
    assert lattice(p, p, 2, 3, 4, r) == 0
    assert rec.cpu().tolist() == [0, 0, 0, 0] + [ic.INT_MAX] * 3 + [-1] * 3 + [0] * 6

    vals = torch.tensor([0.5, -0.5, 0.25], dtype=torch.float32, device="cuda")
    rec8 = torch.full((8,), 99, dtype=torch.int32, device="cuda")
    points = lambda f, cap, cnt, tau, rr: L.asdf_interaction_points(f, cap, cnt, ctypes.c_float(tau), rr, st)
    f, r8 = vals.data_ptr(), rec8.data_ptr()
    assert points(None, 3, None, 0.01, r8) == EINVAL and points(f, -1, None, 0.01, r8) == EINVAL and points(f, 3, None, 0.01, None) == EINVAL
    assert points(f, 3, None, float("nan"), r8) == EINVAL and points(f, 3, None, -0.001, r8) == EINVAL
    torch.cuda.synchronize()
    assert rec8.cpu().tolist() == [99] * 8
    # cap == 0 is the record of nothing, with or without a pointer
    for ptr in (None, f):
        rec8.fill_(99)
        assert points(ptr, 0, None, 0.01, r8) == 0
        assert rec8.cpu().tolist() == [0, 0, 0, 0, ic.INF_BITS, -1, 0, 0]
    assert points(f, 3, None, 0.0, r8) == 0
    assert rec8.cpu().tolist() == [3, 1, 1, 0, int(_bits1(np.float32(-0.5))), 1, 0, 0]


# ---- 4. the pass inside the sample pipeline: grasp9, N = 32 -----------------------------------------------------------------------------
def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _pipeline(decoder, specs, tag, indices, cube=N, source=None, **options):
    """Run the sample pipeline to its end; [(index, result)] and the evaluator that ran."""
    from alignsdf_amd.reconstruct import synthetic_code_source
    from alignsdf_amd.sample_pipeline import pipelined_two_pass
    source = source or synthetic_code_source(tag)
    report = {}
    with torch.no_grad():
        out = list(pipelined_two_pass(decoder, specs, ((k, *source("%08d" % k, k)) for k in indices), cube, host_copy=True, report=report,
                                      **options))
    torch.cuda.synchronize()
    return out, report["evaluator"], report


def _measure_again(hip, specs, tag, index, r, contact_m=CONTACT_M):
    """The numpy statements over the sample's OWN returned volumes and over decode_points at its OWN kept vertices: (words [32], the
    other head's values per surface)."""
    from alignsdf_amd.utils.mesh import lattice_points
    from alignsdf_amd.utils.utils import bind_sample
    latent, mano, obj = syn.sample_inputs(tag, index)
    bind_sample(hip, specs, torch.from_numpy(latent), _t(mano), _t(obj))
    tau = ia.contact_tau(contact_m, specs["SdfScaleFactor"])
    words, others = [ic.overlap_statement(r["vol_hand"].cpu().numpy(), r["vol_obj"].cpu().numpy())], {}
    for k, part in enumerate(PARTS):
        if "kept_dev_" + part not in r:
            words.append(np.zeros(8, np.int32))
            continue
        kv, _, counts = r["kept_dev_" + part]
        others[part] = hip.decode_points(lattice_points(kv, r["origin"], r["voxel_size"]))[1 - k].cpu().numpy()
        words.append(ic.contact_statement(others[part], tau, int(counts[0])))
    return np.concatenate(words), others


def _check_sample(label, hip, specs, tag, index, r):
    """A result's interaction words and per-vertex values are the statements' over its own volumes and vertices, bit for bit; returns
    (words, record)."""
    assert "host_interaction" in r and r["interaction_contact_m"] == CONTACT_M, label
    r["copy_done_interaction"].synchronize()
    got = r["host_interaction"].numpy()
    want, others = _measure_again(hip, specs, tag, index, r)
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), (label, got, want)
    have = [part for part in PARTS if "verts_" + part in r]
    for part in have:
        n = int(r["host_kept_counts_" + part][0])
        assert np.array_equal(_bits(r["host_other_sdf_" + part].numpy()[:n]), _bits(others[part][:n])), (label, part)
    rec = ia.interaction_record(ia.split_words(got, have), float(r["voxel_size"]), specs["SdfScaleFactor"], CONTACT_M)
    assert rec == ia.interaction_record(ia.split_words(want, have), float(r["voxel_size"]), specs["SdfScaleFactor"], CONTACT_M)
    return got, rec


@pytest.fixture(scope="module")
def grasp_runs():
    """The grasp9 runs the tests below share, made on first use: name -> ([(index, result)], evaluator)."""
    dec, specs = gc.module_for(ic.TAG), syn.specs_for(ic.TAG)
    options = {"plain": {}, "on": {"interaction": {"contact_m": CONTACT_M}}, "fast": {"interaction": {"contact_m": CONTACT_M}, "fast": True},
               "polish": {"interaction": {"contact_m": CONTACT_M}, "polish": True}, "polish_plain": {"polish": True}}
    made = {}

    def get(name):
        if name not in made:
            indices = range(4) if name == "on" else range(3)          # (the truth table below has four samples)
            made[name] = _pipeline(dec, specs, ic.TAG, indices, **options[name])[:2]
            if options[name].get("fast"):
                made[name][1].set_fast(False)
        return made[name]
    get.specs = specs
    return get


def _kept(r, part):
    r["copy_done_" + part].synchronize()
    c = r["host_kept_counts_" + part].numpy()
    return r["host_kept_verts_" + part].numpy()[:c[0]], r["host_kept_faces_" + part].numpy()[:c[1]]


def test_pipeline_records_are_the_statements_over_the_samples_own_volumes_and_vertices(grasp_runs):
    results, hip = grasp_runs("on")
    for index, r in results[:3]:
        words, rec = _check_sample("grasp9 sample %d" % index, hip, grasp_runs.specs, ic.TAG, index, r)
        print("INTERACTION grasp9 N=32 sample %d: %s" % (index, json.dumps(rec)))
        assert rec["intersection_voxels"] > 0 and rec["hand_vertices"] > 0 and rec["obj_vertices"] > 0 and rec["nan_voxels"] == 0
        assert rec["contact"] is True and rec["penetration_depth_cm"] > 0 and rec["hand_vertices_inside"] > 0      # built to interpenetrate
        assert rec["hand_vertices_in_contact"] >= rec["hand_vertices_inside"] and rec["min_distance_cm"] < 0


def test_meshes_are_bit_identical_with_and_without_the_option(grasp_runs):
    plain, _ = grasp_runs("plain")
    on, _ = grasp_runs("on")
    for (i, a), (j, b) in zip(plain, on):
        assert i == j and "interaction" not in a and "host_interaction" not in a
        assert torch.equal(a["vol_hand"], b["vol_hand"]) and torch.equal(a["vol_obj"], b["vol_obj"])
        for part in PARTS:
            (va, fa), (vb, fb) = _kept(a, part), _kept(b, part)
            assert len(va) > 0 and np.array_equal(_bits(va), _bits(vb)) and np.array_equal(fa, fb), (i, part)


def test_fast_sweeps_give_the_same_overlap_words(grasp_runs):
    on, _ = grasp_runs("on")
    fast, hip = grasp_runs("fast")
    for (i, a), (j, b) in zip(on, fast):
        got = b["host_interaction"].numpy()[:16]
        assert i == j and got.tolist() == a["host_interaction"].numpy()[:16].tolist(), (i, got)
        # ... and they are the statement over the sign-correct volumes the fast run returned
        assert got.tolist() == ic.overlap_statement(b["vol_hand"].cpu().numpy(), b["vol_obj"].cpu().numpy()).tolist()


def test_with_polish_the_polished_vertices_are_measured(grasp_runs):
    polished, hip = grasp_runs("polish")
    twin, _ = grasp_runs("polish_plain")
    on, _ = grasp_runs("on")
    for (index, r), (_, t), (_, o) in zip(polished, twin, on):
        words, rec = _check_sample("grasp9 polished sample %d" % index, hip, grasp_runs.specs, ic.TAG, index, r)      # (kept_dev_* hold the polished rows)
        for part in PARTS:
            (v, f), (tv, tf), (ov, of) = _kept(r, part), _kept(t, part), _kept(o, part)
            assert np.array_equal(_bits(v), _bits(tv)) and np.array_equal(f, tf) and np.array_equal(f, of)
            assert v.shape == ov.shape and not np.array_equal(v, ov)           # the file's vertices are the polished ones
            assert np.array_equal(r["kept_dev_" + part][0][:len(v)].cpu().numpy(), v)
        assert words[:16].tolist() == o["host_interaction"].numpy()[:16].tolist()          # the volumes do not move
        assert rec["hand_vertices"] == len(_kept(r, "hand")[0])


def test_a_repeated_fine_pass_reports_the_final_volumes(monkeypatch):
    """fast=True at N = 64 with the narrow-band list's capacity cut to 10 voxels while samples are in flight (the switch of
    tests/test_experiment_io.py): the band sweeps judged then are refused and repeated as ordinary sweeps, which REPLACES vol_*; the
    records are those of the volumes the samples end with."""
    from alignsdf_amd import hip_decoder as hd
    from alignsdf_amd.reconstruct import synthetic_code_source
    dec, specs = gc.module_for(ic.TAG), syn.specs_for(ic.TAG)
    base, real_cap = synthetic_code_source(ic.TAG), hd.BAND_CAP

    def sabotaging_source(name, index):          # (the pipeline fetches sample k + 2 while sample k is being finished)
        monkeypatch.setattr(hd, "BAND_CAP", 10 if index in (3, 4) else real_cap)
        return base(name, index)

    try:
        results, hip, report = _pipeline(dec, specs, ic.TAG, range(6), cube=64, source=sabotaging_source, fast=True,
                                         interaction={"contact_m": CONTACT_M})
    finally:
        monkeypatch.setattr(hd, "BAND_CAP", real_cap)
    rep = hip.sweep_report(report["snapshot"])
    hip.set_fast(False)
    print("INTERACTION repeated fine pass: refused %d, repeated %d" % (rep["sweeps_refused"], rep["sweeps_repeated"]))
    assert rep["sweeps_repeated"] >= 1 and rep["fine_pass"]["refused_and_repeated"] >= 1, rep
    for index, r in results:
        got = r["host_interaction"].numpy()
        assert got[:16].tolist() == ic.overlap_statement(r["vol_hand"].cpu().numpy(), r["vol_obj"].cpu().numpy()).tolist(), index
        assert got[_native.OVERLAP_BOTH] > 0


# ---- 5. truth ---------------------------------------------------------------------------------------------------------------------------------
def test_counts_against_the_cpu_oracle_and_minimum_against_the_fp64_chain(grasp_runs):
    from alignsdf_amd.utils.mesh import lattice_points
    from tests import sdf_project_cases as pc
    results, hip = grasp_runs("on")
    to_cm = 2.0 / grasp_runs.specs["SdfScaleFactor"] * 100.0
    for index, r in results:
        words = r["host_interaction"].numpy()
        both, table, slack = int(words[_native.OVERLAP_BOTH]), ic.ORACLE_BOTH_NEGATIVE[N][index], ic.near_level_voxels(index, N)
        print("INTERACTION truth sample %d: both-negative %d, oracle %d, near-level oracle voxels %d" % (index, both, table, slack))
        assert abs(both - table) <= slack, (index, both, table, slack)
        # the minimum of the object's field over the GPU's own hand vertices, against the fp64 chain at those same points
        kv, _, counts = r["kept_dev_hand"]
        pts = lattice_points(kv, r["origin"], r["voxel_size"])[:int(counts[0])].cpu().numpy()
        low64 = float(pc.sdf64(ic.TAG, index, pts)["obj"].min())
        low = float(words[16 + _native.CONTACT_MIN_BITS:16 + _native.CONTACT_MIN_BITS + 1].view(np.float32)[0])
        # (a property of the fixture, not of this code: how far the TRAINED decoder's depth sits from the analytic scene's)
        analytic = float(syn.grasp_sdf(pts, index)[1].min())
        print("INTERACTION truth sample %d: min object sdf at the hand's vertices %.7f, fp64 chain %.7f (|diff| %.2e); depth %.4f cm, the "
              "analytic scene's at the same points %.4f cm" % (index, low, low64, abs(low - low64), max(0.0, -low) * to_cm, max(0.0, -analytic) * to_cm))
        assert abs(low - low64) <= 1e-5, (index, low, low64)


# ---- 6. other evaluators ------------------------------------------------------------------------------------------------------------------
def test_module_path_and_combined_decoder_produce_records():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.networks.model import build_decoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    for tag, on_module in (("nerf9", True), ("comb3", False)):
        specs = syn.specs_for(tag)
        module = build_decoder(specs, {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict(tag).items()}).eval()
        decoder = TorchModuleDecoder(module, specs, "the interaction kernels need no decoder") if on_module else module
        results, hip, _ = _pipeline(decoder, specs, tag, range(2), interaction={"contact_m": CONTACT_M})
        assert isinstance(hip, TorchModuleDecoder if on_module else HipSdfDecoder) and (on_module or hip.combined)
        for index, r in results:
            words, rec = _check_sample("%s sample %d" % (tag, index), hip, specs, tag, index, r)
            print("INTERACTION %s sample %d: %s" % (tag, index, json.dumps(rec)))
            assert rec["hand_voxels"] + rec["obj_voxels"] > 0 and rec["contact_m"] == CONTACT_M


def test_a_branch_switched_off_raises_before_any_sweep(monkeypatch):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    dec = gc.module_for(ic.TAG)

    def no_sweep(*a, **k):
        raise AssertionError("a sweep in a run that must refuse first")
    for name in ("coarse_begin", "two_pass_begin", "fine_begin"):
        monkeypatch.setattr(HipSdfDecoder, name, no_sweep)
    for off in ("HandBranch", "ObjectBranch"):
        with pytest.raises(ValueError):
            _pipeline(dec, dict(syn.specs_for(ic.TAG), **{off: False}), ic.TAG, range(2), interaction={"contact_m": CONTACT_M})


# ---- 7. the flows -------------------------------------------------------------------------------------------------------------------------
def _split(tmp_path, names):
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["skip/0.jpg"] + ["data/obman/test/rgb/%s.jpg" % n for n in names]}, fh)
    return split


def test_reconstruct_writes_records_shard_files_summary_and_quality(tmp_path, grasp_runs):
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.reconstruct import reconstruct, synthetic_code_source
    dec, specs = gc.module_for(ic.TAG), grasp_runs.specs
    names = ["00000001", "00000002", "00000003"]
    split = _split(tmp_path, names)
    kw = dict(cube_dim=N, code_source=synthetic_code_source(ic.TAG))
    plain_dir, out = str(tmp_path / "plain"), str(tmp_path / "on")
    plain = reconstruct(dec, specs, split, plain_dir, 1, 4, **kw)
    recs = reconstruct(dec, specs, split, out, 1, 4, interaction={"contact_m": CONTACT_M}, **kw)
    assert not any("interaction" in r for r in plain) and not [n for n in os.listdir(plain_dir) if n.startswith("interaction")]
    shard = json.load(open(os.path.join(out, "interaction_1_4.json")))
    merged = json.load(open(os.path.join(out, "interaction.json")))
    assert shard["range"] == [1, 4] and shard["contact_m"] == CONTACT_M and [s["index"] for s in shard["samples"]] == [1, 2, 3]
    assert merged["summary"] == ia.summarise(recs) and merged["summary"]["samples"] == 3 and merged["summary"]["contact_ratio"] == 1.0
    lines = open(os.path.join(out, "interaction.txt")).read().splitlines()
    depths = [float(l.split(",")[1]) for l in lines[1:4]]
    assert len(lines) == 8 and depths == sorted(depths, reverse=True) and lines[7] == "samples:3"
    on_run, _ = grasp_runs("on")
    for rec, before, (index, r) in zip(recs, plain, on_run[1:4]):
        it = rec["interaction"]
        json.dumps(rec["interaction"])
        assert rec["index"] == index and {k: v for k, v in rec.items() if k not in ("interaction", "seconds")} == {k: v for k, v in before.items() if k != "seconds"}
        assert dict(shard["samples"][index - 1]) == dict({"index": index, "name": rec["name"]}, **it)
        # the same sample through the bare pipeline: the same record
        have = [part for part in PARTS if "verts_" + part in r]
        assert it == ia.interaction_record(ia.split_words(r["host_interaction"].numpy(), have), rec["voxel_size"], specs["SdfScaleFactor"], CONTACT_M)
        for k, part in enumerate(PARTS):
            path = os.path.join("meshes", "%s_%s.ply" % (rec["name"], part))
            v, f, q = read_ply(os.path.join(out, path), with_quality=True)
            pv, pf, pq = read_ply(os.path.join(plain_dir, path), with_quality=True)
            assert pq is None and q is not None and np.array_equal(_bits(v), _bits(pv)) and np.array_equal(f, pf) and len(q) == len(v) > 0
            # quality: metres to the OTHER surface, by the other head's SDF at the vertex
            n = len(v)
            want = r["host_other_sdf_" + part].numpy()[:n] * np.float32(2.0 / specs["SdfScaleFactor"])
            assert np.array_equal(_bits(q), _bits(want)), (index, part)
            depth = it["penetration_depth_cm" if part == "hand" else "penetration_depth_obj_cm"]
            assert int((q < 0).sum()) == it[part + "_vertices_inside"] and max(0.0, -float(q.min())) * 100.0 == pytest.approx(depth, rel=1e-5, abs=1e-12)


def test_command_line_flags_reach_the_pipeline(tmp_path, capsys):
    from alignsdf_amd import reconstruct as rc
    from alignsdf_amd.ply import read_ply
    tag = "nerf3"                              # (--synthetic draws the codes of nerf3 / both9 by PointFeatSize: the weights have to match)
    specs = syn.specs_for(tag)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict(tag).items()}
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["data/obman/test/rgb/00000012.jpg"]}, fh)
    model = tmp_path / "experiment"
    os.makedirs(model / "ModelParameters")
    with open(model / "specs.json", "w") as fh:
        json.dump(specs, fh)
    torch.save({"model_state_dict": {"module.decoder." + k: v for k, v in sd.items()}}, str(model / "ModelParameters" / "latest.pth"))
    recs = rc.main(["--model", str(model), "--split", split, "--synthetic", "--cube_dim", str(N), "--interaction", "--contact_mm", "2.5"])
    it = recs[0]["interaction"]
    assert it["contact_m"] == 0.0025 and it["hand_voxels"] > 0 and it["hand_vertices"] > 0
    out = model / "Eval_obman"
    assert json.load(open(out / "interaction_0_1.json"))["contact_m"] == 0.0025 and os.path.exists(out / "interaction.txt")
    assert "interaction: 1 samples" in capsys.readouterr().out
    assert read_ply(str(out / "meshes" / "00000012_hand.ply"), with_quality=True)[2] is not None


def test_create_mesh_returns_the_same_record(tmp_path, grasp_runs):
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.utils.mesh import create_mesh_combined_decoder
    dec, specs = gc.module_for(ic.TAG), grasp_runs.specs
    latent, mano, obj = syn.sample_inputs(ic.TAG, 1)
    args = (True, True, False, dec, torch.from_numpy(latent), _t(mano), _t(obj), None, specs)
    s0 = create_mesh_combined_decoder(*args, str(tmp_path / "plain"), N=N, return_stats=True)
    s1 = create_mesh_combined_decoder(*args, str(tmp_path / "on"), N=N, return_stats=True, interaction={"contact_m": CONTACT_M})
    assert "interaction" not in s0 and s1["hand"] == s0["hand"] and s1["obj"] == s0["obj"]
    for part in PARTS:
        assert open(str(tmp_path / ("plain_%s.ply" % part)), "rb").read() == open(str(tmp_path / ("on_%s.ply" % part)), "rb").read()
    index, r = grasp_runs("on")[0][1]
    have = [part for part in PARTS if "verts_" + part in r]
    want = ia.interaction_record(ia.split_words(r["host_interaction"].numpy(), have), float(r["voxel_size"]), specs["SdfScaleFactor"], CONTACT_M)
    assert index == 1 and s1["interaction"] == want and s1["interaction"]["hand_vertices"] == len(read_ply(str(tmp_path / "on_hand.ply"))[0])
    with pytest.raises(ValueError):
        create_mesh_combined_decoder(True, False, False, *args[3:], str(tmp_path / "off"), N=N, interaction={"contact_m": CONTACT_M})
    assert not os.path.exists(str(tmp_path / "off_hand.ply"))
