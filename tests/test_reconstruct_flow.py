"""The consumer in reconstruct(): what it makes of each result dict of the sample pipeline - files, records, the sweeps report - and how
it ends when something fails.  CPU only: the pipeline is replaced by a stand-in that does at its boundary what the real one does
(lazy fetches two samples ahead, the midpoint hook of sample k between the fetch of sample k+2 and the yield of sample k, canned
result dicts), the two ICP halves by recorders; the ground-truth prefetcher and the file writer are the real ones."""
import concurrent.futures
import json
import logging
import os
import threading
import types

import numpy as np
import pytest
import torch

from alignsdf_amd import gt_worker, reconstruct as rc
from alignsdf_amd.ply import read_ply
from alignsdf_amd.utils.mesh import place_vertices

SWEEPS = {"evaluator": "stand-in", "sweeps_audited": 0, "coarse_pass": {"ordinary_sweeps": 3}}
VOXEL = torch.tensor(0.03125, dtype=torch.float32)
ORIGIN = [-0.75, 0.125, -0.5]
TRANS, SCALE = np.array([0.02, -0.01, 0.03]), np.array([[1.09]])       # what the stand-in ICP "finds" (shapes the consumer reshapes)
MC_ERROR = "Surface level must be within volume data range."
NAMES = ["%08d" % i for i in (12, 47, 100, 7, 3, 51, 9, 64)]


class Result(dict):
    """A result dict that notes which keys are read, in order."""

    def __init__(self, log, *a):
        super().__init__(*a)
        self.log = log

    def __getitem__(self, key):
        self.log.append(("read", key))
        return super().__getitem__(key)


class CopyDone:
    def __init__(self, log, part):
        self.log, self.part = log, part

    def synchronize(self):
        self.log.append(("synchronize", self.part))


def canned(index, log, parts=("hand", "obj"), labels=False, no_surface=()):
    """The result dict of sample `index`: surfaces of index-dependent sizes, the kept component at a capacity above its counts."""
    rng = np.random.default_rng(100 + index)
    r = Result(log, {"V_hand": 0, "F_hand": 0, "V_obj": 0, "F_obj": 0, "voxel_size": VOXEL, "origin": list(ORIGIN)})
    for p, part in enumerate(("hand", "obj")):
        if part not in parts:
            continue
        if part in no_surface:
            r["mc_error_" + part] = MC_ERROR
            continue
        nv, nf = 9 + index + 2 * p, 7 + index + p                           # the whole surface = the capacity of the kept buffers
        kv, kf = 5 + p + index % 2, 3 + p                                   # the kept component
        verts = torch.from_numpy(rng.uniform(0, 40, (nv, 3)).astype(np.float32))
        faces = torch.from_numpy(rng.integers(0, nv, (nf, 3)).astype(np.int32))
        kept_verts = torch.from_numpy(rng.uniform(0, 40, (nv, 3)).astype(np.float32))
        kept_faces = torch.from_numpy(rng.integers(0, kv, (nf, 3)).astype(np.int32))
        counts = torch.tensor([kv, kf, 0, 0, 1 + index + p, 2 + 3 * index + p, 0, 0], dtype=torch.int32)
        r.update({"verts_" + part: verts, "faces_" + part: faces, "V_" + part: nv, "F_" + part: nf,
                  "host_kept_verts_" + part: kept_verts, "host_kept_faces_" + part: kept_faces, "host_kept_counts_" + part: counts,
                  "copy_done_" + part: CopyDone(log, part)})
        if part == "hand":
            r["kept_dev_hand"] = (object(), object(), object())
            if labels:
                r.update({"host_verts_hand": verts.clone(), "host_faces_hand": faces.clone(),
                          "host_labels_hand": torch.from_numpy(rng.integers(0, 6, nv).astype(np.int64))})
    return r


def kept_slice(r, part):
    c = dict.__getitem__(r, "host_kept_counts_" + part).numpy()
    return dict.__getitem__(r, "host_kept_verts_" + part)[:c[0]], dict.__getitem__(r, "host_kept_faces_" + part)[:c[1]]


def placed(r, part, offset=None, scale=None):
    """(vertices as the file holds them, faces) of the kept component of one part."""
    _, faces, points = place_vertices(*kept_slice(r, part), ORIGIN, VOXEL, offset, scale)
    return np.asarray(points, dtype="<f4"), faces


class Flow:
    """One reconstruct() run against the stand-ins; everything that happened is in `log`, every canned result in `results`."""

    def __init__(self, tmp_path, monkeypatch, **canned_kw):
        self.log, self.results, self.on_records, self.canned_kw = [], {}, [], canned_kw
        self.prefetchers, self.writers, self.jobs_at_record = [], [], []
        self.out = str(tmp_path / "Eval_obman")
        self.mesh_dir = os.path.join(self.out, "meshes")
        self.split = str(tmp_path / "split.json")
        self.data_root = str(tmp_path / "data")
        self.decoder = object()
        self.stub = types.SimpleNamespace(sweep_report=lambda snapshot: dict(SWEEPS, snapshot=snapshot))
        with open(self.split, "w") as f:
            json.dump({"filenames": ["data/obman/test/rgb/%s.jpg" % n for n in NAMES]}, f)
        monkeypatch.setenv("ASDF_GT_WORKER", "thread")
        monkeypatch.setattr(rc, "pipelined_two_pass", self.pipeline)
        monkeypatch.setattr("alignsdf_amd.icp.start_alignment_device", self.start_alignment_device)
        monkeypatch.setattr("alignsdf_amd.icp.finish_icp", self.finish_icp)
        flow = self
        gt_init, gt_prefetch, gt_discard, fw_init = (rc.GroundTruthPrefetcher.__init__, rc.GroundTruthPrefetcher.prefetch,
                                                     rc.GroundTruthPrefetcher.discard, rc.FileWriter.__init__)

        def init(self, *a, **kw):
            flow.prefetchers.append(self)
            gt_init(self, *a, **kw)
            flow.log.append(("prefetcher", self.task, self.data_root, self.allow_missing))

        def prefetch(self, path):
            flow.log.append(("prefetch", path))
            gt_prefetch(self, path)

        def discard(self, path):
            flow.log.append(("discard", path))
            gt_discard(self, path)

        def writer_init(self):
            flow.writers.append(self)
            fw_init(self)

        monkeypatch.setattr(rc.GroundTruthPrefetcher, "__init__", init)
        monkeypatch.setattr(rc.GroundTruthPrefetcher, "prefetch", prefetch)
        monkeypatch.setattr(rc.GroundTruthPrefetcher, "discard", discard)
        monkeypatch.setattr(rc.FileWriter, "__init__", writer_init)

    # ---- the stand-ins -------------------------------------------------------------------------------------------------------
    def code_source(self, name, index):
        self.log.append(("codes", name, index))
        return "latent %s" % name, None, None

    def pipeline(self, decoder, specs, samples, N, grid_mode="reference", host_copy=False, label_out=False, midpoint=None, report=None,
                 fast=None):
        self.log.append(("pipeline", decoder, N, grid_mode, host_copy, label_out, midpoint is not None, fast))
        report["evaluator"], report["snapshot"] = self.stub, "counters at the start"

        it = iter(samples)

        def fetch():
            s = next(it, None)
            if s is not None:
                self.log.append(("fetched", s[0]))
            return s

        cur, nxt = fetch(), None
        if cur is not None:
            nxt = fetch()
        while cur is not None:
            after = fetch() if nxt is not None else None
            key = cur[0]
            kw = dict(self.canned_kw)
            kw["no_surface"] = kw.pop("no_surface", {}).get(key[0], ())
            r = self.results[key[0]] = canned(key[0], self.log, **kw)
            if midpoint is not None:
                self.log.append(("midpoint", key))
                midpoint(key, r)
            self.log.append(("yield", key))
            yield key, r
            for w in self.writers:                         # (a write handed over for this sample has finished, or failed, by now)
                concurrent.futures.wait([j for _, j in w.jobs])
            cur, nxt = nxt, after

    def start_alignment_device(self, *args):
        job = ("icp job", len(self.log))
        self.log.append(("start_alignment_device", args, job))
        return job

    def finish_icp(self, job, vertices):
        self.log.append(("finish_icp", job, np.array(vertices, copy=True)))
        return {"vertices": np.asarray(vertices, dtype=np.float64)[::-1] * 0.5 + 0.25, "all_trans": TRANS, "all_scale": SCALE}

    def on_record(self, rec):
        self.on_records.append(rec)
        self.jobs_at_record.append([set(g.jobs) for g in self.prefetchers])

    # ---- helpers -------------------------------------------------------------------------------------------------------------
    def run(self, start, end, specs=None, **kw):
        specs = {"HandBranch": True, "ObjectBranch": True} if specs is None else specs
        kw.setdefault("on_record", self.on_record)
        return rc.reconstruct(kw.pop("model", self.decoder), specs, self.split, self.out, start, end, code_source=self.code_source,
                              data_root=self.data_root, **kw)

    def ground_truth(self, names):
        d = os.path.join(self.data_root, "obman", "test", "mesh_hand")
        os.makedirs(d, exist_ok=True)
        for k, name in enumerate(names):
            with open(os.path.join(d, name + ".obj"), "w") as f:
                for v in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    f.write("v %r %r %r\n" % tuple((1.0 + k) * c for c in v))
                f.write("f 1 2 3\nf 1 2 4\nf 1 3 4\nf 2 3 4\n")

    def mesh(self, name, part):
        return os.path.join(self.mesh_dir, "%s_%s.ply" % (name, part))

    def events(self, *kinds):
        return [e for e in self.log if e[0] in kinds]

    def report(self, start, end):
        with open(os.path.join(self.out, "sweeps_%d_%d.json" % (start, end))) as f:
            return json.load(f)

    def expected_report(self, start, end, indices, cube_dim, parts=("hand", "obj"), **extra):
        counts = [dict.__getitem__(self.results[i], "host_kept_counts_" + p).numpy() for i in indices for p in parts
                  if "host_kept_counts_" + p in self.results[i]]
        return dict({"range": [start, end], "samples": len(indices), "cube_dim": cube_dim,
                     "sweeps": dict(SWEEPS, snapshot="counters at the start")}, **extra,
                    dropped_open_components=int(sum(c[4] for c in counts)), dropped_small_components=int(sum(c[5] for c in counts)),
                    surfaces_filtered=len(counts))


def same_records(got, want):
    """Key by key and type by type (the records travel as JSON), except `seconds`."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g.get("seconds"), float) and g["seconds"] >= 0
        g = {k: v for k, v in g.items() if k != "seconds"}
        assert sorted(g) == sorted(w) and json.dumps(g, sort_keys=True) == json.dumps(w, sort_keys=True), (g, w)


def plain_record(flow, index, name, parts=("hand", "obj")):
    r = flow.results[index]
    rec = {"index": index, "name": name, "voxel_size": float(VOXEL), "origin": list(ORIGIN)}
    rec.update({k: dict.__getitem__(r, k) for k in ("V_hand", "F_hand", "V_obj", "F_obj")})
    if "hand" in parts and "verts_hand" in r:
        rec.update({"icp_trans": [0, 0, 0], "icp_scale": 1.0})
    return rec


def no_helper_threads():
    return not [t.name for t in threading.enumerate() if t.name.startswith(("asdf-ply", "asdf-gt"))]


# ---- A: both branches, plain ---------------------------------------------------------------------------------------------------
def test_plain_run_writes_the_kept_components_and_the_report(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    wrapped = types.SimpleNamespace(module=types.SimpleNamespace(decoder=flow.decoder))
    recs = flow.run(1, 4, model=wrapped, cube_dim=40, grid_mode="integer", fast=True, viz=True)
    assert flow.events("pipeline") == [("pipeline", flow.decoder, 40, "integer", True, False, False, True)]
    assert sorted(os.listdir(flow.mesh_dir)) == sorted("%s_%s.ply" % (n, p) for n in NAMES[1:4] for p in ("hand", "obj"))
    for i in (1, 2, 3):
        r = flow.results[i]
        for part in ("hand", "obj"):
            offset, scale = (None, None) if part == "hand" else (np.array([0, 0, 0]), np.array([1]))
            want_v, want_f = placed(r, part, offset, scale)
            got_v, got_f = read_ply(flow.mesh(NAMES[i], part))
            assert len(got_v) == kept_slice(r, part)[0].shape[0] < dict.__getitem__(r, "V_" + part)
            assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
            # the side-stream copy of a part is waited for, once, before anything of it is read
            first = flow.log.index(("yield", (i, NAMES[i])))
            window = flow.log[first:flow.log.index(("yield", (i + 1, NAMES[i + 1])))] if i < 3 else flow.log[first:]
            reads = [k for k, e in enumerate(window) if e[0] == "read" and e[1].startswith("host_") and e[1].endswith(part)]
            assert reads and window.count(("synchronize", part)) == 1 and window.index(("synchronize", part)) < reads[0]
    same_records(recs, [plain_record(flow, i, NAMES[i]) for i in (1, 2, 3)])
    assert len(flow.on_records) == 3 and all(a is b for a, b in zip(flow.on_records, recs))
    assert flow.report(1, 4) == flow.expected_report(1, 4, (1, 2, 3), 40)
    assert [f for f in os.listdir(flow.out) if f != "meshes"] == ["sweeps_1_4.json"]
    assert not flow.prefetchers and not flow.events("start_alignment_device", "finish_icp") and no_helper_threads()
    # the samples are pulled lazily: codes of sample k+2 are asked for while sample k is finished
    assert [e[1:] for e in flow.events("codes")] == [(NAMES[i], i) for i in (1, 2, 3)]
    order = flow.events("fetched", "yield")
    assert order.index(("fetched", (3, NAMES[3]))) < order.index(("yield", (1, NAMES[1]))) < order.index(("yield", (2, NAMES[2])))


# ---- B: one branch ---------------------------------------------------------------------------------------------------------------
def test_hand_only(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch, parts=("hand",))
    recs = flow.run(0, 2, specs={"HandBranch": True, "ObjectBranch": False}, scale=2.5)
    assert sorted(os.listdir(flow.mesh_dir)) == sorted("%s_hand.ply" % n for n in NAMES[:2])
    for i in (0, 1):
        want_v, want_f = placed(flow.results[i], "hand")
        got_v, got_f = read_ply(flow.mesh(NAMES[i], "hand"))
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    same_records(recs, [plain_record(flow, i, NAMES[i]) for i in (0, 1)])
    assert flow.report(0, 2) == flow.expected_report(0, 2, (0, 1), 128, parts=("hand",))


def test_object_only_is_written_with_the_callers_scale_and_no_offset(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch, parts=("obj",))
    recs = flow.run(0, 2, specs={"HandBranch": False, "ObjectBranch": True}, scale=2.5, eval_mode=True, label_out=True)
    assert not flow.prefetchers and not flow.events("prefetcher", "prefetch", "midpoint")       # eval mode aligns the HAND
    assert flow.events("pipeline") == [("pipeline", flow.decoder, 128, "reference", True, False, False, None)]
    assert sorted(os.listdir(flow.mesh_dir)) == sorted("%s_obj.ply" % n for n in NAMES[:2])
    for i in (0, 1):
        want_v, want_f = placed(flow.results[i], "obj", None, 2.5)
        got_v, got_f = read_ply(flow.mesh(NAMES[i], "obj"))
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
        assert not np.array_equal(got_v, placed(flow.results[i], "obj")[0])
    same_records(recs, [plain_record(flow, i, NAMES[i], parts=("obj",)) for i in (0, 1)])
    assert all("icp_trans" not in r and "icp_scale" not in r and "icp_skipped" not in r for r in recs)


# ---- C: eval mode, ground truth present ----------------------------------------------------------------------------------------
def aligned_record(flow, index, name):
    return dict(plain_record(flow, index, name), icp_trans=TRANS.tolist(), icp_scale=1.09)


def check_aligned_sample(flow, i):
    """Hand file = what the stand-in ICP returned for the placed kept component; object file placed with its trans / scale."""
    r = flow.results[i]
    unaligned, faces = place_vertices(*kept_slice(r, "hand"), ORIGIN, VOXEL)[2], kept_slice(r, "hand")[1].numpy()
    start = [e for e in flow.events("start_alignment_device") if e[1][0] is dict.__getitem__(r, "kept_dev_hand")[0]]
    assert len(start) == 1
    args, job = start[0][1:]
    assert len(args) == 6 and all(a is b for a, b in zip(args[:3], dict.__getitem__(r, "kept_dev_hand")))
    assert args[3] == ORIGIN and args[4] is VOXEL
    path = os.path.join(flow.data_root, "obman", "test", "mesh_hand", NAMES[i] + ".obj")
    assert args[5].dtype == torch.float64 and np.array_equal(args[5].numpy(), gt_worker.load_samples(path, 30000, 1))
    finish = [e for e in flow.events("finish_icp") if e[1] == job]
    assert len(finish) == 1 and np.array_equal(finish[0][2], unaligned)
    got_v, got_f = read_ply(flow.mesh(NAMES[i], "hand"))
    assert np.array_equal(got_v, np.asarray(np.asarray(unaligned, dtype=np.float64)[::-1] * 0.5 + 0.25, dtype="<f4"))
    assert np.array_equal(got_f, faces)
    want_v, want_f = placed(r, "obj", TRANS.reshape(1, 3), SCALE.reshape(1))
    got_v, got_f = read_ply(flow.mesh(NAMES[i], "obj"))
    assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    assert not np.array_equal(got_v, placed(r, "obj")[0])


def test_eval_mode_aligns_the_hand_and_the_object_inherits_the_transform(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    flow.ground_truth(NAMES[:3])
    recs = flow.run(0, 3, eval_mode=True)
    assert [e[1:] for e in flow.events("prefetcher")] == [("obman", flow.data_root, False)]
    assert flow.events("pipeline") == [("pipeline", flow.decoder, 128, "reference", True, False, True, None)]
    for i in (0, 1, 2):
        # the ground truth of a sample is requested before its codes are; its ICP starts in the hook, before the sample is yielded
        assert flow.log.index(("prefetch", flow.mesh(NAMES[i], "hand"))) < flow.log.index(("codes", NAMES[i], i))
        started = [k for k, e in enumerate(flow.log) if e[0] == "start_alignment_device"][i]
        assert flow.log.index(("midpoint", (i, NAMES[i]))) < started < flow.log.index(("yield", (i, NAMES[i])))
        check_aligned_sample(flow, i)
    same_records(recs, [aligned_record(flow, i, NAMES[i]) for i in (0, 1, 2)])
    assert flow.on_records == recs and flow.report(0, 3) == flow.expected_report(0, 3, (0, 1, 2), 128)
    assert not flow.prefetchers[0].jobs and no_helper_threads()


# ---- D: eval mode, ground truth missing ----------------------------------------------------------------------------------------
def test_missing_ground_truth_allowed_writes_unaligned_files(tmp_path, monkeypatch, caplog):
    flow = Flow(tmp_path, monkeypatch)
    flow.ground_truth([NAMES[0]])
    with caplog.at_level(logging.WARNING):
        recs = flow.run(0, 2, eval_mode=True, allow_missing_gt=True)
    assert [e[1:] for e in flow.events("prefetcher")] == [("obman", flow.data_root, True)]
    check_aligned_sample(flow, 0)
    assert len(flow.events("start_alignment_device")) == 1 and len(flow.events("finish_icp")) == 1
    for part, (offset, scale) in (("hand", (None, None)), ("obj", (np.array([0, 0, 0]), np.array([1])))):
        want_v, want_f = placed(flow.results[1], part, offset, scale)
        got_v, got_f = read_ply(flow.mesh(NAMES[1], part))
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    same_records(recs, [aligned_record(flow, 0, NAMES[0]), dict(plain_record(flow, 1, NAMES[1]), icp_skipped=True)])
    missing = os.path.join(flow.data_root, "obman", "test", "mesh_hand", NAMES[1] + ".obj")
    assert any("ground-truth mesh %s not found; writing the unaligned mesh (allow_missing_gt)" % missing in m for m in caplog.messages)


def test_missing_ground_truth_aborts_with_what_was_finished(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    flow.ground_truth([NAMES[0]])
    with pytest.raises(FileNotFoundError, match="pass allow_missing_gt") as err:
        flow.run(0, 4, eval_mode=True)
    same_records(err.value.partial_records, [aligned_record(flow, 0, NAMES[0])])
    assert flow.on_records == err.value.partial_records
    check_aligned_sample(flow, 0)                                      # (the files of the finished sample are on disk)
    assert sorted(os.listdir(flow.mesh_dir)) == ["%s_hand.ply" % NAMES[0], "%s_obj.ply" % NAMES[0]]
    assert flow.report(0, 4) == flow.expected_report(0, 4, (0,), 128)
    assert not flow.prefetchers[0].jobs and no_helper_threads()
    with pytest.raises(RuntimeError):                                  # the helpers are shut down, not only idle
        flow.prefetchers[0].pool.submit(int)
    with pytest.raises(RuntimeError):
        flow.writers[0].pool.submit(int)


# ---- E: a sample without a hand surface ----------------------------------------------------------------------------------------
def test_sample_without_a_hand_surface(tmp_path, monkeypatch, caplog, capsys):
    flow = Flow(tmp_path, monkeypatch, no_surface={1: ("hand",)})
    flow.ground_truth(NAMES[:3])
    with caplog.at_level(logging.WARNING):
        recs = flow.run(0, 3, eval_mode=True)
    assert sorted(os.listdir(flow.mesh_dir)) == sorted(["%s_%s.ply" % (n, p) for n in (NAMES[0], NAMES[2]) for p in ("hand", "obj")] +
                                                       ["%s_obj.ply" % NAMES[1]])
    assert "Cannot reconstruct mesh from '%s'" % flow.mesh(NAMES[1], "hand") in caplog.messages
    assert capsys.readouterr().out.splitlines() == [MC_ERROR]
    # the prefetched ground truth of that sample is dropped in the hook; nothing of it is left when the sample is recorded
    assert flow.events("discard") == [("discard", flow.mesh(NAMES[1], "hand"))]
    assert flow.log.index(("midpoint", (1, NAMES[1]))) < flow.log.index(("discard", flow.mesh(NAMES[1], "hand"))) < flow.log.index(("yield", (1, NAMES[1])))
    assert len(flow.jobs_at_record) == 3 and flow.mesh(NAMES[1], "hand") not in flow.jobs_at_record[1][0]
    assert flow.mesh(NAMES[2], "hand") not in flow.jobs_at_record[2][0]
    assert len(flow.events("start_alignment_device")) == 2 and len(flow.events("finish_icp")) == 2
    want_v, want_f = placed(flow.results[1], "obj", np.array([0, 0, 0]), np.array([1]))
    got_v, got_f = read_ply(flow.mesh(NAMES[1], "obj"))
    assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    check_aligned_sample(flow, 0)
    check_aligned_sample(flow, 2)
    same_records(recs, [aligned_record(flow, 0, NAMES[0]), plain_record(flow, 1, NAMES[1]), aligned_record(flow, 2, NAMES[2])])
    assert recs[1]["V_hand"] == 0 and "icp_trans" not in recs[1] and "icp_skipped" not in recs[1]
    assert flow.report(0, 3) == flow.expected_report(0, 3, (0, 1, 2), 128)


# ---- F: label files --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("viz", [False, True])
def test_label_files_carry_the_hands_transform(tmp_path, monkeypatch, viz):
    flow = Flow(tmp_path, monkeypatch, labels=True)
    flow.ground_truth(NAMES[:2])
    recs = flow.run(0, 2, eval_mode=True, label_out=True, viz=viz)
    assert flow.events("pipeline") == [("pipeline", flow.decoder, 128, "reference", True, True, True, None)]
    extra = ["_hand_label.npz"] + (["_hand_label.obj", "_hand_color.ply"] if viz else [])
    assert sorted(os.listdir(flow.mesh_dir)) == sorted(n + e for n in NAMES[:2] for e in ["_hand.ply", "_obj.ply"] + extra)
    want = []
    for i in (0, 1):
        r = flow.results[i]
        check_aligned_sample(flow, i)
        labels = dict.__getitem__(r, "host_labels_hand")
        whole = place_vertices(dict.__getitem__(r, "host_verts_hand"), dict.__getitem__(r, "host_faces_hand"), ORIGIN, VOXEL)[2]
        z = np.load(os.path.join(flow.mesh_dir, NAMES[i] + "_hand_label.npz"))
        assert sorted(z.files) == ["labels", "points"]
        assert z["labels"].dtype == np.float32 and np.array_equal(z["labels"], labels.numpy().astype(np.float32))
        assert np.array_equal(z["points"], whole * SCALE.reshape(1) + TRANS.reshape(1, 3))
        want.append(dict(aligned_record(flow, i, NAMES[i]), labels_hand=np.bincount(labels.numpy(), minlength=1).tolist()))
        if viz:
            with open(os.path.join(flow.mesh_dir, NAMES[i] + "_hand_label.obj")) as f:
                lines = f.read().splitlines()
            pts = (whole * SCALE.reshape(1) + TRANS.reshape(1, 3)).tolist()
            assert lines == ["v %.4f %.4f %.4f %.2f %.2f %.2f" % (p[0], p[1], p[2], 45.0 * c, 45.0 * c, 45.0 * c)
                             for p, c in zip(pts, labels.tolist())]
            with open(os.path.join(flow.mesh_dir, NAMES[i] + "_hand_color.ply")) as f:
                head = f.read().splitlines()
            assert head[2] == "element vertex %d" % len(whole) and "property uchar red" in head
    same_records(recs, want)


def test_viz_without_labels_writes_no_label_files(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    flow.run(0, 1, viz=True)
    assert sorted(os.listdir(flow.mesh_dir)) == ["%s_hand.ply" % NAMES[0], "%s_obj.ply" % NAMES[0]]


# ---- G: strided range, failing on_record ---------------------------------------------------------------------------------------
def test_strided_range(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    recs = flow.run(1, 8, stride=2, cube_dim=24)
    same_records(recs, [plain_record(flow, i, NAMES[i]) for i in (1, 3, 5, 7)])
    assert [e[1:] for e in flow.events("codes")] == [(NAMES[i], i) for i in (1, 3, 5, 7)]
    assert flow.report(1, 8) == flow.expected_report(1, 8, (1, 3, 5, 7), 24, stride=2)
    assert sorted(os.listdir(flow.mesh_dir)) == sorted("%s_%s.ply" % (NAMES[i], p) for i in (1, 3, 5, 7) for p in ("hand", "obj"))


def test_failing_on_record_keeps_what_was_finished(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    seen = []

    def on_record(rec):
        seen.append(rec)
        if len(seen) == 2:
            raise RuntimeError("records file is gone")

    with pytest.raises(RuntimeError, match="records file is gone") as err:
        flow.run(0, 7, stride=2, cube_dim=24, on_record=on_record)
    same_records(err.value.partial_records, [plain_record(flow, i, NAMES[i]) for i in (0, 2)])
    assert seen == err.value.partial_records
    assert flow.report(0, 7) == flow.expected_report(0, 7, (0, 2), 24, stride=2)
    assert sorted(os.listdir(flow.mesh_dir)) == sorted("%s_%s.ply" % (NAMES[i], p) for i in (0, 2) for p in ("hand", "obj"))
    assert no_helper_threads()


# ---- H: a failing PLY write ----------------------------------------------------------------------------------------------------
def test_failed_ply_write_surfaces_one_sample_later(tmp_path, monkeypatch, caplog):
    flow = Flow(tmp_path, monkeypatch)
    os.makedirs(flow.mesh(NAMES[1], "hand"))                          # a directory where the file should go: open() fails
    with caplog.at_level(logging.ERROR), pytest.raises(OSError) as err:
        flow.run(0, 5)
    # sample 1's hand write fails on the writer thread; the next write that polls it raises - the object of the same sample if the
    # failure is in by then, the hand of sample 2 otherwise - and never later
    partial = err.value.partial_records
    assert len(partial) in (1, 2)
    same_records(partial, [plain_record(flow, i, NAMES[i]) for i in range(len(partial))])
    assert flow.on_records == partial
    assert any("PLY write of %s failed" % flow.mesh(NAMES[1], "hand") in m for m in caplog.messages)
    assert not os.path.exists(flow.mesh(NAMES[2], "obj")) and not os.path.exists(flow.mesh(NAMES[3], "hand"))
    assert os.path.exists(flow.mesh(NAMES[0], "hand")) and os.path.exists(flow.mesh(NAMES[0], "obj"))
    assert flow.report(0, 5)["samples"] == len(partial) and no_helper_threads()


def test_code_source_is_required(tmp_path, monkeypatch):
    flow = Flow(tmp_path, monkeypatch)
    with pytest.raises(ValueError, match="needs a code_source"):
        rc.reconstruct(flow.decoder, {}, flow.split, flow.out, 0, 2)
    assert not flow.writers and not flow.events("pipeline") and no_helper_threads()
