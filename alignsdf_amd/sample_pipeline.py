"""The sample pipeline behind reconstruct(), dist_reconstruct, bench.py and the tools.  decoder_for, bind_sample and marching cubes are
looked up through their modules at call time (tests/test_pipeline_order.py replaces them there)."""
import dataclasses
import os

import torch

from . import marching_cubes as mc
from .utils import mesh as mesh_utils, utils


def pipelined_two_pass(decoder, specs, samples, N, grid_mode="reference", host_copy=False, label_out=False, midpoint=None, report=None,
                       fast=None, normals=False, render=None, polish=False, interaction=None):
    """Software pipeline over independent samples.  `samples` yields (key, latent, mano_results, obj_results); the
    generator yields (key, result) in order, where result holds the pass-2 volumes (device), the zoom cube and the
    marching-cubes output per enabled branch (`verts_*`, `faces_*` device tensors, absent when MC found no surface).

    The pipeline exists to produce meshes: it runs the coarse pass through `coarse_begin` / `coarse_finish` and the fine pass
    through `fine_begin(..., mc_only=True)`.  By default (round 6) both are ORDINARY sweeps: every voxel of both lattices in the
    reference's arithmetic class (<= 1e-5).  `fast=True` (or ASDF_FAST=1 / `--fast`; `fast=None` leaves the decoder as it is
    configured) opts in to the audited one-plane sweeps wherever the decoder supports them - the yielded `vol_*` are then exact only
    where marching cubes reads values and must not be used as SDF volumes.

    Per sample the GPU work is  pass 1 -> [64-byte bbox readback, zoom cube on the host] -> pass 2 -> marching cubes,
    and only the bracketed step and the MC size readbacks synchronise with the host.  Pass 1 of sample k+1 is queued
    right behind pass 2 of sample k, i.e. before sample k's marching cubes and before the consumer's host work
    (D2H copy, component filter, PLY export), so the GPU never waits for the host between samples.

    host_copy=True additionally runs the largest-component filter (K8) behind each marching cubes and copies its result
    to pinned host memory on a side stream (`host_kept_verts_*`, `host_kept_faces_*` at input capacity, `host_kept_counts_*`
    = kept vertices / faces, valid after `copy_done_*`.synchronize(); with label_out also the whole surface as
    `host_verts_hand` / `host_faces_hand`): a plain `.cpu()` on the compute stream would wait behind the NEXT sample's
    queued passes.

    label_out=True runs the label pass (utils/mesh.py:137-157) over the hand mesh vertices right behind the hand's
    marching cubes (`labels_hand`, int64 device tensor; `host_labels_hand` with host_copy).  The decoder holds one
    sample's folded constants at a time, so sample k is re-bound for it and sample k+1 bound again afterwards.

    midpoint(key, result), if given, is called for sample k between queuing pass 2 of sample k+1 and pass 1 of sample
    k+2: GPU work it enqueues (the eval-mode ICP of sample k's hand mesh) lands between two decoder passes instead of
    behind both, and its host part is covered by the pass that is already running.

    normals=True (with host_copy) runs the normal pass behind K8: the analytic SDF gradient of the surface's own head at every kept
    vertex (decode_points_grad at origin + v * voxel_size), normalised, (0, 0, 0) where it has no direction - `kept_normals_*` on the
    device, `host_kept_normals_*` at input capacity with the other copies.  The sample is re-bound first, as for the label pass.  A
    decoder the gradient kernel does not cover raises NotImplementedError before the first sweep.

    render = {"size": (H, W), "camera": key -> (cam_intr, root_joint), "trace": parameters of trace_rays} runs the render pass where the
    normal pass runs, with the same re-bind: one view of the sample ray-cast from the decoder inside the sample's zoom cube
    (render.render_view; a decoder the tracing kernel refuses is traced on the module path, render.view_evaluator, chosen before the
    first sweep) - `render` in the result (its maps on the device), `host_render_*` with host_copy.

    polish=True (with host_copy) runs the polish pass right behind K8 and BEFORE the normal pass, the host copies and the eval-mode
    hook: every kept vertex is moved onto the zero level of its surface's own head by Newton projection inside one kernel
    (project.polish_vertices: project_points at origin + v * voxel_size with a trust box of one fine voxel per axis; a vertex keeps its
    marching-cubes position where the projection is BAD or STALLED or ends with a larger |sdf| than it began with).  The kept vertices
    everything downstream sees - surface sampling and ICP, normals, files - are the polished ones; faces are untouched.  The counts by
    status and of vertices kept in place: `polish_counts_*` on the device, `host_polish_counts_*` with the other copies.  The sample
    is re-bound first, as for the normal pass.  A decoder that cannot project raises NotImplementedError before the first sweep.

    interaction={"contact_m": 0.005} (with host_copy; None = off) runs the interaction pass (interaction.interaction_pass) inside
    post-processing - the fine pass is accepted by then and `vol_*` are final -, behind K8 and the polish pass of BOTH surfaces and
    before the normal pass and the host copies: the overlap of the two fine volumes by sign, and per surface the OTHER head's SDF at its
    kept (polished) vertices, reduced on the device with K8's kept count read there.  `interaction` in the result (device: "words",
    "other_sdf_<part>"), `host_interaction` (int32 [interaction.WORDS]) and `host_other_sdf_<part>` at input capacity behind
    `copy_done_interaction`, and `interaction_contact_m`.  In the decoder's own frame, before the eval-mode hook.  The sample is re-bound
    first, as for the normal pass.  ValueError before the first sweep when a branch is off, or without host_copy.

    report, if given (a dict), receives the evaluator that ran and a snapshot of its sweep counters (see write_sweeps_json)."""
    yield from SamplePipeline(decoder, specs, samples, N, grid_mode, host_copy, label_out, midpoint, report, fast, normals, render, polish,
                              interaction).run()


@dataclasses.dataclass(slots=True, eq=False)
class InFlight:
    """One sample on its way through the pipeline."""
    key: object
    codes: list                        # (latent, mano_results, obj_results)
    coarse: object = None              # the ticket of a step-by-step coarse pass ...
    speculative: dict = None           # ... or that of a sample enqueued in one go (two_pass_begin); the other is None
    fine_ticket: object = None
    mc_tickets: dict = None            # part -> marching-cubes ticket, once the count phases are queued
    result: dict = dataclasses.field(default_factory=lambda: {"V_hand": 0, "F_hand": 0, "V_obj": 0, "F_obj": 0})     # what the caller gets


class SamplePipeline:
    """pipelined_two_pass: the decoder and the state its stages share, one method per stage, and the window over the samples (run)."""

    def __init__(self, decoder, specs, samples, N, grid_mode, host_copy, label_out, midpoint, report, fast, normals=False, render=None, polish=False,
                 interaction=None):
        self.specs, self.N, self.host_copy, self.label_out, self.midpoint = specs, N, host_copy, label_out, midpoint
        self.normals, self.render, self.polish = bool(normals), render, bool(polish)
        self.contact_m = None                      # the contact distance of the interaction pass; None = the pass is off
        if interaction is not None and interaction is not False:
            from .interaction import check_option
            self.contact_m = check_option(interaction, specs)      # (before the first sweep: both branches are needed)
            if not host_copy:
                # (the pass measures K8's kept vertices, which exist with host_copy only: no run that quietly reports nothing)
                raise ValueError("interaction needs host_copy=True: it measures the kept vertices of the component filter")
        self.samples = (InFlight(key, codes) for key, *codes in samples)   # (lazy: a sample is fetched when the window asks for it)
        self.head = next(self.samples, None)
        if self.head is None:                      # (an empty stream: no decoder is asked for)
            return
        # the HIP kernels, or the module on PyTorch-ROCm for variants they do not cover
        self.hip = hip = utils.decoder_for(decoder, specs, self.head.codes[1])
        if self.normals:
            mesh_utils.require_normals(hip)        # (before the first sweep: no run of files without the normals that were asked for)
        if self.polish:
            from .project import require_polish
            require_polish(hip)                    # (before the first sweep as well)
        if self.render is not None:
            # (before the first sweep as well: the evaluator the views are traced on - `hip`, or the module for a decoder whose sweeps
            # are native and which the tracing kernel refuses)
            from .render import view_evaluator
            self.view_eval = view_evaluator(hip, decoder, specs)
        if fast is not None and hasattr(hip, "set_fast"):
            hip.set_fast(bool(fast))
        if report is not None:                     # (the caller's `sweeps.json`: which evaluator ran, and its counters at the start)
            report["evaluator"], report["snapshot"] = hip, hip.sweep_snapshot()
        self.on = {"hand": specs.get("HandBranch", True), "obj": specs.get("ObjectBranch", True)}
        # the enabled (marching-cubes slot, part) pairs: the object's volume takes slot 1 whether or not the hand is on
        self.parts = [(slot, part) for slot, (part, on) in enumerate((("hand", self.on["hand"]), ("obj", self.on["obj"]))) if on]
        self.mode, self.voxel = mesh_utils.GRID_MODES[grid_mode], 2.0 / (N - 1)
        self.copy_stream = torch.cuda.Stream(device=hip.device) if host_copy else None
        # Round 5: wherever the decoder's state allows it (HipSdfDecoder.can_speculate: both one-plane modes on, both
        # whole-lattice comparisons valid, none due) a sample is ENQUEUED IN ONE GO - coarse box sweep, zoom cube on the device, narrow-band
        # fine sweep on that lattice, marching-cubes counts and a capacity-bounded emit - and the host only reads records afterwards: no
        # host round trip between the coarse and the fine pass, none between count and emit.  A refused sweep is repeated step by step, as
        # before.  ASDF_SPECULATE=0 keeps every sample on the step-by-step path.
        self.speculate = os.environ.get("ASDF_SPECULATE", "1") != "0" and hasattr(hip, "two_pass_begin")
        self.seen = {}       # part -> (most vertices, most faces) of the surfaces so far: sizes the next sample's emit buffers
        self.bound = None    # the sample whose folded constants the decoder holds

    def bind(self, s):
        utils.bind_sample(self.hip, self.specs, *s.codes)
        self.bound = s

    def sweep(self, begin, *lattice, **kw):
        return begin(self.N, *lattice, self.mode, hand=self.on["hand"], obj=self.on["obj"], **kw)

    def begin_counts(self, s):
        # count phases of both volumes (no host synchronisation)
        s.mc_tickets = {part: mc.marching_cubes_begin(s.result["vol_" + part], 0.0, slot) for slot, part in self.parts}

    def enqueue(self, s):
        """Pass 1 of a sample - or, where the decoder speculates, the whole sample in one go."""
        self.bind(s)
        s.speculative = self.sweep(self.hip.two_pass_begin, self.voxel) if self.speculate else None
        if s.speculative is None:
            s.coarse = self.sweep(self.hip.coarse_begin, [-1.0, -1.0, -1.0], self.voxel)
            return
        # marching cubes right behind the fine pass - count AND capacity-bounded emit - once the sizes of earlier surfaces are known.  (Never
        # the count alone: its emit would run when the sample is finished, after the NEXT sample's count phase has reused the workspace -
        # found as a memory fault at N = 128.  Without sizes to go by the sample's marching cubes waits for surfaces().)
        if all(part in self.seen for _, part in self.parts):
            caps = {part: (int(1.5 * self.seen[part][0]) + 4096, int(1.5 * self.seen[part][1]) + 8192) for _, part in self.parts}
            s.mc_tickets = {part: mc.marching_cubes_begin(s.speculative["vol_" + part], 0.0, slot, capacity=caps[part])
                            for slot, part in self.parts}

    def enqueue_fine(self, s, b=None):
        """Pass 2 of a sample from its finished coarse record: the zoom cube on the host, then the sweep."""
        if b is None:
            # waits for pass 1 (the zoom cube is data dependent); a coarse sweep whose guards fired (fp16 range, or the error check of the
            # box-only sweep) is repeated in there - the decoder is still bound to this sample
            b = self.hip.coarse_finish(s.coarse)
        nvs, norg = mesh_utils.zoom_cube_of_record(b, self.on["hand"], self.on["obj"], self.N, self.voxel)
        # the fine pass carries a guard record (fp16 range report; error check of the narrow-band sweep): read behind the marching-cubes
        # size read-back in surfaces().  The volumes go to marching cubes only (mc_only).
        vh, vo, s.fine_ticket = self.sweep(self.hip.fine_begin, norg.tolist(), nvs.item(), mc_only=True)
        s.result.update({"vol_hand": vh, "vol_obj": vo, "voxel_size": nvs, "origin": norg.tolist(), "bbox": b})

    def settle(self, s):
        """A sample that was enqueued in one go: judge its coarse record now (everything of it has long run).  Accepted - the usual
        case - means the fine pass ran on exactly the lattice the host arithmetic gives for these boxes (asdf_zoom_cube)."""
        spec = s.speculative
        judged = self.hip.coarse_judge(spec["coarse"])
        if judged[0]:
            origin, nvs = self.hip.lattice_of(spec)
            s.fine_ticket = spec["fine"]
            s.result.update({"vol_hand": spec["vol_hand"], "vol_obj": spec["vol_obj"], "voxel_size": nvs, "origin": origin, "bbox": judged[1]})
        else:
            self.bind(s)                           # refused: this sample again, step by step - and its marching cubes with it
            s.mc_tickets = None
            self.enqueue_fine(s, self.hip.coarse_finish(spec["coarse"], judged=judged))     # (an ordinary sweep now)

    def surfaces(self, s):
        """Marching cubes of one sample: settle it if it is speculative, count, repeat a refused fine pass and its counts, finish."""
        if s.speculative is not None:
            self.settle(s)
        r = s.result
        # the count phases are queued BEFORE the fine pass's guard record is read (it is accepted all but never refused): one host wait then
        # covers the record and the sizes, instead of record -> launch -> sizes with the GPU idle in between (a sample enqueued in one go
        # brings its marching-cubes tickets along: counted, and usually emitted, behind its fine pass)
        if not s.mc_tickets:
            self.begin_counts(s)
        while self.hip.fine_needs_repeat(s.fine_ticket):
            # pass 2 left the fp16 range (the decoder has been re-calibrated, or switched to the fp32 kernel) or its narrow-band form was
            # not accepted: repeat this sample's pass 2 - and its count phases
            self.bind(s)
            r["vol_hand"], r["vol_obj"], s.fine_ticket = self.sweep(self.hip.fine_begin, r["origin"], float(r["voxel_size"]), mc_only=True)
            self.begin_counts(s)
        for _, part in self.parts:
            try:
                v, f = mc.marching_cubes_finish(s.mc_tickets[part])
            except (ValueError, RuntimeError) as e:             # the reference logs and skips (utils/mesh.py:353-358)
                r["mc_error_" + part] = str(e)
                continue
            r["verts_" + part], r["faces_" + part] = v, f
            r["V_" + part], r["F_" + part] = v.shape[0], f.shape[0]
            c = self.seen.get(part, (0, 0))
            self.seen[part] = (max(c[0], v.shape[0]), max(c[1], f.shape[0]))

    def to_host(self, r, key, t):
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.hip.device))
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            h.copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        t.record_stream(self.copy_stream)
        r["host_" + key] = h
        return done

    def post_process(self, s):
        """Label pass, component filter, normal pass and host copies of the surfaces marching cubes found; the render pass."""
        r = s.result
        self.post_process_surfaces(s, r)
        if self.render is not None:
            # one view of the sample, marched inside its zoom cube (the region the meshes come from: the field far outside the clamp is
            # unconstrained) - the decoder holds the next sample's constants by now
            from .render import render_view
            if self.view_eval is not self.hip:
                utils.bind_sample(self.view_eval, self.specs, *s.codes)
            elif self.bound is not s:
                self.bind(s)
            H, W = self.render["size"]
            lo = [float(v) for v in r["origin"]]
            hi = [v + (self.N - 1) * float(r["voxel_size"]) for v in lo]
            view = render_view(self.view_eval, *self.render["camera"](s.key), self.specs["SdfScaleFactor"], H, W, box=(lo, hi), **self.render["trace"])
            r["render"] = dict(view, size=(H, W), trace=dict(self.render["trace"]))
            if self.host_copy:
                for name, t in view.items():
                    r["copy_done_render"] = self.to_host(r, "render_" + name, t)

    def post_process_surfaces(self, s, r):
        """The per-surface part of post_process; with the interaction pass, K8 and the polish pass of both surfaces come first, then
        that pass, then what is left per surface (copy_surface)."""
        finish = []          # with the interaction pass: what follows it per surface (normal pass, host copies)
        for _, part in self.parts:
            if "verts_" + part not in r:
                continue
            v, f = r["verts_" + part], r["faces_" + part]
            if self.label_out and part == "hand":
                # the vertex arithmetic of utils/mesh.py:138-141 in fp32, on the device
                pts = v * float(r["voxel_size"]) + torch.tensor(r["origin"], dtype=torch.float32, device=v.device)
                self.bind(s)
                r["labels_hand"] = self.hip.classify_points(pts, want_sdf=False)[3]
            if self.host_copy:
                # K8 right behind marching cubes: only the largest component (what the file holds) crosses to the host, plus the whole
                # surface when the label pass needs every vertex
                from .mesh_post import keep_largest_component_device
                kv, kf, counts = keep_largest_component_device(v, f, r["voxel_size"], r["origin"])
                polished = None
                if self.polish:
                    # the polish pass, on the kept vertices (rows past the kept count hold no vertex: they are projected along, never
                    # counted and never read) - the decoder holds the next sample's constants by now
                    from .project import polish_vertices
                    if self.bound is not s:
                        self.bind(s)
                    kv, polished = polish_vertices(self.hip, kv, r["origin"], r["voxel_size"], part, count=counts[0])
                    r["polish_counts_" + part] = polished
                r["kept_dev_" + part] = (kv, kf, counts)       # (the eval-mode hook samples the kept surface on the device)
                if self.contact_m is None:
                    self.copy_surface(s, r, part, v, f, polished)
                else:
                    finish.append((part, v, f, polished))
        if self.contact_m is not None:
            # the interaction pass, once both surfaces have their kept (polished) vertices and before anything of them is copied - the
            # decoder holds the next sample's constants by now
            from .interaction import interaction_pass
            if self.bound is not s:
                self.bind(s)
            r["interaction"] = res = interaction_pass(self.hip, r, self.specs, self.contact_m)
            r["interaction_contact_m"] = self.contact_m
            for args in finish:
                self.copy_surface(s, r, *args)
            for name, t in res.items():
                r["copy_done_interaction"] = self.to_host(r, "interaction" if name == "words" else name, t)

    def copy_surface(self, s, r, part, v, f, polished):
        """Normal pass and host copies of one surface behind K8 (and the polish pass)."""
        kv, kf, counts = r["kept_dev_" + part]
        copies = {"kept_verts_": kv, "kept_faces_": kf, "kept_counts_": counts}
        if polished is not None:
            copies["polish_counts_"] = polished
        if self.normals:
            # the normal pass, on the kept vertices (rows past the kept count hold no vertex: whatever comes out of them is
            # never read) - the decoder holds the next sample's constants by now
            if self.bound is not s:
                self.bind(s)
            res = self.hip.decode_points_grad(mesh_utils.lattice_points(kv, r["origin"], r["voxel_size"]), hand=part == "hand",
                                              obj=part == "obj")
            r["kept_normals_" + part] = copies["kept_normals_"] = mesh_utils.unit_normals(res[1] if part == "hand" else res[3])
        if "labels_" + part in r:
            copies.update({"verts_": v, "faces_": f, "labels_": r["labels_" + part]})
        for name, t in copies.items():
            r["copy_done_" + part] = self.to_host(r, name + part, t)       # the side stream is in order: the last event covers all

    def run(self):
        """The window: sample k (`cur`) is finished while k+1 (`nxt`) is in the queue and k+2 (`after`) is fetched and enqueued."""
        cur = self.head
        if cur is None:
            return
        self.enqueue(cur)
        if cur.coarse is not None:
            self.enqueue_fine(cur)
        nxt = next(self.samples, None)
        if nxt is not None:
            self.enqueue(nxt)
        while cur is not None:
            # fetch sample k+2 while the queue is short: a source that uploads its codes with a blocking copy would otherwise sit behind
            # pass 2 of sample k+1 and hold the consumer back for a whole pass
            after = next(self.samples, None) if nxt is not None else None
            self.surfaces(cur)                     # MC of sample k, queued behind pass 1 of sample k+1
            if nxt is not None:
                # pass 2 of the next sample goes in once the marching-cubes launches are queued (it may overwrite the volumes only behind
                # the emits) and BEFORE the component filter, label pass and host copies are: the ~40 small launches of the post-processing
                # never sit between a pass-1 read-back and the pass-2 launch (eval-mode trace: 1.3 ms of idle GPU per sample).  The decoder
                # is bound to the next sample again if this one had to be repeated.  Of a sample enqueued in one go both passes are in
                # flight already: nothing to launch, and nothing is READ here either - its records are judged when it is finished (settle),
                # so the host never waits in the middle of this sample's post-processing.
                if self.bound is not nxt:
                    self.bind(nxt)
                if nxt.coarse is not None:
                    self.enqueue_fine(nxt)
            self.post_process(cur)
            if self.midpoint is not None:
                self.midpoint(cur.key, cur.result)
            if after is not None:
                self.enqueue(after)
            yield cur.key, cur.result
            cur, nxt = nxt, after
