"""Drop-in counterpart of the reference's utils/mesh.py hot path (create_mesh_combined_decoder,
get_higher_res_cube, convert_sdf_samples_to_ply) on the HIP kernels.

Signatures follow utils/mesh.py:17, :198 and :331.  Volumes stay on the device; only the extracted mesh
(verts / faces) is copied to the host for export.  There is no CPU path: without the HIP library or an
MI355X the functions raise.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from .. import _native
from ..marching_cubes import marching_cubes_device
from ..mesh_post import keep_largest_component_device
from ..ply import write_ply
from .utils import bind_sample, decoder_for

GRID_MODES = {"reference": _native.GRID_REFERENCE, "integer": _native.GRID_INTEGER}


def neg_bbox(volume):
    """int32[7] host array (min0,min1,min2,max0,max1,max2,count) of the voxels with value < 0 of a device volume."""
    vol = volume.detach().to(torch.float32).contiguous()
    if not vol.is_cuda:
        raise TypeError("neg_bbox needs a CUDA tensor (there is no CPU fallback)")
    out = torch.empty(16, dtype=torch.int32, device=vol.device)
    with torch.cuda.device(vol.device):
        _native.check(_native.lib().asdf_neg_bbox(vol.data_ptr(), vol.shape[0], vol.shape[1], vol.shape[2], out.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(vol.device).cuda_stream)),
                      "asdf_neg_bbox")
    return out[:7].cpu().numpy()


def zoom_cube_from_bboxes(bboxes, N, voxel_size):
    """The fp32 arithmetic of get_higher_res_cube (utils/mesh.py:239-254) on per-branch bounding boxes
    [(min3, max3, count)]; an empty branch contributes zeros (utils/mesh.py:209-211,225-227).
    Returns (new_voxel_size 0-dim fp32 tensor, new_origin [3] fp32 tensor) on the CPU, like the reference."""
    los, his = [], []
    for lo, hi, count in bboxes:
        if count == 0:
            los.append(torch.zeros(3)); his.append(torch.zeros(3))
        else:
            los.append(torch.tensor([float(v) for v in lo])); his.append(torch.tensor([float(v) for v in hi]))
    min_index = los[0] if len(los) == 1 else torch.min(los[0], los[1])
    max_index = his[0] if len(his) == 1 else torch.max(his[0], his[1])
    new_cube_size = (torch.max(max_index - min_index) + 4) * voxel_size
    new_voxel_size = new_cube_size / (N - 1)
    new_origin = (min_index - 2) * voxel_size - 1.0
    return new_voxel_size, new_origin


def zoom_cube_of_record(record, hand_branch, obj_branch, N, voxel_size):
    """The zoom cube of a box / sweep record (the hand's box at head 0, the object's at head 1).  A branch that is switched off is not
    used for the zoom cube (utils/mesh.py:239-247)."""
    boxes = [_native.box_of(record, head) for head, on in enumerate((hand_branch, obj_branch)) if on]
    return zoom_cube_from_bboxes(boxes, N, voxel_size)


def get_higher_res_cube(hand_branch, obj_branch, sdf_values_hand, sdf_values_obj, N, voxel_origin, voxel_size):
    """Zoom cube around the negative voxels of the enabled branches (utils/mesh.py:198-256)."""
    record = np.zeros(_native.BOX_WORDS, dtype=np.int32)
    for head, (on, vol) in enumerate(((hand_branch, sdf_values_hand), (obj_branch, sdf_values_obj))):
        if on:
            record[_native.BOX_STRIDE * head:][:_native.BOX_RANGE] = neg_bbox(vol)
    return zoom_cube_of_record(record, hand_branch, obj_branch, N, voxel_size)


def place_vertices(verts_d, faces_d, voxel_grid_origin, voxel_size, offset=None, scale=None):
    """MC output (device or already-copied host tensors) -> host arrays with the vertex arithmetic of
    utils/mesh.py:354-369 (spacing, origin, optional scale / offset).  Returns (verts, faces, mesh_points)."""
    verts, faces = verts_d.cpu().numpy(), faces_d.cpu().numpy()
    vs = voxel_size.item() if isinstance(voxel_size, torch.Tensor) else voxel_size
    spacing = [np.float32(vs)] * 3 if isinstance(voxel_size, torch.Tensor) else [vs] * 3
    if not np.array_equal(spacing, (1, 1, 1)):
        verts = verts * np.r_[spacing]
    mesh_points = np.zeros_like(verts)
    for a in range(3):
        mesh_points[:, a] = voxel_grid_origin[a] + verts[:, a]
    if scale is not None:
        mesh_points = mesh_points * scale
    if offset is not None:
        mesh_points = mesh_points + offset
    return verts, faces, mesh_points


def ground_truth_mesh_path(ply_filename_out, task, data_root="data"):
    """Where the reference looks for the ground-truth mesh of an output file (utils/mesh.py:386-388):
    <data_root>/<task>/test/mesh_<hand|obj>/<sample id>.obj."""
    mesh_dir = "mesh_" + ply_filename_out.split("_")[-1].split(".")[0]
    gt_mesh_name = ply_filename_out.split("/")[-1].split("_")[0] + ".obj"
    return os.path.join(data_root, task, "test", mesh_dir, gt_mesh_name)


def apply_icp(job, points):
    """Wait for the eval-mode ICP enqueued for a surface (icp.start_alignment / start_alignment_device) and apply it to its placed
    vertices.  Returns (points, trans [1,3], scale [1]); without a job the points as they are and zeros / one, like the reference
    outside eval mode."""
    if job is None:
        return points, np.array([0, 0, 0]), np.array([1])
    from ..icp import finish_icp
    r = finish_icp(job, points)
    return r["vertices"], np.asarray(r["all_trans"]).reshape(1, 3), np.asarray(r["all_scale"]).reshape(1)


def normals_refusal(evaluator):
    """Why (a string) this evaluator cannot give SDF gradients, or None: the native gradient kernel covers SeparateDecoder with point
    features affine in xyz (hip_decoder.grad_refusal); the module path differentiates whatever it evaluates."""
    refusal = getattr(evaluator, "grad_refusal", None)
    return refusal() if callable(refusal) else None


def require_normals(evaluator):
    """Raise before anything is swept or written when `evaluator` cannot give the gradients vertex normals are made of."""
    why = normals_refusal(evaluator)
    if why is not None:
        raise NotImplementedError("vertex normals need the SDF gradient, which the native kernel does not cover here: %s" % why)


def unit_normals(grad):
    """grad [V, 3] (device) -> grad / |grad|, (0, 0, 0) where the gradient has zero length or is not finite.  The SDF is negative
    inside, so the normals point out of the shape."""
    length = torch.linalg.vector_norm(grad, dim=1, keepdim=True)
    ok = torch.isfinite(length) & (length > 0)
    return torch.where(ok, grad / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(grad))


def lattice_points(verts_d, voxel_grid_origin, voxel_size):
    """Marching-cubes vertices (lattice units, device) -> their normalised fp32 positions origin + v * voxel_size, on the device (the
    vertex arithmetic of utils/mesh.py:138-141): where the normal pass evaluates the decoder.  Spacing and origin travel as launch
    arguments - no host-to-device copy, so nothing here waits for the stream."""
    pts = verts_d * float(voxel_size)
    for a in range(3):
        pts[:, a] += float(voxel_grid_origin[a])
    return pts


def count_degenerate(normals):
    """Number of (0, 0, 0) rows of a host array of unit normals."""
    return int((~np.asarray(normals).any(axis=1)).sum())


class VertexNormals:
    """points [V, 3] (normalised coordinates, device) -> unit normals [V, 3] of one surface: grad / |grad| of the surface's own head
    of the BOUND evaluator (HipSdfDecoder / TorchModuleDecoder.decode_points_grad).  `degenerate` is the number of (0, 0, 0) normals of
    the last call."""

    def __init__(self, evaluator, part):
        require_normals(evaluator)
        self.evaluator, self.part, self.degenerate = evaluator, part, 0

    def __call__(self, points):
        res = self.evaluator.decode_points_grad(points, hand=self.part == "hand", obj=self.part == "obj")
        grad = res[1] if self.part == "hand" else res[3]
        if grad is None:
            raise ValueError("the evaluator has no %s head to take normals from" % self.part)
        n = unit_normals(grad)
        self.degenerate = int((~n.any(dim=1)).sum().item())
        return n


def _normals_callable(normals, ply_filename_out, part=None):
    """The `normals` option of export_surface: a callable as it is; an evaluator with decode_points_grad -> VertexNormals of head
    `part` ("hand" / "obj"; None: the head the file name ends in, <name>_hand.ply / <name>_obj.ply, as ground_truth_mesh_path reads
    it)."""
    if not normals:
        return None
    if hasattr(normals, "decode_points_grad"):
        part = part or str(ply_filename_out).split("_")[-1].split(".")[0]
        if part not in ("hand", "obj"):
            raise ValueError("normals from an evaluator need normals_part=\"hand\" / \"obj\" or a file name that ends in _hand.ply / "
                             "_obj.ply (got %r)" % (ply_filename_out,))
        return VertexNormals(normals, part)
    if not callable(normals):
        raise TypeError("normals: a bound evaluator (decode_points_grad) or a callable points -> unit normals")
    return normals


def _polish_callable(polish, ply_filename_out, part=None):
    """The `polish` option of export_surface: a callable as it is; an evaluator with project_points -> project.VertexPolish of head
    `part` (None: the head the file name ends in, as for the normals)."""
    if not polish:
        return None
    if hasattr(polish, "project_points"):
        from ..project import VertexPolish
        part = part or str(ply_filename_out).split("_")[-1].split(".")[0]
        if part not in ("hand", "obj"):
            raise ValueError("polish on an evaluator needs normals_part=\"hand\" / \"obj\" or a file name that ends in _hand.ply / "
                             "_obj.ply (got %r)" % (ply_filename_out,))
        return VertexPolish(polish, part)
    if not callable(polish):
        raise TypeError("polish: a bound evaluator (project_points) or a callable (verts, origin, voxel_size) -> verts")
    return polish


def export_surface(verts_d, faces_d, voxel_grid_origin, voxel_size, ply_filename_out, offset=None, scale=None, eval_mode=False,
                   task="obman", largest_component=True, data_root="data", kept=None, allow_missing_gt=False, normals=False,
                   normals_part=None, polish=False, kept_out=None):
    """The host tail of convert_sdf_samples_to_ply for an already extracted surface (utils/mesh.py:360-397): place_vertices, the
    largest-component filter, in eval mode the translate+scale ICP (K7) against the ground-truth mesh, export.
    Returns (verts, faces, trans, scale).  `kept` = (verts, faces) of the largest component in lattice units when the caller has
    already run the device filter; otherwise the surface is filtered here on the device (K8; host arrays are uploaded for it -
    there is no host implementation in the product).  A missing ground-truth file aborts like the reference (its trimesh.load
    raises at utils/mesh.py:389) - a wrong data_root must not produce a full run of silently unaligned meshes; with
    allow_missing_gt the mesh is written unaligned.
    `normals`: the bound evaluator, or a callable that maps normalised points (device, [V, 3]) to unit normals - the file then carries
    nx / ny / nz per vertex, evaluated at origin + v * voxel_size of the written vertices (before offset, scale and ICP: a
    translation and a positive uniform scale leave a normal as it is).  An evaluator gives the normals of head `normals_part`
    ("hand" / "obj"; by default the one the file name ends in).
    `polish`: the bound evaluator, or a callable (verts in lattice units on the device, origin, voxel_size) -> verts - the vertices
    that are written (the kept component, or the whole surface without the filter) are moved onto the zero level of head `normals_part`
    behind the filter and before everything else: the ICP, the normals and the file see the polished positions; faces stay.
    `kept_out` (a dict, optional) receives under "kept" the written surface as it stands on the device, in lattice units: (verts, faces,
    counts) - the kept component, polished where that is on; counts = K8's int32 record when the filter ran here, else None."""
    normals = _normals_callable(normals, ply_filename_out, normals_part)
    polish = _polish_callable(polish, ply_filename_out, normals_part)
    counts = None
    if kept is None and largest_component:
        vd = verts_d if isinstance(verts_d, torch.Tensor) else torch.as_tensor(np.asarray(verts_d))
        fd = faces_d if isinstance(faces_d, torch.Tensor) else torch.as_tensor(np.asarray(faces_d))
        kv, kf, counts = keep_largest_component_device(vd.cuda().float(), fd.cuda().int(), voxel_size, voxel_grid_origin)
        c = counts.cpu().numpy()                   # (synchronises)
        kept = kv[:c[0]], kf[:c[1]]
    if polish is not None:
        target = kept[0] if kept is not None else verts_d
        target = target if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target))
        moved = polish(target.cuda().float(), voxel_grid_origin, voxel_size)
        if kept is not None:
            kept = moved, kept[1]
        else:
            verts_d = moved
    if kept_out is not None and kept is not None:
        kept_out["kept"] = (kept[0], kept[1], counts)
    verts, faces, out_v = place_vertices(verts_d, faces_d, voxel_grid_origin, voxel_size, offset, scale)
    out_f = faces
    if kept is not None:
        _, out_f, out_v = place_vertices(kept[0], kept[1], voxel_grid_origin, voxel_size, offset, scale)
    job = None
    if eval_mode:
        gt_path = ground_truth_mesh_path(ply_filename_out, task, data_root)
        if os.path.exists(gt_path):
            from ..icp import load_obj, start_alignment
            gt_v, gt_f = load_obj(gt_path)
            job = start_alignment(out_v, out_f, gt_v, gt_f)                         # 30 000 samples, <= 100 iterations
        elif allow_missing_gt:
            logging.warning("eval_mode: ground-truth mesh %s not found; writing the unaligned mesh (allow_missing_gt)" % gt_path)
        else:
            raise FileNotFoundError("eval_mode: ground-truth mesh %s not found (data_root=%r); pass allow_missing_gt to write "
                                    "unaligned meshes instead" % (gt_path, data_root))
    out_v, trans, sc = apply_icp(job, out_v)
    if ply_filename_out:
        out_n = None
        if normals is not None:
            written = kept[0] if kept is not None else verts_d
            written = written if isinstance(written, torch.Tensor) else torch.as_tensor(np.asarray(written))
            out_n = normals(lattice_points(written.cuda().float(), voxel_grid_origin, voxel_size)).cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(ply_filename_out)), exist_ok=True)
        write_ply(ply_filename_out, out_v, out_f, out_n)
    return verts, faces, trans, sc


def convert_sdf_samples_to_ply(pytorch_3d_sdf_tensor, voxel_grid_origin, voxel_size, ply_filename_out, offset=None,
                               scale=None, eval_mode=False, task="obman", largest_component=True, data_root="data",
                               allow_missing_gt=False, normals=False, normals_part=None, polish=False, kept_out=None):
    """Iso-surface of one SDF volume -> .ply (utils/mesh.py:331-399).  Returns (verts, faces, trans, scale) with
    verts / faces the raw marching-cubes output like the reference.  MC failures are logged and skipped exactly
    like the reference (utils/mesh.py:353-358).  The written file holds the largest watertight component when the
    surface splits into several (utils/mesh.py:371-381, K8 / alignsdf_amd.mesh_post); in eval mode it is first aligned to
    the ground-truth mesh by the translate+scale ICP (utils/mesh.py:385-395, alignsdf_amd.icp) and `trans`, `scale`
    are the ICP's; otherwise they are zeros / one.  `normals`, `normals_part`, `polish`, `kept_out`: see export_surface."""
    vol = pytorch_3d_sdf_tensor if isinstance(pytorch_3d_sdf_tensor, torch.Tensor) else torch.as_tensor(np.asarray(pytorch_3d_sdf_tensor))
    if not vol.is_cuda:
        vol = vol.cuda()
    try:
        verts_d, faces_d = marching_cubes_device(vol, 0.0)
    except (ValueError, RuntimeError) as e:
        logging.warning("Cannot reconstruct mesh from '{}'".format(ply_filename_out))
        print(e)
        return None, None, np.array([0, 0, 0]), np.array([1])
    return export_surface(verts_d, faces_d, voxel_grid_origin, voxel_size, ply_filename_out, offset, scale, eval_mode, task,
                          largest_component, data_root, allow_missing_gt=allow_missing_gt, normals=normals, normals_part=normals_part,
                          polish=polish, **({} if kept_out is None else {"kept_out": kept_out}))


# colour per part label of the `--viz` output (the table of utils/mesh.py:305-310)
PART_COLORS = np.array([[13, 212, 128], [250, 70, 42], [131, 66, 37], [78, 137, 54], [187, 246, 163], [67, 220, 74]], dtype=np.uint8)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _scaled(points, offset, scale):
    pts = _host(points)
    if scale is not None:
        pts = pts * scale
    if offset is not None:
        pts = pts + offset
    return pts


def write_verts_label_to_obj(xyz, labels, obj_filename_out, offset=None, scale=None):
    """`v x y z g g g` lines with grey level 45 * label (utils/mesh.py:259-277)."""
    pts, lab = _scaled(xyz, offset, scale), _host(labels)
    with open(obj_filename_out, "w") as fp:
        fp.write("".join("v %.4f %.4f %.4f %.2f %.2f %.2f\n" % (v[0], v[1], v[2], c, c, c)
                         for v, c in zip(pts.tolist(), (lab * 45.0).tolist())))


def write_verts_label_to_npz(xyz, labels, npz_filename_out, offset=None, scale=None):
    """points / labels arrays (utils/mesh.py:280-296)."""
    np.savez(npz_filename_out, points=_scaled(xyz, offset, scale), labels=_host(labels))


def write_color_labeled_ply(xyz, faces, labels, ply_filename_out, offset=None, scale=None):
    """ASCII PLY coloured by part label (utils/mesh.py:299-326)."""
    from ..ply import write_ply_ascii
    pts, lab = _scaled(xyz, offset, scale), _host(labels)
    write_ply_ascii(ply_filename_out, pts, faces, PART_COLORS[lab.astype(np.int32)])


def label_points(decoder, latent_vec, mano_results, obj_results, specs, points):
    """Part label of every point [V,3] (normalised coordinates, any device): the label pass of utils/mesh.py:137-157
    in one launch (the reference chunks by max_batch).  Returns a float32 CPU tensor like `out_labels`."""
    hip = decoder_for(decoder, specs, mano_results)
    bind_sample(hip, specs, latent_vec, mano_results, obj_results)
    return hip.classify_points(points, want_sdf=False)[3].float().cpu()


def write_label_outputs(vertices, faces, labels, ply_filename_hand, offset, scale, viz):
    """The label files of one hand mesh (utils/mesh.py:160-184)."""
    if viz:
        write_verts_label_to_obj(vertices, labels, ply_filename_hand + "_label.obj", offset, scale)
        write_color_labeled_ply(vertices, faces, labels, ply_filename_hand + "_color.ply", offset, scale)
    write_verts_label_to_npz(vertices, labels, ply_filename_hand + "_label.npz", offset, scale)


def decode_two_pass(hand_branch, obj_branch, decoder, latent_vec, mano_results, obj_results, specs, N, grid_mode="reference",
                    cam_intr=None, mc_only=False):
    """Pass 1 on [-1,1]^3, zoom cube, pass 2 (utils/mesh.py:21-121) entirely on the device.
    Returns dict(vol_hand, vol_obj device tensors of pass 2, voxel_size 0-dim fp32 tensor, origin list,
    bbox int32[16] of pass 1).  mc_only=True declares that the volumes are handed to marching cubes and nothing else: a
    decoder set to the narrow-band fine sweep (ASDF_FINE=band) may then deliver them exact next to the surface only.""" 
    hip = decoder_for(decoder, specs, mano_results)
    bind_sample(hip, specs, latent_vec, mano_results, obj_results, cam_intr)
    mode = GRID_MODES[grid_mode]
    voxel_size = 2.0 / (N - 1)
    # a branch that is switched off is neither meshed nor used for the zoom cube (utils/mesh.py:239-247), so its
    # head is not evaluated at all (the reference computes and discards it)
    # coarse pass: consumed only through its boxes (ordinary sweep, or the box-only sweep when the decoder is set to it);
    # a sweep whose range / error guards fired is repeated inside coarse_finish
    b = hip.coarse_finish(hip.coarse_begin(N, [-1.0, -1.0, -1.0], voxel_size, mode, hand=hand_branch, obj=obj_branch))
    new_voxel_size, new_origin = zoom_cube_of_record(b, hand_branch, obj_branch, N, voxel_size)
    # fine pass: an ordinary sweep (range report through its bbox record), or - when the decoder is set to it and the caller
    # declares that the volumes go to marching cubes only - the narrow-band sweep; either is repeated if its guards fired
    for _ in range(6):
        vol_hand, vol_obj, ticket = hip.fine_begin(N, new_origin.tolist(), new_voxel_size.item(), mode, hand=hand_branch, obj=obj_branch,
                                                   mc_only=mc_only)
        if not hip.fine_needs_repeat(ticket):
            break
    return {"vol_hand": vol_hand, "vol_obj": vol_obj, "voxel_size": new_voxel_size, "origin": new_origin.tolist(), "bbox": b}


def write_hand_and_object(r, filename, hand_branch, obj_branch, offset=None, scale=None, eval_mode=False, task="obman", after_hand=None,
                          normals=None, polish=None, kept_out=None):
    """<filename>_hand.ply, then <filename>_obj.ply, from the volumes of decode_two_pass.  As in the reference, the object mesh is
    written with the hand mesh's ICP translation / scale as its offset / scale (utils/mesh.py:123-133,186-195); the caller's
    `offset` / `scale` reach it only when the hand branch is off.  `after_hand(verts, faces, offset, scale, stats)` runs between the
    two files when the hand has a surface.  `normals`: the evaluator, still bound to this sample - the files then carry vertex normals
    and the stats their `normals_degenerate_<part>` counts.  `polish`: the same evaluator - the written vertices are moved onto the
    zero level of their own head first (export_surface) and the stats carry `polish_<part>` (project.count_record).  `kept_out` (a
    dict, optional) receives per surface that was written ("hand" / "obj") what its file holds, on the device: export_surface's
    (verts, faces, counts).  Returns the per-surface (V, F) counts."""
    stats = {}
    out = {part: {} for part in ("hand", "obj")}
    keep = lambda part: {} if kept_out is None else {"kept_out": out[part]}
    pol = {part: _polish_callable(polish, "", part) or False for part in ("hand", "obj")}
    fn = {part: VertexNormals(normals, part) if normals is not None else False for part in ("hand", "obj")}
    if hand_branch:
        v, f, offset, scale = convert_sdf_samples_to_ply(r["vol_hand"], r["origin"], r["voxel_size"], filename + "_hand.ply", None,
                                                         None, eval_mode, task, normals=fn["hand"], polish=pol["hand"], **keep("hand"))
        stats["hand"] = (0, 0) if v is None else (len(v), len(f))
        if polish is not None and v is not None:
            stats["polish_hand"] = pol["hand"].counts
        if normals is not None and v is not None:
            stats["normals_degenerate_hand"] = fn["hand"].degenerate
        if after_hand is not None and v is not None:
            after_hand(v, f, offset, scale, stats)
    if obj_branch:
        v, f, _, _ = convert_sdf_samples_to_ply(r["vol_obj"], r["origin"], r["voxel_size"], filename + "_obj.ply", offset, scale,
                                                False, normals=fn["obj"], polish=pol["obj"], **keep("obj"))
        stats["obj"] = (0, 0) if v is None else (len(v), len(f))
        if polish is not None and v is not None:
            stats["polish_obj"] = pol["obj"].counts
        if normals is not None and v is not None:
            stats["normals_degenerate_obj"] = fn["obj"].degenerate
    if kept_out is not None:
        kept_out.update({part: o["kept"] for part, o in out.items() if "kept" in o})
    return stats


def create_mesh_combined_decoder(hand_branch, obj_branch, cls_branch, decoder, latent_vec, mano_results, obj_results, cam_intr,
                                 specs, filename, N=256, max_batch=32 ** 3, offset=None, scale=None, device="cpu",
                                 label_out=False, viz=False, eval_mode=False, task="obman", grid_mode="reference", return_stats=False,
                                 normals=False, polish=False, interaction=None):
    """Hand + object meshes of one sample (utils/mesh.py:17-195): writes <filename>_hand.ply / _obj.ply.
    `max_batch` and `device` are accepted for signature compatibility; chunking is internal to the kernel and
    the decoder's device is used.  `grid_mode="reference"` reproduces the true-division lattice of
    utils/mesh.py:33-34 bit for bit; "integer" is the axis-aligned lattice.  Returns None like the reference; with
    `return_stats=True` a dict of per-surface (V, F) counts (and the labels of the label pass).

    `cls_branch` only makes the reference store a per-voxel class column that nothing reads (utils/mesh.py:59-60,
    111-112); it is accepted and has no effect.  `label_out` runs the label pass over the hand mesh vertices
    (utils/mesh.py:137-184) and needs a decoder with a classifier head.  As in the reference, the object mesh is
    written with the hand mesh's ICP translation / scale as its offset / scale (utils/mesh.py:123-133,186-195).
    `normals=True`: both files carry per-vertex unit normals (nx / ny / nz) - the analytic SDF gradient of the surface's own head at
    the vertex, normalised - and the stats dict their `normals_degenerate_hand` / `_obj` counts; a decoder the gradient kernel does
    not cover raises NotImplementedError before anything is swept.
    `polish=True`: the written vertices of both files are moved onto the zero level of their surface's own head (Newton projection,
    at most one fine voxel per axis: project.polish_vertices) - same faces and vertex count, normals taken at the polished positions,
    `polish_hand` / `polish_obj` in the stats; an evaluator that cannot project raises NotImplementedError before anything is swept.
    `interaction={"contact_m": 0.005}`: the stats carry `interaction` - penetration depth, intersection volume and contact of the two
    surfaces from the decoder's own SDFs (interaction.measure_surfaces, the dict of interaction.interaction_record), measured on the
    very vertices the files hold (write_hand_and_object hands them over on the device), in the decoder's frame (before the eval-mode ICP); ValueError before anything is swept when a branch is
    off.  The files themselves are the ones written without it."""
    decoder.eval() if hasattr(decoder, "eval") else None
    evaluator = None
    contact_m = None
    if interaction is not None and interaction is not False:
        from ..interaction import check_option
        contact_m = check_option(interaction, dict(specs, HandBranch=hand_branch, ObjectBranch=obj_branch))
    if normals or polish or contact_m is not None:
        evaluator = decoder_for(decoder, specs, mano_results)
    if normals:
        require_normals(evaluator)
    if polish:
        from ..project import require_polish
        require_polish(evaluator)
    # (the volumes go to marching cubes only: a decoder set to the narrow-band fine sweep may use it)
    r = decode_two_pass(hand_branch, obj_branch, decoder, latent_vec, mano_results, obj_results, specs, N, grid_mode, cam_intr,
                        mc_only=True)

    def label_pass(v, f, offset, scale, stats):       # (between the two files: its launch stays ahead of the object's marching cubes)
        vertices = np.array(v, copy=True)
        for a in range(3):
            vertices[:, a] = r["origin"][a] + vertices[:, a]
        vertices = torch.from_numpy(vertices)
        labels = label_points(decoder, latent_vec, mano_results, obj_results, specs, vertices)
        write_label_outputs(vertices, f, labels, filename + "_hand", offset, scale, viz)
        stats["labels"] = labels

    kept = {}          # with the interaction option: part -> what its file holds, on the device
    stats = write_hand_and_object(r, filename, hand_branch, obj_branch, offset, scale, eval_mode, task, label_pass if label_out else None,
                                  normals=evaluator if normals else None, polish=evaluator if polish else None,
                                  **({} if contact_m is None else {"kept_out": kept}))
    if contact_m is not None:
        from ..interaction import measure_surfaces
        bind_sample(evaluator, specs, latent_vec, mano_results, obj_results, cam_intr)      # (whatever ran in between)
        stats["interaction"] = measure_surfaces(evaluator, r, kept, specs, contact_m)
    return stats if return_stats else None
