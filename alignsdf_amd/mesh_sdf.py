"""The signed distance field of a triangle mesh (csrc/mesh_sdf.hip; the rule is worded in include/alignsdf_hip.h): exact point-triangle
distance, sign from the generalised winding number.  What the data side of a hand-object SDF reconstruction needs and the decoder
cannot give: the field of a GROUND-TRUTH mesh - for its interaction metrics (gt_interaction.py), for (xyz, sdf) fit targets
(`sdf_samples`, fit.fit_sample) and for "how far is this vertex from that surface, and on which side".

Every pair (query, face) is visited - the winding sum needs every face - so a call costs M x T pairs; there is no culling.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _native

MeshSdf = collections.namedtuple("MeshSdf", "sdf winding face closest")
DEFAULT_SIGMAS = (0.005, 0.02)          # standard deviations of the near-surface displacements, in the mesh's units


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _bytes(num_faces, M):
    n = ctypes.c_size_t()
    _native.check(_native.lib().asdf_mesh_sdf_workspace_bytes(int(num_faces), int(M), ctypes.byref(n)), "asdf_mesh_sdf_workspace_bytes")
    return n.value


class MeshField:
    """The field of one mesh: `verts` [V, 3] and `faces` [T, 3] as host arrays (float64 / int64 of load_obj are fine) or device tensors.
    Uploads, runs the prep launch once and owns the workspace; nothing here waits for the stream (`.info` does, when first read)."""

    def __init__(self, verts, faces, device=None):
        if device is None:
            device = verts.device if torch.is_tensor(verts) and verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("a CUDA device is needed (there is no CPU fallback)")
        as_t = lambda a: a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        self.verts = as_t(verts).reshape(-1, 3).to(self.device, torch.float32).contiguous()
        f = as_t(faces).reshape(-1, 3)
        if f.dtype != torch.int32:
            # (indices that do not fit int32 are bad indices: they stay out of range instead of wrapping into it)
            f = f.to(torch.int64)
            f = torch.where((f < 0) | (f > 0x7fffffff), torch.full_like(f, -1), f)
        self.faces = f.to(self.device, torch.int32).contiguous()
        self.num_verts, self.num_faces = int(self.verts.shape[0]), int(self.faces.shape[0])
        self._ws = torch.empty(_bytes(self.num_faces, 0), dtype=torch.uint8, device=self.device)
        self._info_dev = torch.empty(_native.MESH_SDF_INFO_WORDS, dtype=torch.int32, device=self.device)
        self._info = None
        self._scratch = None
        # (host arrays are kept as given - float64 vertices stay float64 for bounds() and enclosed_volume())
        self._host = None if torch.is_tensor(verts) or torch.is_tensor(faces) else (np.asarray(verts, np.float64).reshape(-1, 3),
                                                                                    np.asarray(faces, np.int64).reshape(-1, 3))
        with torch.cuda.device(self.device):
            _native.check(_native.lib().asdf_mesh_sdf_prepare(
                self.verts.data_ptr() if self.num_verts else None, self.num_verts, self.faces.data_ptr() if self.num_faces else None,
                self.num_faces, self._ws.data_ptr(), self._info_dev.data_ptr(), _stream(self.device)), "asdf_mesh_sdf_prepare")

    @property
    def info(self):
        """{"skipped": faces with a bad index or a non-finite corner, "zero_area": faces that are a segment or a point}."""
        if self._info is None:
            w = self._info_dev.cpu().numpy()
            self._info = {"skipped": int(w[_native.MESH_SDF_INFO_SKIPPED]), "zero_area": int(w[_native.MESH_SDF_INFO_ZERO_AREA])}
        return self._info

    def at(self, xyz, winding=False, face=False, closest=False):
        """MeshSdf(sdf [M], winding [M] or None, face int32 [M] or None, closest [M, 3] or None) at the device points xyz [M, 3]."""
        if not torch.is_tensor(xyz) or not xyz.is_cuda:
            raise TypeError("a CUDA tensor is needed (there is no CPU fallback)")
        p = xyz.detach().reshape(-1, 3).to(self.device, torch.float32).contiguous()
        M = int(p.shape[0])
        new = lambda want, shape, dt: torch.empty(shape, dtype=dt, device=self.device) if want else None
        out = MeshSdf(new(True, (M,), torch.float32), new(winding, (M,), torch.float32), new(face, (M,), torch.int32),
                      new(closest, (M, 3), torch.float32))
        need = _bytes(self.num_faces, M) if M else 0
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        with torch.cuda.device(self.device):
            _native.check(_native.lib().asdf_mesh_sdf_points(self._ws.data_ptr(), self.num_faces, ptr(p), M, ptr(out.sdf), ptr(out.winding),
                                                              ptr(out.face), ptr(out.closest), ptr(self._scratch), _stream(self.device)),
                          "asdf_mesh_sdf_points")
        return out

    def volume(self, origin, voxel_size, dims):
        """fp32 [n0, n1, n2] device volume of the field: voxel (i0, i1, i2) sits at origin + (i0, i1, i2) * voxel_size - where
        utils.mesh.lattice_points puts a marching-cubes vertex with integer coordinates, so the volume goes straight into
        interaction.lattice_overlap and marching_cubes."""
        from .utils.mesh import lattice_points
        n0, n1, n2 = (int(n) for n in dims)
        ax = [torch.arange(n, dtype=torch.float32, device=self.device) for n in (n0, n1, n2)]
        idx = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
        return self.at(lattice_points(idx, [float(o) for o in origin], float(voxel_size))).sdf.reshape(n0, n1, n2)

    def bounds(self):
        """(lo [3], hi [3]) float64 on the host, over the vertices that a face uses and that are finite."""
        return mesh_bounds(*self.host_mesh())

    def enclosed_volume(self):
        """The divergence-theorem volume sum a . (b x c) / 6 in fp64 on the host, absolute (either orientation); faces the field
        leaves out are left out here."""
        return enclosed_volume(*self.host_mesh())

    def host_mesh(self):
        """(verts float64 [V, 3], faces int64 [T, 3]) on the host: the arrays the field was made from, or a copy of its tensors."""
        if self._host is None:
            self._host = (self.verts.cpu().numpy().astype(np.float64), self.faces.cpu().numpy().astype(np.int64))
        return self._host


def _valid_faces(verts, faces):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    f = f[ok]
    return v, f[np.isfinite(v[f]).all((1, 2))] if len(f) else f


def mesh_bounds(verts, faces):
    v, f = _valid_faces(verts, faces)
    if not len(f):
        return np.full(3, np.inf), np.full(3, -np.inf)
    used = v[np.unique(f)]
    return used.min(0), used.max(0)


def enclosed_volume(verts, faces):
    v, f = _valid_faces(verts, faces)
    if not len(f):
        return 0.0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return abs(float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum()) / 6.0)


def sample_points(verts, faces, n_near, n_uniform, sigmas=DEFAULT_SIGMAS, seed=0):
    """The positions of sdf_samples on the host, float32 [n_near + n_uniform, 3]: surface picks of the seeded sampler
    (surface_sampling.sample_surface) displaced by seeded normal noise - pick i by sigmas[i % len(sigmas)] -, then uniform points in
    the mesh's box grown by 10 %.  Draws come from synthetic's counters: the same seed gives the same bits."""
    from . import surface_sampling, synthetic
    verts, faces = _valid_faces(verts, faces)
    parts = []
    if n_near:
        if not len(faces):
            raise ValueError("sdf_samples: the mesh has no face to sample")
        surf = surface_sampling.sample_surface(verts, faces, int(n_near), seed=seed)
        sig = np.asarray(sigmas, np.float64)[np.arange(int(n_near)) % len(sigmas)]
        parts.append(surf + synthetic.normal((int(n_near), 3), 9300 + seed) * sig[:, None])
    if n_uniform:
        lo, hi = mesh_bounds(verts, faces)
        pad = 0.05 * (hi - lo)                      # grown by 10 %: 5 % on either side
        parts.append(lo - pad + synthetic.uniform((int(n_uniform), 3), 9400 + seed) * (hi - lo + 2.0 * pad))
    return (np.concatenate(parts) if parts else np.zeros((0, 3))).astype(np.float32)


def sdf_samples(field, n_near, n_uniform, sigmas=DEFAULT_SIGMAS, seed=0):
    """(xyz [n, 3], sdf [n]) on the device, n = n_near + n_uniform: the (xyz, sdf) samples an SDF auto-decoder is fitted to
    (fit.fit_sample's sdf_hand / sdf_obj) - sample_points of the field's mesh, valued by the field."""
    xyz = torch.from_numpy(sample_points(*field.host_mesh(), n_near, n_uniform, sigmas, seed)).to(field.device)
    return xyz, field.at(xyz).sdf
