"""`DefTet` geometry module with the reference's method names and signatures
(/root/reference/layers/DefTet/deftet.py), HIP-backed for the per-tetrahedron pieces:

    get_boundary_index / get_internal_index   (:186-203)  -> deftet_boundary_index_i64
    paste_occ                                 (:132-136)  -> deftet_paste_occ_*_f32
    volume_variance / amips_energy / edge_length (:239-338) -> deftet_tet_energies_*_f32
    tet_inverse_v / my_inverse                (:205-233,:300-318)  torch (init-time, T 3x3 inverses)
    point queries                             (:110-112)  -> check_condition_f_base
    gather_tet_pos (vertex -> tet gather)     (:65-68)    -> deftet_tet_gather_{fwd,bwd}_f32

    check_tet_inside_sdfs                     (:33-49)    -> deftet_check_sign_f32 (Kaolin's
                                                             check_sign restated; parity unpinned)

    forward_surface_align / forward           (:51-184)   composed from the operators above plus the surface
                                                             terms in deftet_amd/surface_losses.py (A8/A9/A10); same
                                                             arguments, same tuple order as the reference
    laplacian_sparse                          (:340-343)  adj a hip_ops.VertexAdjacency -> deftet_vertex_laplacian_*_f32
                                                             (fused, atomic-free backward); adj a torch sparse tensor ->
                                                             torch.sparse.mm (vendor SpMM), unchanged
"""
import collections
import threading
import torch
import torch.nn as nn

from deftet_amd import hip_ops, surface_losses
from deftet_amd.layers.DefTet.check_condition_tetrahedron_base.utils import (check_condition_f_base, paste_occ, point_in_tet_occ_indexed,
                                                                             point_in_tet_occ_vertices)

EPS = 1e-10


class _TetGather(torch.autograd.Function):
    """tet_bxfx4x3 = gather(vertice_pos, tetrahedron) with an atomic-free, deterministic backward."""

    @staticmethod
    def forward(ctx, vertice_pos, tet_idx, csr):
        ctx.csr = csr
        ctx.n_vertex = vertice_pos.shape[1]
        return hip_ops.tet_gather(vertice_pos, tet_idx)

    @staticmethod
    def backward(ctx, grad_tet):
        return hip_ops.tet_gather_bwd(grad_tet.contiguous(), ctx.csr, ctx.n_vertex), None, None


class TetTopology:
    """Per-topology cache for the vertex<->tet gather: the incidence CSR is built once (the tet
    list is static during training, train_multigpu.py:72-77) and reused by every backward."""

    _serials = __import__("itertools").count(1)

    def __init__(self, tet_idx, n_vertex):
        self.serial = next(TetTopology._serials)              # identifies the tet LIST: hip_ops.auto_tet_order keys its decision on it
        idx = tet_idx.long()
        # The reference hands every shape of a batch the SAME tet list (`tet_fx4.unsqueeze(0).expand(B, -1, -1)`,
        # train_multigpu.py:72-77): keep one copy then — the gather reads 8 MB of indices instead of 66 MB at res 70, B = 8,
        # the incidence CSR is built once instead of B times.  (One comparison + sync here, at build time only.)
        if idx.dim() == 3 and idx.shape[0] > 1 and bool((idx == idx[:1]).all()):
            idx = idx[:1]
        self.tet_idx = idx.contiguous()
        self.n_vertex = int(n_vertex)
        self.csr = hip_ops.tet_vertex_csr(self.tet_idx, self.n_vertex)     # (raises on an index outside [0, n_vertex))
        self.tet_idx32 = self.tet_idx.to(torch.int32).contiguous()         # what the indexed query reads (hip_ops.point_in_tet_indexed)
        self._vertex_adjacency = {}                                         # normalize -> hip_ops.VertexAdjacency (vertex_adjacency)
        self._edges = None                                                  # hip_ops.TetEdges (edges)

    def gather(self, vertice_pos):
        return _TetGather.apply(vertice_pos, self.tet_idx, self.csr)

    def centroid_sample(self, volumes, vertice_pos, select=None, first=0, count=None, append_pos=True):
        """hip_ops.tet_centroid_sample on this tet list: the volumes read at the centroids of the chosen tets, [B, sum C (+3), K],
        with the gradient on vertice_pos through the cached incidence CSR and no [B,T,4,3] tensor in either direction."""
        return hip_ops.tet_centroid_sample(volumes, vertice_pos, self.tet_idx32, csr=self.csr, select=select, first=first, count=count,
                                           append_pos=append_pos)

    def field_sample(self, field, vertice_pos, pts, fill=0.0, return_index=False):
        """hip_ops.tet_field_sample on this tet list: the per-vertex field [B,V,C] read at the points pts [B,Q,3] with the
        barycentric weights of the tet that holds each, [B,Q,C] (`fill` outside the mesh), differentiable in field, vertice_pos and
        pts through the cached incidence CSR."""
        return hip_ops.tet_field_sample(field, vertice_pos, self.tet_idx32, pts, topology=self, fill=fill,
                                        return_index=return_index)

    def field_gradient(self, field, vertice_pos, return_volume=False):
        """hip_ops.tet_field_gradient on this tet list: the gradient of the per-vertex field [B,V,C] on every tet, [B,T,C,3] (and
        the volumes [B,T]), differentiable in field and vertice_pos through the cached incidence CSR."""
        return hip_ops.tet_field_gradient(field, vertice_pos, self.tet_idx32, topology=self, return_volume=return_volume)

    def field_energies(self, field, vertice_pos, target=1.0):
        """hip_ops.tet_field_energies on this tet list: [B,C,2] = the volume-weighted Dirichlet energy and Eikonal term
        (|grad f| - target)^2 of the per-vertex field, differentiable in field and vertice_pos."""
        return hip_ops.tet_field_energies(field, vertice_pos, self.tet_idx32, topology=self, target=target)

    def iso_fraction(self, field, vertice_pos, iso=0.0, return_area=False, return_volume=False):
        """hip_ops.tet_iso_fraction on this tet list: per tet the share of its volume inside {field > iso} of the per-vertex field
        [B,V] / [B,V,1], [B,T] (then the iso polygon's area, then the volume), differentiable in field and vertice_pos."""
        return hip_ops.tet_iso_fraction(field, vertice_pos, self.tet_idx32, iso=iso, topology=self, return_area=return_area,
                                        return_volume=return_volume)

    def iso_measures(self, field, vertice_pos, iso=0.0, weights=None):
        """hip_ops.tet_iso_measures on this tet list: [B,5] = (enclosed volume, surface area, intersection with the per-tet
        occupancy `weights`, that occupancy's volume, live volume), differentiable in field and vertice_pos."""
        return hip_ops.tet_iso_measures(field, vertice_pos, self.tet_idx32, iso=iso, weights=weights, topology=self)

    def to_vertices(self, values_bxtxc, weights=None, fill=0.0):
        """hip_ops.tet_to_vertex on this tet list: per-tet values [B,T,C] as the (weighted) mean over each vertex's incident
        tets, [B,V,C]; differentiable in the values, the weights a constant."""
        return hip_ops.tet_to_vertex(values_bxtxc, self, self.n_vertex, weights=weights, fill=fill)

    def vertex_adjacency(self, normalize=True):
        """hip_ops.VertexAdjacency of this tet list (D⁻¹A with `normalize`, else A), for DefTet.laplacian_sparse; built on the
        first call per `normalize` and kept."""
        key = bool(normalize)
        adj = self._vertex_adjacency.get(key)
        if adj is None:
            tets = self.tet_idx32
            if tets.dim() == 3:
                if tets.shape[0] != 1:
                    raise RuntimeError("TetTopology.vertex_adjacency: the shapes of this batch have different tet lists")
                tets = tets[0]
            adj = hip_ops.VertexAdjacency.from_tets(tets, self.n_vertex, normalize=key)
            self._vertex_adjacency[key] = adj
        return adj

    def edges(self):
        """hip_ops.TetEdges of this tet list (unique edges, tet -> edge table, vertex -> edge-end CSR), for
        hip_ops.marching_tets; built on the first call and kept."""
        if self._edges is None:
            tets = self.tet_idx
            if tets.dim() == 3:
                if tets.shape[0] != 1:
                    raise RuntimeError("TetTopology.edges: the shapes of this batch have different tet lists")
                tets = tets[0]
            self._edges = hip_ops.TetEdges(tets, self.n_vertex)
        return self._edges


# Cache of the incidence CSR, per device and index shape, at MODULE level: nn.DataParallel (train_multigpu.py:138)
# re-replicates the layer every step and discards whatever a replica stored on itself, and scatters a fresh copy of the
# index tensor.  Fast path: the very same tensor object, unmodified (a reference is kept, so its storage cannot be
# recycled for another tensor behind our back).  Otherwise the CONTENT is compared with the cached indices (one small
# kernel + sync; the CSR rebuild it avoids is 40x that) — never address or shape alone.
# nn.DataParallel runs the replicas' forward in threads of one process: the cache is shared by them, so every access is
# under a lock; least-recently-used entries go first (at most _TOPOLOGIES_MAX (device, shape, n_vertex) keys stay pinned in
# GPU memory; clear_topology_cache() drops them all).
_TOPOLOGIES = collections.OrderedDict()
_TOPOLOGIES_MAX = 16
_TOPOLOGIES_LOCK = threading.Lock()


def clear_topology_cache():
    with _TOPOLOGIES_LOCK:
        _TOPOLOGIES.clear()


def _topology_for(tetrahedron_bxfx4, n_vertex):
    key = (tetrahedron_bxfx4.device, tuple(tetrahedron_bxfx4.shape), int(n_vertex))
    with _TOPOLOGIES_LOCK:
        hit = _TOPOLOGIES.get(key)
    if hit is not None:
        topo, src, version = hit
        same = src is tetrahedron_bxfx4 and version == tetrahedron_bxfx4._version
        if not same:
            same = bool((tetrahedron_bxfx4 == topo.tet_idx).all())     # (broadcasts over the batch when one shared copy is kept)
        if same:
            with _TOPOLOGIES_LOCK:
                _TOPOLOGIES[key] = (topo, tetrahedron_bxfx4, tetrahedron_bxfx4._version)
                _TOPOLOGIES.move_to_end(key)
            return topo
    topo = TetTopology(tetrahedron_bxfx4, n_vertex)                   # (built outside the lock: a host sync and a few launches)
    with _TOPOLOGIES_LOCK:
        _TOPOLOGIES[key] = (topo, tetrahedron_bxfx4, tetrahedron_bxfx4._version)
        _TOPOLOGIES.move_to_end(key)
        while len(_TOPOLOGIES) > _TOPOLOGIES_MAX:
            _TOPOLOGIES.popitem(last=False)
    return topo


def save_tet_face(tri_fx3x3, f_name):
    """Triangle soup as an OBJ file: three `v` lines and one `f a c b` line per triangle, `%f` formatting
    (utils/mesh_utils.py:258-267)."""
    lines = []
    for i, t in enumerate(tri_fx3x3):
        for k in range(3):
            lines.append('v %f %f %f\n' % (t[k][0], t[k][1], t[k][2]))
        lines.append('f %d %d %d\n' % (i * 3 + 1, i * 3 + 3, i * 3 + 2))
    with open(f_name, 'w') as f:
        f.write(''.join(lines))


class DefTet(nn.Module):
    def __init__(self, device=None):
        super(DefTet, self).__init__()
        self.pow = 4
        self.device = device
        self.features_fixed = False
        self.z_window_radius = 0.025
        self.inverse_v = None

    # --- N2: tet_bxfx4x3 from vertex positions (deftet.py:65-68)
    def gather_tet_pos(self, vertice_pos, tetrahedron_bxfx4):
        return _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]).gather(vertice_pos)

    # --- N1: GT occupancy of the tet centroids (deftet.py:33-49)
    def check_tet_inside_sdfs(self, tet_bxfx4x3, mesh_list, method="parity"):
        """method="parity" (the reference's): +x ray parity, meaningful on watertight meshes only.  method="winding": the centroids
        are labelled by their generalised winding number (w > 0.5), which also reads open, nested and self-intersecting meshes."""
        if method not in ("parity", "winding"):
            raise ValueError("check_tet_inside_sdfs: method %r is not 'parity' or 'winding'" % (method,))
        verts, faces = mesh_list[0], mesh_list[1]
        with torch.no_grad():
            center = torch.mean(tet_bxfx4x3, dim=2)                     # [B,T,3], same reduction as per shape
            f0 = faces[0][0]                                            # f[0] makes a new view object each time: compare storage
            same_mesh = all(f[0].data_ptr() == f0.data_ptr() and f[0].shape == f0.shape and f[0].stride() == f0.stride()
                            for f in faces) and all(v.shape == verts[0].shape for v in verts)
            if same_mesh and len(verts) == tet_bxfx4x3.shape[0]:
                # one launch sequence for the whole batch (faces shared, per-shape vertices)
                v = torch.cat([x.reshape(1, -1, 3) for x in verts], dim=0)
                if method == "winding":
                    return hip_ops.winding_inside(hip_ops.winding_number(v, faces[0][0], center, check=False)).unsqueeze(-1).float()
                return hip_ops.check_sign(v, faces[0][0], center, check=False).unsqueeze(-1).float()
            # a different ground-truth mesh per shape (the reference loops over the batch): one ragged call
            if method == "winding":
                w = hip_ops.winding_number_ragged(list(verts), [f[0] for f in faces], center, check=False)
                return hip_ops.winding_inside(w).unsqueeze(-1).float()
            return hip_ops.check_sign_ragged(list(verts), [f[0] for f in faces], center).unsqueeze(-1).float()

    # --- A7
    def get_boundary_index(self, tet_face_fx3, tet_idx_fx2, occ_bxn):
        return hip_ops.boundary_index(tet_face_fx3, tet_idx_fx2, occ_bxn, mode=1)

    def get_internal_index(self, tet_face_fx3, tet_idx_fx2, occ_bxn):
        return hip_ops.boundary_index(tet_face_fx3, tet_idx_fx2, occ_bxn, mode=2)

    # --- what the reference leaves to trimesh on the host ("use trimesh to fix the surface", utils/tet_utils.py:474)
    def clean_occupancy(self, occ_bxn, nbr, thres=0.5, keep_largest=True, min_size=0, fill_voids=False):
        """occ_bxn [B,T] / [B,T,1] with its floaters dropped and its enclosed voids filled, on the device (hip_ops.occupancy_cleanup
        on the mask occ > thres): float32 of the input's shape, 0 where an inside tet was dropped, 1 where an outside tet was
        filled, the input's value everywhere else — a 0 / 1 occupancy stays 0 / 1 and goes straight into get_boundary_index and
        hip_ops.surface_extract(mode="binary").  nbr: hip_ops.tet_face_neighbours of the tet list (or the reference's list of
        four sparse matrices).  No gradient."""
        occ = occ_bxn.detach().float()
        if occ.dim() not in (2, 3) or (occ.dim() == 3 and occ.shape[2] != 1):
            raise RuntimeError("clean_occupancy: occ [B,T] or [B,T,1] expected, got %s" % (tuple(occ_bxn.shape),))
        flat = occ.reshape(occ.shape[0], -1)
        nbr = hip_ops.neighbours_from_adj_list(nbr, flat.device)
        inside = flat > thres
        keep = hip_ops.occupancy_cleanup(inside, nbr, keep_largest=keep_largest, min_size=min_size, fill_voids=fill_voids)
        return hip_ops.cleaned_occupancy(flat, inside, keep).reshape(occ.shape)

    # --- A1 / A1b
    def check_condition(self, tet_bxfx4x3, point_pos_bxpx3):
        return check_condition_f_base(tet_bxfx4x3, point_pos_bxpx3)

    def paste_occ(self, pred_tet_occ, condition):
        return paste_occ(pred_tet_occ, condition)

    # --- A1 + A1b + paste_occ for a caller that holds the VERTICES (build-defined, like point_in_tet_occ): the gradient of the
    #     weights lands on vertice_pos without the dense per-tet gradient in between
    def occupancy_query(self, vertice_pos, tetrahedron_bxfx4, point_pos_bxpx3, pred_tet_occ, tet_bxfx4x3=None, indexed=False):
        """(condition [B,Q,1], weights [B,Q,4], occ [B,Q]) of the query points in the mesh (vertice_pos, tetrahedron_bxfx4);
        tet_bxfx4x3 = self.gather_tet_pos(vertice_pos, tetrahedron_bxfx4) when the caller has it already.
        indexed=True (and no tet_bxfx4x3): the query reads the vertices through the index list and never materialises the
        [B,T,4,3] tensor, neither as a temporary nor as memory kept for the backward; the same bits either way."""
        topo = _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1])
        if indexed and tet_bxfx4x3 is None:
            return point_in_tet_occ_indexed(vertice_pos, point_pos_bxpx3, pred_tet_occ, topo)
        return point_in_tet_occ_vertices(vertice_pos, point_pos_bxpx3, pred_tet_occ, topo, tet_bxfx4x3)

    # --- a per-vertex field (an SDF, an occupancy, features) at the query points: located as in occupancy_query, then interpolated
    def field_query(self, vertice_pos, tetrahedron_bxfx4, point_pos_bxpx3, field):
        """[B,Q,C]: field [B,V,C] interpolated at the query points with their barycentric weights in the mesh (vertice_pos,
        tetrahedron_bxfx4), 0 where no tet holds the point; the gradient reaches field, vertice_pos and the points."""
        return _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]).field_sample(field, vertice_pos, point_pos_bxpx3)

    # --- the geometry-aware regularisers of a per-vertex field: volume-weighted Dirichlet energy and Eikonal term
    def field_regularizers(self, vertice_pos, tetrahedron_bxfx4, field, target=1.0):
        """[B,C,2] = (sum w |grad f_c|^2 / W, sum w (|grad f_c| - target)^2 / W) over the live tets, w their volumes, of the
        per-vertex field [B,V,C] (1 <= C <= 8); the gradient reaches field and vertice_pos (hip_ops.tet_field_energies)."""
        return _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]).field_energies(field, vertice_pos, target=target)

    # --- the solid {field > iso} of a per-vertex field, measured per tet and per shape (hip_ops.tet_iso_fraction / tet_iso_measures)
    def field_measures(self, vertice_pos, tetrahedron_bxfx4, field, iso=0.0, gt_occ_bxt=None):
        """[B,5] = (enclosed volume, iso-surface area, intersection with gt_occ_bxt, volume of gt_occ_bxt, live volume) of the
        per-vertex field [B,V] / [B,V,1]; gt_occ_bxt [B,T] / [B,T,1] is a constant (None = 1).  The gradient reaches field and
        vertice_pos: the area as a minimal-surface regulariser, the volume as a prior."""
        w = None if gt_occ_bxt is None else gt_occ_bxt.detach().reshape(gt_occ_bxt.shape[0], -1).float().contiguous()
        return _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]).iso_measures(field, vertice_pos, iso=iso, weights=w)

    def field_occupancy(self, vertice_pos, tetrahedron_bxfx4, field, iso=0.0):
        """[B,T] in [0,1]: the exact share of every tet inside {field > iso} — the per-tet occupancy of a per-vertex field, usable
        wherever pred_tet_occ is (the BCE against center_occ, paste_occ, get_boundary_index after a threshold); its gradient sees
        where in the tet the surface is."""
        return _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]).iso_fraction(field, vertice_pos, iso=iso)

    def field_iou(self, vertice_pos, tetrahedron_bxfx4, field, gt_occ_bxt, iso=0.0):
        """[B]: the exact volumetric IoU of {field > iso} with the per-tet ground-truth occupancy gt_occ_bxt [B,T] / [B,T,1]
        (validate_iou's quantity, without sampling points); differentiable in field and vertice_pos."""
        return hip_ops.iso_iou(self.field_measures(vertice_pos, tetrahedron_bxfx4, field, iso=iso, gt_occ_bxt=gt_occ_bxt))

    # --- the welded iso-surface of a per-TET occupancy: to the vertices, then marching tetrahedra
    def iso_surface(self, vertice_pos, tetrahedron_bxfx4, pred_tet_occ, iso=0.5, volume_weighted=True, subdivide=0, keep_largest=False, min_faces=0,
                    drop_voids=False):
        """hip_ops.IsoMesh (lists of B tensors) of the per-tet occupancy pred_tet_occ [B,T] / [B,T,1]: every vertex takes the mean
        of its incident tets' values (weighted by their volumes with volume_weighted, as constants) and hip_ops.marching_tets
        takes the level `iso` of that per-vertex field on the tet list's edges.  Differentiable in pred_tet_occ and vertice_pos.
        The shapes share one tet list.  subdivide = n > 0: every shape's mesh after n rounds of Loop subdivision
        (hip_ops.loop_subdivide_list: one topology build and one read-back per round for the whole batch), verts and faces only.
        keep_largest / min_faces / drop_voids clean every shape's mesh on the device BEFORE the subdivision (hip_ops.mesh_cleanup_list:
        cavity shells and floaters dropped, one launch sequence and one read-back for the whole batch); with all three left at
        their defaults nothing of it runs."""
        levels = int(subdivide)
        if levels < 0:
            raise ValueError("iso_surface: subdivide = %d is negative" % levels)
        topo = _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1])
        occ = pred_tet_occ.reshape(pred_tet_occ.shape[0], -1, 1)
        weights = hip_ops.tet_volumes(vertice_pos, topo.tet_idx32) if volume_weighted else None
        field = topo.to_vertices(occ, weights=weights)
        mesh = hip_ops.marching_tets(vertice_pos, field.squeeze(-1), topo.edges(), iso=iso)
        if bool(keep_largest) or int(min_faces) > 0 or bool(drop_voids):
            mesh = hip_ops.mesh_cleanup_list(mesh, keep_largest=keep_largest, min_faces=min_faces, drop_voids=drop_voids)
        if levels:
            verts, faces, _attr = hip_ops.loop_subdivide_list(mesh.verts, mesh.faces, None, levels=levels)
            mesh = hip_ops.IsoMesh(verts, faces, None, None, None, None)
        return mesh

    # --- A11 (each call evaluates the fused kernel and returns its own component)
    def volume_variance(self, tet_bxfx4x3, base_area_mask=None, area_normalize=(20, 20), pow=2, center_occ=None):
        return hip_ops.tet_energies(tet_bxfx4x3, None, pow_v=pow, pow_e=self.pow)[:, 0]

    def amips_energy(self, tet_bxfx4x3, inverse_v, scale=20, center_occ=None, square=False):
        if square:
            # never used by the reference's callers (deftet.py:286-287): the per-tet energies squared before the mean.  The
            # fused operator only hands out the means, so this option is the reference's own torch composition (on the GPU).
            n_batch = tet_bxfx4x3.shape[0]
            a, b, c, d = (tet_bxfx4x3[:, :, k, :].unsqueeze(2) * scale for k in range(4))
            offset_vec = torch.cat([b - a, c - a, d - a], dim=2)
            jac = torch.bmm(offset_vec.reshape(-1, 3, 3), inverse_v.unsqueeze(0).expand_as(offset_vec).reshape(-1, 3, 3))
            trace = (jac ** 2).sum(-1).sum(-1)
            det = (jac[:, 0, :] * torch.linalg.cross(jac[:, 1, :], jac[:, 2, :], dim=-1)).sum(-1)       # utils/matrix_utils.py:42-47
            energy = trace * torch.pow(det ** 2 + EPS, -1.0 / 3.0) * (det >= 0.0).float()
            return (energy.reshape(n_batch, -1) ** 2).mean(-1)
        return hip_ops.tet_energies(tet_bxfx4x3, inverse_v, pow_v=self.pow, pow_e=self.pow, scale=scale)[:, 1]

    def edge_length(self, tet_bxfx4x3, pow=2):
        return hip_ops.tet_energies(tet_bxfx4x3, None, pow_v=self.pow, pow_e=pow, scale=20)[:, 2]

    def energies(self, tet_bxfx4x3, inverse_v):
        """(volume_variance, amips_energy, edge_length) from ONE fused evaluation — what
        forward_surface_align (:82-83,:105) needs per step."""
        out = hip_ops.tet_energies(tet_bxfx4x3, inverse_v, pow_v=self.pow, pow_e=self.pow, scale=20.0)
        return out[:, 0], out[:, 1], out[:, 2]

    # --- the per-step composition (deftet.py:51-130): one fused launch sequence per operator for the whole
    #     batch; only the surface terms loop over shapes (a different predicted surface per shape)
    def forward_surface_align(self, vertice_pos, point_pos_bxpx3, tetrahedron_bxfx4=None, mesh_list=None,
                              gt_surface_points=None, tet_face_bxfx3=None, inference=False, pred_occ=None,
                              tet_face_tet_bx4fx2=None, save=False, save_name=None, inference_threshold=0.4, tet_bxfx4x3=None):
        # tet_bxfx4x3 (not in the reference's signature; its `forward` has the same optional argument, deftet.py:140): a
        # caller that has gathered the tet positions already — e.g. for the occupancy query of the same step — hands them
        # in instead of having them gathered (and their gradient scattered) a second time
        n_shape = vertice_pos.shape[0]
        if tet_bxfx4x3 is None:
            tet_bxfx4x3 = self.gather_tet_pos(vertice_pos, tetrahedron_bxfx4)
        center_occ = self.check_tet_inside_sdfs(tet_bxfx4x3, mesh_list)                       # [B,T,1], no grad
        face_fx3, face_tet_fx2 = tet_face_bxfx3[0], tet_face_tet_bx4fx2[0]
        boundary = self.get_boundary_index(face_fx3, face_tet_fx2, center_occ.squeeze(dim=-1))
        if save:
            # eval.py --save: the ground-truth-occupancy surface of the first five shapes as triangle-soup OBJ files
            # (deftet.py:72-80, utils/mesh_utils.py:258-267)
            for idx in range(min(len(boundary), 5)):
                tri = vertice_pos[idx][boundary[idx].long()]                               # [F,3,3]
                save_tet_face(tri.detach().cpu().numpy(), save_name + '_device_%d_%d.obj' % (torch.cuda.current_device(), idx))
        inv_v = self.inverse_v.to(tet_bxfx4x3.device)
        volume_variance, amips_energy, edge = self.energies(tet_bxfx4x3, inv_v)
        # The surface terms differ per shape (its own predicted boundary, a different face count).  The reference loops
        # over the shapes (deftet.py:89-103); here ONE ragged launch sequence covers the batch: the per-shape chains of
        # small launches would otherwise be bound by the host (8 shapes x ~150 framework + library calls ~ 25 ms).
        terms = surface_losses.surface_terms_batched(vertice_pos, boundary, gt_surface_points, per_face=20, stacked=True,
                                                     uv=getattr(self, "sample_uv", None))             # [3,B] (sample_uv: tests only)
        sum_chamfer, sum_analytic, sum_normal = terms.mean(1, keepdim=True)                          # three [1] tensors (:104-110)
        center_occ = center_occ.squeeze(-1)
        if inference:
            assert point_pos_bxpx3 is not None, 'point_pos_bxpx3 not given'
            # (the traversal order of the query is decided per TOPOLOGY when the index list is at hand; positions only otherwise)
            topo = _topology_for(tetrahedron_bxfx4, vertice_pos.shape[1]) if tetrahedron_bxfx4 is not None else None
            condition = check_condition_f_base(tet_bxfx4x3, point_pos_bxpx3, topo)
            pred_surface_face = self.get_boundary_index(face_fx3, face_tet_fx2, (pred_occ > inference_threshold).float())
            return (amips_energy, edge, volume_variance, sum_analytic, sum_normal, center_occ, condition, boundary,
                    pred_surface_face, sum_chamfer)
        return (amips_energy, edge, volume_variance, sum_analytic, sum_normal, center_occ, boundary, sum_chamfer,
                torch.zeros_like(sum_normal))

    def forward(self, v_pos_bxnx3=None, tet_bxfx4=None, boundary_bxfx3=None, gt_surface_point=None, inverse_offset=None,
                tet_bxfx4x3=None, calculate_amips_volume=True):
        """(chamfer, analytic, normal[, volume variance, amips, tet positions]) of one predicted surface
        (deftet.py:138-184); all ones when the surface is empty (:159-163)."""
        extra = ()
        if calculate_amips_volume:
            tet_pos = tet_bxfx4x3 if tet_bxfx4x3 is not None else self.gather_tet_pos(v_pos_bxnx3, tet_bxfx4)
            if inverse_offset is not None:
                vv, am, _ = self.energies(tet_pos, inverse_offset.to(tet_pos.device))
            else:
                vv = self.volume_variance(tet_pos, pow=self.pow)
                am = torch.zeros_like(vv)
            extra = (vv, am, tet_pos)
        if boundary_bxfx3.shape[1] == 0:
            one = torch.ones(1, device=boundary_bxfx3.device)
            return (one, one, one) + extra
        return surface_losses.surface_terms(v_pos_bxnx3, boundary_bxfx3, gt_surface_point, per_face=20) + extra

    def laplacian_sparse(self, offset, adj):
        """sum over vertices and coordinates of (mean of the neighbours' offsets - own offset)^2, per shape;
        adj = row-normalised vertex adjacency [V,V] (c_tet_to_adj_sparse(normalize=True)).  A hip_ops.VertexAdjacency adj
        (e.g. TetTopology.vertex_adjacency()) takes the fused HIP operator, hip_ops.vertex_laplacian; a torch sparse adj
        takes torch.sparse.mm as before."""
        if isinstance(adj, hip_ops.VertexAdjacency):
            return hip_ops.vertex_laplacian(offset, adj, reduction="shape")
        n_shape, n_vertex, width = offset.shape
        flat = offset.permute(1, 0, 2).reshape(n_vertex, n_shape * width)
        nei = torch.sparse.mm(adj, flat).reshape(n_vertex, n_shape, width).permute(1, 0, 2)
        return ((nei - offset) ** 2).sum(dim=(1, 2))

    # --- init-time helpers (pure torch, as in the reference)
    def my_inverse(self, T):
        det_m = (torch.abs(torch.det(T)) < 1e-10).float()                     # :215
        iden_m = torch.eye(T.shape[-1], dtype=torch.float, device=T.device).unsqueeze(0).expand(T.shape[0], -1, -1)
        tmp_m = T * (1 - det_m.unsqueeze(-1).unsqueeze(-1)) + iden_m * det_m.unsqueeze(-1).unsqueeze(-1)
        return torch.inverse(tmp_m).contiguous(), 1 - det_m              # (row-major: the energies would copy it per call)

    def tet_inverse_v(self, init_tet_pos, init_tet_fx4, scale=20):
        vertice_pos = init_tet_pos.float()
        tet = vertice_pos[init_tet_fx4.long()]                                 # [T,4,3]
        A, B, C, D = (tet[:, i:i + 1, :] * scale for i in range(4))
        offset_vec = torch.cat([B - A, C - A, D - A], dim=1)                   # :316
        return self.my_inverse(offset_vec)[0]
