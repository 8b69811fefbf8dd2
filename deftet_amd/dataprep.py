"""Ground-truth preparation on the GPU: what the reference's dataloader.py does with Kaolin — a watertight remesh
of every shape (MakeSurfaceMesh, dataloader.py:24-61) and signed-distance labels (kaolin_mesh_to_sdf, :91-97) — on this
library's kernels (csrc/dataprep.hip), under `no_grad` (label preparation has no gradient).

PARITY UNPINNED: Kaolin is not part of the reference tree and cannot be read or run next to this library.  The voxel rule, the
depth-map order and the surface of a grid are this library's own, stated in include/deftet_hip.h and restated in numpy in
tests/dataprep_ref.py; closedness and volume properties pin them.  Two known differences: the voxelization is the conservative
13-axis overlap test, and voxelgrids_to_trianglemeshes gives the voxel faces (cuberille) where Kaolin runs marching cubes — on a
binary grid both surfaces lie on the voxel faces and differ by the chamfer at the corners, and MakeSurfaceMesh rescales the result
to the input's box afterwards, so offset and unit do not matter.

    mesh_voxelize, extract_odms, project_odms, voxel_fill, voxel_surface_mesh      the stages (hip_ops)
    trianglemeshes_to_voxelgrids, voxelgrids_to_trianglemeshes, adjacency_matrix, face_normals     with Kaolin's parameter names
    smooth_vertices, make_surface_mesh, mesh_to_sdf                                the transforms
"""
import torch

from . import _lib, hip_ops, metrics
from .hip_ops import VertexAdjacency, VoxelBits, extract_odms, mesh_voxelize, project_odms, voxel_fill, voxel_pack, voxel_surface_mesh

__all__ = ["VoxelBits", "mesh_voxelize", "extract_odms", "project_odms", "voxel_fill", "voxel_pack", "voxel_surface_mesh",
           "trianglemeshes_to_voxelgrids", "voxelgrids_to_trianglemeshes", "adjacency_matrix", "face_normals", "smooth_vertices",
           "make_surface_mesh", "mesh_to_sdf"]


def trianglemeshes_to_voxelgrids(vertices, faces, resolution, origin=None, scale=None, return_sparse=False):
    """kaolin.ops.conversions.trianglemeshes_to_voxelgrids: float32 [B,R,R,R] of hip_ops.mesh_voxelize (parity unpinned)."""
    if return_sparse:
        raise NotImplementedError("trianglemeshes_to_voxelgrids: return_sparse=True is not supported")
    return mesh_voxelize(vertices, faces, resolution, origin=origin, scale=scale).float()


def voxelgrids_to_trianglemeshes(voxelgrids, iso_value=0.5):
    """kaolin.ops.conversions.voxelgrids_to_trianglemeshes: (list of verts, list of faces) of hip_ops.voxel_surface_mesh — the
    voxel faces, not marching cubes (parity unpinned)."""
    return voxel_surface_mesh(voxelgrids, iso_value=iso_value)


def adjacency_matrix(num_vertices, faces, sparse=True):
    """kaolin.ops.mesh.adjacency_matrix: the 0/1 torch sparse COO [V,V] of the unique undirected edges (hip_ops.face_edges)."""
    if not sparse:
        raise NotImplementedError("adjacency_matrix: sparse=False is not supported")
    V = int(num_vertices)
    pairs = hip_ops.face_edges(faces, V).long()
    return torch.sparse_coo_tensor(pairs.t(), torch.ones(pairs.shape[0], device=pairs.device, dtype=torch.float32), (V, V)).coalesce()


def face_normals(face_vertices, unit=False):
    """kaolin.ops.mesh.face_normals: face_vertices [B,F,3,3] -> (v1 - v0) x (v2 - v0) [B,F,3], divided by its length with `unit`
    (a torch restatement; a zero-area face gives a zero normal)."""
    if face_vertices.dim() != 4 or tuple(face_vertices.shape[2:]) != (3, 3):
        raise ValueError("face_normals: face_vertices [B,F,3,3] expected")
    n = torch.cross(face_vertices[:, :, 1] - face_vertices[:, :, 0], face_vertices[:, :, 2] - face_vertices[:, :, 0], dim=-1)
    if unit:
        length = n.norm(dim=-1, keepdim=True)
        n = n / torch.where(length == 0, torch.ones_like(length), length)
    return n


def smooth_vertices(verts, adjacency, iterations):
    """`iterations` rounds of v <- neighbour mean (dataloader.py:49-53) on hip_ops.vertex_aggregate at C = 3; verts f32 [V,3] or
    [B,V,3], adjacency = VertexAdjacency.from_faces(faces, V, normalize=True)."""
    _lib.require_gpu(verts)
    x = verts if verts.dim() == 3 else verts.unsqueeze(0)
    with torch.no_grad():
        for _ in range(int(iterations)):
            x = hip_ops.vertex_aggregate(x, adjacency)
    return x if verts.dim() == 3 else x[0]


def make_surface_mesh(vertices, faces, resolution=100, smoothing_iterations=3, max_length=0.9):
    """MakeSurfaceMesh.__call__ (dataloader.py:24-61) as one function: vertices f32 [V,3], faces int [F,3] -> (verts f32 [V',3],
    faces int64 [F',3]) on the GPU, a closed mesh.  Rescale by the largest extent to `max_length`, centre, voxelize, fill, extract
    the surface, smooth, rescale to the box of the centred input.  No tensor leaves the GPU; two small reads do, the per-shape counts
    of the surface extraction and the edge count of the adjacency (parity unpinned, see the module text)."""
    _lib.require_gpu(vertices, faces)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("make_surface_mesh: vertices [V,3] expected, got %s" % (tuple(vertices.shape),))
    with torch.no_grad():
        v = vertices.float()
        vmin, vmax = v.amin(dim=0), v.amax(dim=0)
        v = (v / (vmax - vmin).amax()) * max_length
        vmin, vmax = v.amin(dim=0), v.amax(dim=0)
        v = v - ((vmax + vmin) / 2).unsqueeze(0)
        bits = voxel_fill(mesh_voxelize(v.unsqueeze(0), faces, resolution, return_bits=True))
        new_v, new_f = voxel_surface_mesh(bits)
        new_v, new_f = new_v[0], new_f[0]
        if new_v.shape[0] == 0:
            return new_v, new_f
        new_v = smooth_vertices(new_v, VertexAdjacency.from_faces(new_f, new_v.shape[0], normalize=True), smoothing_iterations)
        omin, omax = v.amin(dim=0), v.amax(dim=0)
        nmin, nmax = new_v.amin(dim=0), new_v.amax(dim=0)
        new_v = (new_v - nmin) / (nmax - nmin)
        return new_v * (omax - omin) + omin, new_f


def mesh_to_sdf(verts, faces, points, sign="parity"):
    """kaolin_mesh_to_sdf (dataloader.py:91-97): verts f32 [B,V,3], faces [F,3], points f32 [B,N,3] -> f32 [B,N] =
    (2 check_sign - 1) · point_to_mesh_distance, positive inside.  The reference's quirk is kept: the distance is the SQUARED one
    (Kaolin's point_to_mesh_distance returns squared distances and the reference does not take the root).
    sign="winding" takes the sign from the generalised winding number (w > 0.5) instead of ray parity: for meshes that are not
    watertight."""
    if sign not in ("parity", "winding"):
        raise ValueError("mesh_to_sdf: sign %r is not 'parity' or 'winding'" % (sign,))
    with torch.no_grad():
        if sign == "winding":
            sign = hip_ops.winding_inside(hip_ops.winding_number(verts, faces, points))
        else:
            sign = hip_ops.check_sign(verts, faces, points)
        distance, _, _ = metrics.point_to_mesh_distance(points, metrics.index_vertices_by_faces(verts, faces))
        return (sign.float() * 2.0 - 1.0) * distance
