"""A smooth surface out of a render-side model: marching tetrahedra on the per-vertex occupancy `processfunc` returns
(DESIGN.md section 6l), where `Deftet.saveobj` (diff_render/diftet_6_subdiv/3_model/deftet.py:503-557) thresholds the maximum
over a tet's corners and emits whole tet faces."""
from deftet_amd import hip_ops


def model_tet_edges(model, n_vertex, device):
    """The TetEdges of model.tftet_tx4, kept on the model and keyed by the tet-list OBJECT (as model_topology keeps the
    FaceTopology of tff_fx3): rebuilt when `tftet_tx4` is another object, as after a subdivision or a deletion."""
    tets = model.tftet_tx4
    kept = getattr(model, "_deftet_tet_edges", None)
    if kept is None or kept[0] is not tets or kept[1].n_vertex != n_vertex or kept[1].device != device:
        kept = (tets, hip_ops.TetEdges(tets, n_vertex, device=device))
        model._deftet_tet_edges = kept
    return kept[1]


def _subdivided(mesh, levels, normals=False):
    """the one-shape IsoMesh `mesh` after `levels` rounds of Loop subdivision (hip_ops.loop_subdivide_mesh): verts, faces and
    vert_attr of the fine mesh; normals: vert_attr holds directions, normalised again after the weighting"""
    verts, faces, attr = hip_ops.loop_subdivide_mesh(mesh.verts, mesh.faces, mesh.vert_attr, levels=levels)
    if normals:
        attr = hip_ops.unit_normals(-attr)                            # (unit_normals negates: these are normals already)
    return hip_ops.IsoMesh(verts, faces, attr, None, None, None)


def _levels(subdivide, return_index=False):
    levels = int(subdivide)
    if levels < 0:
        raise ValueError("subdivide = %d is negative" % levels)
    if levels and return_index:
        raise ValueError("return_index describes the coarse mesh: its edge ids do not describe a subdivided one (subdivide = %d)" % levels)
    return levels


def _cleaned(mesh, keep_largest, min_faces, drop_voids):
    """the one-shape IsoMesh `mesh` after hip_ops.mesh_cleanup; with every option off, or without faces, `mesh` itself"""
    if not (bool(keep_largest) or int(min_faces) > 0 or bool(drop_voids)) or not mesh.faces.shape[0]:
        return mesh
    clean = hip_ops.mesh_cleanup(mesh.verts, mesh.faces, mesh.vert_attr, keep_largest=keep_largest, min_faces=min_faces, drop_voids=drop_voids)
    edge_id, t, tet_id = (None if x is None else x[m] for x, m in ((mesh.edge_id, clean.vertex_map), (mesh.t, clean.vertex_map),
                                                                   (mesh.tet_id, clean.face_map)))
    return hip_ops.IsoMesh(clean.verts, clean.faces, clean.attr, edge_id, t, tet_id)


def marching_tets(model, iso, processfunc, return_index=False, subdivide=0, keep_largest=False, min_faces=0, drop_voids=False):
    """hip_ops.IsoMesh of a reference-shaped `model` (get_point(True), get_feat(), tftet_tx4) at the level `iso` of the
    per-vertex weights: (weights [P,1], colours [P,C]) = processfunc(points, features) as in saveobj (:509-510).  The fields are
    tensors of the one shape, not lists: verts [Nv,3], faces int64 [Nf,3], vert_attr [Nv,C] = the colours at the vertices.
    Differentiable in whatever points, weights and colours depend on.  subdivide = n > 0: the mesh after n rounds of Loop
    subdivision (4^n times the faces; the colours take the positions' weights); not with return_index (ValueError).
    keep_largest / min_faces / drop_voids clean the mesh on the device BEFORE the subdivision (hip_ops.mesh_cleanup: cavity shells
    and floaters dropped, the mesh compacted, still differentiable); with return_index the rows of edge_id, t and tet_id are
    those of the kept vertices and faces.  With all three left at their defaults nothing of it runs."""
    levels = _levels(subdivide, return_index)
    points = model.get_point(True)
    weights, colours = processfunc(points, model.get_feat())
    topology = model_tet_edges(model, points.shape[0], points.device)
    mesh = hip_ops.marching_tets(points, weights.reshape(1, -1), topology, iso=iso, attr=colours, return_index=return_index)
    mesh = _cleaned(hip_ops.IsoMesh(*[None if x is None else x[0] for x in mesh]), keep_largest, min_faces, drop_voids)
    return _subdivided(mesh, levels) if levels and mesh.faces.shape[0] else mesh


def model_tet_csr(model, n_vertex, device):
    """(int32 tet list [1,T,4], its incidence CSR) of model.tftet_tx4, kept on the model and keyed by the tet-list object like
    model_tet_edges."""
    import torch
    tets = model.tftet_tx4
    kept = getattr(model, "_deftet_tet_csr", None)
    if kept is None or kept[0] is not tets or kept[1] != n_vertex or kept[2].device != device:
        idx = torch.as_tensor(tets).to(device).to(torch.int32).reshape(1, -1, 4).contiguous()
        kept = (tets, n_vertex, idx, hip_ops.tet_vertex_csr(idx, n_vertex))
        model._deftet_tet_csr = kept
    return kept[2], kept[3]


def marching_tets_normals(model, iso, processfunc, subdivide=0, keep_largest=False, min_faces=0, drop_voids=False):
    """marching_tets(model, iso, processfunc) with vert_attr [Nv,3] holding the unit OUTWARD normal instead of the colours: the
    per-vertex gradient of the weights (hip_ops.vertex_field_gradient, the volume-weighted mean of the tets' gradients)
    interpolated along each crossing edge, normalised and negated — inside is weights > iso, so the field falls towards the
    outside.  A zero gradient gives a zero normal.  Differentiable like marching_tets.  subdivide = n > 0: n rounds of Loop
    subdivision, the normals weighted like the positions and normalised again.  keep_largest / min_faces / drop_voids: the
    clean-up of marching_tets, before the subdivision."""
    levels = _levels(subdivide)
    points = model.get_point(True)
    weights, _colours = processfunc(points, model.get_feat())
    P, dev = points.shape[0], points.device
    idx, csr = model_tet_csr(model, P, dev)
    grad = hip_ops.vertex_field_gradient(weights.reshape(1, P, 1), points.reshape(1, P, 3), idx, csr=csr)
    mesh = hip_ops.marching_tets(points, weights.reshape(1, -1), model_tet_edges(model, P, dev), iso=iso, attr=grad.reshape(1, P, 3))
    mesh = mesh._replace(vert_attr=[hip_ops.unit_normals(a) for a in mesh.vert_attr])
    mesh = _cleaned(hip_ops.IsoMesh(*[None if x is None else x[0] for x in mesh]), keep_largest, min_faces, drop_voids)
    return _subdivided(mesh, levels, normals=True) if levels and mesh.faces.shape[0] else mesh
