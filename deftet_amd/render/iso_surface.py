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


def marching_tets(model, iso, processfunc, return_index=False):
    """hip_ops.IsoMesh of a reference-shaped `model` (get_point(True), get_feat(), tftet_tx4) at the level `iso` of the
    per-vertex weights: (weights [P,1], colours [P,C]) = processfunc(points, features) as in saveobj (:509-510).  The fields are
    tensors of the one shape, not lists: verts [Nv,3], faces int64 [Nf,3], vert_attr [Nv,C] = the colours at the vertices.
    Differentiable in whatever points, weights and colours depend on."""
    points = model.get_point(True)
    weights, colours = processfunc(points, model.get_feat())
    topology = model_tet_edges(model, points.shape[0], points.device)
    mesh = hip_ops.marching_tets(points, weights.reshape(1, -1), topology, iso=iso, attr=colours, return_index=return_index)
    return hip_ops.IsoMesh(*[None if x is None else x[0] for x in mesh])
