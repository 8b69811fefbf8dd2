"""The per-vertex quantities of a render-side model read at free points: what `processfunc` makes of the
vertex features (or the features themselves) interpolated with the barycentric weights of the tet that holds each point, so that
labels given at points (an SDF, an occupancy, colours) can supervise what `marching_tets` and the renderer consume at vertices."""
import torch

from deftet_amd import hip_ops


def model_tet_topology(model, n_vertex, device):
    """The TetTopology (int32 list + incidence CSR) of model.tftet_tx4, kept on the model and keyed by the tet-list OBJECT, as
    model_tet_edges keeps its TetEdges: rebuilt when `tftet_tx4` is another object, as after a subdivision or a deletion."""
    from deftet_amd.layers.DefTet.deftet import TetTopology
    tets = model.tftet_tx4
    kept = getattr(model, "_deftet_tet_topology", None)
    if kept is None or kept[0] is not tets or kept[1].n_vertex != n_vertex or kept[1].tet_idx.device != device:
        kept = (tets, TetTopology(tets.to(device), n_vertex))
        model._deftet_tet_topology = kept
    return kept[1]


def field_at_points(model, points_qx3, processfunc=None):
    """(values [Q,C], hit bool [Q]) of a reference-shaped `model` (get_point(True), get_feat(), tftet_tx4) at the points [Q,3]:
    the vertex features, or with `processfunc` cat(weights [P,1], colours [P,K]) = processfunc(points, features) as marching_tets
    reads them, interpolated in the tet that holds each point; 0 and hit False where none does.  Differentiable in whatever the
    vertex positions, the features and the points depend on."""
    points = model.get_point(True)
    field = model.get_feat()
    if processfunc is not None:
        weights, colours = processfunc(points, field)
        field = torch.cat([weights.reshape(points.shape[0], -1), colours.reshape(points.shape[0], -1)], dim=1)
    topology = model_tet_topology(model, points.shape[0], points.device)
    out, cond, _bary = topology.field_sample(field[None], points[None], points_qx3[None], return_index=True)
    return out[0], cond[0, :, 0] >= 0
