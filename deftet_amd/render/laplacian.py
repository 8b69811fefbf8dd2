"""`Deftet.get_featlap` of diff_render/diftet_6_subdiv/3_model/deftet.py:221-241 on the fused vertex Laplacian
(hip_ops.vertex_laplacian): the mean of each point's neighbours' features minus its own, squared, per entry."""
from deftet_amd import hip_ops


def get_featlap(pointfeat_pxc, adjacency):
    """f32 [P,C] = mse_loss(Σ_m feat[nei] / w, feat, reduction='none') — the reference's get_featlap output, differentiable
    w.r.t. pointfeat_pxc [P,C] (1 <= C <= 16).  adjacency: a hip_ops.VertexAdjacency of the model's point table, e.g.
    VertexAdjacency.from_table(model.tfpoint_adj_idx_pxm, model.tfpoint_adj_weights_px1, index_base=1)."""
    if pointfeat_pxc.dim() != 2:
        raise RuntimeError("get_featlap: point features [P,C] expected, got %s" % (tuple(pointfeat_pxc.shape),))
    return hip_ops.vertex_laplacian(pointfeat_pxc.unsqueeze(0), adjacency, reduction="none")[0]
