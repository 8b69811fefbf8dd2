"""The point-voxel operators of the point-cloud encoder (layers/pv_module/functional) on this library's HIP kernels
(pointvoxel.hip): average voxelization and trilinear devoxelization, with the reference's signatures.

    avg_voxelize(features, coords, resolution)            functional/voxelization.py
    trilinear_devoxelize(c, coords, r, training=None)     functional/devoxelization.py:44-50 (the live, grid_sample form)
    trilinear_devoxelize_ori(features, coords, r, is_training=True)   the extension's own pair
    sample_f(point_pos, c_list, append_pos=False)         pc_model.py:182-194 in one operator
    decode_occ_features(pos, tet_bxfx4, c_list, ...)      pc_model.py:276-306: the decoder's input from the vertices, in one operator
    backend                                               the twelve names of functional/src/bindings.cpp

`overlay.install(point_voxel=True)` registers `backend` as `layers.pv_module.functional.backend._backend` and this module as
`layers.pv_module.functional.devoxelization`.  Every entry point raises on non-GPU tensors.
"""
import torch
from torch.autograd import Function

from . import hip_ops

__all__ = ["avg_voxelize", "trilinear_devoxelize", "trilinear_devoxelize_ori", "sample_f", "decode_occ_features", "backend"]


class AvgVoxelization(Function):
    @staticmethod
    def forward(ctx, features, coords, resolution):
        features = features.contiguous().float()
        coords = coords.int().contiguous()
        b, c, _ = features.shape
        out, indices, counts = hip_ops.avg_voxelize_fwd(features, coords, resolution)
        ctx.save_for_backward(indices, counts)
        return out.view(b, c, resolution, resolution, resolution)

    @staticmethod
    def backward(ctx, grad_output):
        b, c = grad_output.shape[:2]
        indices, counts = ctx.saved_tensors
        return hip_ops.avg_voxelize_bwd(grad_output.contiguous().view(b, c, -1), indices, counts), None, None


avg_voxelize = AvgVoxelization.apply


class TrilinearDevoxelization(Function):
    @staticmethod
    def forward(ctx, features, coords, resolution, is_training=True):
        B, C = features.shape[:2]
        features = features.contiguous().view(B, C, -1).float()
        coords = coords.contiguous().float()
        outs, inds, wgts = hip_ops.trilinear_devoxelize_fwd(resolution, is_training, coords, features)
        if is_training:
            ctx.save_for_backward(inds, wgts)
            ctx.r = resolution
        return outs

    @staticmethod
    def backward(ctx, grad_output):
        inds, wgts = ctx.saved_tensors
        grad_inputs = hip_ops.trilinear_devoxelize_bwd(grad_output.contiguous(), inds, wgts, ctx.r)
        return grad_inputs.view(grad_output.size(0), grad_output.size(1), ctx.r, ctx.r, ctx.r), None, None, None


trilinear_devoxelize_ori = TrilinearDevoxelization.apply


def trilinear_devoxelize(c, coords, r, training=None):
    """c f32 [B,C,r,r,r] read at coords f32 [B,3,N] in voxel units -> [B,C,N]: what grid_sample (border, align_corners=False, the
    coordinate flip) computes for these arguments, with gradients to c and coords.  `training` is accepted and ignored, as in the
    live reference function (nothing is recorded for the backward: it sorts the points itself).  c and coords are read as f32."""
    if c.shape[-1] != int(r):
        raise RuntimeError("trilinear_devoxelize: r = %d does not match the volume %s" % (int(r), tuple(c.shape)))
    return hip_ops.voxel_sample([c.float()], coords.float(), voxel_units=True)


def sample_f(point_pos, c_list, append_pos=False):
    """point_pos f32 [B,N,3] in [-0.5, 0.5], c_list of volumes [B,C_k,R_k,R_k,R_k] -> [B, sum C_k (+3), N]: sample_f, and with
    append_pos the torch.cat([feat, pos.permute(0,2,1)], 1) that decode_pos / decode_occ put behind it, in one result."""
    return hip_ops.voxel_sample(c_list, point_pos, append_pos=append_pos)


def decode_occ_features(pos, tet_bxfx4, c_list, center_idx=None, first=0, count=None):
    """occ_feature f32 [B, sum C_k + 3, K] of decode_occ (pc_model.py:276-306, pos_encoder = None): the volumes c_list read at the
    centroids of the tets of (pos f32 [B,V,3], tet_bxfx4 int [B,T,4]) and the centroids behind them.  center_idx int [K]: the
    tets the training step keeps (`randperm(T)[:10000]`); otherwise the range [first, first + count) of split_decode_occ's walk
    (count=None: to the end).  The gathered [B,T,4,3] tensor, its mean and the index step are never built; the gradient reaches
    pos through the topology's cached incidence CSR and every volume of c_list (hip_ops.tet_centroid_sample)."""
    from .layers.DefTet.deftet import _topology_for
    topo = _topology_for(tet_bxfx4, pos.shape[1])
    return topo.centroid_sample(c_list, pos, select=center_idx, first=first, count=count, append_pos=True)


class _Backend:
    """functional/src/bindings.cpp by name.  The network of pc_model.py reaches the four below only."""

    @staticmethod
    def avg_voxelize_forward(features, coords, resolution):
        return list(hip_ops.avg_voxelize_fwd(features, coords, resolution))

    @staticmethod
    def avg_voxelize_backward(grad_y, indices, cnt):
        return hip_ops.avg_voxelize_bwd(grad_y, indices, cnt)

    @staticmethod
    def trilinear_devoxelize_forward(r, is_training, coords, features):
        return list(hip_ops.trilinear_devoxelize_fwd(r, is_training, coords, features))

    @staticmethod
    def trilinear_devoxelize_backward(grad_y, indices, weights, r):
        return hip_ops.trilinear_devoxelize_bwd(grad_y, indices, weights, r)


UNIMPLEMENTED = ("gather_features_forward", "gather_features_backward", "furthest_point_sampling", "ball_query", "grouping_forward",
                 "grouping_backward", "three_nearest_neighbors_interpolate_forward", "three_nearest_neighbors_interpolate_backward")


def _unimplemented(name):
    def fn(*args, **kwargs):
        raise NotImplementedError("%s: this PointNet++ kernel of the extension is not part of deftet_amd "
                                  "(create_pointnet_components never calls it)" % name)
    fn.__name__ = name
    return staticmethod(fn)


for _name in UNIMPLEMENTED:
    setattr(_Backend, _name, _unimplemented(_name))

backend = _Backend()
