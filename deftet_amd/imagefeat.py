"""Pixel-aligned image features for the single-image branch (DeformableTetNetwork(point_cloud=False), layers/pc_model.py with
layers/disn.py) on this library's HIP kernels (image_sample.hip): the counterpart of pointvoxel.py.

    project_to_image(pos, cam_rot, cam_pos, cam_proj, flip_y=True)     render.camera.perspective's arithmetic, as uv
    project_with_matrix(pos, camera_matrix)                            DISNDecoder._project_points_to_image (disn.py:257-276)
    extract_point_image_features(feature_maps, query_points, camera_matrix)
                                                                       DISNDecoder._extract_point_image_features (disn.py:278-305)
    sample_f(point_pos, encoder_features, cam_pos, cam_rot, cam_proj, append_pos=True)
                                                                       the image form of pc_model.sample_f: DISNDecoder's whole input

The two projections are plain torch (differentiable, any device and dtype); the sampling is hip_ops.image_sample and raises on
non-GPU tensors.
"""
import torch

from . import hip_ops

__all__ = ["project_to_image", "project_with_matrix", "extract_point_image_features", "sample_f"]


def project_to_image(pos, cam_rot, cam_pos, cam_proj, flip_y=True):
    """uv [B,N,2] of pos [B,N,3] under the camera (rotation [B,3,3], position [B,3], projection [3,1]): the camera-space points
    (pos - cam_pos) R^T, scaled by the projection vector and divided by the scaled depth (cameraop.py:19-33).  flip_y negates y:
    the camera's y points up, row 0 of an image is its top row, and grid_sample's v = -1 is that row."""
    cam = torch.matmul(pos - cam_pos.view(-1, 1, 3), cam_rot.permute(0, 2, 1))
    scaled = cam * cam_proj.view(-1, 1, 3)
    uv = scaled[:, :, :2] / scaled[:, :, 2:3]
    if flip_y:
        uv = torch.stack([uv[..., 0], -uv[..., 1]], dim=-1)
    return uv


def project_with_matrix(pos, camera_matrix):
    """uv [B,N,2] of pos [B,N,3]: the homogeneous row vector (x, y, z, 1) times camera_matrix [B,4,4], divided by its component
    2, first two components."""
    ones = torch.ones(pos.shape[0], pos.shape[1], 1, device=pos.device, dtype=pos.dtype)
    proj = torch.matmul(torch.cat((pos, ones), dim=2), camera_matrix)
    proj = proj / proj[:, :, 2:3]
    return proj[:, :, :2]


def extract_point_image_features(feature_maps, query_points, camera_matrix):
    """[B,N,sum C] (a permuted view of the operator's [B,sum C,N]): the map, or the list of maps, [B,C_k,H_k,W_k] read bilinearly
    (zeros padding, align_corners=False) at the projections of query_points [B,N,3] under camera_matrix [B,4,4]."""
    maps = [feature_maps] if torch.is_tensor(feature_maps) else list(feature_maps)
    uv = project_with_matrix(query_points, camera_matrix)
    return hip_ops.image_sample(maps, uv.float()).permute(0, 2, 1)


def sample_f(point_pos, encoder_features, cam_pos, cam_rot, cam_proj, append_pos=True):
    """[B, G + sum C_k (+3), N]: the complete input of DISNDecoder for the points point_pos [B,N,3] seen by the camera.
    encoder_features is DISNEncoder.forward's list [global [B,G], map_1, ...] (disn.py:242-243): the global rows first, then
    every map read at the projected points, then (append_pos) the positions transposed, in one result tensor."""
    feats = list(encoder_features)
    uv = project_to_image(point_pos, cam_rot, cam_pos, cam_proj)
    return hip_ops.image_sample(feats[1:], uv.float(), global_features=feats[0], append=point_pos.float() if append_pos else None)
