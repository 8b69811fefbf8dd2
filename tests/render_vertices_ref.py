"""Torch restatement of the render path from the vertices, independent of deftet_amd: every function
follows the dtype of its inputs, so it runs in fp64 as the reference of the GPU tests, and in fp32 it performs the operations of
the HIP kernels in the same order.  Host restatements of the face CSR and of the slot-ordered reduction are here too."""
import numpy as np
import torch

ALPHA_EPS = 1e-10


def perspective(points_bxvx3, cameras):
    """cam = R (p - c), every row summed left to right, and (cam.x px, cam.y py) / (cam.z pz) (3_model/cameraop.py:19-33)"""
    rot, pos, proj = cameras
    proj = proj.reshape(-1)
    d = points_bxvx3 - pos[:, None, :]
    cam = torch.stack([(d[..., 0] * rot[:, None, i, 0] + d[..., 1] * rot[:, None, i, 1]) + d[..., 2] * rot[:, None, i, 2]
                       for i in range(3)], -1)
    scaled = cam * proj
    return cam, scaled[..., :2] / scaled[..., 2:3]


def project_vertices(points, features, cameras, multiplier=1.0, depth=False):
    """(z [B,V], xy [B,V,2], act [B,V,Do]); [V,*] / [1,V,*] inputs are shared by the B views"""
    B = cameras[0].shape[0]
    points = points[None] if points.dim() == 2 else points
    features = features[None] if features.dim() == 2 else features
    cam, xy = perspective(points.expand(B, -1, -1), cameras)
    act = torch.sigmoid(features).expand(B, -1, -1)
    if depth:
        act = torch.cat([cam[..., 2:3], act], -1)
    return cam[..., 2], xy * multiplier, act


def face_attributes(vertex_features_bxvxk, faces_fx3):
    """[B,F,3*K]: the K attributes of corner 0, 1, 2 of every face (4_render/vertex2face.py:12-28)"""
    B, K = vertex_features_bxvxk.shape[0], vertex_features_bxvxk.shape[2]
    return vertex_features_bxvxk[:, faces_fx3.reshape(-1)].reshape(B, -1, 3 * K)


def face_gather(z, xy, act, faces_fx3):
    B, F = z.shape[0], faces_fx3.shape[0]
    return (face_attributes(z[..., None], faces_fx3).reshape(B, F, 3), face_attributes(xy, faces_fx3).reshape(B, F, 3, 2),
            face_attributes(act, faces_fx3).reshape(B, F, 3, act.shape[-1]))


def alpha_composite(layers_bxpxkxd, depth_bxpxkx1=None, background=1.0, far_depth=-6.0):
    """front-to-back compositing, opacity = channel 0 (peel2mask, 5_rendereq/deftetrneder.py:31-64)"""
    alpha = layers_bxpxkxd[..., :1].clamp(ALPHA_EPS, 1.0 - ALPHA_EPS)
    through = torch.cumprod(1.0 - alpha, dim=2)
    weight = alpha * torch.cat([torch.ones_like(through[:, :, :1]), through[:, :, :-1]], dim=2)
    coverage = weight.sum(2)
    colour = (weight * layers_bxpxkxd[..., 1:]).sum(2) + background * (1.0 - coverage)
    depth = None if depth_bxpxkx1 is None else (weight * depth_bxpxkx1).sum(2) + far_depth * (1.0 - coverage)
    return colour, coverage, depth


def face_vertex_csr(faces_fx3, n_vertex):
    """(offsets int32 [V+1], slots int32 [3F]): slots 3*f+corner in ascending order per vertex (a stable sort by vertex)"""
    flat = np.asarray(faces_fx3, np.int64).reshape(-1)
    slots = np.argsort(flat, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertex))]).astype(np.int32)
    return offsets, slots


def slot_table(offsets, slots, n_vertex):
    """(table int64 [V,maxdeg] of slots, padded with the index 3F of a zero row; maxdeg)"""
    deg = np.diff(offsets.astype(np.int64))
    maxdeg = int(deg.max()) if deg.size else 0
    table = np.full((n_vertex, max(maxdeg, 1)), slots.size, np.int64)
    for v in range(n_vertex):
        table[v, :deg[v]] = slots[offsets[v]:offsets[v + 1]]
    return table, maxdeg


def slot_ordered_sum(grad_bxfx3xc, table):
    """[B,V,C]: per vertex the rows of grad (flattened to [B,3F,C], a zero row appended) at the table's slots, the columns
    added left to right in the dtype of grad — the exact oracle of deftet_face_gather_bwd_f32"""
    B, C = grad_bxfx3xc.shape[0], grad_bxfx3xc.shape[-1]
    rows = torch.cat([grad_bxfx3xc.reshape(B, -1, C), grad_bxfx3xc.new_zeros(B, 1, C)], 1)
    t = torch.as_tensor(table, device=rows.device)
    acc = rows[:, t[:, 0]]
    for k in range(1, t.shape[1]):
        acc = acc + rows[:, t[:, k]]
    return acc
