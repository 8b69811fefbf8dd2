"""Evaluation metrics on the library's kernels: what eval.py:237-260 (Engine.validate_iou) and utils/point_cloud_utils.py compute
with Kaolin, forward only.

Kaolin-shaped entry points (the overlay's shim exposes them under Kaolin's names):
    sided_distance(p1, p2)                         -> dist f32 [B,N], idx int64 [B,N]
    point_to_mesh_distance(points, face_vertices)  -> dist f32 [B,P] (squared), face_idx int64 [B,P], dist_type int32 [B,P]
    sample_points(vertices, faces, num_samples)    -> points f32 [B,N,3], face_choice int64 [B,N]
    index_vertices_by_faces(vertices, faces)       -> face_vertices [B,F,3,3]
and the batched metric block, surface_metrics(...), which never synchronises the host.
"""
from __future__ import annotations

import torch

from deftet_amd import _lib, hip_ops

ESP = 1e-15          # utils/point_cloud_utils.py `esp`


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("deftet_amd.metrics is forward only: call it under torch.no_grad() (eval.py does) or detach the inputs")


def _n_face_dev(n_face, B, F, dev):
    if n_face is None:
        return None
    if not torch.is_tensor(n_face):
        return hip_ops.host_ints([int(v) for v in n_face], dev, i32=True)
    if n_face.numel() != B:
        raise ValueError("n_face: one count per shape expected (got %d for %d shapes)" % (n_face.numel(), B))
    return n_face.to(device=dev, dtype=torch.int32).contiguous()


def point_to_mesh_distance(points, face_vertices, n_face=None, brute=False):
    """points f32 [B,P,3], face_vertices f32 [B,F,3,3], n_face int32 [B] (optional, per-shape face counts) ->
    (dist f32 [B,P] squared, face_idx int64 [B,P], dist_type int32 [B,P]).  brute=True: the streaming scan (same bits)."""
    _lib.require_gpu(points, face_vertices, n_face if torch.is_tensor(n_face) else None)
    _no_grad(points, face_vertices)
    if points.dim() != 3 or points.shape[2] != 3 or face_vertices.dim() != 4 or face_vertices.shape[2:] != (3, 3) or \
            face_vertices.shape[0] != points.shape[0]:
        raise ValueError("point_to_mesh_distance: points [B,P,3] and face_vertices [B,F,3,3] expected")
    p, fv = points.detach().contiguous().float(), face_vertices.detach().contiguous().float()
    B, P, F, dev = p.shape[0], p.shape[1], fv.shape[1], p.device
    nf = _n_face_dev(n_face, B, F, dev)
    d = torch.empty(B, P, device=dev, dtype=torch.float32)
    fi = torch.empty(B, P, device=dev, dtype=torch.int64)
    dt = torch.empty(B, P, device=dev, dtype=torch.int32)
    if brute:
        _lib.call("deftet_point_mesh_distance_scan_f32", dev, p, fv, nf, B, P, F, d, fi, dt)
    else:
        _lib.call("deftet_point_mesh_distance_f32", dev, p, fv, nf, B, P, F, d, fi, dt,
                  ws=_lib.load().deftet_point_mesh_distance_workspace_bytes(B, P, F))
    return d, fi, dt


def _sided(p1, p2, want_i64=True):
    idx = hip_ops.nn_index(p1, p2)                                   # A10, unchanged
    B, N, M, dev = p1.shape[0], p1.shape[1], p2.shape[1], p1.device
    d = torch.empty(B, N, device=dev, dtype=torch.float32)
    i64 = torch.empty(B, N, device=dev, dtype=torch.int64) if want_i64 else None
    _lib.call("deftet_nn_distance_f32", dev, p1, p2, idx, B, N, M, d, i64)
    return d, i64, idx


def sided_distance(p1, p2):
    """kal.metrics.pointcloud.sided_distance: p1 [B,N,3], p2 [B,M,3] -> (dist f32 [B,N] squared, idx int64 [B,N]) of the nearest
    point of p2 (the first one with the strictly smallest fp32 distance)."""
    _lib.require_gpu(p1, p2)
    _no_grad(p1, p2)
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[2] != 3 or p2.shape[2] != 3 or p1.shape[0] != p2.shape[0]:
        raise ValueError("sided_distance: p1 [B,N,3] and p2 [B,M,3] expected")
    if p2.shape[1] == 0:
        raise ValueError("sided_distance: p2 has no points")
    d, i64, _ = _sided(p1.detach().contiguous().float(), p2.detach().contiguous().float())
    return d, i64


def index_vertices_by_faces(vertices_features, faces):
    """kal.ops.mesh.index_vertices_by_faces: [B,V,D] and faces [F,3] -> [B,F,3,D] (a gather; no kernel of its own)."""
    if faces.dim() != 2 or vertices_features.dim() != 3:
        raise ValueError("index_vertices_by_faces: vertices [B,V,D] and faces [F,3] expected")
    return vertices_features[:, faces.long()]


def sample_faces(face_vertices, n_face, uniforms, areas=None):
    """Batched, no host sync: face_vertices f32 [B,F,3,3], n_face int32 [B] (or None), uniforms f32 [B,N,3] in [0,1) ->
    (points f32 [B,N,3], face_choice int64 [B,N], empty int32 [B]); empty[b] = 1 for a shape with no faces or zero area
    (its points are NaN, its faces -1)."""
    _lib.require_gpu(face_vertices, uniforms, areas, n_face if torch.is_tensor(n_face) else None)
    _no_grad(face_vertices, areas)
    lib = _lib.load()
    fv, u = face_vertices.detach().contiguous().float(), uniforms.contiguous().float()
    B, F, N, dev = fv.shape[0], fv.shape[1], u.shape[1], fv.device
    if u.shape != (B, N, 3):
        raise ValueError("sample_faces: uniforms [B,N,3] expected")
    a = None if areas is None else areas.detach().reshape(B, F).contiguous().float()
    nf = _n_face_dev(n_face, B, F, dev)
    pts = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    ch = torch.empty(B, N, device=dev, dtype=torch.int64)
    empty = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.call("deftet_sample_points_f32", dev, fv, a, nf, u, B, F, N, pts, ch, empty, ws=lib.deftet_sample_points_workspace_bytes(B, F))
    return pts, ch, empty


def sample_points(vertices, faces, num_samples, areas=None, generator=None, face_features=None):
    """kal.ops.mesh.sample_points: vertices [B,V,3], faces [F,3] -> (points f32 [B,N,3], face_choice int64 [B,N]), faces drawn
    with probability proportional to their area.  Raises, as torch.multinomial would, when a shape has no area to sample."""
    if face_features is not None:
        raise NotImplementedError("sample_points: face_features is not supported (nothing in the evaluation uses it)")
    _lib.require_gpu(vertices, faces, areas)
    _no_grad(vertices, areas)
    fv = index_vertices_by_faces(vertices.detach(), faces)
    B = fv.shape[0]
    u = torch.rand(B, int(num_samples), 3, device=vertices.device, dtype=torch.float32, generator=generator)
    pts, ch, empty = sample_faces(fv, None, u, areas=areas)
    if int(empty.max().item()) if B > 0 else 0:
        raise RuntimeError("sample_points: a mesh has no faces or zero total area (nothing to sample)")
    return pts, ch


def metric_block(surface_points, pred_points, dist_a=None, dist_b=None, radius=0.01):
    """The fused reduction: surface_points [B,N1,3] (ground truth), pred_points [B,N2,3], optional squared point-to-mesh distances
    dist_a [B,Nh] (surface points to the predicted mesh) and dist_b [B,Nh] (predicted samples to the ground-truth mesh) ->
    f32 [B,5]: chamfer, chamfer_l1, f_score, mean_hausdorff, max_hausdorff."""
    lib = _lib.load()
    s, p = surface_points.contiguous().float(), pred_points.contiguous().float()
    B, N1, N2, dev = s.shape[0], s.shape[1], p.shape[1], s.device
    idx12 = hip_ops.nn_index(s, p)
    idx21 = hip_ops.nn_index(p, s)
    if (dist_a is None) != (dist_b is None) or (dist_a is not None and dist_a.shape != dist_b.shape):
        raise ValueError("metric_block: dist_a and dist_b must both be given, with the same shape")
    da = None if dist_a is None else dist_a.contiguous().float()
    db = None if dist_b is None else dist_b.contiguous().float()
    Nh = 0 if da is None else da.shape[1]
    out = torch.empty(B, 5, device=dev, dtype=torch.float32)
    _lib.call("deftet_surface_metrics_f32", dev, s, p, idx12, idx21, da, db, B, N1, N2, Nh, float(radius), out,
              ws=lib.deftet_surface_metrics_workspace_bytes(B))
    return out


def surface_metrics(pred_faces, pred_n_face, gt_faces, gt_n_face, surface_points, num_samples=100000, uniforms=None, generator=None,
                    radius=0.01, pred_verts=None, pred_faces_idx=None, sdf_points=None, gt_occ=None, inside_test="parity"):
    """eval.py's metric block for a batch of shapes, with no host synchronisation.

    pred_faces f32 [B,Fp,3,3] / gt_faces f32 [B,Fg,3,3]: padded face vertices, pred_n_face / gt_n_face int32 [B] their counts;
    surface_points f32 [B,N1,3]: the ground-truth surface cloud.  The predicted surface is sampled (num_samples points per shape,
    from `uniforms` f32 [B,N,3] or torch.rand with `generator`), both sided distances are taken once each, both point-to-mesh
    queries are run, and one fused reduction gives f32 [B] tensors keyed chamfer, chamfer_l1, f_score, mean_hausdorff,
    max_hausdorff.  With pred_verts / pred_faces_idx (lists of [V_b,3] / [F_b,3] per shape), sdf_points [B,Q,3] and gt_occ [B,Q],
    also iou (check_sign of the predicted mesh against gt_occ > 0, as eval.py's point_cloud_iou at thresh 0.5; with
    inside_test="winding" the generalised winding number, w > 0.5, labels the points instead of ray parity: for predicted meshes
    that are not watertight).
    A shape with nothing to sample gets NaN metrics."""
    _lib.require_gpu(pred_faces, gt_faces, surface_points, uniforms, sdf_points, gt_occ)
    if inside_test not in ("parity", "winding"):
        raise ValueError("surface_metrics: inside_test %r is not 'parity' or 'winding'" % (inside_test,))
    _no_grad(pred_faces, gt_faces, surface_points)
    B, dev = pred_faces.shape[0], pred_faces.device
    if uniforms is None:
        uniforms = torch.rand(B, int(num_samples), 3, device=dev, dtype=torch.float32, generator=generator)
    pred_pts, _, _ = sample_faces(pred_faces, pred_n_face, uniforms)
    s = surface_points.contiguous().float()
    if s.shape[1] != pred_pts.shape[1]:
        raise ValueError("surface_metrics: the Hausdorff mean pairs surface points with samples; %d surface points against %d samples"
                         % (s.shape[1], pred_pts.shape[1]))
    da, _, _ = point_to_mesh_distance(s, pred_faces, pred_n_face)
    db, _, _ = point_to_mesh_distance(pred_pts, gt_faces, gt_n_face)
    out = metric_block(s, pred_pts, da, db, radius)
    res = {"chamfer": out[:, 0], "chamfer_l1": out[:, 1], "f_score": out[:, 2], "mean_hausdorff": out[:, 3], "max_hausdorff": out[:, 4]}
    if sdf_points is not None:
        if inside_test == "winding":
            inside = hip_ops.winding_inside(hip_ops.winding_number_ragged(pred_verts, pred_faces_idx, sdf_points, check=False))
        else:
            inside = hip_ops.check_sign_ragged(pred_verts, pred_faces_idx, sdf_points)
        a, g = inside.float(), (gt_occ > 0.0).float()
        res["iou"] = (a * g).sum(-1) / (a + g).clamp(0, 1).sum(-1)
    return res
