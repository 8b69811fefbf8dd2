"""Rendering a tet mesh straight from its vertices: one differentiable call from the optimiser's per-vertex parameters and a
camera to the composited image, with the gradient landing on the vertices.

    render_vertices(points, features, topology, cameras, pixels, ranges, ...)   project -> gather -> rasterize + composite
    model_forward(model, impixsample_hxw, camrot, camtrans, camproj, depth)     the same behind the argument and return order of
                                                                                 the reference's Deftet.forward
                                                                                 (diff_render/diftet_6_subdiv/3_model/deftet.py:407-478)

Every stage is a HIP operator: hip_ops.project_vertices, hip_ops.face_gather (its backward is a CSR reduction: no atomics, the
same bits on every run) and deftet_sparse_render_composite.  Points and features shared by the views are never repeated."""
import torch

from deftet_amd import hip_ops
from .deftet_sparse_render import NEAREST, deftet_sparse_render_composite


def _per_view(t, B, what):
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[2] != 2 or t.shape[0] not in (1, B):
        raise RuntimeError("render_vertices: %s [P,2], [1,P,2] or [B,P,2] expected" % what)
    return t.expand(B, -1, -1)


def render_vertices(points, features, topology, cameras, pixels, ranges, multiplier=1.0, knum=300, eps=1e-8, policy=NEAREST,
                    depth=False, background=1.0, far_depth=-6.0):
    """(colour [B,P,D-1], coverage [B,P,1], depth [B,P,1] | None) of the face soup `topology` (a hip_ops.FaceTopology) with
    vertices points [V,3] | [B,V,3] and features [V,D] | [B,V,D] (opacity, colour...; before the sigmoid) seen by cameras =
    (rotation [B,3,3], position [B,3], projection [3] | [3,1]) at `pixels` within `ranges` ([P,2], [1,P,2] or [B,P,2]; pixels in
    the units of the image coordinates AFTER `multiplier`).  It is exactly

        z, xy, act = hip_ops.project_vertices(points, features, cameras, multiplier, depth)
        deftet_sparse_render_composite(pixels, ranges, *hip_ops.face_gather(z, xy, act, topology), knum, eps, policy, depth, ...)[:3]

    with depth=True the camera-space z travels as feature channel 0 and comes back as the expected depth.  Gradients flow to
    points and features."""
    if not isinstance(topology, hip_ops.FaceTopology):
        raise TypeError("render_vertices: topology must be a hip_ops.FaceTopology (built once per face list)")
    B = cameras[0].shape[0]
    z, xy, act = hip_ops.project_vertices(points, features, cameras, multiplier, depth)
    face_z, face_xy, face_feat = hip_ops.face_gather(z, xy, act, topology)
    colour, coverage, dep, _ = deftet_sparse_render_composite(_per_view(pixels, B, "pixels"), _per_view(ranges, B, "ranges"), face_z,
                                                              face_xy, face_feat, knum=knum, eps=eps, policy=policy, depth=depth,
                                                              background=background, far_depth=far_depth)
    return colour, coverage, dep


def model_topology(model, n_vertex, device):
    """The FaceTopology of model.tff_fx3, kept on the model and keyed by the face-list OBJECT: it is rebuilt when `tff_fx3` is
    another object (the reference assigns a new tensor after a subdivision or a deletion, 3_model/deftet.py:147), never compared
    by pointer or version."""
    faces = model.tff_fx3
    kept = getattr(model, "_deftet_face_topology", None)
    if kept is None or kept[0] is not faces or kept[1].n_vertex != n_vertex or kept[1].device != device:
        kept = (faces, hip_ops.FaceTopology(faces, n_vertex, device=device))
        model._deftet_face_topology = kept
    return kept[1]


def model_forward(model, impixsample_hxw, camrot_bx3x3, camtrans_bx3, camproj_3x1, depth=False, viewpoint=False, knum=300):
    """Deftet.forward (3_model/deftet.py:407-478) with rendermeshcolor as its render function, on a reference-shaped `model`
    (get_point(True), get_feat(), xy_px2, multiplier, tff_fx3): (colour [B,P,3], mask [B,P,1]) and, with depth=True, the expected
    depth [B,P,1].  The pixels are model.xy_px2 at the flat indices `impixsample_hxw`; the ranges are the reference's [-1000, 0]."""
    if viewpoint:
        raise AssertionError("model_forward: viewpoint=True is not supported (the reference's renderer asserts `not viewdir`, "
                             "5_rendereq/deftetrneder.py:81)")
    points, features = model.get_point(True), model.get_feat()
    topology = model_topology(model, points.shape[0], points.device)
    pixels = (model.xy_px2[impixsample_hxw.reshape(-1)] * model.multiplier)[None]
    ranges = torch.zeros_like(pixels)
    ranges[:, :, 0] = -1000
    colour, mask, dep = render_vertices(points, features, topology, (camrot_bx3x3, camtrans_bx3, camproj_3x1), pixels, ranges,
                                        multiplier=model.multiplier, knum=knum, depth=depth)
    return (colour, mask, dep) if depth else (colour, mask)
