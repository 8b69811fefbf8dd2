"""HIP-backed twin of /root/reference/diff_render/diftet_6_subdiv/3_model/utils_tetsv.py (same names, argument order and return
values): the thresholded surface of a per-tet occupancy and its OBJ writers.

    tet_adj_share            (:16-75)     get_face_use_occ        (:79-128)     save_tet_face        (:131-141)
    get_face_use_occ_color   (:145-225)   save_tet_face_color     (:228-239)

Like render/prepare_for_wz.py these take numpy arrays (returned as numpy, like the reference) or GPU torch tensors (returned as
tensors).  `tet_adj` is what tet_adj_share of THIS module returns first (a neighbour table on the GPU) or the reference's own
list of four scipy / torch sparse matrices (converted on every call: convert once with hip_ops.neighbours_from_adj_list and
pass the result instead).  The reference asserts one shape; any batch size works here, with
center_occ [T,1] for one shape or [B,T] / [B,T,1].
"""
import numpy as np
import torch

from deftet_amd import hip_ops
from deftet_amd.render import export
from deftet_amd.render.prepare_for_wz import _dev, _in


def tet_adj_share(tet_list_tx4, n_point):
    """(neighbour table by local face, tet_neighbour_idx [T,4]) — the first stands in for the list of four matrices."""
    dev = _dev()
    tet = np.asarray(tet_list_tx4.cpu() if isinstance(tet_list_tx4, torch.Tensor) else tet_list_tx4)
    return hip_ops.tet_face_neighbours(tet, n_point, dev), hip_ops.tet_neighbours(tet, n_point, dev).cpu().numpy()


def _extract(tet_bxfx4x3, center_occ, tet_adj, htres, colour=None):
    tet, npy = _in(tet_bxfx4x3, torch.float32)
    occ, _ = _in(center_occ, torch.float32)
    hip_ops._lib.require_gpu(tet, occ)
    attr = None if colour is None else _in(colour, torch.float32)[0]
    nbr = hip_ops.neighbours_from_adj_list(tet_adj, tet.device)
    soup = hip_ops.surface_extract(tet, occ, nbr, "threshold", thres=htres, attr=attr)
    conv = (lambda xs: [x.cpu().numpy() for x in xs]) if npy else (lambda xs: xs)
    return conv(soup.face), (None if attr is None else conv(soup.face_attr))


def get_face_use_occ(tet_bxfx4x3, center_occ_cuda, tet_adj, htres=0.25):
    return _extract(tet_bxfx4x3, center_occ_cuda, tet_adj, htres)[0]


def get_face_use_occ_color(tet_bxfx4x3, tetcolor_bxfx4x3, center_occ_cuda, tet_adj, htres=0.25):
    return _extract(tet_bxfx4x3, center_occ_cuda, tet_adj, htres, tetcolor_bxfx4x3)


def save_tet_face(tet_fx3x3, f_name):
    with open(f_name, "w") as f:
        f.write(export.soup_obj_text(tet_fx3x3))


def save_tet_face_color(tet_fx3x3, tetcolor_fx3x3, f_name):
    with open(f_name, "w") as f:
        f.write(export.soup_color_obj_text(tet_fx3x3, tetcolor_fx3x3))
