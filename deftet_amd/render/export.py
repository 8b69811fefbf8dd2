"""Surface export: the OBJ writers of the reference, formatted a whole array at a time, and the threshold sweep of
`Deftet.saveobj` (/root/reference/diff_render/diftet_6_subdiv/3_model/deftet.py:503-557) on the GPU extraction.

    soup_obj_text / soup_color_obj_text   the text save_tet_face / save_tet_face_color write (utils/tet_utils.py:473-482,
                                          3_model/utils_tetsv.py:131-141, 228-239), byte for byte: 'v %f %f %f\\n' per corner
                                          (six numbers with colours) and 'f %d %d %d\\n' with idx+1, idx+3, idx+2 per triangle
    mesh_obj_text                         an indexed mesh in the same conventions (new: the reference has no indexed writer)
    save_surface_objs                     the eight files of saveobj (+ the indexed `tet-mesh-...` files with welded=True, + the
                                          marching-tetrahedra `mt-geo-...` / `mt-color-...` files with iso)

The reference formats per triangle in a Python loop and grows one string; here one '%' application formats a block of rows.
'%f' of inf and nan is left as Python prints it.
"""
import os

import numpy as np
import torch

from deftet_amd import hip_ops

_BLOCK = 1 << 15                                             # rows per '%' application (bounds the argument tuple)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _format_rows(fmt, table):
    """''.join(fmt % tuple(row) for row in table) with one '%' per block of rows; table is float64 [n, k] ('%d' of an integral
    double prints the integer)."""
    out = []
    for i in range(0, table.shape[0], _BLOCK):
        blk = table[i:i + _BLOCK]
        out.append((fmt * blk.shape[0]) % tuple(blk.ravel().tolist()))
    return "".join(out)


def _soup_table(cols, n_per_corner):
    F = cols.shape[0]
    idx = np.arange(F, dtype=np.float64)[:, None] * 3
    return np.concatenate([cols.reshape(F, 3 * n_per_corner).astype(np.float64), idx + 1, idx + 3, idx + 2], axis=1)


def soup_obj_text(tet_fx3x3):
    tri = _np(tet_fx3x3).reshape(-1, 3, 3)
    return _format_rows("v %f %f %f\n" * 3 + "f %d %d %d\n", _soup_table(tri, 3))


def soup_color_obj_text(tet_fx3x3, tetcolor_fx3x3):
    tri, col = _np(tet_fx3x3).reshape(-1, 3, 3), _np(tetcolor_fx3x3).reshape(-1, 3, 3)
    if tri.shape[0] != col.shape[0]:
        raise ValueError("%d triangles, %d colour rows" % (tri.shape[0], col.shape[0]))
    return _format_rows("v %f %f %f %f %f %f\n" * 3 + "f %d %d %d\n", _soup_table(np.concatenate([tri, col], axis=2), 6))


def mesh_obj_text(verts_vx3, faces_fx3, colors_vx3=None, normals_vx3=None):
    """Indexed mesh: one 'v' line per vertex (with colours: six numbers) and 'f a+1 c+1 b+1' per face — the soup writers' 1,3,2
    order, which turns the extraction's inward triangles outward.  With normals_vx3: one 'vn' line per vertex after the 'v'
    lines and faces as 'f a//a c//c b//b'."""
    v = _np(verts_vx3).reshape(-1, 3).astype(np.float64)
    f = _np(faces_fx3).reshape(-1, 3).astype(np.float64) + 1
    if colors_vx3 is None:
        head = _format_rows("v %f %f %f\n", v)
    else:
        head = _format_rows("v %f %f %f %f %f %f\n", np.concatenate([v, _np(colors_vx3).reshape(-1, 3).astype(np.float64)], axis=1))
    if normals_vx3 is not None:
        vn = _np(normals_vx3).reshape(-1, 3).astype(np.float64)
        if vn.shape[0] != v.shape[0]:
            raise ValueError("%d vertices, %d normals" % (v.shape[0], vn.shape[0]))
        return head + _format_rows("vn %f %f %f\n", vn) + _format_rows("f %d//%d %d//%d %d//%d\n", f[:, [0, 0, 2, 2, 1, 1]])
    return head + _format_rows("f %d %d %d\n", f[:, [0, 2, 1]])


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)


def save_surface_objs(points_px3, feat, tet_tx4, nbr, savedir, prefix, thresholds=(0.005, 0.05, 0.15, 0.25), welded=False,
                      iso=None, keep_largest=False, min_component=0, fill_voids=False, normals=False, subdivide=0,
                      iso_keep_largest=False, iso_min_faces=0, iso_drop_voids=False):
    """Writes what Deftet.saveobj writes (3_model/deftet.py:533-557): for every threshold `tet-geo-<prefix>-thres-<t>.obj` and
    `tet-color-<prefix>-thres-<t>.obj`.  `feat` = (weights [P] / [P,1], colours [P,3]) as `processfunc` returns them, or one
    [P,4] tensor holding them side by side; the colours are written reversed (colorsnp_px3[:, ::-1], :513).  The per-tet
    occupancy is the maximum of the four corner weights (:522-523), fused into the extraction.  nbr: hip_ops.tet_face_neighbours
    of the tet list (or the reference's list of four sparse matrices).  welded=True adds `tet-mesh-<prefix>-thres-<t>.obj`, the
    same surface as an indexed mesh with colours.  Returns the list of paths.  An export path, not a training step: every threshold is
    one surface_extract call (its own read-back of the offsets, the fused maximum computed again) and, with welded, one more
    read-back in surface_weld.  With `iso` it additionally writes `mt-geo-<prefix>-iso-<iso>.obj` and `mt-color-<prefix>-iso-<iso>.obj`:
    the marching-tetrahedra surface of the per-vertex weights at that level (hip_ops.marching_tets) as an indexed mesh, without and
    with the colours, faces in the operator's winding (normals towards the lower weights).
    keep_largest / min_component / fill_voids clean the occupancy of every threshold on the device before its surface is taken
    (hip_ops.occupancy_cleanup: floaters dropped, enclosed voids filled; the reference leaves this to trimesh, utils_tetsv.py:132):
    the per-tet occupancy is then a torch maximum over the corner weights (the fused maximum, bit for bit, on finite weights),
    inside = occ > float32(2 thres) — the threshold mode's own inside test — a dropped tet gets 0, a filled one 1, and the result
    goes to surface_extract as `occ`.  With all three left at their defaults nothing of this runs.  The `mt-` files are not
    cleaned: a per-vertex field has no per-tet mask (by these three, that is: iso_keep_largest / iso_min_faces / iso_drop_voids below
    clean them as a mesh).  normals=True (with iso): the `mt-geo` file also carries one `vn` line per
    vertex — the unit outward normal, minus the normalised gradient of the weights (hip_ops.vertex_field_gradient) interpolated
    along the crossing edge, zero where that gradient is zero — and its faces read `f a//a b//b c//c`.  subdivide = n > 0 (with
    iso): the `mt-` files hold the mesh after n rounds of Loop subdivision (hip_ops.loop_subdivide_mesh), colours and normals
    weighted like the positions, the normals normalised again; with 0 nothing of it runs.
    iso_keep_largest / iso_min_faces / iso_drop_voids (with iso) are the way to clean the `mt-` files: the marching-tetrahedra
    mesh goes through hip_ops.mesh_cleanup on the device before the subdivision — cavity shells (closed components of negative
    volume) and floaters dropped, the mesh compacted, colours and normals carried along.  They leave the `tet-` files alone, as
    keep_largest / min_component / fill_voids leave the `mt-` files; with all three left at their defaults nothing of it runs."""
    levels = int(subdivide)
    if levels < 0:
        raise ValueError("save_surface_objs: subdivide = %d is negative" % levels)
    if isinstance(feat, (tuple, list)):
        weights, colours = feat
    else:
        weights, colours = feat[:, :1], feat[:, 1:4]
    pts = hip_ops._f32c(points_px3 if isinstance(points_px3, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points_px3)))
    hip_ops._lib.require_gpu(pts, weights, colours)
    dev = pts.device
    tet = torch.as_tensor(tet_tx4).to(dev).long()
    nbr = hip_ops.neighbours_from_adj_list(nbr, dev)
    col = hip_ops._f32c(colours).flip(-1)
    tet_p = pts[tet.reshape(-1)].reshape(1, -1, 4, 3)
    tet_c = col[tet.reshape(-1)].reshape(1, -1, 4, 3)
    w = hip_ops._f32c(weights).reshape(1, -1)
    paths = []
    clean = bool(keep_largest) or int(min_component) > 0 or bool(fill_voids)
    occ = w[:, tet.reshape(-1)].reshape(1, -1, 4).amax(dim=2) if clean else None
    for thres in thresholds:
        if clean:
            inside = occ > float(np.float32(2.0 * thres))
            keep, _comps, bad = hip_ops._occupancy_cleanup(inside, nbr, keep_largest, min_component, fill_voids, False)
            soup = hip_ops.surface_extract(tet_p, hip_ops.cleaned_occupancy(occ, inside, keep), nbr, "threshold", thres=thres, attr=tet_c,
                                           tet_idx=tet, return_faces=welded)
            hip_ops._bad_neighbour("save_surface_objs", bad)   # (read behind the extraction's own synchronisation)
        else:
            soup = hip_ops.surface_extract(tet_p, None, nbr, "threshold", thres=thres, attr=tet_c, vertex_weights=w, tet_idx=tet,
                                           return_faces=welded)
        face, fcol = soup.face[0].cpu().numpy(), soup.face_attr[0].cpu().numpy()
        paths.append("%s/tet-geo-%s-thres-%.3f.obj" % (savedir, prefix, thres))
        _write(paths[-1], soup_obj_text(face))
        paths.append("%s/tet-color-%s-thres-%.3f.obj" % (savedir, prefix, thres))
        _write(paths[-1], soup_color_obj_text(face, fcol))
        if welded:
            v, c, f, _old = hip_ops.surface_weld(pts, soup.faces[0], col)
            paths.append("%s/tet-mesh-%s-thres-%.3f.obj" % (savedir, prefix, thres))
            _write(paths[-1], mesh_obj_text(v, f, c))
    if iso is not None:
        attr, vn = col, None
        if normals:                                                   # the gradient rides along with the colours: one extraction
            grad = hip_ops.vertex_field_gradient(w.reshape(1, -1, 1), pts[None], tet)
            attr = torch.cat([col, grad.reshape(-1, 3)], dim=1)
        mesh = hip_ops.marching_tets(pts, w, hip_ops.TetEdges(tet, pts.shape[0]), iso=iso, attr=attr)
        v, f, c = mesh.verts[0].detach(), mesh.faces[0], mesh.vert_attr[0].detach()
        if (bool(iso_keep_largest) or int(iso_min_faces) > 0 or bool(iso_drop_voids)) and f.shape[0]:
            clean = hip_ops.mesh_cleanup(v, f, c, keep_largest=iso_keep_largest, min_faces=iso_min_faces, drop_voids=iso_drop_voids)
            v, f, c = clean.verts, clean.faces, clean.attr
        if levels and f.shape[0]:
            if normals:                                               # unit normals go in, and are normalised again below
                c = torch.cat([c[:, :3], hip_ops.unit_normals(c[:, 3:6])], dim=1)
            v, f, c = hip_ops.loop_subdivide_mesh(v, f, c, levels=levels)
            if normals:                                               # (unit_normals below negates: these are normals already)
                c = torch.cat([c[:, :3], -c[:, 3:6]], dim=1)
        f = f[:, [0, 2, 1]]                                           # (the writer swaps them back)
        if normals:
            c, vn = c[:, :3], hip_ops.unit_normals(c[:, 3:6])
        paths.append("%s/mt-geo-%s-iso-%.3f.obj" % (savedir, prefix, iso))
        _write(paths[-1], mesh_obj_text(v, f, normals_vx3=vn))
        paths.append("%s/mt-color-%s-iso-%.3f.obj" % (savedir, prefix, iso))
        _write(paths[-1], mesh_obj_text(v, f, c))
    return paths
