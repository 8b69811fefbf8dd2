"""INTEGRATION.md section A as code: make an UNCHANGED DefTet checkout import this repository's
HIP-backed operators.

    import deftet_amd.overlay as overlay
    overlay.install()            # before `import layers`, `import utils.tet_utils`, `import kaolin`
    import train_multigpu        # the reference's own scripts, unmodified

`install()` registers, under the reference's module names, the drop-in modules of this package for
every import the hot path goes through:

    layers.DefTet.check_condition_tetrahedron_base.utils   check_condition_f_base
    layers.DefTet.tet_face_adj_m_idx.utils                 tet_face_adj_m_f_idx
    layers.DefTet.tet_analytic_distance_batch.utils        tet_analytic_distance_f_batch
    layers.nearest_neighbor                                NearestNeighbor
    utils.lib.{tet_point_adj,tet_face_adj,tet_adj_share,colaps_v}.interface
    kaolin.ops.mesh.check_sign, kaolin.render.mesh.deftet_sparse_render   (only when Kaolin itself is not
                                                           importable, or with kaolin=True; parity unpinned)
    kaolin.ops.mesh.{sample_points,index_vertices_by_faces}, kaolin.metrics.pointcloud.sided_distance,
    kaolin.metrics.trianglemesh.point_to_mesh_distance    (the evaluation metrics, same condition)
    kaolin.ops.conversions.{trianglemeshes_to_voxelgrids,voxelgrids_to_trianglemeshes}, kaolin.ops.voxelgrid.{extract_odms,
    project_odms}, kaolin.ops.mesh.{adjacency_matrix,face_normals}   (ground-truth preparation, dataloader.py; same condition)
    cv2                                                    empty stub (imported, never used: check_condition.../utils.py:14)

With `deftet_module=True` also `layers.DefTet.deftet` (the `DefTet` nn.Module built on the fused
operators) — otherwise the reference's own module runs on top of the replaced L1 operators.
With `render_model=True` also the flat module name `utils_tetsv` (a render-side checkout puts
diff_render/diftet_6_subdiv/3_model on sys.path and imports it by that name): the surface extraction and its OBJ writers.
With `point_voxel=True` also `layers.pv_module.functional.backend` (a module whose `_backend` carries the extension's twelve
names on this library's kernels, so importing it compiles nothing) and `layers.pv_module.functional.devoxelization`
(`deftet_amd.pointvoxel`); the reference's own functional/*.py, voxelization.py and pvconv.py run unchanged on top.
With `graph_conv=True` also `utils.matrix_utils` (`deftet_amd.utils.matrix_utils`): an unchanged layers/gcn_decoder.py then runs
the sparse product of every GraphConv (`sparse_batch_matmul`, gcn_decoder.py:55-56) on `hip_ops.vertex_aggregate`, with the
adjacency converted once per tensor and device; `convert_torch_sparse`, `cross_dot_torch`, `det_m` and `MySparse` come with it.
Nothing here touches a CPU fallback: every replaced entry point raises on non-GPU tensors.
"""
import importlib
import importlib.util
import sys
import types

L1_MODULES = {
    "layers.DefTet.check_condition_tetrahedron_base.utils": "deftet_amd.layers.DefTet.check_condition_tetrahedron_base.utils",
    "layers.DefTet.tet_face_adj_m_idx.utils": "deftet_amd.layers.DefTet.tet_face_adj_m_idx.utils",
    "layers.DefTet.tet_analytic_distance_batch.utils": "deftet_amd.layers.DefTet.tet_analytic_distance_batch.utils",
    "layers.nearest_neighbor": "deftet_amd.layers.nearest_neighbor",
    "utils.lib.tet_point_adj.interface": "deftet_amd.utils.lib.tet_point_adj.interface",
    "utils.lib.tet_face_adj.interface": "deftet_amd.utils.lib.tet_face_adj.interface",
    "utils.lib.tet_adj_share.interface": "deftet_amd.utils.lib.tet_adj_share.interface",
    "utils.lib.colaps_v.interface": "deftet_amd.utils.lib.colaps_v.interface",
}


def _kaolin_check_sign(verts, faces, points, hash_resolution=512):
    """kal.ops.mesh.check_sign(verts [B,V,3], faces [F,3], points [B,N,3]) -> bool [B,N]
    (`hash_resolution` only steers Kaolin's own acceleration structure)."""
    from deftet_amd import hip_ops
    return hip_ops.check_sign(verts, faces, points)


def kaolin_shim():
    """A module tree exposing the two Kaolin entry points the hot path calls
    (layers/DefTet/deftet.py:46, diff_render/diftet_6_subdiv/5_rendereq/deftetrneder.py:97-100) and the four the evaluation
    metrics call, and the six of the ground-truth preparation (dataloader.py:33-46, :80; deftet_amd.dataprep)."""
    from deftet_amd.render.deftet_sparse_render import deftet_sparse_render
    kal = types.ModuleType("kaolin")
    kal.__path__ = []                                  # a package, so `import kaolin.ops.mesh` resolves through sys.modules
    ops, render = types.ModuleType("kaolin.ops"), types.ModuleType("kaolin.render")
    ops.__path__, render.__path__ = [], []
    ops_mesh, render_mesh = types.ModuleType("kaolin.ops.mesh"), types.ModuleType("kaolin.render.mesh")
    ops_mesh.check_sign = _kaolin_check_sign
    render_mesh.deftet_sparse_render = deftet_sparse_render
    kal.ops, kal.render, ops.mesh, render.mesh = ops, render, ops_mesh, render_mesh
    # the evaluation metrics (eval.py:237-260, utils/point_cloud_utils.py, dataloader.py:76-99)
    from deftet_amd import metrics
    ops_mesh.sample_points = metrics.sample_points
    ops_mesh.index_vertices_by_faces = metrics.index_vertices_by_faces
    met, met_pc, met_tm = (types.ModuleType(n) for n in ("kaolin.metrics", "kaolin.metrics.pointcloud", "kaolin.metrics.trianglemesh"))
    met.__path__ = []
    met_pc.sided_distance = metrics.sided_distance
    met_tm.point_to_mesh_distance = metrics.point_to_mesh_distance
    kal.metrics, met.pointcloud, met.trianglemesh = met, met_pc, met_tm
    from deftet_amd import dataprep
    ops_conv, ops_vox = types.ModuleType("kaolin.ops.conversions"), types.ModuleType("kaolin.ops.voxelgrid")
    ops_conv.trianglemeshes_to_voxelgrids = dataprep.trianglemeshes_to_voxelgrids
    ops_conv.voxelgrids_to_trianglemeshes = dataprep.voxelgrids_to_trianglemeshes
    ops_vox.extract_odms, ops_vox.project_odms = dataprep.extract_odms, dataprep.project_odms
    ops_mesh.adjacency_matrix, ops_mesh.face_normals = dataprep.adjacency_matrix, dataprep.face_normals
    ops.conversions, ops.voxelgrid = ops_conv, ops_vox
    kal.__deftet_amd_shim__ = True
    return {"kaolin": kal, "kaolin.ops.conversions": ops_conv, "kaolin.ops.voxelgrid": ops_vox, "kaolin.ops": ops, "kaolin.render": render, "kaolin.ops.mesh": ops_mesh,
            "kaolin.render.mesh": render_mesh, "kaolin.metrics": met, "kaolin.metrics.pointcloud": met_pc,
            "kaolin.metrics.trianglemesh": met_tm}


def point_voxel_modules():
    """The two modules `point_voxel=True` registers: the extension's backend by name, and the devoxelization functions."""
    from deftet_amd import pointvoxel
    backend = types.ModuleType("layers.pv_module.functional.backend")
    backend._backend = pointvoxel.backend
    backend.__all__ = ["_backend"]
    return {"layers.pv_module.functional.backend": backend, "layers.pv_module.functional.devoxelization": pointvoxel}


def install(kaolin=None, deftet_module=False, stub_cv2=True, render_model=False, point_voxel=False, graph_conv=False):
    """Register the overlay in sys.modules; returns the list of names it registered.
    kaolin: True = always shim, False = never, None = shim only if `import kaolin` would fail."""
    done = []
    for ref_name, ours in L1_MODULES.items():
        sys.modules[ref_name] = importlib.import_module(ours)
        done.append(ref_name)
    if deftet_module:
        sys.modules["layers.DefTet.deftet"] = importlib.import_module("deftet_amd.layers.DefTet.deftet")
        done.append("layers.DefTet.deftet")
    if render_model:
        sys.modules["utils_tetsv"] = importlib.import_module("deftet_amd.render.utils_tetsv")
        done.append("utils_tetsv")
    if point_voxel:
        for name, mod in point_voxel_modules().items():
            sys.modules[name] = mod
            done.append(name)
    if graph_conv:
        sys.modules["utils.matrix_utils"] = importlib.import_module("deftet_amd.utils.matrix_utils")
        done.append("utils.matrix_utils")
    if kaolin is None:
        kaolin = "kaolin" not in sys.modules and importlib.util.find_spec("kaolin") is None
    if kaolin:
        for name, mod in kaolin_shim().items():
            sys.modules[name] = mod
            done.append(name)
    if stub_cv2 and "cv2" not in sys.modules and importlib.util.find_spec("cv2") is None:
        sys.modules["cv2"] = types.ModuleType("cv2")
        done.append("cv2")
    return done


def uninstall(names):
    for n in names:
        sys.modules.pop(n, None)
