"""Callers written the way the reference's dataloader.py reaches Kaolin — the same import statement, the same call shapes
(dataloader.py:9, :24-61 MakeSurfaceMesh.__call__, :73-84 SamplePointsFromMesh, :91-97 kaolin_mesh_to_sdf) — used to prove that
`deftet_amd.overlay.install(kaolin=True)` covers ground-truth preparation.  Import this module only AFTER the overlay is installed."""


def import_like_reference():
    import kaolin as kal
    return dict(trianglemeshes_to_voxelgrids=kal.ops.conversions.trianglemeshes_to_voxelgrids,
                extract_odms=kal.ops.voxelgrid.extract_odms, project_odms=kal.ops.voxelgrid.project_odms,
                voxelgrids_to_trianglemeshes=kal.ops.conversions.voxelgrids_to_trianglemeshes,
                adjacency_matrix=kal.ops.mesh.adjacency_matrix, face_normals=kal.ops.mesh.face_normals)


def make_surface_mesh(vertices, faces, resolution=100, smoothing_iterations=3, max_length=0.9):
    """MakeSurfaceMesh.__call__ with the tensors already on the GPU and left there"""
    import kaolin as kal
    import torch
    max_l = max(vertices[..., 0].max() - vertices[..., 0].min(),
                vertices[..., 1].max() - vertices[..., 1].min(),
                vertices[..., 2].max() - vertices[..., 2].min())
    vertices = (vertices / max_l) * max_length
    mid_p = (vertices.max(dim=0)[0] + vertices.min(dim=0)[0]) / 2
    vertices = vertices - mid_p.unsqueeze(dim=0)
    voxelgrid = kal.ops.conversions.trianglemeshes_to_voxelgrids(
        vertices.unsqueeze(0), faces,
        resolution=resolution)
    odms = kal.ops.voxelgrid.extract_odms(voxelgrid)
    voxelgrid = kal.ops.voxelgrid.project_odms(odms)
    new_vertices, new_faces = kal.ops.conversions.voxelgrids_to_trianglemeshes(
        voxelgrid,
    )
    new_vertices = new_vertices[0]
    new_faces = new_faces[0]
    adj_mat = kal.ops.mesh.adjacency_matrix(
        new_vertices.shape[0],
        new_faces)
    num_neighbors = torch.sparse.sum(
        adj_mat, dim=1).to_dense().view(-1, 1)
    for i in range(smoothing_iterations):
        neighbor_sum = torch.sparse.mm(adj_mat, new_vertices)
        new_vertices = neighbor_sum / num_neighbors
    orig_min = vertices.min(dim=0)[0]
    orig_max = vertices.max(dim=0)[0]
    new_min = new_vertices.min(dim=0)[0]
    new_max = new_vertices.max(dim=0)[0]
    new_vertices = (new_vertices - new_min) / (new_max - new_min)
    new_vertices = new_vertices * (orig_max - orig_min) + orig_min
    return new_vertices, new_faces


def unit_normals(vertices_1xvx3, faces):
    """SamplePointsFromMesh.__call__, the normals of every face"""
    import kaolin as kal
    face_vertices = kal.ops.mesh.index_vertices_by_faces(vertices_1xvx3, faces)
    return kal.ops.mesh.face_normals(face_vertices, unit=True)


def kaolin_mesh_to_sdf(verts_bxnx3, face_fx3, points_bxnx3):
    """dataloader.py:91-97, as written there"""
    import kaolin as kal
    sign = kal.ops.mesh.check_sign(verts_bxnx3, face_fx3, points_bxnx3, hash_resolution=512)
    face_vertices = kal.ops.mesh.index_vertices_by_faces(verts_bxnx3, face_fx3)
    distance, index, dist_type = kal.metrics.trianglemesh.point_to_mesh_distance(points_bxnx3, face_vertices)
    sign = sign.float() * 2.0 - 1.0  # (1: inside; -1: outside)
    sdf = sign * distance
    return sdf
