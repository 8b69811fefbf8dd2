from .deftet_sparse_render import deftet_sparse_render, deftet_sparse_render_composite  # noqa: F401
from .compositing import alpha_composite  # noqa: F401
from .camera import perspective, face_attributes, render_mesh_color  # noqa: F401
from .laplacian import get_featlap  # noqa: F401
from .vertices import render_vertices, model_forward  # noqa: F401
from .iso_surface import marching_tets, marching_tets_normals, model_tet_edges  # noqa: F401
from .field_points import field_at_points, model_tet_topology  # noqa: F401
