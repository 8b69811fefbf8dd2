"""Drop-in for utils/matrix_utils.py: the same five names and signatures.

sparse_batch_matmul is the sparse product of the GCN position decoder (layers/gcn_decoder.py:55-56).  The reference transposes
[B,V,C] into [V, B·C], runs torch.sparse.mm and hands back a strided view; here it is one hip_ops.vertex_aggregate call on a
hip_ops.VertexAdjacency, which the caller passes itself or which is built once per torch sparse tensor OBJECT and device and
kept for as long as that tensor lives (GCNMLPDecoder.get_normalized_adj hands the same object per device on every step).
The rest is plain torch.
"""
import threading
import weakref

import torch
from torch import nn

from deftet_amd import hip_ops
from deftet_amd.utils.tet_utils import convert_torch_sparse  # noqa: F401  (utils/matrix_utils.py:14-20)

# id(tensor) -> (weak reference to the tensor, its VertexAdjacency).  The id only finds the slot: an entry counts when its
# reference still gives that very object, and the reference's callback drops the entry when the tensor dies, so a new tensor at
# a recycled address (or id) never meets a stale adjacency.
_adjacencies = {}
_adjacencies_lock = threading.RLock()                  # (re-entrant: a tensor may die, and its callback run, inside a build)


def _adjacency_of(sparse_matrix):
    key = id(sparse_matrix)
    with _adjacencies_lock:
        hit = _adjacencies.get(key)
        if hit is not None and hit[0]() is sparse_matrix:
            return hit[1]

        def _drop(ref, key=key):
            with _adjacencies_lock:
                cur = _adjacencies.get(key)
                if cur is not None and cur[0] is ref:
                    del _adjacencies[key]

        adj = hip_ops.VertexAdjacency.from_sparse(sparse_matrix)
        _adjacencies[key] = (weakref.ref(sparse_matrix, _drop), adj)
        return adj


def sparse_batch_matmul(sparse_matrix, dense_matrix_batch):
    """sparse_matrix (n, n): a hip_ops.VertexAdjacency, or a torch sparse COO tensor on the GPU (converted once per tensor
    object); dense_matrix_batch (b, n, p) -> (b, n, p), contiguous.  Differentiable w.r.t. the dense operand."""
    if isinstance(sparse_matrix, hip_ops.VertexAdjacency):
        return hip_ops.vertex_aggregate(dense_matrix_batch, sparse_matrix)
    from deftet_amd import _lib
    _lib.require_gpu(dense_matrix_batch, sparse_matrix)
    return hip_ops.vertex_aggregate(dense_matrix_batch, _adjacency_of(sparse_matrix))


def cross_dot_torch(a, b):
    """a × b along the last axis (despite the name, as in the reference)"""
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    return torch.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], dim=-1)


def det_m(m_bx3x3):
    """determinants of a batch of 3x3 matrices as the triple product row0 · (row1 × row2)"""
    return (m_bx3x3[:, 0, :] * cross_dot_torch(m_bx3x3[:, 1, :], m_bx3x3[:, 2, :])).sum(dim=-1)


class MySparse(nn.Module):
    """Carries a sparse matrix through nn.DataParallel as its indices, values and size; construct() puts it together again."""

    def __init__(self, sparse_m):
        super().__init__()
        self.indices = sparse_m._indices()
        self.values = sparse_m._values()
        self.indices.requires_grad = False
        self.values.requires_grad = False
        self.shape = sparse_m.size()

    def construct(self):
        return torch.sparse_coo_tensor(self.indices, self.values, self.shape)
