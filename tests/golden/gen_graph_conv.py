#!/usr/bin/env python
"""Generates tests/golden/graph_conv.npz: one GraphConvBlock of the reference's GCN position decoder (layers/gcn_decoder.py:90-129)
run on the host with use_sparse=True, i.e. through the reference's own sparse_batch_matmul (utils/matrix_utils.py:22-33,
torch.sparse.mm).  The module is imported from the reference tree as it is; `layers.pv_utils`, which gcn_decoder.py imports for
its MLP tail and the block never touches, is stubbed in sys.modules.  Only numbers are stored.

    REF=<reference tree> python tests/golden/gen_graph_conv.py

Case: the res-8 Kuhn grid (V = 125), D⁻¹A of its vertex adjacency, B = 2, GraphConvBlock(size_in=12, size_out=8), seed 20.
Stored: the adjacency triplets (rows, cols, vals, n_vertex), every weight and bias of the block by its state_dict name
(w.<name>), the input x, the output y, the upstream gradient gy and the input gradient gx.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF") or ""


def normalized_adjacency(tets, V):
    """D⁻¹A of the tets' vertex graph: the unique directed pairs i != j that share a tet, row-major, 1/deg(i) rounded once
    from fp64"""
    t = np.asarray(tets, np.int64)
    pairs = np.concatenate([t[:, [a, b]] for a in range(4) for b in range(4) if a != b], 0)
    pairs = np.unique(pairs, axis=0)
    rows, cols = pairs[:, 0], pairs[:, 1]
    deg = np.bincount(rows, minlength=V).astype(np.float64)
    return rows, cols, (1.0 / deg[rows]).astype(np.float32)


def main():
    if not os.path.isdir(os.path.join(REF, "layers")):
        sys.exit("set REF to the reference tree")
    sys.path.insert(0, ROOT)
    from deftet_amd import grids
    sys.path.insert(0, REF)
    stub = types.ModuleType("layers.pv_utils")
    stub.create_mlp_components = None                      # (imported by name at gcn_decoder.py:13; GraphConvBlock never calls it)
    sys.modules["layers.pv_utils"] = stub
    from layers.gcn_decoder import GraphConvBlock

    torch.manual_seed(20)
    verts, tets = grids.kuhn_grid(8)
    V = verts.shape[0]
    rows, cols, vals = normalized_adjacency(tets, V)
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (V, V))
    block = GraphConvBlock(size_in=12, size_out=8)
    x = torch.randn(2, V, 12).requires_grad_(True)
    y = block(x, adj, use_sparse=True)
    gy = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x, gy)
    out = dict(rows=rows.astype(np.int64), cols=cols.astype(np.int64), vals=vals, n_vertex=np.int64(V), x=x.detach().numpy(),
               y=y.detach().numpy(), gy=gy.numpy(), gx=gx.numpy())
    for name, w in block.state_dict().items():
        out["w." + name] = w.numpy()
    path = os.path.join(HERE, "graph_conv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", sorted(k for k in out if k.startswith("w.")))


if __name__ == "__main__":
    main()
