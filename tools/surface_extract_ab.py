#!/usr/bin/env python
"""A/B of the surface extraction at res 70, B = 8 (jittered Kuhn grid; sphere occupancy r = 0.3 for BINARY, smooth vertex weights
through the per-tet maximum for THRESHOLD, colours with C = 3):

  (a) hip      hip_ops.surface_extract: count + scan + fill for the whole batch, one read-back of the offsets
  (b) torch    utils/tet_utils.py:427-471 restated in torch on the same GPU — four sparse matmuls, the has_adj rule, boolean-mask
               indexing of three [B,T,4,3] concatenations shape by shape (one sync per mask): the route the reference takes.
               For THRESHOLD the same route with the thresholded predicate (float64 difference) and the colour gathers
  (c) host     THRESHOLD only, one shape: the render side's route — scipy float64 products and numpy masks on the host plus the
               per-triangle '%f' writer — against (a) for one shape plus the whole-array writer

The variants alternate inside one process; every call ends in a synchronise (the outputs are lists whose lengths are on the host)
and is timed with the host clock.  Every timed step checks that (a) and (b) give the same bits.  One JSON line per variant and
mode: median ms and spread, the bytes the new path moves, and the count pass's time as a fraction of the copy rate
(deftet_profile_select("k_sx_count") against deftet_bandwidth_probe over the same bytes).

    python tools/surface_extract_ab.py [--steps 20] [--warmup 3] [--res 70 --batch 8]
    python tools/surface_extract_ab.py --check      # a tiny size; argument parsing and input generation up to the first GPU call
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deftet_amd import grids  # noqa: E402

CORNER = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 0], [3, 2, 1]])     # local face i -> corners (a, b, c)


def obj_text_loop(tri, col=None):
    """the reference's writers (utils_tetsv.py:131-141, 228-239): one '%' per line, per triangle"""
    out = ""
    parts = []
    for k, t in enumerate(tri):
        for c in range(3):
            if col is None:
                parts.append('v %f %f %f\n' % (t[c][0], t[c][1], t[c][2]))
            else:
                parts.append('v %f %f %f %f %f %f\n' % (t[c][0], t[c][1], t[c][2], col[k][c][0], col[k][c][1], col[k][c][2]))
        parts.append('f %d %d %d\n' % (3 * k + 1, 3 * k + 3, 3 * k + 2))
    return out.join(parts)


def make_inputs(res, batch):
    verts, tets = grids.kuhn_grid(res)
    pos = grids.jittered_positions(verts, res, batch)
    cen = pos[:, tets.astype(np.int64)].mean(2)
    occ = (np.linalg.norm(cen, axis=-1) < 0.3).astype(np.float32)
    rng = np.random.default_rng(70)
    k = rng.uniform(2, 9, (batch, 1, 3))
    w = (0.5 + 0.5 * np.sin((pos.astype(np.float64) * k).sum(-1) + rng.uniform(0, 6, (batch, 1)))).astype(np.float32) * 0.6
    col = rng.random((batch, verts.shape[0], 3)).astype(np.float32)
    return verts, tets, pos, occ, w, col


def moved_bytes(B, T, F, C, fused_max, V):
    """what the new path reads and writes: count = occupancy + the int32 table (+ the neighbours' occupancies from cache); fill =
    the same again plus, per emitted row, its source records and the rows"""
    count = B * T * (4 + 16) + (B * T * (16 + 4) + B * V * 4 if fused_max else 0)
    fill = B * T * (4 + 16) + F * (36 + 36 + (24 * C if C else 0))
    return dict(count=count, fill=fill)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--res", type=int, default=70)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="tiny size, stop before the first GPU call")
    args = ap.parse_args(argv)
    if args.check:
        args.res, args.batch = 4, 2
    verts, tets, pos, occ, w, col = make_inputs(args.res, args.batch)
    B, V, T = args.batch, len(verts), len(tets)
    if args.check:
        print(json.dumps({"check": "ok", "B": B, "V": V, "T": T, "occupied": int(occ.sum()), "bytes_without_rows": moved_bytes(B, T, 0, 0, False, V)}))
        return 0

    import torch
    from deftet_amd import _lib, hip_ops
    from deftet_amd.render import export
    dev = torch.device("cuda:0")
    lib = _lib.load()
    t64 = torch.from_numpy(tets.astype(np.int64)).to(dev)
    nbr = hip_ops.tet_face_neighbours(tets, V, dev)
    pos_d, occ_d, w_d, col_d = (torch.from_numpy(x).to(dev) for x in (pos, occ, w, col))
    tet_p = pos_d[:, t64]                                       # [B,T,4,3]
    tet_c = col_d[:, t64]
    occ_w = w_d[:, t64].max(-1).values                          # (b)'s THRESHOLD input: the occupancy, computed outside the timed region
    # (b)'s adjacency: the four sparse matrices of get_tet_adj
    table = nbr.table
    adj = []
    for i in range(4):
        rows = torch.nonzero(table[:, i] >= 0)[:, 0]
        adj.append(torch.sparse_coo_tensor(torch.stack([rows, table[rows, i]]), torch.ones(rows.numel(), device=dev), (T, T)).coalesce())
    has_adj = [torch.sparse.sum(a, dim=1).to_dense().bool()[None, :, None] for a in adj]

    def torch_route(occ_bxt, mode, h=None, colour=None):
        o = occ_bxt[:, :, None]
        eq = []
        for i in range(4):
            dense = o.transpose(0, 1).reshape(T, -1)
            no = torch.sparse.mm(adj[i], dense).reshape(T, B, 1).transpose(0, 1)
            if mode == "binary":
                eq.append((no != o) & (o == 1) & has_adj[i])
            else:
                eq.append(((no.double() - o.double()).abs() > h) & (o > np.float32(h * 2)))
        eq = torch.cat(eq, -1)
        outs = []
        for src in ([tet_p] if colour is None else [tet_p, colour]):
            A, Bc, Cc, D = (src[:, :, k:k + 1] for k in range(4))
            fa, fb, fc = torch.cat([A, Bc, Cc, D], 2), torch.cat([Bc, A, D, Cc], 2), torch.cat([Cc, D, A, Bc], 2)
            m = eq[..., None].expand_as(fa)
            outs.append([torch.cat([fa[b][m[b]].reshape(-1, 1, 3), fb[b][m[b]].reshape(-1, 1, 3), fc[b][m[b]].reshape(-1, 1, 3)], 1) for b in range(B)])
        return outs

    def hip_binary():
        return [hip_ops.surface_extract(tet_p, occ_d, nbr, "binary").face]

    def hip_threshold():
        s = hip_ops.surface_extract(tet_p, None, nbr, "threshold", thres=0.15, attr=tet_c, vertex_weights=w_d, tet_idx=t64)
        return [s.face, s.face_attr]

    pairs = [("binary", hip_binary, lambda: torch_route(occ_d, "binary")),
             ("threshold+colour", hip_threshold, lambda: torch_route(occ_w, "threshold", 0.15, tet_c))]
    for mode, f_hip, f_torch in pairs:
        times = {"hip": [], "torch": []}
        rows = 0
        for step in range(args.warmup + args.steps):
            outs = {}
            for name, fn in (("hip", f_hip), ("torch", f_torch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
            for x, y in zip(outs["hip"], outs["torch"]):
                for b in range(B):
                    if not torch.equal(x[b].view(torch.int32), y[b].view(torch.int32)):
                        raise SystemExit("%s step %d shape %d: the new path differs from the torch route" % (mode, step, b))
            rows = sum(int(x.shape[0]) for x in outs["hip"][0])
        nbytes = moved_bytes(B, T, rows, 3 if "colour" in mode else 0, "colour" in mode, V)
        # the count pass under the library's kernel timer, against a copy of the same bytes
        kern_ms = {}
        for kname in (b"k_sx_count", b"k_sx_fill"):
            lib.deftet_profile_select(kname)
            for _ in range(10):
                f_hip()
            ms, n = ctypes.c_double(), ctypes.c_longlong()
            lib.deftet_profile_read(ctypes.byref(ms), ctypes.byref(n))
            lib.deftet_profile_select(b"")
            kern_ms[kname.decode()] = ms.value / max(n.value, 1)
        count_ms = kern_ms["k_sx_count"]
        idx = hip_ops.surface_extract(tet_p, occ_d if mode == "binary" else occ_w, nbr, "binary" if mode == "binary" else "threshold",
                                      thres=0.15, return_index=True).index
        nonempty = sum(int(torch.unique(i[:, 0] // 256).numel()) for i in idx)
        nblk = (T + 255) // 256
        nb = max(B * T * 20 // 32768 * 32768, 32768)
        src, dst = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
        cp = []
        for _ in range(13):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.deftet_bandwidth_probe(src.data_ptr(), dst.data_ptr(), nb, 0, None, _lib.current_stream(dev))
            e1.record()
            e1.synchronize()
            cp.append(e0.elapsed_time(e1))
        copy_ms = float(np.median(cp[3:])) / 2                   # the copy moves nb bytes each way; the count pass only reads
        for name in ("hip", "torch"):
            t = np.asarray(times[name])
            line = {"variant": name, "mode": mode, "config": "res=%d B=%d T=%d V=%d" % (args.res, B, T, V), "rows": rows, "steps": len(t),
                    "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}
            if name == "hip":
                line.update(bytes=nbytes, count_kernel_ms=round(count_ms, 5), fill_kernel_ms=round(kern_ms["k_sx_fill"], 5),
                            nonempty_workgroup_fraction=round(nonempty / (B * nblk), 4), copy_same_bytes_ms=round(copy_ms, 5),
                            count_fraction_of_copy_rate=round(copy_ms / count_ms, 3) if count_ms > 0 else None,
                            speedup_vs_torch=round(float(np.median(times["torch"]) / np.median(t)), 2))
            print(json.dumps(line), flush=True)

    # (c) the render side's host route for one shape: scipy products + numpy masks + the per-triangle writer
    from scipy.sparse import coo_matrix
    tab = table.cpu().numpy()
    mats = []
    for i in range(4):
        rows = np.nonzero(tab[:, i] >= 0)[0]
        mats.append(coo_matrix((np.ones(rows.size), (rows, tab[rows, i])), shape=(T, T)).tocsr())
    tp, tc_, ow = tet_p[0].cpu().numpy(), tet_c[0].cpu().numpy(), occ_w[0].cpu().numpy().reshape(T, 1)
    with tempfile.TemporaryDirectory() as d:
        def host_route():
            eq = np.concatenate([(np.abs(m.dot(ow) - ow) > 0.15) & (ow > 0.15 * 2) for m in mats], -1)
            t, i = np.nonzero(eq)
            face, fcol = tp[t[:, None], CORNER[i]], tc_[t[:, None], CORNER[i]]
            open(os.path.join(d, "a.obj"), "w").write(obj_text_loop(face))
            open(os.path.join(d, "b.obj"), "w").write(obj_text_loop(face, fcol))
            return face

        def hip_route():
            s = hip_ops.surface_extract(tet_p[:1], None, nbr, "threshold", thres=0.15, attr=tet_c[:1], vertex_weights=w_d[:1], tet_idx=t64)
            face, fcol = s.face[0].cpu().numpy(), s.face_attr[0].cpu().numpy()
            open(os.path.join(d, "c.obj"), "w").write(export.soup_obj_text(face))
            open(os.path.join(d, "e.obj"), "w").write(export.soup_color_obj_text(face, fcol))
            return face
        th, tn = [], []
        for _ in range(3):
            t0 = time.perf_counter(); f0 = host_route(); th.append((time.perf_counter() - t0) * 1e3)   # noqa: E702
            t0 = time.perf_counter(); f1 = hip_route(); tn.append((time.perf_counter() - t0) * 1e3)    # noqa: E702
            assert f0.tobytes() == f1.tobytes()
            assert open(os.path.join(d, "a.obj")).read() == open(os.path.join(d, "c.obj")).read()
            assert open(os.path.join(d, "b.obj")).read() == open(os.path.join(d, "e.obj")).read()
    print(json.dumps({"variant": "host numpy/scipy + per-triangle writer", "mode": "threshold+colour, one shape, two files", "rows": int(f0.shape[0]),
                      "median_ms": round(float(np.median(th)), 2)}))
    print(json.dumps({"variant": "hip + whole-array writer", "mode": "threshold+colour, one shape, two files", "rows": int(f1.shape[0]),
                      "median_ms": round(float(np.median(tn)), 2), "speedup_vs_host": round(float(np.median(th) / np.median(tn)), 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
