"""_lib.call on the GPU: every form of its `ws` argument, a None pointer, the error text and the stream, each against the
written-out convention (_lib.check(lib.f(_lib.ptr(..), .., _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)), "f")) or the
front end in hip_ops.  Tiny inputs: the whole file is a handful of launches."""
import pytest
import torch

from deftet_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu

EXCLUSIVE, INCLUSIVE = 0, 1


def _vector(n, dev):
    g = torch.Generator().manual_seed(n)
    return torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).to(dev)


def _points(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _scan_written_out(x, kind):
    lib, dev, n = _lib.load(), x.device, x.numel()
    out = torch.empty_like(x)
    with _lib.on_device(dev):
        ws = _lib.workspace(dev, lib.deftet_scan_workspace_bytes(n, 4))
        _lib.check(lib.deftet_scan(_lib.ptr(x), _lib.ptr(out), n, 4, kind, _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)), "deftet_scan")
    return out


def _cumsum(x, kind):
    inc = torch.cumsum(x, 0).to(torch.int32)
    return inc if kind == INCLUSIVE else inc - x


# 2,048 elements per workgroup (prims.hpp kTile): 1, 64 and 65 are one partial tile (one lane, one wave, one lane more), 5,000
# is three tiles, the last one partial, so the carried tile prefixes are read
@pytest.mark.parametrize("n", [1, 64, 65, 5000])
@pytest.mark.parametrize("kind", [EXCLUSIVE, INCLUSIVE])
def test_workspace_by_byte_count(cuda, n, kind):
    x = _vector(n, cuda)
    out = torch.empty_like(x)
    assert _lib.call("deftet_scan", cuda, x, out, n, 4, kind, ws=_lib.load().deftet_scan_workspace_bytes(n, 4)) is None
    assert torch.equal(out, _scan_written_out(x, kind))
    assert torch.equal(out, _cumsum(x, kind))


@pytest.mark.parametrize("n", [65, 5000])
def test_workspace_owned_by_the_caller(cuda, n):
    x = _vector(n, cuda)
    out = torch.empty_like(x)
    ws = torch.empty(_lib.load().deftet_scan_workspace_bytes(n, 4), dtype=torch.uint8, device=cuda)     # exactly what the scan asks for
    _lib.call("deftet_scan", cuda, x, out, n, 4, INCLUSIVE, ws=ws)
    assert torch.equal(out, _cumsum(x, INCLUSIVE))


def test_no_workspace(cuda):
    pos = _points((1, 8, 3), 1, cuda)
    idx = torch.tensor([[0, 1, 2, 3], [7, 5, 3, 1], [4, 4, 6, 0], [2, 7, 1, 6]], device=cuda)[None]      # int64 [1,4,4]
    out = torch.empty(1, 4, 4, 3, device=cuda)
    _lib.call("deftet_tet_gather_fwd_f32", cuda, pos, idx, out, None, 1, 8, 4, 1)
    assert torch.equal(out, pos[:, idx[0]])
    assert torch.equal(out, hip_ops.tet_gather(pos, idx[0]))


def test_workspace_none_is_null_and_zero(cuda):
    q, p = _points((1, 7, 3), 2, cuda), _points((1, 5, 3), 3, cuda)
    out = torch.zeros(1, 7, device=cuda, dtype=torch.int32)
    _lib.call("deftet_nn_index_f32", cuda, q, p, out, 1, 7, 5, ws=None)          # (NULL, 0): the brute path
    assert torch.equal(out, hip_ops.nn_index(q, p, brute=True))
    assert torch.equal(out.long(), torch.cdist(q.double(), p.double()).argmin(-1))


def test_none_tensor_is_a_null_pointer(cuda):
    tets = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]]
    _f3, t2, tf2, _b3, n_multi = hip_ops.tet_to_face(tets, 6, cuda, with_boundary=True)
    assert n_multi == 0
    T = len(tets)
    nbr = torch.empty(T, 4, dtype=torch.int64, device=cuda)
    _lib.call("deftet_tet_neighbours_i64", cuda, t2, tf2, int(t2.shape[0]), T, nbr, None,
              ws=_lib.load().deftet_tet_neighbours_workspace_bytes(T))
    assert torch.equal(nbr, hip_ops.tet_neighbours(tets, 6, cuda))
    assert (nbr >= 0).sum().item() == 4                                           # two shared faces, seen from both sides


def test_error_names_the_entry_the_status_and_the_reason(cuda):
    x = _vector(8, cuda)
    out = torch.empty_like(x)
    nbytes = _lib.load().deftet_scan_workspace_bytes(8, 4)
    with pytest.raises(_lib.DefTetHipError) as e:                                 # kind 3: refused before any launch
        _lib.call("deftet_scan", cuda, x, out, 8, 4, 3, ws=nbytes)
    assert str(e.value).startswith("deftet_scan failed (-1): ") and "bad argument" in str(e.value)
    with pytest.raises(_lib.DefTetHipError) as e:
        _lib.call("deftet_scan", cuda, x, out, 8, 4, 3, ws=nbytes, what="x(count)")
    assert str(e.value).startswith("x(count) failed (-1): ") and "bad argument" in str(e.value)


def test_runs_on_the_current_stream(cuda):
    x = _vector(5000, cuda)
    want = _cumsum(x, INCLUSIVE)
    out = torch.zeros_like(x)
    torch.cuda.synchronize(cuda)                                                  # the inputs are ready: only `side` orders the scan
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        _lib.call("deftet_scan", cuda, x, out, 5000, 4, INCLUSIVE, ws=_lib.load().deftet_scan_workspace_bytes(5000, 4))
    side.synchronize()
    assert torch.equal(out.cpu(), want.cpu())
